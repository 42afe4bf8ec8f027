"""signerf_amd.engine without a GPU: the reader/writer lock, the handle's lifecycle decision, and what a CPU model shows of its engine."""
import gc
import os
import threading
import time
import weakref

import pytest
import torch

from helpers import small_config
from signerf_amd import _lib, engine

JOIN_S = 5.0      # every wait that must succeed; a timeout fails the test
REFUSED_S = 0.05  # every wait that must NOT succeed (a thread that has to stay blocked)


def test_rwlock_readers_share_and_a_waiting_writer_goes_first():
    lock = engine._RWLock()
    ev = {k: threading.Event() for k in ("a_in", "a_go", "b_in", "b_go", "w_in", "w_go", "c_started", "c_in", "c_go")}

    def reader(name):
        if name == "c":
            ev["c_started"].set()
        lock.acquire_read()
        ev[name + "_in"].set()
        ev[name + "_go"].wait(JOIN_S)
        lock.release_read()

    def writer():
        lock.acquire_write()
        ev["w_in"].set()
        ev["w_go"].wait(JOIN_S)
        lock.release_write()

    threads = {k: threading.Thread(target=reader, args=(k,), daemon=True) for k in "abc"}
    threads["w"] = threading.Thread(target=writer, daemon=True)
    threads["a"].start()
    threads["b"].start()
    assert ev["a_in"].wait(JOIN_S) and ev["b_in"].wait(JOIN_S)      # two readers hold the lock together (neither has released)
    threads["w"].start()
    deadline = time.monotonic() + JOIN_S
    while lock._writers_waiting != 1:                                 # (the lock's own state, not the clock, says the writer is waiting)
        assert time.monotonic() < deadline
        time.sleep(0.001)
    threads["c"].start()                                              # a reader inside, a writer waiting: a NEW reader stays out
    assert ev["c_started"].wait(JOIN_S) and not ev["c_in"].wait(REFUSED_S)
    ev["a_go"].set()
    threads["a"].join(JOIN_S)
    assert not threads["a"].is_alive() and not ev["w_in"].wait(REFUSED_S)   # one reader is still inside: the writer waits
    ev["b_go"].set()
    assert ev["w_in"].wait(JOIN_S) and not ev["c_in"].is_set()        # the writer before the reader that came after it
    ev["w_go"].set()
    assert ev["c_in"].wait(JOIN_S)                                    # after release_write readers proceed
    ev["c_go"].set()
    for t in threads.values():
        t.join(JOIN_S)
        assert not t.is_alive()
    assert (lock._readers, lock._writer, lock._writers_waiting) == (0, False, 0)


# (handle present, device moved, weights dirty, half grid wanted, handle has the half grid) -> (destroy, create, upload), written out from
# NerfactoModel._ensure_engine as it stood before the engine module: "start over" = a handle whose device moved, or precision="fp16" wanted on
# a handle created without the grid's fp16 storage; create = no handle (left); upload = dirty, and starting over marks dirty.  Without a
# handle the model was always dirty (both are set together), so those rows upload whatever the flag says: a new handle is empty.
LIFECYCLE = """
00000 011   00001 011   00010 011   00011 011   00100 011   00101 011   00110 011   00111 011
01000 011   01001 011   01010 011   01011 011   01100 011   01101 011   01110 011   01111 011
10000 000   10001 000   10010 111   10011 000   10100 001   10101 001   10110 111   10111 001
11000 111   11001 111   11010 111   11011 111   11100 111   11101 111   11110 111   11111 111
"""


def test_lifecycle_over_all_32_inputs():
    rows = LIFECYCLE.split()
    table = {tuple(c == "1" for c in k): tuple(c == "1" for c in v) for k, v in zip(rows[0::2], rows[1::2])}
    assert len(table) == 32
    for facts, want in table.items():
        assert engine.lifecycle(*facts) == want, facts
    assert engine.lifecycle(False, False, True, False, False) == (False, True, True)       # no handle
    assert engine.lifecycle(True, False, False, False, False) == (False, False, False)     # handle, same device, clean, half not wanted
    assert engine.lifecycle(True, True, False, False, False) == (True, True, True)         # handle, device moved
    assert engine.lifecycle(True, False, False, True, False) == (True, True, True)         # half wanted and missing


def test_cpu_model_shows_its_engine_only_through_the_delegators():
    model = small_config().setup()
    with pytest.raises(_lib.SignerfHipError, match="renders on the GPU only"):
        model._ensure_engine()
    for dirties in (model.mark_weights_dirty, lambda: model.load_state_dict(model.state_dict()), lambda: model.to(torch.float32)):
        model._weights_dirty = False
        assert not model._engine.dirty
        dirties()
        assert model._weights_dirty is True and model._engine.dirty is True
    assert isinstance(model._engine, engine.Engine) and not isinstance(model._engine, torch.nn.Module)
    assert not any("engine" in k for k in model.state_dict()) and not any("engine" in n for n, _ in model.named_modules())
    assert model.effective_precision == model.config.precision      # (no handle yet: the request)
    model._engine.close()                                           # nothing to destroy: no library call
    assert not model._engine.handle


def test_model_is_released_by_its_refcount_alone():
    """No model -> engine -> model cycle: with the collector off, dropping the only reference frees the model (and with it the handle)."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        model = small_config().setup()
        ref = weakref.ref(model)
        del model
        assert ref() is None
    finally:
        if was_enabled:
            gc.enable()


def test_ops_reaches_the_handle_through_the_engine_only():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "signerf_amd", "ops.py")).read()
    assert not any(name in text for name in ("._handle", "._engine_rw", "._march_stats", "._opts", "._render_ex"))
