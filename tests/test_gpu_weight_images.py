"""The device holds what the CPU packed: for the cases of tests/weights_cases.py that the GPU half names, a handle is created through the C
ABI, the tensors uploaded and finalized, and the five weight buffers read back (sn_debug_read, what = 2 .. 6) -- byte for byte the files
tests/c/weights_pack.cpp writes for the same input, and the digests of tests/golden/weight_images.json; the effective precisions and the
feature scales are the recorded ones.  No rendering."""
import ctypes as C
import hashlib

import pytest
import torch

import weights_cases as wc
from signerf_amd import _lib
from test_weights_host import gold, packed  # noqa: F401  (the recorded digests; the CPU program's output for every case, built once)

pytestmark = pytest.mark.gpu
CASES = wc.cases()


def _create(case):
    h = C.c_void_p(None)
    d = wc.field_desc(case)
    _lib.check(_lib.load().sn_create(C.byref(d), C.byref(h)), None, "sn_create")
    return h


def _check(handle, case, packed, gold, gpu):  # noqa: F811
    images, scal = wc.read_back(_lib.load(), handle, case, gpu)
    gold = gold["cases"][case.name]
    assert set(images) == set(case.images())
    for im, blob in images.items():
        assert blob == packed[case.name][1][im], (case.name, im)
        assert hashlib.sha256(blob).hexdigest() == gold["sha256"][im], (case.name, im)
    assert scal["precision"] == gold["precision"] and scal["feature_scale"] == gold["feature_scale"], (case.name, scal)


@pytest.mark.parametrize("name", wc.GPU_CASES)
def test_device_images_are_the_cpu_programs(gpu, packed, gold, name):  # noqa: F811
    lib, case = _lib.load(), CASES[name]
    h = _create(case)
    try:
        wc.upload_and_finalize(lib, h, case, gpu)
        _check(h, case, packed, gold, gpu)
        # the selectors: an image of the main field ignores `which`, a proposal pack needs one; the size must be the buffer's
        buf = torch.zeros(wc.IMAGE_BYTES["prop0"], dtype=torch.uint8, device=gpu)
        assert lib.sn_debug_read(h, -1, 6, buf.data_ptr(), buf.numel(), _lib.current_stream()) == _lib.SN_ERR_INVALID
        assert lib.sn_debug_read(h, 0, 2, buf.data_ptr(), buf.numel(), _lib.current_stream()) == _lib.SN_ERR_INVALID
        assert lib.sn_debug_read(h, -1, 7, buf.data_ptr(), buf.numel(), _lib.current_stream()) == _lib.SN_ERR_INVALID
    finally:
        lib.sn_destroy(h)


def test_second_finalize_overwrites_the_buffers_of_the_first(gpu, packed, gold):  # noqa: F811
    """The upload helper's reuse path: other tensors into the handle that held the first case, finalized again.  (The descriptor fixes the
    tensor shapes, so the second set has the first one's shapes and other values.)"""
    lib, first, second = _lib.load(), CASES[wc.REUSE[0]], CASES[wc.REUSE[1]]
    h = _create(first)
    try:
        wc.upload_and_finalize(lib, h, first, gpu)
        _check(h, first, packed, gold, gpu)
        wc.upload_and_finalize(lib, h, second, gpu)
        _check(h, second, packed, gold, gpu)
    finally:
        lib.sn_destroy(h)
