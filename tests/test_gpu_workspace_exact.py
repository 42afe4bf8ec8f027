"""sn_workspace_bytes is exact on the GPU: a colour render with expected_depth and a normals render with reuse_final_bins, handed
exactly the bytes it promises in the middle of a buffer filled with 0xA5, leave the 4096 bytes in front of and behind the workspace
untouched and give every output bit for bit what the same calls give with a 64 MiB workspace.  Frames: 60x72 (20 workgroups of 2x2
tiles, 5x4 with ragged edges -- at 256 CUs the split-depth tail, whose segment scratch is the last region of the plan) and 7x70 (the
64x1 tiles of frames under 8 rows, ragged).  Models: the uniform sampler alone, and two proposal nets."""
import ctypes as C

import pytest
import torch

from helpers import make_model, small_config
from signerf_amd import Cameras, _lib, scene

pytestmark = pytest.mark.gpu

GUARD = 4096
MODELS = {"uniform": dict(num_proposal_iterations=0, num_nerf_samples_per_ray=40),
          "proposals": dict(num_proposal_samples_per_ray=(48, 24), num_nerf_samples_per_ray=16)}


def _render_both(model, lib, o, d, H, W, opts):
    """Colour with expected_depth, then normals and predicted normals from the bins that render left: {name: tensor}."""
    n = H * W
    out = {k: torch.full((n, c), -5.0, dtype=torch.float32, device=o.device)
           for k, c in (("rgb", 3), ("depth", 1), ("acc", 1), ("exp", 1), ("p0", 1), ("p1", 1), ("normals", 3), ("pred_normals", 3))}
    opts.reuse_final_bins = 0
    st = lib.sn_render_rays(model._handle, _lib.ptr(o), _lib.ptr(d), None, None, H, W, C.byref(opts), _lib.ptr(out["rgb"]), _lib.ptr(out["depth"]),
                            _lib.ptr(out["acc"]), _lib.ptr(out["exp"]), _lib.ptr(out["p0"]), _lib.ptr(out["p1"]), _lib.current_stream())
    assert st == 0, lib.sn_last_error(model._handle)
    opts.reuse_final_bins = 1
    st = lib.sn_render_normals(model._handle, _lib.ptr(o), _lib.ptr(d), None, None, H, W, C.byref(opts), _lib.ptr(out["normals"]),
                               _lib.ptr(out["pred_normals"]), _lib.current_stream())
    assert st == 0, lib.sn_last_error(model._handle)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("frame", [(60, 72), (7, 70)], ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("sampler", list(MODELS))
def test_renders_stay_inside_the_promised_workspace(gpu, sampler, frame):
    H, W = frame
    model, _ = make_model(small_config(predict_normals=True, **MODELS[sampler]), gpu)
    lib = model._ensure_engine()
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], float(W), float(W), W / 2, H / 2, W, H).to(gpu)
    b = cams[0].generate_rays(camera_indices=0)
    o, d = b.origins.reshape(-1, 3).contiguous(), b.directions.reshape(-1, 3).contiguous()
    opts, keep = model._opts(H, W, lib)
    need = lib.sn_workspace_bytes(model._handle, H, W, C.byref(opts))
    assert need > 0 and need % 256 == 0

    roomy = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)
    opts.workspace, opts.workspace_bytes = roomy.data_ptr(), roomy.numel()
    want = _render_both(model, lib, o, d, H, W, opts)

    guarded = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    assert (guarded.data_ptr() + GUARD) % 256 == 0
    opts.workspace, opts.workspace_bytes = guarded.data_ptr() + GUARD, need
    got = _render_both(model, lib, o, d, H, W, opts)

    for k in want:
        assert torch.equal(want[k].view(torch.int32), got[k].view(torch.int32)), k
    for k in ("rgb", "depth", "acc", "exp", "normals", "pred_normals"):      # (the renders wrote their outputs: none keeps its fill)
        assert float(want[k].min()) > -5.0, k
    assert bool((guarded[:GUARD] == 0xA5).all()), "bytes in front of the workspace were written"
    assert bool((guarded[GUARD + need:] == 0xA5).all()), "bytes behind the promised workspace size were written"
    assert not bool((guarded[GUARD:GUARD + need] == 0xA5).all())      # (and the workspace itself was used)
