"""BASELINE.json configs[2] with REAL renders crossing a process boundary (VERDICT r01 "What's missing" #2): two processes, each
with its own HIP context, library handle and weight upload, render the cameras they own through the reference's two calls and
exchange the finished tiles -- `sheet.render_reference_sheet` on the 8 `circle_poses` cameras (camera i -> rank i % 2) and
`sheet.render_camera_row_sharded` on one camera.  The GPU box has one GPU, so both ranks sit on cuda:0 and the process group is
gloo (tiles staged through the host; RCCL refuses two ranks on one device) -- the sharding, ownership, gather and re-ordering code is
the code that runs over RCCL.  Every rank must end up with the sheet a single process renders, bit for bit.
Also a world-2 dry run of bench.py's N > 1 branch (same arrangement), so that code has executed."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, size):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from helpers import make_model
    from signerf_amd import Cameras, scene, sheet

    cfg = scene.benchmark_config(64)            # configs[1]'s field: L=16, T=2^19, 64 samples, no proposal nets
    model, _ = make_model(cfg, dev)
    model.eval()
    W = H = size
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], float(W), float(W), W / 2, H / 2, W, H).to(dev)
    rendered = []
    orig = model.get_outputs_for_camera_ray_bundle

    def counting(bundle):
        rendered.append(tuple(bundle.origins.shape[:2]))
        return orig(bundle)

    model.get_outputs_for_camera_ray_bundle = counting
    tiles = sheet.render_reference_sheet(model, cams)                 # [8, H, W, 4], every rank
    n_sheet = len(rendered)
    rows = sheet.render_camera_row_sharded(model, cams[2])            # [H, W, 4], every rank
    row_shapes = rendered[n_sheet:]
    model.get_outputs_for_camera_ray_bundle = orig
    # what ONE process renders, in this process
    local = []
    for i in range(8):
        out = model.get_outputs_for_camera_ray_bundle(cams[i].generate_rays(camera_indices=0, aabb_box=model.render_aabb))
        local.append(torch.cat([out["rgb"], out["depth"]], dim=-1))
    local = torch.stack(local)
    torch.cuda.synchronize()
    torch.save({"tiles": tiles.cpu(), "rows": rows.cpu(), "local": local.cpu(), "n_sheet_renders": n_sheet, "row_shapes": row_shapes},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_reference_sheet_rendered_by_two_processes(gpu, tmp_path):
    world, size = 2, 160
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), size), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(world)]
    single = got[0]["local"]
    assert single.shape == (8, size, size, 4) and float(single[..., :3].std()) > 0.05          # a non-trivial sheet
    for r in range(world):
        assert got[r]["n_sheet_renders"] == 4                                                 # camera i -> rank i % 2: four each
        assert torch.equal(got[r]["local"], single)                                           # the two processes render identically
        assert torch.equal(got[r]["tiles"], single), f"rank {r}: gathered sheet differs from the single-process sheet"
        assert torch.equal(got[r]["rows"], single[2]), f"rank {r}: row-sharded camera differs from the single-process render"
        assert got[r]["row_shapes"] == [(size // 2, size)]                                    # half the rows each (8-row bands)


def test_bench_n2_branch_dry_run(gpu, tmp_path):
    """bench.py --gpus 2 under torch.distributed.run with both ranks on the one GPU (gloo): the N > 1 code path -- process-group
    set-up, camera-per-rank, the depth-1 gather pipeline, drain, barrier, max-over-ranks timing, the JSON line -- runs once."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
           "--backend", "gloo", "--width", "200", "--height", "200", "--no-cpu-baseline", "--no-alt-precision"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                                                  # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak" and d["config"]["ranks_share_a_gpu"] is True
    assert d["config"]["backend"] == "gloo" and "camera-sharded x2" in d["config"]["parallelism"]
    assert d["value"] > 0 and abs(d["value"] - 2 * 200 * 200 * 64 * 4 / d["timed_region_s"]) / d["value"] < 1e-6   # whole-job aggregate
    assert "cpu_baseline" not in d                                                            # N = 1 only


@pytest.mark.parametrize("gather", ["all", "root"])
def test_bench_strong_scaling_dry_run(gpu, gather):
    """bench.py --scaling strong at world 2 (gloo, both ranks on the one GPU): a step is the whole 8-camera sheet
    (datasetgenerator.py:517-519), four cameras per rank, ONE tile gather per sheet (all-gather, or gather to rank 0)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--backend", "gloo", "--width", "160", "--height", "160", "--no-cpu-baseline", "--no-alt-precision", "--scaling", "strong",
           "--gather", gather]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["cameras_per_step"] == 8 and d["config"]["gather"] == gather
    assert d["config"]["dist_world_size"] == 2 and d["config"]["dist_backend"] == "gloo" and d["config"]["cuda_device_count"] >= 1
    assert abs(d["ms_per_sheet"] - d["ms_per_step"]) < 1e-9 and d["gather_ms"]["exposed"] > 0
    # every exchange strategy ran on the N > 1 path (ring all-gather vs direct pushes): the first RCCL run yields a comparison, not one point
    assert set(d["gather_ms"]["exposed_by_strategy"]) == {"all_gather", "p2p", "all_to_all"}
    assert all(v is not None and v > 0 for v in d["gather_ms"]["exposed_by_strategy"].values())
    assert abs(d["value"] - 8 * 160 * 160 * 64 * 3 / d["timed_region_s"]) / d["value"] < 1e-6      # total work fixed: 8 cameras per step


def test_bench_strong_scaling_single_gpu(gpu):
    """The N = 1 point of the strong-scaling curve: all eight cameras on one GPU, no exchange."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--width", "160", "--height", "160",
           "--no-cpu-baseline", "--no-alt-precision", "--no-others", "--no-traffic", "--scaling", "strong"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["gather_ms"] is None and d["config"]["dist_world_size"] == 1
    assert abs(d["value"] - 8 * 160 * 160 * 64 * 3 / d["timed_region_s"]) / d["value"] < 1e-6
    # `frac` is priced at the part's 2.4 GHz peak clock (r04), the sustained-clock figure sits beside it; no PMC child pass was asked for
    assert d["roofline"]["frac"] <= d["roofline"]["frac_at_sustained_clock"] * 1.02 and d["roofline"]["frac"] <= 1.0
    # r06: the leading keys of `roofline` are flat scalars in the order the driver's record keeps (bench.ROOFLINE_LEADING_KEYS)
    import bench
    assert tuple(d["roofline"])[:len(bench.ROOFLINE_LEADING_KEYS)] == bench.ROOFLINE_LEADING_KEYS
    assert all(d["roofline"][k] is None or isinstance(d["roofline"][k], (int, float, str)) for k in bench.ROOFLINE_LEADING_KEYS)
    assert d["roofline"]["one_launch_ms"] == d["roofline"]["kernel_ms"] and 2.0 < d["roofline"]["issue_cycles_per_wave_instruction"] < 4.0
    # r06: the issue roof is priced per opcode class (2 / 4 / 8 cycles); with it the L1 gather path is the largest busy fraction
    assert d["roofline"]["bound"] in ("l1-gather-issue", "simd-issue") and d["roofline"]["frac"] == max(d["roofline"]["simd_issue_frac"], d["roofline"]["l1_gather_issue_frac"], d["roofline"]["matrix_pipe_frac"])
    assert d["roofline"]["traffic"] is None and "not measured" in d["roofline"]["traffic_source"]


def _bench_line(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_prints_the_headline_and_dumps_the_last_step(gpu, tmp_path):
    """A plain bench.py run (no --full) times its steps and prints the headline only; --dump-outputs writes what the LAST timed step
    returned.  Every step of a run repeats the same renders, so "last" is checked twice: the line names the timed step the arrays came from
    (= --steps), and in a whole-sheet step (--scaling strong) the render outputs are those of the step's last camera (7) while `tiles` holds
    all eight.  Bit for bit the renders of the same cameras in this process (fixed inputs: weights seed 0, benchmark cameras)."""
    import numpy as np

    from signerf_amd import Cameras, scene

    size = ["--width", "96", "--height", "96"]
    d = _bench_line("--gpus", "1", "--steps", "5", "--warmup", "2", *size, "--dump-outputs", str(tmp_path / "weak"))
    assert d["full"] is False and d["steps"] == 5 and d["unit"] == "ray-samples/s" and d["higher_is_better"] is True and d["dtype"]
    assert abs(d["ms_per_step"] * 5 - d["timed_region_s"] * 1e3) < 1e-6 and abs(d["value"] - 96 * 96 * 64 * 5 / d["timed_region_s"]) / d["value"] < 1e-6
    assert not {"kernel_ms", "roofline", "roofline_hbm", "roofline_mfma", "alt_precision", "others", "cpu_baseline", "traffic_in_run"} & set(d)
    assert d["dumped_outputs"]["timed_step"] == 5
    s = _bench_line("--gpus", "1", "--steps", "3", "--warmup", "1", *size, "--scaling", "strong", "--dump-outputs", str(tmp_path / "strong"))
    assert s["dumped_outputs"]["timed_step"] == 3 and not any(a["sampled"] for a in s["dumped_outputs"]["arrays"].values())

    cfg = scene.benchmark_config(64)
    cfg.precision = "fp16x2"
    model = cfg.setup()
    model.load_state_dict(scene.synthetic_state_dict(cfg, seed=0), strict=False)
    model = model.to(gpu).eval()
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], 96.0, 96.0, 48.0, 48.0, 96, 96).to(gpu)
    want = [{k: v.cpu().numpy() for k, v in dict.items(model.get_outputs_for_camera_ray_bundle(cams[i].generate_rays(camera_indices=0, aabb_box=model.render_aabb)))}
            for i in range(8)]
    for run, line, cam in (("weak", d, 0), ("strong", s, 7)):
        names = sorted(want[cam]) + (["tiles"] if run == "strong" else [])
        assert sorted(p.name for p in (tmp_path / run).iterdir()) == sorted(k + ".npy" for k in names) == sorted(k + ".npy" for k in line["dumped_outputs"]["arrays"])
        for k, v in want[cam].items():
            got = np.load(tmp_path / run / f"{k}.npy")
            assert got.dtype == np.float32 and np.array_equal(got, v, equal_nan=True), (run, k)
    tiles = np.load(tmp_path / "strong" / "tiles.npy")
    assert tiles.dtype == np.float32 and tiles.shape == (8, 96, 96, 4)
    assert not np.array_equal(want[0]["rgb"], want[7]["rgb"])                     # the cameras differ: the check above tells them apart
    for i in range(8):
        assert np.array_equal(tiles[i], np.concatenate([want[i]["rgb"], want[i]["depth"]], axis=-1), equal_nan=True), i
