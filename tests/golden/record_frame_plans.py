"""Records tests/golden/frame_plans.json:  python tests/golden/record_frame_plans.py <libsignerf_hip.so of the reference commit>

Where the three fused kernels write in the caller's workspace, how large sn_workspace_bytes says it must be, the grids they are launched
with and the split-depth tail of the main kernel are host arithmetic over the frame size, the options and the device's CU count.  The
reference library -- the commit named in PARENT below, built as a variant (signerf_amd.build.build(out_path=...)), unchanged -- is run
here with its HIP runtime calls served by hip_host_stub.c, as record_launch_variants.py runs it: device memory is one host arena, kernels
do nothing and are logged with grid, block, LDS bytes and parameter block, pointers into the arena as offsets.  The stub reports the CU
count of the environment variable HIP_STUB_CUS; one handle is created per CU count.  Every case of CASES goes through that library's own
sn_workspace_bytes, sn_render_rays without and with expected_depth, and sn_render_normals, on a workspace of exactly the size
sn_workspace_bytes returned.  Kept per case: that size and, for every launch in order, the kernel, grid, block, LDS bytes and -- read
from the parameter block at the offsets of the ctypes mirrors below, which are checked against the code object's argument sizes and the
frame size -- the workspace offsets (ebins_out, scratch, tile_counter; ebins, exp_raw, chunk_minmax, seg_scratch; null = None),
seg_first_block, n_seg, seg_len, n_chunks and the tile fields.  torch is not imported: it would bring the real runtime into the process.

    --out FILE   write there instead (tests/test_frame_plan_host.py runs this file on the tree's own library and compares)"""
import ctypes as C, json, os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT = "2a98fe414b45e5b599be2cf97c681a553aa41922"
PROP_SAMPLES = (64, 32)


def case(name, height, width, S=48, cus=256, chunk_rays=1000, nprop=(0, 1, 2), prec=1):
    return [dict(name=f"{name} nprop={k}", height=height, width=width, S=S, cus=cus, chunk_rays=chunk_rays, nprop=k, prec=prec) for k in nprop]


# every return of plan_tail an input reaches (the workgroup counts are of 2x2 tiles of 8x8 pixels; slots = 3 x CUs), frames below one
# workgroup, the 64x1 tiles of frames under 8 rows, 0 / 1 / 2 proposal iterations, chunk sizes that do and do not divide the frame
CASES = sum([
    case("S below 8", 64, 64, S=7),
    case("empty tail: 768 workgroups", 384, 512, chunk_rays=1 << 15),
    case("tail above slots / 8: 169 workgroups", 200, 200),
    case("tail above slots / 8: 2500 workgroups, tail 196", 800, 800),
    *[case(f"split S={S}", 64, 64, S=S, nprop=(0, 2)) for S in (8, 16, 48, 64, 256)],
    case("split behind full rounds: 1600 workgroups", 640, 640),
    case("split behind full rounds at 64 CUs", 800, 800, cus=64, nprop=(0, 2)),
    case("first_block 750 is no multiple of 8", 385, 512, cus=250, nprop=(0, 2)),
    case("not worth a second kernel: 72 workgroups of 9 samples", 128, 144, S=9, nprop=(0, 2)),
    case("one pixel", 1, 1, chunk_rays=1),
    case("below one workgroup", 10, 12, chunk_rays=7),
    case("64x1 tiles, two wide, ragged", 7, 65),
    case("64x1 tiles, ragged", 7, 70, S=40, nprop=(0, 2)),
    case("20 workgroups, ragged: split", 60, 72, chunk_rays=1 << 15),
    case("20 workgroups, exact fp32", 60, 72, nprop=(0, 2), prec=0),
    case("one CU: 8 workgroups, 3 slots", 32, 64, cus=1, nprop=(0, 2)),
], [])

u32, i32, f32, ptr = C.c_uint32, C.c_int32, C.c_float, C.c_uint64


class Dense(C.Structure):      # sn_device.h SnDenseCopy
    _fields_ = [("base", ptr), ("bytes", u32), ("off", u32 * 12), ("res", u32 * 12), ("n_bc", u32)]


RAYS = [("origins", ptr), ("directions", ptr), ("nears", ptr), ("fars", ptr)]
TILES = [("tile_w_log2", i32), ("tile_h_log2", i32), ("tiles_x", i32), ("tiles_y", i32)]


class MainParams(C.Structure):      # sn_main.h SnMainParams
    _fields_ = RAYS + [("sbins", ptr), ("ebins", ptr), ("table", ptr), ("wimg", ptr), ("rgb", ptr), ("depth", ptr), ("acc", ptr), ("exp_raw", ptr),
                       ("chunk_minmax", ptr), ("n_chunks", i32), ("scal", f32 * 16), ("height", i32), ("width", i32), ("n_samples", i32)] + TILES + [
        ("log2_t", i32), ("near_plane", f32), ("far_plane", f32), ("avg_density", f32), ("sh_remap", i32), ("chunk_rays", i32), ("feat_scale", f32),
        ("hquads", Dense), ("hrows", ptr), ("hrows_bytes", u32), ("hpinfo", u32 * 16), ("pairs", ptr), ("pairs_bytes", u32), ("pinfo", u32 * 16),
        ("grid", u32 * 4), ("dense", Dense), ("seg_first_block", i32), ("n_seg", i32), ("seg_len", i32), ("seg_scratch", ptr), ("early_term", i32),
        ("march_stats", ptr), ("bg_mode", i32), ("bg", f32 * 3), ("spacing_uniform", i32), ("pm", f32 * 7), ("dump_fetch", ptr), ("dump_q", ptr),
        ("dump_median", ptr)]


class PropParams(C.Structure):      # sn_proposal.h SnPropParams
    _fields_ = RAYS + [("sbins0", ptr), ("pdf_u", ptr * 2), ("ebins_out", ptr), ("prop_depth", ptr * 2), ("feat_scale", f32 * 2), ("dump_fetch", ptr * 2),
                       ("dump_q", ptr * 2), ("dump_pdf", ptr * 2), ("scratch", ptr), ("tile_counter", ptr), ("tables", ptr * 2), ("table_bytes", u32 * 2),
                       ("grid", u32 * 4 * 2), ("dense", Dense * 2), ("pairs", ptr * 2), ("pinfo", u32 * 16 * 2), ("pairs_bytes", u32 * 2), ("wpack", ptr * 2),
                       ("scal", f32 * 5 * 2), ("log2_t", i32 * 2), ("n_samples", i32 * 2), ("n_levels", i32), ("n_final", i32), ("height", i32),
                       ("width", i32)] + TILES + [("near_plane", f32), ("far_plane", f32), ("avg_density", f32), ("hist_pad", f32), ("pdf_ieee", i32),
                                                  ("early_term", i32), ("march_stats", ptr), ("cache_off", i32), ("spacing_uniform", i32), ("pm", f32 * 7)]


class NormalsParams(C.Structure):      # sn_normals.h SnNormalsParams
    _fields_ = RAYS + [("sbins", ptr), ("ebins", ptr), ("table", ptr), ("wimg", ptr), ("normals", ptr), ("pred_normals", ptr), ("scal", f32 * 16),
                       ("height", i32), ("width", i32), ("n_samples", i32)] + TILES + [
        ("log2_t", i32), ("near_plane", f32), ("far_plane", f32), ("avg_density", f32), ("grid", u32 * 4), ("dense", Dense), ("inv_feat_scale", f32),
        ("feat_scale", f32), ("grad_scale", f32), ("pe_rev_scale", f32), ("spacing_uniform", i32), ("pm", f32 * 7)]


# parameter block and what is kept of it: (workspace pointers, integers), by the kernel's name
MIRRORS = {"sn_render_main_kernel": (MainParams, ("ebins", "exp_raw", "chunk_minmax", "seg_scratch"), ("n_chunks", "seg_first_block", "n_seg", "seg_len")),
           "sn_main_combine_kernel": (MainParams, ("ebins", "exp_raw", "chunk_minmax", "seg_scratch"), ("n_chunks", "seg_first_block", "n_seg", "seg_len")),
           "sn_proposal_kernel": (PropParams, ("ebins_out", "scratch", "tile_counter"), ()),
           "sn_normals_kernel": (NormalsParams, ("ebins",), ())}


if __name__ == "__main__":
    lib_path = os.path.abspath(sys.argv[1])
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "frame_plans.json")
    import stub_host
    host = stub_host.boot(lib_path)
    _lib, wc, stub, lib, ARGS, dev = host._lib, host.wc, host.stub, host.lib, host.args, host.dev
    for name, sizes in ARGS.items():      # the mirrors have the size the kernels take
        for base, (mirror, _, _) in MIRRORS.items():
            if base in name:
                assert sizes == [C.sizeof(mirror)], (name, sizes, C.sizeof(mirror))

    ARENA = dev(256)      # the arena's first block: no buffer of the caller has offset 0, which a logged parameter block shows as null
    N_MAX = max(c["height"] * c["width"] for c in CASES)
    BUF = {k: dev(N_MAX * 12) for k in ("origins", "directions", "rgb", "normals")}
    BUF.update({k: dev(N_MAX * 4) for k in ("depth", "acc", "expected_depth")})

    wcase = wc.cases()["ordinary"]
    handles = {}


    def handle(cus):
        """One finalized handle per CU count: sn_create reads the count from the device."""
        if cus not in handles:
            os.environ["HIP_STUB_CUS"] = str(cus)
            stub.stub_set_absmax((C.c_uint32 * 3)(*[int(np.float32(a).view(np.uint32)) for a in wcase.absmax]))
            d = wc.field_desc(wcase)
            h = C.c_void_p(None)
            assert lib.sn_create(C.byref(d), C.byref(h)) == 0, lib.sn_last_error(None)
            named = [(n, wcase.tensors[n]) for n, _ in wc.tensor_names(wcase.app_dim, wcase.pred_normals, wcase.n_prop)]
            named.append(("field.mlp_base.encoder.hash_table", wcase.table(-1)))
            named += [(f"proposal_networks.{i}.mlp_base.encoder.hash_table", wcase.table(i)) for i in range(wcase.n_prop)]
            for n, a in named:
                a = np.ascontiguousarray(a, dtype=np.float32)
                assert lib.sn_upload_weights(h, n.encode(), a.ctypes.data, a.size * 4, None) == 0, (n, lib.sn_last_error(h))
            assert lib.sn_finalize_weights(h, None) == 0, lib.sn_last_error(h)
            del os.environ["HIP_STUB_CUS"]
            handles[cus] = h
        return handles[cus]


    KERNELS = sorted(ARGS)


    def logged(c, ws):
        """The launches since stub_clear: kernel, grid, block, LDS bytes and the kept fields of the parameter block."""
        out = []
        for i in range(stub.stub_launches()):
            geom = (C.c_uint64 * 7)()
            stub.stub_launch_geometry(i, geom)
            name = stub.stub_launch_name(i).decode()
            g = list(geom)
            rec = {"kernel": KERNELS.index(name), "grid": g[0:3], "block": g[3:6], "lds": g[6]}
            for base, (mirror, pointers, integers) in MIRRORS.items():
                if base not in name:
                    continue
                n = stub.stub_launch_args(i, None, 0)
                assert n == C.sizeof(mirror), (name, n)
                p = mirror()
                stub.stub_launch_args(i, C.byref(p), n)
                assert (p.height, p.width) == (c["height"], c["width"]) and p.origins == BUF["origins"] - ARENA, name      # the mirror reads the right words
                for f in pointers:
                    v = getattr(p, f)
                    rec[f] = None if v == 0 else v - (ws - ARENA)
                for f in integers + tuple(n for n, _ in TILES):
                    rec[f] = getattr(p, f)
            out.append(rec)
        return out


    cases = []
    for c in CASES:
        h = handle(c["cus"])
        o = _lib.SnRenderOpts()
        o.num_proposal_iterations, o.num_nerf_samples, o.near_plane, o.far_plane, o.chunk_rays = c["nprop"], c["S"], 0.05, 1000.0, c["chunk_rays"]
        o.num_proposal_samples[0], o.num_proposal_samples[1] = PROP_SAMPLES
        o.precision = c["prec"]
        need = lib.sn_workspace_bytes(h, c["height"], c["width"], C.byref(o))
        assert need > 0, (c, lib.sn_last_error(h))
        ws = dev(need)
        o.workspace, o.workspace_bytes = ws, need
        rays = (BUF["origins"], BUF["directions"], None, None, c["height"], c["width"], C.byref(o))
        calls = {}
        for call, expd in (("rays", None), ("rays_expected_depth", BUF["expected_depth"])):
            stub.stub_clear()
            assert lib.sn_render_rays(h, *rays, BUF["rgb"], BUF["depth"], BUF["acc"], expd, None, None, None) == 0, (c, lib.sn_last_error(h))
            calls[call] = logged(c, ws)
        stub.stub_clear()
        assert lib.sn_render_normals(h, *rays, BUF["normals"], None, None) == 0, (c, lib.sn_last_error(h))
        calls["normals"] = logged(c, ws)
        o.workspace_bytes = need - 1      # the size is exact: one byte less is refused, with the size in the text
        assert lib.sn_render_rays(h, *rays, BUF["rgb"], BUF["depth"], BUF["acc"], None, None, None, None) == _lib.SN_ERR_WORKSPACE
        assert str(need) in lib.sn_last_error(h).decode()
        assert stub.hipFree(C.c_void_p(ws)) == 0
        cases.append(dict(c, workspace_bytes=need, effective_precision=[lib.sn_effective_precision(h, c["prec"], k) for k in (0, 1)], calls=calls))
        print(c["name"], need, flush=True)
    for h in handles.values():
        lib.sn_destroy(h)
    used = sorted({l["kernel"] for c in cases for ls in c["calls"].values() for l in ls})
    for c in cases:
        for ls in c["calls"].values():
            for l in ls:
                l["kernel"] = used.index(l["kernel"])
    with open(out_path, "w") as f:      # one line per kernel and case
        f.write('{\n "provenance": ' + json.dumps({"parent_commit": PARENT, "procedure": __doc__}) + ',\n "kernels": [\n'
                + ",\n".join("  " + json.dumps(KERNELS[k]) for k in used) + '\n ],\n "cases": [\n' + ",\n".join("  " + json.dumps(c) for c in cases) + "\n ]\n}\n")
