"""Records tests/golden/launch_variants.json:  python tests/golden/record_launch_variants.py <libsignerf_hip.so of the reference commit>

Which instantiation of sn_render_main_kernel, sn_proposal_kernel and sn_normals_kernel a call launches, with which grid, block, LDS bytes
and parameter block, is host logic; the device only runs what it is handed.  So the reference library -- the commit named in PARENT below,
built as a variant (signerf_amd.build.build(out_path=...)), unchanged -- is run here with its HIP runtime calls served by hip_host_stub.c:
device memory is one host arena, kernels do nothing and are logged.  A matrix of handles (HANDLES) and calls (calls_of) goes through that
library's own sn_create, sn_upload_weights, sn_finalize_weights, sn_render_rays, sn_render_rays_debug, sn_render_normals and
sn_effective_precision.  Kept for every call, in the order of calls_of: its outcome "<return code> <index into errors> <indices into kernels of the
ordered launches>", as an index into "outcomes".  Kept per handle, entry point, frame and precision: a digest over the accepted calls' launches,
each "<kernel> <grid> <block> <LDS bytes> <SHA-256 of its arguments>", the arguments with every pointer into the arena replaced by its offset (the
stub does that; every buffer of the caller -- rays, outputs, workspace -- comes from the arena too).  torch is not imported: it would bring the
real runtime into the process.

    --out FILE   write there instead (tests/test_launch_variants_host.py runs this file on the tree's own library and compares)"""
import ctypes as C, hashlib, itertools, json, math, os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT = "1cb37c69c0f7f29a5c4c5f51db0d6990b4f830de"
FUSED = ("sn_render_main_kernel", "sn_proposal_kernel", "sn_normals_kernel")
FRAMES = {"small": (10, 12),     # below the 2 x 2 tiles (16 x 16 pixels) of one workgroup
          "split": (60, 72)}     # 20 workgroups = the last (only) round of 768 slots at the stub's 256 CUs: cut into segment jobs
N_MAX, S, PROP_SAMPLES = 60 * 72, 48, (64, 32)
WS_BYTES = 64 << 20


def nerfacto_scalings(levels, base, max_res, tcnn):
    growth = math.exp((math.log(max_res) - math.log(base)) / (levels - 1))
    return [base * growth ** l - 1.0 if tcnn else float(math.floor(base * growth ** l)) for l in range(levels)]


NOT_A_PREFIX = [5.0, 0.5] + [5.0] * 14     # tiny-cuda-nn at T = 16: level 1 is indexed densely, level 0 is not


def H(case="ordinary", main=0, prop=0, dense=0, nerfacto_prop=True, half=0, nprop=2, box=0, main_scal=None, prop0_scal=None, env=None):
    return dict(case=case, main=main, prop=prop, dense=dense, nerfacto_prop=nerfacto_prop, half=half, nprop=nprop, box=box, main_scal=main_scal,
                prop0_scal=prop0_scal, env=env or {})


HANDLES = {
    "torch_11": H(), "torch_9": H(dense=9), "torch_0": H(dense=-1), "torch_11_other_prop_copies": H(nerfacto_prop=False),
    "torch_default_scalings": H(main_scal="cases", nerfacto_prop=False),
    "tcnn_11": H(main=1, prop=1), "tcnn_11_half": H(main=1, prop=1, half=1), "tcnn_9_half": H(main=1, prop=1, half=1, dense=9),
    "tcnn_0": H(main=1, prop=1, dense=-1, half=1), "tcnn_dense_levels_not_a_prefix": H(main=1, prop=1, main_scal=NOT_A_PREFIX, prop0_scal=NOT_A_PREFIX[:5], half=1),
    "tcnn_other_prop_copies": H(main=1, prop=1, nerfacto_prop=False),
    "torch_main_tcnn_prop": H(main=0, prop=1), "tcnn_main_torch_prop": H(main=1, prop=0),
    "torch_11_box": H(box=1), "tcnn_11_half_box": H(main=1, prop=1, half=1, box=1),
    "torch_11_one_net": H(nprop=1), "torch_11_no_net": H(nprop=0), "tcnn_11_one_net": H(main=1, prop=1, nprop=1, half=1),
    "torch_11_no_split": H(case="density_weight_leaves_fp16"), "tcnn_11_half_no_split": H(case="density_weight_leaves_fp16", main=1, prop=1, half=1),
    "torch_11_bare": H(case="bare", nprop=1), "torch_0_bare": H(case="bare", nprop=1, dense=-1),
    "torch_11_tail_split_off": H(env={"SN_TAIL_SPLIT": "0"}), "torch_11_early_term_off": H(env={"SN_EARLY_TERM": "0"}),
}
FAR = {"far": 1000.0, "far2e7": 2.0e7, "farnan": float("nan")}


def calls_of(hd, has_pred):
    """The calls one handle gets, in order: (key, dict).  entry r = sn_render_rays, d = sn_render_rays_debug, n = sn_render_normals."""
    out = []

    def add(entry, nprop, prec, frame="small", spacing=0, far="far", march=0, expd=0, reuse=0, ws="ws_a", pred=has_pred, **bad):
        key = f"{entry} {frame} nprop={nprop} prec={prec}" + " spacing=1" * spacing + f" {far}" * (far != "far") + " march" * march + " expd" * expd
        key += " reuse" * reuse + f" {ws}" * (ws != "ws_a") + f" pred={pred}" * (pred != has_pred) + "".join(f" {k}={v}" for k, v in bad.items())
        out.append((key, dict(entry=entry, nprop=nprop, prec=prec, frame=frame, spacing=spacing, far=far, march=march, expd=expd, reuse=reuse, ws=ws,
                              pred=pred, bad=bad)))

    nets = range(hd["nprop"] + 1)
    for entry, nprop, prec, (spacing, far), march in itertools.product("rdn", nets, (0, 1, 2), ((0, "far"), (1, "far"), (0, "far2e7"), (0, "farnan")), (0, 1)):
        add(entry, nprop, prec, spacing=spacing, far=far, march=march)
    for entry, nprop, prec in itertools.product("rn", (0, hd["nprop"]), (0, 1, 2)):
        add(entry, nprop, prec, frame="split")
    add("d", hd["nprop"], 1, frame="split")
    for nprop in (0, hd["nprop"]):
        add("r", nprop, 1, expd=1)
        add("r", nprop, 1, frame="split", expd=1)
    add("n", 0, 1, pred=1 - has_pred)      # (a handle without the predicted-normals head refuses to render them)
    if hd["nprop"]:     # SnRenderOpts.reuse_final_bins: after the render that wrote the bins, after another one, on a workspace nobody rendered into
        add("r", hd["nprop"], 1)
        add("n", hd["nprop"], 1, reuse=1)
        add("n", hd["nprop"], 0, reuse=1, spacing=1)
        add("n", hd["nprop"], 1, reuse=1, far="far2e7")
        add("n", hd["nprop"], 1, reuse=1, frame="split")
        add("n", hd["nprop"], 1, reuse=1, march=1)
        add("n", hd["nprop"], 1, reuse=1, ws="ws_b")
        add("n", hd["nprop"], 1, ws="ws_b")
        add("n", hd["nprop"], 1, reuse=1, ws="ws_b")
    if hd is HANDLES["torch_11"] or hd is HANDLES["tcnn_11_half"]:      # an invalid value for every field valid_opts checks
        for entry in "rdn":
            for bad in (dict(num_proposal_iterations=3), dict(num_proposal_iterations=-1), dict(num_nerf_samples=0), dict(num_nerf_samples=1025),
                        dict(chunk_rays=0), dict(precision=3), dict(precision=-1), dict(background_mode=2), dict(spacing_mode=2), dict(spacing_mode=-1),
                        dict(samples0=1), dict(samples1=257)):
                add(entry, 2, 1, **bad)
    return out


def make_handle(hd):
    case = wc.cases()[hd["case"]]
    assert case.n_prop >= hd["nprop"]
    stub.stub_set_absmax((C.c_uint32 * 3)(*[int(np.float32(a).view(np.uint32)) for a in case.absmax]))
    d = wc.field_desc(case)
    d.num_proposals, d.dense_levels, d.half_grid, d.disable_scene_contraction = hd["nprop"], hd["dense"], hd["half"], hd["box"]
    d.main_field.grid_mode = hd["main"]
    if hd["main_scal"] != "cases":
        for l, s in enumerate(hd["main_scal"] or nerfacto_scalings(16, 16, 2048, hd["main"])):
            d.main_field.scalings[l] = s
    for i in range(hd["nprop"]):
        d.proposals[i].grid_mode = hd["prop"]
        if hd["nerfacto_prop"]:
            for l, s in enumerate(nerfacto_scalings(5, 16, (128, 256)[i], hd["prop"])):
                d.proposals[i].scalings[l] = s
        if i == 0 and hd["prop0_scal"]:
            for l, s in enumerate(hd["prop0_scal"]):
                d.proposals[i].scalings[l] = s
    for k in range(3):
        d.aabb[k], d.aabb[3 + k] = -1.0 - k, 1.5 + k
    for k, v in hd["env"].items():
        os.environ[k] = v
    h = C.c_void_p(None)
    assert lib.sn_create(C.byref(d), C.byref(h)) == 0, lib.sn_last_error(None)
    named = [(n, case.tensors[n]) for n, _ in wc.tensor_names(case.app_dim, case.pred_normals, hd["nprop"])]
    named.append(("field.mlp_base.encoder.hash_table", case.table(-1)))
    named += [(f"proposal_networks.{i}.mlp_base.encoder.hash_table", case.table(i)) for i in range(hd["nprop"])]
    for n, a in named:
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert lib.sn_upload_weights(h, n.encode(), a.ctypes.data, a.size * 4, None) == 0, (n, lib.sn_last_error(h))
    assert lib.sn_finalize_weights(h, None) == 0, lib.sn_last_error(h)
    for k in hd["env"]:
        del os.environ[k]
    lay = [_lib.SnDebugLayout() for _ in range(1 + hd["nprop"])]
    for which, l in enumerate(lay):
        assert lib.sn_debug_layout(h, which - 1, C.byref(l)) == 0
    eff = [[lib.sn_effective_precision(h, req, k) for k in (0, 1, 2)] for req in (-1, 0, 1, 2, 3)]
    # what sn_variant.h selects on, as far as this ABI shows it (tests/test_variant_select_host.py feeds it to the selectors)
    facts = dict(main_grid_mode=hd["main"], prop_grid_mode=hd["prop"], log2_hashmap_size=wc.LOG2_T, main_scalings=[float(d.main_field.scalings[l]) for l in range(16)],
                 prop_scalings=[[float(d.proposals[i].scalings[l]) for l in range(5)] for i in range(hd["nprop"])],
                 nd_torch=lay[0].n_dense, nd_prop=[l.n_dense for l in lay[1:]], split_ok=eff[2][0], normals_split_ok=eff[2][1],
                 has_half_grid=int(lay[0].half_grid_bytes > 0), has_dense_main=int(lay[0].dense_bytes > 0), box=hd["box"], num_proposals=hd["nprop"],
                 has_pred_normals=int(case.pred_normals))
    return h, case, facts, eff


def run_call(h, c):
    Hh, Ww = FRAMES[c["frame"]]
    o = _lib.SnRenderOpts()
    o.num_proposal_iterations, o.num_nerf_samples, o.near_plane, o.far_plane, o.chunk_rays = c["nprop"], S, 0.05, FAR[c["far"]], 1 << 15
    o.num_proposal_samples[0], o.num_proposal_samples[1] = PROP_SAMPLES
    o.precision, o.spacing_mode, o.reuse_final_bins = c["prec"], c["spacing"], c["reuse"]
    o.march_stats = BUF["march_stats"] if c["march"] else None
    for k, v in c["bad"].items():
        if k.startswith("samples"):
            o.num_proposal_samples[int(k[-1])] = v
        else:
            setattr(o, k, v)
    o.workspace, o.workspace_bytes = BUF[c["ws"]], WS_BYTES
    stub.stub_clear()
    rays = (BUF["origins"], BUF["directions"], None, None, Hh, Ww, C.byref(o))
    if c["entry"] == "n":
        rc = lib.sn_render_normals(h, *rays, BUF["normals"], BUF["pred_normals"] if c["pred"] else None, None)
    else:
        outs = (BUF["rgb"], BUF["depth"], BUF["acc"], BUF["expected_depth"] if c["expd"] else None, BUF["prop_depth_0"], BUF["prop_depth_1"])
        rc = lib.sn_render_rays(h, *rays, *outs, None) if c["entry"] == "r" else lib.sn_render_rays_debug(h, *rays, *outs, C.byref(DUMP), None)
    launches = []
    for i in range(stub.stub_launches()):
        geom = (C.c_uint64 * 7)()
        stub.stub_launch_geometry(i, geom)
        n = stub.stub_launch_args(i, None, 0)
        buf = (C.c_ubyte * max(n, 1))()
        stub.stub_launch_args(i, buf, n)
        name = stub.stub_launch_name(i).decode()
        assert n > 0 and name in ARGS, name
        g = list(geom)
        launches.append(f"{KERNELS.index(name)} {g[0]},{g[1]},{g[2]} {g[3]},{g[4]},{g[5]} {g[6]} {hashlib.sha256(bytes(buf)[:n]).hexdigest()[:16]}")
    err = lib.sn_last_error(h).decode() if rc else ""
    if err not in ERRORS:
        ERRORS.append(err)
    return rc, ERRORS.index(err), launches


if __name__ == "__main__":
    lib_path = os.path.abspath(sys.argv[1])
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "launch_variants.json")
    import stub_host
    host = stub_host.boot(lib_path)
    _lib, wc, stub, lib, ARGS, dev = host._lib, host.wc, host.stub, host.lib, host.args, host.dev

    # every buffer of the caller, once, before the first handle: their arena offsets do not depend on the handles
    BUF = {k: dev(N_MAX * 12) for k in ("origins", "directions", "rgb", "normals", "pred_normals")}
    BUF.update({k: dev(N_MAX * 4) for k in ("depth", "acc", "expected_depth", "prop_depth_0", "prop_depth_1")})
    BUF.update({k: dev(WS_BYTES) for k in ("ws_a", "ws_b")})
    BUF["march_stats"] = dev(256)
    DUMP = _lib.SnDebugDump()
    DUMP.main_fetch, DUMP.main_q, DUMP.median_index = dev(256), dev(256), dev(256)
    for i in range(2):
        DUMP.prop_fetch[i], DUMP.prop_q[i], DUMP.pdf_index[i] = dev(256), dev(256), dev(256)


    KERNELS, ERRORS, OUTCOMES = sorted(ARGS), [""], []   # a launch names its kernel, a call its error text and its outcome, by index into these
    handles, reached = {}, set()
    for hname, hd in HANDLES.items():
        h, case, facts, eff = make_handle(hd)
        calls, digests = [], {}
        for key, c in calls_of(hd, int(case.pred_normals)):
            rc, err, launches = run_call(h, c)
            reached.update(KERNELS[int(l.split()[0])] for l in launches)
            outcome = " ".join([str(rc), str(err)] + [l.split()[0] for l in launches])     # "<return code> <error> <kernel> ..."
            if outcome not in OUTCOMES:
                OUTCOMES.append(outcome)
            calls.append(OUTCOMES.index(outcome))
            # geometry, LDS bytes and arguments of what the accepted calls launched: one digest per entry point, frame and precision
            group = f"{c['entry']} {c['frame']} prec={c['prec']}"
            digests.setdefault(group, hashlib.sha256()).update((key + "|" + ("|".join(launches) if rc == 0 else "") + "\n").encode())
        lib.sn_destroy(h)
        handles[hname] = {"facts": facts, "effective_precision": eff, "calls": " ".join(map(str, calls)),
                          "launch_digests": {g: d.hexdigest()[:16] for g, d in digests.items()}}
        print(hname, len(calls), "calls", flush=True)
    built = sorted(k for k in ARGS if any(f in k for f in FUSED))
    missing = [k for k in built if k not in reached]
    print(f"{len(built) - len(missing)} of the {len(built)} fused-kernel instantiations launched; never launched:")
    print("\n".join("  " + m for m in missing))
    used = sorted({int(k) for o in OUTCOMES for k in o.split()[2:]})       # only the kernels some call launched are listed
    OUTCOMES = [" ".join(o.split()[:2] + [str(used.index(int(k))) for k in o.split()[2:]]) for o in OUTCOMES]
    doc = {"provenance": {"parent_commit": PARENT, "procedure": __doc__}, "kernels": [KERNELS[k] for k in used], "errors": ERRORS, "outcomes": OUTCOMES,
           "handles": handles, "never_launched": missing}
    with open(out_path, "w") as f:      # one line per kernel, error, outcome and handle
        parts = []
        for k, v in sorted(doc.items()):
            if isinstance(v, list):
                body = "[\n" + ",\n".join("  " + json.dumps(x) for x in v) + "\n ]"
            elif k == "handles":
                body = "{\n" + ",\n".join(f"  {json.dumps(n)}: {json.dumps(hh, sort_keys=True)}" for n, hh in v.items()) + "\n }"
            else:
                body = json.dumps(v, sort_keys=True)
            parts.append(f" {json.dumps(k)}: {body}")
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
