"""Records tests/golden/weight_images.json:  python tests/golden/record_weight_images.py <libsignerf_hip.so of the reference commit>

The weight images are host arithmetic; the device only stores them.  So the reference library -- the commit named in PARENT below, built
as a variant (signerf_amd.build.build(out_path=...)) with one uncommitted change, sn_debug_read accepting what = 2 .. 6 -- is run here
with its HIP runtime calls served by hip_host_stub.c: device memory is host memory, kernels do nothing, and the table abs-max scan
returns the abs-max the case's tables have (tests/weights_cases.py builds them so, bit for bit).  Every case then goes through that
library's own sn_create, sn_upload_weights, sn_finalize_weights, sn_debug_read, sn_debug_layout and sn_effective_precision.  torch is
not imported: it would bring the real runtime into the process."""
import ctypes as C, hashlib, json, os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT = "ed0fdd52dd7be26183825987e8c228b0a2eb9134"
lib_path = sys.argv[1]
import stub_host
host = stub_host.boot(lib_path, kernel_args=False)
_lib, wc, stub, lib = host._lib, host.wc, host.stub, host.lib
out = {}
for name, case in wc.cases().items():
    bits = (C.c_uint32 * 3)(*[int(np.float32(a).view(np.uint32)) for a in case.absmax])
    stub.stub_set_absmax(bits)
    h = C.c_void_p(None)
    d = wc.field_desc(case)
    assert lib.sn_create(C.byref(d), C.byref(h)) == 0, lib.sn_last_error(None)
    named = [(n, case.tensors[n]) for n, _ in wc.tensor_names(case.app_dim, case.pred_normals, case.n_prop)]
    named.append(("field.mlp_base.encoder.hash_table", case.table(-1)))
    named += [(f"proposal_networks.{i}.mlp_base.encoder.hash_table", case.table(i)) for i in range(case.n_prop)]
    for n, a in named:
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert lib.sn_upload_weights(h, n.encode(), a.ctypes.data, a.size * 4, None) == 0, (n, lib.sn_last_error(h))
    assert lib.sn_finalize_weights(h, None) == 0, lib.sn_last_error(h)
    sha = {}
    for im in case.images():
        which = int(im[4:]) if im.startswith("prop") else -1
        buf = np.zeros(wc.IMAGE_BYTES[im], dtype=np.uint8)
        assert lib.sn_debug_read(h, which, wc.DEBUG_READ_WHAT[im], buf.ctypes.data, buf.size, None) == 0, (im, lib.sn_last_error(h))
        sha[im] = hashlib.sha256(buf.tobytes()).hexdigest()
    scales = []
    for which in range(-1, case.n_prop):
        lay = _lib.SnDebugLayout()
        assert lib.sn_debug_layout(h, which, C.byref(lay)) == 0
        scales.append(float(lay.feature_scale))
    out[name] = {"sha256": sha, "precision": [lib.sn_effective_precision(h, 1, 0), lib.sn_effective_precision(h, 1, 1)], "feature_scale": scales}
    lib.sn_destroy(h)
    print(name, out[name]["precision"], scales, flush=True)
doc = {"provenance": {"parent_commit": PARENT, "procedure": __doc__,
                      "not_recorded": "s1 .. s4 and grad_scale_normals were not readable through that commit's ABI; they are part of the image bytes"},
       "cases": out}
json.dump(doc, open(os.path.join(HERE, "weight_images.json"), "w"), indent=1, sort_keys=True)
