"""Inputs of the weight-image tests (tests/test_weights_host.py, tests/test_gpu_weight_images.py): seeded parameter tensors for the
smallest cases that reach every branch of the host packers (signerf_amd/csrc/sn_weights.h), the raw input file of
tests/c/weights_pack.cpp, and hash tables that really have the abs-max a case names.

Input file of the program, float32 little-endian: a header of 8 values
    appearance_embed_dim, has_pred_normals, num_proposals, geo_feat_dim, sh_levels, abs-max of the main table, of proposal table 0, of table 1
then the tensors in the order of `tensor_names` below (row-major, as the state dict holds them)."""
import numpy as np

GEO, SH_LEVELS, SH = 15, 4, 16
LOG2_T = 4                     # the smallest table sn_create accepts: 16 rows per level
MAIN_LEVELS, PROP_LEVELS = 16, 5
IMAGES = ("main", "main_h", "normals", "normals_h", "prop0", "prop1")   # <image>.bin, as weights_pack writes them
DEBUG_READ_WHAT = {"main": 2, "main_h": 3, "normals": 4, "normals_h": 5, "prop0": 6, "prop1": 6}   # sn_debug_read `what`
GPU_CASES = ("ordinary", "bare", "density_weight_leaves_fp16", "proposal_leaves_fp16")
REUSE = ("ordinary", "ordinary_again")     # the second is uploaded into the handle that held the first


def tensor_names(app_dim, pred_normals, n_prop):
    """[(state-dict name, shape)] in file order."""
    cin = SH + GEO + app_dim
    out = [("field.mlp_base.mlp.layers.0.weight", (64, 32)), ("field.mlp_base.mlp.layers.0.bias", (64,)),
           ("field.mlp_base.mlp.layers.1.weight", (16, 64)), ("field.mlp_base.mlp.layers.1.bias", (16,)),
           ("field.mlp_head.layers.0.weight", (64, cin)), ("field.mlp_head.layers.0.bias", (64,)),
           ("field.mlp_head.layers.1.weight", (64, 64)), ("field.mlp_head.layers.1.bias", (64,)),
           ("field.mlp_head.layers.2.weight", (3, 64)), ("field.mlp_head.layers.2.bias", (3,))]
    if app_dim:
        out.append(("field.embedding_appearance.mean", (app_dim,)))
    if pred_normals:
        out += [("field.mlp_pred_normals.layers.0.weight", (64, 12 + GEO)), ("field.mlp_pred_normals.layers.0.bias", (64,)),
                ("field.mlp_pred_normals.layers.1.weight", (64, 64)), ("field.mlp_pred_normals.layers.1.bias", (64,)),
                ("field.mlp_pred_normals.layers.2.weight", (64, 64)), ("field.mlp_pred_normals.layers.2.bias", (64,)),
                ("field.field_head_pred_normals.net.weight", (3, 64)), ("field.field_head_pred_normals.net.bias", (3,))]
    for i in range(n_prop):
        pre = f"proposal_networks.{i}.mlp_base.mlp.layers."
        out += [(pre + "0.weight", (16, 10)), (pre + "0.bias", (16,)), (pre + "1.weight", (1, 16)), (pre + "1.bias", (1,))]
    return out


class Case:
    def __init__(self, name, seed=0, app_dim=32, pred_normals=True, n_prop=2, absmax=(1e-3, 1e-3, 1e-3)):
        self.name, self.app_dim, self.pred_normals, self.n_prop = name, app_dim, pred_normals, n_prop
        self.absmax = [np.float32(a) for a in absmax]
        rng = np.random.default_rng(1000 + seed)
        self.tensors = {n: (rng.standard_normal(s) * 0.1).astype(np.float32) for n, s in tensor_names(app_dim, pred_normals, n_prop)}
        self._rng = rng

    def table(self, which):
        """The hash table of field `which` (-1 main, i proposal net i), [levels << LOG2_T, 2]: uniform in (-a, a) with one entry at -a, so
        that its abs-max is the case's, bit for bit; a non-finite or zero abs-max fills accordingly."""
        a = self.absmax[which + 1]
        n = (MAIN_LEVELS if which < 0 else PROP_LEVELS) << LOG2_T
        t = np.random.default_rng(77 + which).uniform(-0.999, 0.999, (n, 2)).astype(np.float32)
        t = (t * a).astype(np.float32) if np.isfinite(a) else t
        t[3, 1] = -a
        assert (np.abs(t).max() == a) or not np.isfinite(a)
        return t

    def input_file(self):
        head = np.array([self.app_dim, int(self.pred_normals), self.n_prop, GEO, SH_LEVELS, *self.absmax], dtype=np.float32)
        return np.concatenate([head] + [self.tensors[n].reshape(-1) for n, _ in tensor_names(self.app_dim, self.pred_normals, self.n_prop)])

    def images(self):
        return [im for im in IMAGES if not im.startswith("prop") or int(im[4:]) < self.n_prop]


def cases():
    """name -> Case.  What each one reaches in sn_weights.h is said next to it."""
    W1, B1, W2 = "field.mlp_base.mlp.layers.0.weight", "field.mlp_base.mlp.layers.0.bias", "field.mlp_base.mlp.layers.1.weight"
    out = [Case("ordinary"),                                         # every plane of every image, pred-normal head fused
           Case("ordinary_again", seed=1),                           # (the buffer-reuse half of the GPU test)
           Case("bare", seed=2, app_dim=0, pred_normals=False, n_prop=1)]   # zero-filled normals path, no appearance fold
    c = Case("small_table", seed=3, absmax=(1e-4, 1e-4, 1e-4))       # large t0 and s_l; fp16 subnormals and the lo planes
    c.tensors[W1][:, 5] *= np.float32(1e-6)
    out.append(c)
    # one weight of the density row (h0 feeds no colour input): s2 collapses, the geo columns of colour layer 1 take s3 / s2 and leave fp16
    c = Case("density_weight_leaves_fp16", seed=4)
    c.tensors[W2][0, 9] = np.float32(1e9)
    out.append(c)
    out.append(Case("table_not_finite", seed=5, absmax=(np.inf, 1e-3, np.inf)))   # first early return of plan_split_scales
    c = Case("bias_infinite", seed=9)                                # its second early return ("non-finite MLP parameters")
    c.tensors[B1][5] = np.float32(np.inf)
    out.append(c)
    # A NaN does NOT take that return: std::max(m, NaN) keeps m, so the bound of the unit is dropped, the layers behind it get scale 1 and
    # the images carry the NaN.  The case pins what the packers do with it.
    c = Case("bias_not_a_number", seed=6)
    c.tensors[B1][5] = np.float32(np.nan)
    out.append(c)
    # a finite weight so large that the clamp of pow2_floor (2^-80) cannot bring it into fp16: the net stays unconditioned, t0p = s1p = 1
    c = Case("proposal_leaves_fp16", seed=7)
    c.tensors["proposal_networks.1.mlp_base.mlp.layers.0.weight"][2, 3] = np.float32(3e38)
    out.append(c)
    c = Case("zero_table_zero_wc3", seed=8, absmax=(0.0, 0.0, 0.0))  # the pow2_floor fallbacks to 1 (t0, t0p, s5)
    c.tensors["field.mlp_head.layers.2.weight"][:] = 0
    out.append(c)
    return {c.name: c for c in out}


# ---- the same cases on the device, through the C ABI (the GPU test; the golden digests were recorded with these functions) ----------
IMAGE_BYTES = {"main": 42640, "main_h": 46752, "normals": 50960, "normals_h": 50832, "prop0": 5008, "prop1": 5008}   # sn_layout.h


def field_desc(case):
    """A descriptor sn_create accepts, with no de-hashed copies (the images do not depend on them) and the smallest tables."""
    from signerf_amd import _lib

    def grid(levels, hidden, out_dim):
        g = _lib.SnHashMlpDesc()
        g.num_levels, g.features_per_level, g.log2_hashmap_size, g.hidden_dim, g.num_layers, g.out_dim, g.grid_mode = levels, 2, LOG2_T, hidden, 2, out_dim, 0
        for lv in range(levels):
            g.scalings[lv] = float(int(16 * 1.4 ** lv))
        return g

    d = _lib.SnFieldDesc()
    d.main_field = grid(MAIN_LEVELS, 64, 16)
    d.geo_feat_dim, d.hidden_dim_color, d.appearance_embed_dim, d.sh_levels, d.sh_remap = GEO, 64, case.app_dim, SH_LEVELS, 0
    d.num_proposals = case.n_prop
    for i in range(case.n_prop):
        d.proposals[i] = grid(PROP_LEVELS, 16, 1)
    d.average_init_density, d.histogram_padding = 0.01, 0.01
    d.dense_levels = -1
    return d


def upload_and_finalize(lib, handle, case, device):
    import torch
    from signerf_amd import _lib

    stream = _lib.current_stream()
    named = [(n, case.tensors[n]) for n, _ in tensor_names(case.app_dim, case.pred_normals, case.n_prop)]
    named.append(("field.mlp_base.encoder.hash_table", case.table(-1)))
    named += [(f"proposal_networks.{i}.mlp_base.encoder.hash_table", case.table(i)) for i in range(case.n_prop)]
    for name, a in named:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        _lib.check(lib.sn_upload_weights(handle, name.encode(), t.data_ptr(), t.numel() * 4, stream), handle, name)
    _lib.check(lib.sn_finalize_weights(handle, stream), handle, "sn_finalize_weights")


def read_back(lib, handle, case, device):
    """({image: bytes}, {"precision": [kernel 0, kernel 1] for a split-precision request, "feature_scale": [main, proposal nets ...]})"""
    import ctypes as C

    import torch
    from signerf_amd import _lib

    images = {}
    for im in case.images():
        which = int(im[4:]) if im.startswith("prop") else -1
        buf = torch.zeros(IMAGE_BYTES[im], dtype=torch.uint8, device=device)
        _lib.check(lib.sn_debug_read(handle, which, DEBUG_READ_WHAT[im], buf.data_ptr(), buf.numel(), _lib.current_stream()), handle, "sn_debug_read " + im)
        torch.cuda.synchronize()
        images[im] = buf.cpu().numpy().tobytes()
    scales = []
    for which in range(-1, case.n_prop):
        lay = _lib.SnDebugLayout()
        _lib.check(lib.sn_debug_layout(handle, which, C.byref(lay)), handle, "sn_debug_layout")
        scales.append(float(lay.feature_scale))
    return images, {"precision": [lib.sn_effective_precision(handle, 1, 0), lib.sn_effective_precision(handle, 1, 1)], "feature_scale": scales}
