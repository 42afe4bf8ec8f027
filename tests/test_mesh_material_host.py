"""Proxy-mesh materials, CPU side: the OBJ / MTL readers, the ``materials`` field, the companion C header
include/signerf_hip_mesh_material.h against the binding and the library's exports, its argument checks, known answers of the float64
oracle (tests/mesh_material_oracle.py), and the caps on what the GPU tests (tests/test_gpu_mesh_material.py) may leave out, evaluated on
the oracle's own flags for every scene and view those tests use.  No GPU.

The consumer of the pyrender fixtures (tools/make_pyrender_fixture.py --materials) is at the end, skipped until the files exist: the
constants of ``material_defaults`` are UNPINNED until then.
"""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import mesh_material_oracle as mmo
import mesh_oracle as mo
import mesh_rays_oracle as mro
from abi_helpers import c99_probe, refusal_sweep
from helpers import ROOT
from signerf_amd import _lib
from signerf_amd import renderer as R
from signerf_amd.renderer import Renderer, RendererConfig, load_mtl, load_obj, load_obj_materials, material_defaults, object_pose, pack_materials


OBJ = """# a quad and two triangles
mtllib two.mtl
v 0 0 0 1 0 0
v 1 0 0 0 1 0
v 1 1 0 0 0 1
v 0 1 0 1 1 0
v 2 0 0 1 0 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
f 1/1 2/2 3/3
usemtl red
f 1/1 2/2 3/3 4/4
vt 0.25 0.75
usemtl checker
f 3/-1 2/-4/1 5/-3
usemtl red
f 1 2 5
usemtl nowhere
f 2//1 3//1 5//1
vn 0 0 1
"""
MTL = """# written by hand
newmtl red
Ns 96.078431
Ka 1.000000 1.000000 1.000000
Kd 0.8 0.1 0.05
Ks 0.5 0.5 0.5
d 1.0
illum 2

newmtl checker
map_Kd -s 2 2 -o 0.5 0.5 -clamp on my texture.png
map_Ks other.png

newmtl twin
Kd 1 1 1
map_Kd my texture.png
"""


def _write(tmp_path, obj=OBJ, mtl=MTL, texture=True):
    from PIL import Image

    (tmp_path / "two.obj").write_text(obj)
    if mtl is not None:
        (tmp_path / "two.mtl").write_text(mtl)
    if texture:
        t = np.zeros((2, 3, 3), np.uint8)
        t[0, :, 0], t[1, :, 1] = (10, 20, 30), (40, 50, 60)
        Image.fromarray(t, "RGB").save(tmp_path / "my texture.png")
    return str(tmp_path / "two.obj")


# ---- the readers -------------------------------------------------------------------------------------------------------------------------
def test_load_obj_is_unchanged_by_material_lines(tmp_path):
    """``load_obj`` on an OBJ with vt / usemtl / mtllib lines: exactly the arrays of the parent commit, written out here."""
    path = _write(tmp_path)
    v, f = load_obj(path)
    want_v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0]], np.float32)
    want_f = np.array([[0, 1, 2], [0, 1, 2], [0, 2, 3], [2, 1, 4], [0, 1, 4], [1, 2, 4]], np.int32)
    assert v.dtype == np.float32 and f.dtype == np.int32
    np.testing.assert_array_equal(v, want_v)
    np.testing.assert_array_equal(f, want_f)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v2, f2, c = load_obj(path, with_colors=True)
    np.testing.assert_array_equal(v2, want_v)
    np.testing.assert_array_equal(f2, want_f)
    np.testing.assert_array_equal(c, np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255], [255, 255, 0, 255], [255, 0, 255, 255]], np.uint8))


def test_material_reader(tmp_path):
    path = _write(tmp_path)
    with pytest.warns(UserWarning, match="nowhere"):
        uv, tm, mats = load_obj_materials(path)
    assert [m.name for m in mats] == ["red", "checker", "twin"]
    assert mats[0].kd == (0.8, 0.1, 0.05) and mats[0].texture is None and mats[0].map_kd is None
    # map_Kd with options (skipped, not applied) and a file name with spaces; no Kd
    assert mats[1].kd is None and mats[1].map_kd == str(tmp_path / "my texture.png") and mats[1].texture.shape == (2, 3, 4)
    assert mats[1].texture.dtype == np.uint8 and (mats[1].texture[..., 3] == 255).all() and mats[1].texture[0, 1, 0] == 20
    # faces before any usemtl and a name the .mtl does not define: -1; usemtl switches mid-file; the quad is fanned with its uv
    np.testing.assert_array_equal(tm, np.array([-1, 0, 0, 1, 0, -1], np.int32))
    assert uv.shape == (6, 3, 2) and uv.dtype == np.float32
    np.testing.assert_array_equal(uv[0], [[0, 0], [1, 0], [1, 1]])
    np.testing.assert_array_equal(uv[1], [[0, 0], [1, 0], [1, 1]])
    np.testing.assert_array_equal(uv[2], [[0, 0], [1, 1], [0, 1]])
    # negative indices are relative to the vt read so far (five then): -1 = the fifth, -4 = the second, -3 = the third
    np.testing.assert_array_equal(uv[3], np.array([[0.25, 0.75], [1, 0], [1, 1]], np.float32))
    assert np.isnan(uv[4]).all() and np.isnan(uv[5]).all()   # corners without vt: drawn without texture
    # two materials sharing one texture: stored once
    mm = pack_materials(uv, tm, mats)
    assert mm.records["texel_offset"].tolist() == [0, 0, 0] and mm.records["tex_width"].tolist() == [0, 3, 3]
    assert mm.records["tex_height"].tolist() == [0, 2, 2] and mm.texels.size == 2 * 3 * 4 and mm.textured
    np.testing.assert_allclose(mm.records["base_color"], [[0.8, 0.1, 0.05, 1], [0.4, 0.4, 0.4, 1], [1, 1, 1, 1]], rtol=1e-7)
    assert C.sizeof(_lib.SnMeshMaterial) == R.MATERIAL_RECORD.itemsize == 32
    d = material_defaults()
    assert d == {"texture_srgb": True, "default_base_color": R.PYRENDER_DEFAULT_BASE_COLOR, "missing_kd": (0.4, 0.4, 0.4),
                 "vertex_colors_with_materials": False}
    # an OBJ without vt: corner_uv is None, nothing is textured
    uv0, tm0, mats0 = load_obj_materials(_write(tmp_path, "mtllib two.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl twin\nf 1 2 3\n"))
    assert uv0 is None and tm0.tolist() == [2] and not pack_materials(uv0, tm0, mats0).textured


@pytest.mark.parametrize("obj,line,what", [
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/2 3/1\n", 5, "outside the 1 texture"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/0 2/1 3/1\n", 5, "index 0"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/-2 2/1 3/1\n", 5, "outside the 1 texture"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/x 2/1 3/1\n", 5, "bad face corner"),
    ("v 0 0 0\nvt zero 0\n", 2, "bad texture coordinate"),
    ("v 0 0 0\nvt\n", 2, "at least u"),
    ("mtllib\n", 1, "file name"),
])
def test_material_reader_errors_name_file_and_line(tmp_path, obj, line, what):
    path = _write(tmp_path, obj)
    with pytest.raises(ValueError, match=re.escape(f"{path}:{line}:") + ".*" + what):
        load_obj_materials(path)


@pytest.mark.parametrize("mtl,line,what", [
    ("newmtl a\nKd 0.5 oops 0.5\n", 2, "bad Kd"),
    ("newmtl a\nKd 0.5 0.5\n", 2, "three finite"),
    ("newmtl a\nKd nan 0 0\n", 2, "three finite"),
    ("Kd 1 1 1\n", 1, "before any newmtl"),
    ("newmtl\n", 1, "needs a name"),
    ("newmtl a\nmap_Kd -clamp on\n", 2, "file name"),
])
def test_mtl_errors_name_file_and_line_in_setup(tmp_path, mtl, line, what):
    path = _write(tmp_path, mtl=mtl)
    with pytest.raises(ValueError, match=re.escape(f"{tmp_path / 'two.mtl'}:{line}:") + ".*" + what):
        load_mtl(tmp_path / "two.mtl")
    r = Renderer(RendererConfig(object_path=path, materials="mtl"), device="cpu")
    with pytest.raises(ValueError, match=re.escape(f"two.mtl:{line}:")):
        r.setup()
    Renderer(RendererConfig(object_path=path), device="cpu").setup()   # "none" never opens the .mtl


def test_missing_pieces_degrade_with_a_warning(tmp_path):
    # 1. the mtllib file is absent (the reference's bunny): no materials, the "none" image
    path = _write(tmp_path, mtl=None)
    with pytest.warns(UserWarning, match="two.mtl not found"):
        uv, tm, mats = load_obj_materials(path)
    assert mats == [] and (tm == -1).all()
    r = Renderer(RendererConfig(object_path=path, materials="mtl"), device="cpu")
    with pytest.warns(UserWarning, match="not found"):
        r.setup()
    assert r._host_materials is None
    # 2. the map_Kd file is absent: that material is Kd only
    path = _write(tmp_path, texture=False)
    os.remove(tmp_path / "my texture.png") if os.path.exists(tmp_path / "my texture.png") else None
    with pytest.warns(UserWarning, match="my texture.png not found"):
        mats = load_mtl(tmp_path / "two.mtl")
    assert mats[1].texture is None and mats[2].texture is None and mats[2].kd == (1.0, 1.0, 1.0)
    # 3. the map_Kd file cannot be decoded: the same
    (tmp_path / "my texture.png").write_bytes(b"not a picture")
    with pytest.warns(UserWarning, match="cannot be decoded"):
        mats = load_mtl(tmp_path / "two.mtl")
    assert mats[1].texture is None
    with pytest.warns(UserWarning):
        r = Renderer(RendererConfig(object_path=path, materials="mtl"), device="cpu")
        r.setup()
    assert r._host_materials is not None and not r._host_materials.textured and r._host_materials.records.shape[0] == 3


# ---- the config field --------------------------------------------------------------------------------------------------------------------
def test_materials_field_default_validation_and_config_yml(tmp_path):
    import yaml

    from signerf_amd.datasetgenerator import DatasetGenerator, DatasetGeneratorConfig

    assert RendererConfig().materials == "none"
    assert Renderer(RendererConfig(materials="mtl"), device="cpu").config.materials == "mtl"
    with pytest.raises(ValueError, match="materials.*none, mtl"):
        Renderer(RendererConfig(materials="pbr"), device="cpu")
    cfg = DatasetGeneratorConfig(path=tmp_path, dataset_name="s", width=8, height=8, combine_shape_with_depth=True,
                                 renderer=RendererConfig(object_path="proxy.obj", materials="mtl"))
    g = DatasetGenerator(cfg, device="cpu", write_images=False)
    g.init_directory()
    assert yaml.safe_load((tmp_path / "s" / "config.yml").read_text())["renderer"]["materials"] == "mtl"
    g.dataset.close()


def test_setup_reads_no_mtl_for_none(tmp_path):
    path = _write(tmp_path)
    os.remove(tmp_path / "two.mtl")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = Renderer(RendererConfig(object_path=path), device="cpu")
        r.setup()
    assert r._host_materials is None and r.num_triangles == 6


# ---- the companion C header ----------------------------------------------------------------------------------------------------------------
def test_material_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    lib = _lib.load()
    assert lib.sn_mesh_material_abi_version() == _lib.header("mesh_material").version == 1
    assert lib.sn_mesh_abi_version() == 1 and lib.sn_mesh_color_abi_version() == 1 and lib.sn_mesh_rays_abi_version() == 1   # untouched
    blob = open(built_lib, "rb").read()
    assert b"sn_mesh_tile_material_kernel" in blob and b"sn_mesh_rays_material_kernel" in blob


def test_material_structs_layout_matches_c(tmp_path):
    rec = ["base_color", "texel_offset", "tex_width", "tex_height", "reserved"]
    mats = ["struct_size", "n_materials", "materials", "host_materials", "triangle_material", "corner_uv", "texels", "texel_bytes", "texture_srgb",
            "reserved"]
    exprs = ["sizeof(SnMeshMaterial)", "sizeof(SnMeshMaterials)", "SN_MESH_MATERIAL_ABI_VERSION"] + \
            [f"offsetof(SnMeshMaterial, {k})" for k in rec] + [f"offsetof(SnMeshMaterials, {k})" for k in mats]
    got = [int(x) for x in c99_probe(tmp_path, "signerf_hip_mesh_material.h", "%zu %zu %d" + " %zu" * (len(rec) + len(mats)), ", ".join(exprs))]
    a, b = _lib.SnMeshMaterial, _lib.SnMeshMaterials
    want = [C.sizeof(a), C.sizeof(b), _lib.header("mesh_material").version] + [getattr(a, k).offset for k in rec] + [getattr(b, k).offset for k in mats]
    assert got == want and C.sizeof(a) == 32
    assert _lib.SnMeshMaterials().struct_size == C.sizeof(b)


_NULL_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
fake = 0x1000   # never dereferenced: every call below is refused before the device is touched
fwd = (C.c_float * 3)(0, 0, -1)
F = 10
nb = lib.sn_mesh_accel_bytes(F)
mv = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
ws_bytes = lib.sn_mesh_color_workspace_bytes(F, 4, 4)
keep = []
def records(n=2, w=4, h=4, off=0, nan=False):
    r = (_lib.SnMeshMaterial * max(n, 1))()
    for k in range(max(n, 1)):
        r[k].base_color[:] = [0.5, 0.5, 0.5, 1.0]
    r[0].tex_width, r[0].tex_height, r[0].texel_offset = w, h, off
    if nan: r[0].base_color[1] = float("nan")
    keep.append(r)
    return r
def mats(n=2, dev=fake, host="default", tm=fake, uv=fake, texels=fake, nbytes=64, size=None, **kw):
    m = _lib.SnMeshMaterials()
    m.n_materials, m.materials, m.triangle_material, m.corner_uv, m.texels, m.texel_bytes = n, dev, tm, uv, texels, nbytes
    if host == "default": m.host_materials = C.cast(records(n, **kw), C.POINTER(_lib.SnMeshMaterial))
    if size is not None: m.struct_size = size
    keep.append(m)
    return C.byref(m)
def ropts():
    o = _lib.SnMeshRasterOpts(); o.znear, o.zfar = 1e-4, 10.0; keep.append(o); return C.byref(o)
def yopts():
    o = _lib.SnMeshRaysOpts(); o.znear, o.zfar = 1e-4, 10.0; keep.append(o); return C.byref(o)
def sopts(size=None):
    o = _lib.SnMeshShadeOpts(); o.base_color[:] = [0.3, 0.3, 0.3, 1.0]; o.ambient[:] = [1.0, 1.0, 1.0]; o.background[:] = [1.0, 1.0, 1.0]
    if size is not None: o.struct_size = size
    keep.append(o); return C.byref(o)
def raster(m, shade="default", color=fake, ws=fake, h=4):
    return lib.sn_mesh_raster_color_materials(fake, 30, m, fake, F, mv, 10.0, 10.0, 2.0, 2.0, h, 4, ropts(), sopts() if shade == "default" else shade,
                                              fake, color, ws, ws_bytes, N)
def cast(m, shade="default", color=fake, accel=fake, depth=fake):
    return lib.sn_mesh_cast_rays_materials(fake, fake, 4, 4, fwd, accel, nb, N, F, m, 0, yopts(), sopts() if shade == "default" else shade,
                                           depth, color, N)
calls = {"abi": lambda: lib.sn_mesh_material_abi_version()}
for name, fn in (("raster", raster), ("cast", cast)):
    calls.update({
     name + "_null_materials": lambda fn=fn: fn(None),
     name + "_size0": lambda fn=fn: fn(mats(size=0)),
     name + "_newer": lambda fn=fn: fn(mats(size=256)),
     name + "_m0": lambda fn=fn: fn(mats(n=0)),
     name + "_m65536": lambda fn=fn: fn(mats(n=65536, host=None)),
     name + "_null_records": lambda fn=fn: fn(mats(dev=N)),
     name + "_null_host_records": lambda fn=fn: fn(mats(host=None)),
     name + "_null_triangle_material": lambda fn=fn: fn(mats(tm=N)),
     name + "_misaligned_records": lambda fn=fn: fn(mats(dev=fake + 8)),
     name + "_misaligned_uv": lambda fn=fn: fn(mats(uv=fake + 4)),
     name + "_null_texels": lambda fn=fn: fn(mats(texels=N)),
     name + "_side_0": lambda fn=fn: fn(mats(w=0, h=4)),
     name + "_side_big": lambda fn=fn: fn(mats(w=16385, h=1, nbytes=1 << 20)),
     name + "_side_negative": lambda fn=fn: fn(mats(w=-4, h=4)),
     name + "_blob_small": lambda fn=fn: fn(mats(nbytes=60)),
     name + "_offset_beyond": lambda fn=fn: fn(mats(off=1)),
     name + "_kd_nan": lambda fn=fn: fn(mats(nan=True)),
     name + "_no_shade": lambda fn=fn: fn(mats(), shade=None),
     name + "_shade_size0": lambda fn=fn: fn(mats(), shade=sopts(0)),
     name + "_no_color": lambda fn=fn: fn(mats(), color=N),
    })
calls["raster_no_workspace"] = lambda: raster(mats(), ws=N)
calls["raster_height_0"] = lambda: raster(mats(), h=0)
calls["cast_null_accel"] = lambda: cast(mats(), accel=N)
calls["cast_no_depth"] = lambda: cast(mats(), depth=N)
for k, f in calls.items():
    print(k, f(), flush=True)
    if k.endswith("_blob_small"): print(k + "_text", int(b"texel" in lib.sn_last_error(None)), flush=True)
"""


def test_material_calls_refuse_bad_arguments_before_the_device(built_lib):
    """NULL where not allowed, M outside [1, 65535], a texture side outside [1, 16384], a texel blob smaller than the (host copy of the)
    records claim, a struct_size of 0 or of a newer layout: refused with SN_ERR_INVALID (the workspace: SN_ERR_WORKSPACE) and a text, in
    a child process -- nothing is launched (every pointer is a fake), and a crash would be a segfault, not an exception."""
    got = refusal_sweep(_NULL_SWEEP)
    want = {k: "1" for k in got}
    want["raster_no_workspace"] = "4"
    assert len(got) == 1 + 2 * 21 + 4 and got == want, got


# ---- known answers of the oracle ------------------------------------------------------------------------------------------------------------
def test_oracle_sampler_known_answers():
    tex = np.array([[[10, 20, 30], [40, 50, 60]], [[70, 80, 90], [100, 110, 120]]], np.float64)   # row 0 is the TOP row: v = 1
    # texel centres return the texels; the v flip: (u, v) = (0.25, 0.75) is column 0 of the top row
    for (u, v), want in (((0.25, 0.75), tex[0, 0]), ((0.75, 0.75), tex[0, 1]), ((0.25, 0.25), tex[1, 0]), ((0.75, 0.25), tex[1, 1])):
        got, four = mmo.sample(tex, np.array([u]), np.array([v]))
        np.testing.assert_allclose(got[0], want, atol=1e-12)
    # u = 0: the mean of the first and the last column (the wrap), continuous across the seam; the same one period on
    for u in (0.0, 1.0, -1.0, 1e-12, -1e-12):
        got, _ = mmo.sample(tex, np.array([u]), np.array([0.75]))
        np.testing.assert_allclose(got[0], 0.5 * (tex[0, 0] + tex[0, 1]), atol=1e-9)
    got, _ = mmo.sample(tex, np.array([0.25]), np.array([1.0]))   # v = 1: the top and the bottom row blend
    np.testing.assert_allclose(got[0], 0.5 * (tex[0, 0] + tex[1, 0]), atol=1e-12)
    got, four = mmo.sample(tex, np.array([0.4, np.nan]), np.array([0.6, 0.5]))
    np.testing.assert_allclose(got[0], 0.49 * tex[0, 0] + 0.21 * tex[0, 1] + 0.21 * tex[1, 0] + 0.09 * tex[1, 1], atol=1e-9)
    assert np.isnan(got[1]).all() and four.shape == (2, 4, 3)


def test_oracle_shading_known_answers():
    tri = np.array([[0, 1, -1, 2]])
    bary = np.tile(np.array([1 / 3, 1 / 3, 1 / 3]), (1, 4, 1))
    kd = (0.8, 0.1, 0.05)
    flat = np.full((4, 4, 4), 128, np.uint8)
    uv = np.tile(np.array([[0.1, 0.1], [0.4, 0.1], [0.1, 0.4]], np.float32), (3, 1, 1))
    x, spread = mmo.shade(tri, bary, uv, np.array([0, 1, 7]), [(kd, None), ((1.0, 1.0, 1.0), flat)])
    np.testing.assert_allclose(x[0, 0], 255.0 * np.power(kd, 1 / 2.2), rtol=1e-12)          # Kd only: 255 * Kd^(1 / 2.2)
    np.testing.assert_allclose(x[0, 1], 128.0, rtol=1e-12)                                  # the sRGB round trip of a flat texture
    np.testing.assert_allclose(x[0, 2], 255.0)                                              # the background
    np.testing.assert_allclose(x[0, 3], 255.0 * 0.3 ** (1 / 2.2), rtol=1e-12)               # index outside the list: the default grey (148)
    assert (spread == 0).all() and np.floor(x[0, 3] + 0.5).tolist() == [148, 148, 148]
    # spread: the four texels' final levels
    ramp = np.zeros((2, 2, 4), np.uint8)
    ramp[..., :3] = np.array([[100, 110], [120, 160]])[..., None]
    x, spread = mmo.shade(tri[:, 1:2], bary[:, 1:2], np.tile(np.array([[0.5, 0.5]] * 3, np.float32), (2, 1, 1)), np.array([0, 0]),
                          [((1.0, 1.0, 1.0), ramp)])
    np.testing.assert_allclose(spread[0, 0], 60.0, rtol=1e-12)
    np.testing.assert_allclose(x[0, 0], 122.5, rtol=1e-12)   # the texels are blended, then linearised: the round trip gives their mean
    assert abs(mmo.tie_window(60.0, 96) - (1e-3 + 60 * 96 / 2 ** 20)) < 1e-15


def test_procedural_scene_inputs():
    for k, (w, h) in enumerate(mmo.TEXTURE_SIZES):
        t = procedural = mmo.procedural_texture(w, h, seed=k)
        assert t.shape == (h, w, 4) and t[..., :3].min() >= 51 and (t[..., 3] == 255).all() and len(np.unique(t[..., :3])) > 50
        assert np.abs(np.diff(procedural[..., :3].astype(int), axis=1)).max() < 40   # smooth
    v, f = mo.icosphere(3)
    uv = mmo.spherical_corner_uv(v, f)
    assert uv.shape == (f.shape[0], 3, 2) and uv[..., 0].max() > 1.0   # crosses the seam
    assert np.bincount(mmo.thirds(10)).tolist() == [4, 3, 3]


# ---- the cap on what the GPU tests may leave out -------------------------------------------------------------------------------------------
def _caps(name, ok, covered):
    of_pixels, of_covered = mro.flagged_shares(~ok, covered)
    print(f"{name}: covered {covered.mean():.4f}; flagged {int((~ok).sum())} = {of_pixels:.5f} of the pixels, {of_covered:.5f} of the covered")
    assert of_pixels <= mro.MAX_FLAGGED_OF_PIXELS and of_covered <= mro.MAX_FLAGGED_OF_COVERED, (name, of_pixels, of_covered)
    assert int((ok & covered).sum()) > 500


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("name", sorted(mmo.RASTER_CASES))
def test_flagged_share_of_the_raster_scenes(name, cull):
    mesh, mv, fx, fy, cx, cy, H, W = mmo.RASTER_CASES[name]
    v, f = mesh()
    tri, bary, ok, cov = mmo.raster_flags(v, f, mv, fx, fy, cx, cy, H, W, cull=cull)
    _caps(f"{name} cull={cull}", ok, cov)


@pytest.mark.parametrize("name", mmo.RAY_VIEWS)
def test_flagged_share_of_the_ray_views(name):
    v, f, _ = mro.bumpy_sphere()
    world = mro.posed(v, object_pose(RendererConfig(scale=mro.BUNNY_SCALE)))
    view = mro.views()[name]
    o, d = mro.cpu_rays(view)
    tri, bary, ok, z = mmo.ray_flags(o, d, mro.forward_of(view["c2w"]), world, f)
    _caps(name, ok, z > 0)
    if name.startswith("pinhole"):   # (G4) compares the raster with the ray cast there: the raster's own ambiguous pixels count as well
        from signerf_amd.renderer import model_view

        mv = model_view(view["c2w"].reshape(-1).tolist(), object_pose(RendererConfig(scale=mro.BUNNY_SCALE)))
        _, amb, graze = mo.raster_depth(v, f, mv, view["fx"], view["fy"], view["cx"], view["cy"], view["H"], view["W"])
        _caps(name + " with the raster's flags", ok & ~(amb | graze).reshape(-1), z > 0)


def test_kd_of_the_exact_test_are_off_the_rounding_boundaries():
    for kd in mmo.KD_EXACT:
        x = 255.0 * np.power(np.asarray(kd, dtype=np.float64), 1.0 / 2.2)
        assert (np.abs(x - np.floor(x) - 0.5) > 1e-3).all(), (kd, x)


# ---- the pyrender fixtures -----------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden", "pyrender_materials")


@pytest.mark.parametrize("which", ["kd", "textured"])
def test_material_constants_against_the_pyrender_fixture(which):
    """Pins ``material_defaults`` (and the shading above) once someone with pyrender and trimesh has run
    ``tools/make_pyrender_fixture.py --materials``: each fixture holds the mesh as trimesh loaded it from the OBJ / MTL / PNG the tool
    wrote, the camera, and pyrender's colour image.  Compared away from silhouette edges (pyrender resolves a multisampled image there)
    and, for the textured one, with one level of slack per level of local slope (pyrender samples a mip-mapped texture)."""
    path = os.path.join(GOLDEN, f"{which}.npz")
    if not os.path.exists(path):
        pytest.skip(f"{os.path.relpath(path, ROOT)} not recorded yet (tools/make_pyrender_fixture.py --materials): the constants of "
                    "material_defaults are UNPINNED")
    z = np.load(path)
    v, f, mv = z["vertices"], z["triangles"], z["model_view"]
    fx, fy, cx, cy = (float(a) for a in z["intrinsics"])
    H, W = z["color"].shape[:2]
    tri, bary, ok, cov = mmo.raster_flags(v, f, mv, fx, fy, cx, cy, H, W)
    edge = np.zeros_like(ok)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            edge |= np.roll(np.roll(cov, dy, 0), dx, 1) != cov
    ok &= ~edge
    d = material_defaults()
    mats = []
    for k, kd in enumerate(z["kd"]):
        tex = z[f"texture_{k}"] if f"texture_{k}" in z.files else None
        mats.append((tuple(float(q) for q in kd) if np.isfinite(kd).all() else d["missing_kd"], tex))
    uv = z["corner_uv"] if "corner_uv" in z.files and z["corner_uv"].size else None
    x, spread = mmo.shade(tri, bary, uv, z["triangle_material"], mats, default_base=d["default_base_color"][:3], texture_srgb=d["texture_srgb"])
    got = z["color"].astype(np.int64)
    assert ok.sum() > 100
    assert (np.abs(got - np.floor(x + 0.5)) <= 1 + spread[..., None])[ok].all()
