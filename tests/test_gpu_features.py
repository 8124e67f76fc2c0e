"""Feature buffers on the GPU (lumo_render_features / lumo_debug_features): the per-sample records
against bounce 0 of the oracle, the shading normal, the albedo, the alignment with the beauty film,
the filtered planes against the reference film of tests/features_ref.py, the kernel forms, and the
isolation from lumo_render_tiles.  Tiles of 16 x 16 or less at 2-3 spp: oracle_debug_trace renders
the whole task again for every sample it is asked about."""
import ctypes as C

import numpy as np
import pytest

import features_ref as FR
import lumo_amd as L
import oracle_ffi as O
import scenes as S
from lumo_amd import _ffi
from parity import oracle_threads

pytestmark = pytest.mark.gpu

SEED = 0xFEA70001
F64_EPS = np.finfo(np.float64).eps


def ulps(a, b):
    """|a - b| in units of the spacing of b."""
    return np.abs(a - b) / np.spacing(np.abs(b))


def tile_task(x0, y0, x1, y1, samples, seed):
    return _ffi.TileTask((x0, y0), (x1, y1), 0, samples, samples, seed)


def look(origin, towards, res):
    return L.Camera.builder().origin(*origin).towards(*towards).resolution(res).build()


# scene name -> (scene factory, camera factory of the resolution)
SCENES = {
    "cornell": (L.Scene.cornell_box, L.Camera.cornell_box),
    "zoo": (S.material_zoo, S.default_camera),
    "instances": (S.scaled_instances, lambda res: look((1e4 + 1.0, 1.0, -1e4 + 6.0), (1e4 + 1.0, 0.3, -1e4), res)),
    "spheres": (S.sphere_field, lambda res: look((0.0, 0.3, 6.0), (0.0, 0.0, 0.0), res)),
    # the open scene: a finite plane seen from above its near edge; the frame's upper part looks past it
    # (chosen with the oracle: 74 % of the compared tile's camera rays miss)
    "flat": (S.flat_mesh, lambda res: look((0.1, 0.8, 1.6), (0.1, 0.25, 0.2), res)),
    "textures": (S.texture_zoo, S.default_camera),
}
_built = {}


def built(name, res):
    """(built scene, camera) of a SCENES entry, built once per resolution."""
    if (name, res) not in _built:
        make, cam = SCENES[name]
        _built[name, res] = (make().build(), cam(res))
    return _built[name, res]


_oracle = {}


def oracle_samples(name, res, task, accel=0, sampler=0):
    """The oracle's bounce-0 records and per-path raster / wavelengths of a task, computed once."""
    key = (name, res, bytes(task), accel, sampler)
    if key not in _oracle:
        sc, cam = built(name, res)
        _oracle[key] = (FR.first_hits(sc.desc(), cam.desc, task, sampler=sampler, accel=accel),
                        O.trace_paths(sc.desc(), cam.desc, task, sampler=sampler, accel=accel))
    return _oracle[key]


def device(name, res, **opts):
    sc, cam = built(name, res)
    dev = L.Device(0, **opts)
    dev.upload(sc, cam)
    return dev


def assert_records_equal(g, hits, paths):
    """The dump of one task against the oracle's bounce-0 records (a miss: no record) and paths."""
    np.testing.assert_array_equal(g["kind"] != 0, hits["hit"], err_msg="hit")
    for k in ("kind", "object", "t", "p", "ng", "backface"):
        np.testing.assert_array_equal(g[k], hits[k], err_msg=k)
    np.testing.assert_array_equal(g["raster"], paths["raster"], err_msg="raster")
    # trace_paths reports a path's wavelengths as they are when it ends: a dispersive dielectric on
    # the way terminates all but the hero wavelength (zeros).  The features carry the camera
    # sample's four: equal where the path kept them, the hero equal always.
    kept = (paths["lam"][:, 1:] != 0.0).all(axis=1)
    assert kept.any()
    np.testing.assert_array_equal(g["lambda_"][kept], paths["lam"][kept], err_msg="lambda")
    np.testing.assert_array_equal(g["lambda_"][:, 0], paths["lam"][:, 0], err_msg="hero wavelength")
    assert not paths["lam"][~kept][:, 1:].any()
    assert ((g["lambda_"] >= 360.0) & (g["lambda_"] <= 830.0)).all()
    miss = g["kind"] == 0
    for k in ("t", "p", "ng", "ns", "n", "uv", "albedo", "albedo_rgb", "backface"):
        assert not g[k][miss].any(), k  # zeros, written explicitly (the buffers start poisoned)
    for k in ("object", "prim", "material"):
        assert (g[k][miss] == -1).all(), k
    np.testing.assert_array_equal(g["n"], np.where(g["backface"][:, None] != 0, -g["ns"], g["ns"]))


# ---------------------------------------------------------------- 1. per-sample equality with the oracle
# (scene, resolution, tile, samples, accel, device options)
RECORD_CASES = [
    ("cornell", (16, 16), (0, 0, 16, 16), 2, 0, {}),                      # exactly a block, LDS-staged
    ("cornell", (16, 16), (0, 0, 16, 16), 2, 0, {"lds_staging": 0}),
    ("cornell", (24, 20), (16, 16, 24, 20), 3, 1, {}),                    # the ragged frame corner, wide accel
    ("zoo", (16, 16), (4, 6, 12, 14), 2, 0, {}),                          # a partial wave, FX 1
    ("zoo", (16, 16), (4, 6, 12, 14), 2, 1, {}),
    ("instances", (16, 16), (4, 4, 12, 12), 2, 0, {}),
    ("instances", (16, 16), (4, 4, 12, 12), 2, 1, {}),
    ("spheres", (16, 16), (4, 4, 12, 12), 2, 0, {}),
    ("spheres", (16, 16), (4, 4, 12, 12), 2, 1, {}),
    ("flat", (16, 16), (2, 0, 14, 10), 2, 0, {}),
    ("flat", (16, 16), (2, 0, 14, 10), 2, 1, {}),
]


@pytest.mark.parametrize("name,res,tile,samples,accel,opts", RECORD_CASES,
                         ids=[f"{c[0]}-{c[2][2] - c[2][0]}x{c[2][3] - c[2][1]}-accel{c[4]}" + ("-nolds" if c[5] else "")
                              for c in RECORD_CASES])
def test_records_match_oracle(name, res, tile, samples, accel, opts):
    task = tile_task(*tile, samples, SEED)
    hits, paths = oracle_samples(name, res, task, accel=accel)
    if name == "flat":  # the miss share is real
        share = 1.0 - hits["hit"].mean()
        assert 0.05 <= share <= 0.95, share
    dev = device(name, res, accel=accel, **opts)
    try:
        info = dev.scene_info()
        assert info.accel == accel
        if name == "cornell":
            assert (info.lds_bytes > 0) == (not opts) and info.full_kernels == 0
        g = dev.debug_features(task)
    finally:
        dev.close()
    assert_records_equal(g, hits, paths)


# ---------------------------------------------------------------- 2. shading normal
@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_shading_normal_is_geometric_without_vertex_normals(name):
    """Meshes without vertex normals, rectangles and spheres: ns == ng bit for bit."""
    task = tile_task(0, 0, 16, 16, 2, SEED + 1)
    dev = device(name, (16, 16))
    try:
        g = dev.debug_features(task)
    finally:
        dev.close()
    assert (g["kind"] != 0).any()
    np.testing.assert_array_equal(g["ns"], g["ng"])


def test_bump_mapped_shading_normal():
    """texture_zoo's bump-mapped cube: ns leaves ng, stays a unit vector, and the normal feature
    follows ng's face convention (backface = ray direction . ng > 0, hit.rs:47)."""
    sc, cam = built("textures", (32, 32))
    d = sc.desc()
    bumped = [i for i in range(d.num_materials) if d.materials[i].normal_map >= 0]
    assert bumped
    task = tile_task(0, 0, 32, 32, 1, SEED + 2)  # the whole frame as one task
    dev = device("textures", (32, 32))
    try:
        assert dev.scene_info().full_kernels == 2
        g = dev.debug_features(task)
    finally:
        dev.close()
    on = np.isin(g["material"], bumped)
    assert on.sum() >= 16
    assert (g["ns"][on] != g["ng"][on]).any(axis=1).any()
    length = np.sqrt((g["ns"][on] ** 2).sum(axis=1))
    assert (np.abs(length - 1.0) <= 4 * F64_EPS).all(), np.abs(length - 1.0).max() / F64_EPS
    off = (g["kind"] != 0) & ~on
    np.testing.assert_array_equal(g["ns"][off], g["ng"][off])
    # default camera: a pinhole at the origin, so the ray direction is along p
    hit = g["kind"] != 0
    side = (g["p"][hit] * g["ng"][hit]).sum(axis=1)
    sure = np.abs(side) > 1e-9 * np.sqrt((g["p"][hit] ** 2).sum(axis=1))
    np.testing.assert_array_equal(g["backface"][hit][sure] != 0, side[sure] > 0.0)
    np.testing.assert_array_equal(g["n"], np.where(g["backface"][:, None] != 0, -g["ns"], g["ns"]))


# ---------------------------------------------------------------- 3. albedo
class PatchedScene:
    """A built scene whose description carries an edited copy of the material table."""

    def __init__(self, scene, edit):
        self._base = scene
        d = scene.desc()
        self._mats = (_ffi.Material * d.num_materials)()
        C.memmove(self._mats, d.materials, C.sizeof(self._mats))
        for i in range(d.num_materials):
            edit(i, self._mats[i])
        self._desc = _ffi.SceneDesc()
        C.memmove(C.byref(self._desc), C.byref(d), C.sizeof(_ffi.SceneDesc))
        self._desc.materials = self._mats

    def build(self):
        return self

    def desc(self):
        return self._desc


def as_lambertian(i, m):
    """The material's albedo slot (kd, ks or tf by kind) as a Lambertian of the same spectrum."""
    if m.kind == _ffi.MAT_MF_CONDUCTOR:
        m.albedo = m.ks
    elif m.kind == _ffi.MAT_MF_DIELECTRIC:
        m.albedo = m.tf
    if m.kind in (_ffi.MAT_MF_DIFFUSE, _ffi.MAT_MF_CONDUCTOR, _ffi.MAT_MF_DIELECTRIC):
        m.kind = _ffi.MAT_LAMBERTIAN


def lambertian_albedo(desc, material, lam):
    """pi f of a Lambertian material from the oracle's BSDF probe, at one sample's wavelengths."""
    _, f = O.bsdf_eval(desc, int(material), (0.0, 0.0, 1.0), lam, [(0.0, 0.0, 1.0)])
    return np.pi * f[0]


def test_albedo_of_solid_materials():
    """The zoo's tile across its cubes and walls: Lambertian and MfDiffuse give kd, the conductors
    ks, the dielectrics tf, each within 4 ulp of pi f of a Lambertian of that spectrum from the
    oracle's BSDF probe (a multiply and a divide apart); lights give 1."""
    sc, cam = built("zoo", (32, 32))
    ref = PatchedScene(sc, as_lambertian).desc()
    d = sc.desc()
    kinds = np.array([d.materials[i].kind for i in range(d.num_materials)])
    dev = device("zoo", (32, 32))
    try:
        g = dev.debug_features(tile_task(0, 0, 32, 32, 1, SEED + 3))  # the whole frame as one task
    finally:
        dev.close()
    hit = g["kind"] != 0
    seen = set(kinds[g["material"][hit]].tolist())
    assert {_ffi.MAT_LAMBERTIAN, _ffi.MAT_MF_DIFFUSE, _ffi.MAT_MF_CONDUCTOR, _ffi.MAT_MF_DIELECTRIC,
            _ffi.MAT_LIGHT} <= seen, seen
    worst = 0.0
    for i in np.flatnonzero(hit):
        kind = kinds[g["material"][i]]
        if kind == _ffi.MAT_LIGHT:
            assert g["kind"][i] == 2
            np.testing.assert_array_equal(g["albedo"][i], 1.0)
            continue
        want = lambertian_albedo(ref, g["material"][i], g["lambda_"][i])
        worst = max(worst, float(ulps(g["albedo"][i], want).max()))
    print("albedo against pi f: worst", worst, "ulp")
    assert worst <= 4.0


def test_albedo_of_blank_is_zero():
    """A Blank material (the zoo's Lambertian cube turned Blank in the description) gives 0."""
    sc, _ = built("zoo", (32, 32))
    d = sc.desc()
    target = [i for i in range(d.num_materials) if d.materials[i].kind == _ffi.MAT_LAMBERTIAN]
    assert target

    def blank(i, m):
        if i in target:
            m.kind = _ffi.MAT_BLANK

    patched = PatchedScene(sc, blank)
    dev = L.Device(0)
    try:
        dev.upload(patched, S.default_camera((32, 32)))
        g = dev.debug_features(tile_task(0, 0, 32, 32, 1, SEED + 5))
    finally:
        dev.close()
    on = np.isin(g["material"], target)
    assert on.sum() >= 8
    assert not g["albedo"][on].any() and not g["albedo_rgb"][on].any()
    assert (g["t"][on] > 0.0).all()


def spectrum_at(s, lam):
    """Spectrum::sample (spectrum.rs:108-124): f32 arithmetic, as the device's spec_one."""
    f = np.float32
    l = np.asarray(lam, dtype=np.float64).astype(f)
    x = f(s.c0) * l * l + f(s.c1) * l + f(s.c2)
    sig = f(0.5) + x / (f(2.0) * np.sqrt(f(1.0) + x * x))
    return (f(s.scale) * sig).astype(np.float64)


def test_checkerboard_albedo_and_rgb():
    """texture_zoo's dielectric cube, tf a checkerboard of two solids: every sample on it has one
    child's spectrum or the other's, both occur, uv is wrapped; and albedo_rgb of every sample is the
    reference colour pipeline's value of its albedo (1e-12 of the sample's largest channel: the
    matrices mix channels, so the bound is norm-wise)."""
    sc, cam = built("textures", (32, 32))
    d = sc.desc()
    mats = [i for i in range(d.num_materials)
            if d.materials[i].kind == _ffi.MAT_MF_DIELECTRIC and d.materials[i].tf_tex >= 0
            and d.textures[d.materials[i].tf_tex].kind == _ffi.TEX_CHECKERBOARD]
    assert len(mats) == 1
    tex = d.textures[d.materials[mats[0]].tf_tex]
    kids = [d.textures[tex.first], d.textures[tex.second]]
    assert all(k.kind == _ffi.TEX_SOLID for k in kids)
    task = tile_task(0, 0, 32, 32, 1, SEED + 6)  # the whole frame as one task
    dev = device("textures", (32, 32))
    try:
        g = dev.debug_features(task)
    finally:
        dev.close()
    on = g["material"] == mats[0]
    assert on.sum() >= 16
    a, lam = g["albedo"][on], g["lambda_"][on]
    is0 = (a == spectrum_at(kids[0].spec, lam)).all(axis=1)
    is1 = (a == spectrum_at(kids[1].spec, lam)).all(axis=1)
    assert (is0 | is1).all() and is0.any() and is1.any()
    hit = g["kind"] != 0
    assert hit.all()  # the scene has an environment map
    assert ((g["uv"] >= 0.0) & (g["uv"] < 1.0)).all()
    want = FR.color_rgb(d, cam.desc, g["albedo"], g["lambda_"])
    err = np.abs(g["albedo_rgb"] - want).max(axis=1)
    bound = 1e-12 * np.abs(want).max(axis=1)
    print("albedo_rgb: worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()


# ---------------------------------------------------------------- 4. alignment with the beauty film
def cornell_camera(kind, res):
    b = L.Camera.cornell_box_builder().resolution(res)
    if kind == "thin_lens":
        b = b.lens_radius(10.0).focal_length(1000.0)
    elif kind == "orthographic":
        b = L.Camera.builder().origin(278.0, 273.0, -800.0).towards(278.0, 273.0, 0.0).resolution(res) \
            .camera_type(L.CameraType.Orthographic)
    return b.build()


@pytest.mark.parametrize("camera,sampler", [("pinhole", L.SamplerType.MultiJittered), ("pinhole", L.SamplerType.Sobol),
                                            ("thin_lens", L.SamplerType.MultiJittered),
                                            ("orthographic", L.SamplerType.Jittered),
                                            ("pinhole", L.SamplerType.Uniform)])
def test_weights_equal_the_beauty_film(camera, sampler):
    """Channel 3 of all three planes is render_tasks' sum w of the same tasks bit for bit, and the
    oracle's; a render cut into chunks by max_paths gives the same planes."""
    res = (24, 20)  # 16 x 16, 8 x 16, 16 x 4 and 8 x 4 tiles
    sc = L.Scene.cornell_box().build()
    cam = cornell_camera(camera, res)
    tasks = L.make_tasks(*res, 3, SEED + 7)
    assert len(tasks) == 4
    dev = L.Device(0)
    try:
        dev.upload(sc, cam)
        if camera == "thin_lens":
            assert cam.desc.lens_radius != 0.0
        planes = dev.render_features(tasks, sampler=sampler)
        chunked = dev.render_features(tasks, max_paths=300, sampler=sampler)  # 256 | 128 + 64 + 32
        bufs, _ = dev.render_tasks(tasks, sampler=sampler)
    finally:
        dev.close()
    obufs, _, _ = O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads(), sampler=sampler)
    for p, q, b, ob in zip(planes, chunked, bufs, obufs):
        w = b.reshape(-1, 4)[:, 3]
        assert (w > 0.0).all()
        np.testing.assert_array_equal(w, ob.reshape(-1, 4)[:, 3])
        for plane, again in zip(p, q):
            np.testing.assert_array_equal(plane.reshape(-1, 4)[:, 3], w)
            np.testing.assert_array_equal(plane, again)
        np.testing.assert_array_equal(p[2].reshape(-1, 4)[:, 2], 0.0)


# ---------------------------------------------------------------- 5. filtered planes
def plane_sources(g):
    """The three planes' per-sample values from a dump."""
    hit = (g["kind"] != 0).astype(np.float64)
    return g["albedo_rgb"], g["n"], np.stack([g["t"] * hit, hit, np.zeros_like(hit)], axis=1)


@pytest.mark.parametrize("name", ["cornell", "flat"])
@pytest.mark.parametrize("shape", ["tiles", "large"])
def test_planes_match_reference_film(name, shape):
    """The planes against the reference film fed with the dump's own per-sample features: within
    1e-12 sum w |f| per channel (the normal plane is signed).  tiles: one block per task, two tasks
    of different sample counts and the ragged corner in one call; large: a 20 x 15 tile (more than
    256 pixels) takes every task of the call through the per-slot gather."""
    res = (24, 20)
    sc, cam = built(name, res)
    if shape == "tiles":
        tasks = [tile_task(0, 0, 16, 16, 2, SEED + 8), tile_task(16, 0, 24, 16, 3, SEED + 9),
                 tile_task(16, 16, 24, 20, 3, SEED + 10)]
    else:
        tasks = [tile_task(2, 3, 22, 18, 2, SEED + 11), tile_task(0, 16, 16, 20, 3, SEED + 12)]
    dev = device(name, res)
    try:
        planes = dev.render_features(tasks)
        dumps = [dev.debug_features(t) for t in tasks]
    finally:
        dev.close()
    if name == "flat":
        miss = np.concatenate([g["kind"] == 0 for g in dumps]).mean()
        assert 0.05 <= miss <= 0.95, miss
    for t, p, g in zip(tasks, planes, dumps):
        for label, got, src in zip(("albedo", "normal", "depth"), p, plane_sources(g)):
            want, mag = FR.film_tile(t, cam.desc, g["raster"], src, with_abs=True)
            bound = 1e-12 * np.concatenate([mag, want[..., 3:4]], axis=-1)
            err = np.abs(got.reshape(want.shape) - want)
            print(label, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), label


# ---------------------------------------------------------------- 6. kernel forms
@pytest.fixture(scope="module")
def mid_bistro():
    from lumo_amd import scenes
    from lumo_amd.procedural import bistro_standin
    return scenes.bistro(bistro_standin(groups=48, lamps=160, n=8)).build(), scenes.bistro_camera((96, 64))


@pytest.mark.parametrize("accel", [0, 1])
def test_top_staged_and_plain_forms_agree(mid_bistro, accel):
    """A scene too large to stage whole: the closest hits come from the TOP-staged walk or, with TOP
    staging off, from the plain one; planes and records are identical, and the weights are the beauty's."""
    sc, cam = mid_bistro
    tasks = L.make_tasks(96, 64, 2, SEED + 13)[8:12]
    out = []
    for top in (1, 0):
        dev = L.Device(0, top_staging=top, accel=accel)
        try:
            dev.upload(sc, cam)
            info = dev.scene_info()
            assert info.accel == accel and info.lds_bytes == 0 and (info.top_bytes > 0) == bool(top)
            planes = dev.render_features(tasks)
            dump = dev.debug_features(tasks[0])
            bufs = dev.render_tasks(tasks)[0] if top else None
        finally:
            dev.close()
        out.append((planes, dump, bufs))
    (p1, d1, bufs), (p0, d0, _) = out
    assert (d1["kind"] != 0).any()
    for k in d1:
        np.testing.assert_array_equal(d1[k], d0[k], err_msg=k)
    for a, b, beauty in zip(p1, p0, bufs):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(x.reshape(-1, 4)[:, 3], beauty.reshape(-1, 4)[:, 3])


# ---------------------------------------------------------------- 7. isolation
def test_feature_render_leaves_the_beauty_alone():
    """Beauty, features, beauty on one context: the two beauty results are bit-identical, the
    schedule record is the beauty render's, and the feature render counts its camera rays as closest
    queries with one k_features and one film launch per pass."""
    sc, cam = built("cornell", (32, 32))
    tasks = L.make_tasks(32, 32, 3, SEED + 14)
    dev = device("cornell", (32, 32))
    try:
        b0, r0 = dev.render_tasks(tasks)
        sched = bytes(dev.last_schedule())
        before = dev.stats()
        dev.render_features(tasks)
        after = dev.stats()
        assert bytes(dev.last_schedule()) == sched
        b1, r1 = dev.render_tasks(tasks)
        assert bytes(dev.last_schedule()) == sched
    finally:
        dev.close()
    for x, y, rx, ry in zip(b0, b1, r0, r1):
        np.testing.assert_array_equal(x, y)
        assert (rx.num_rays, rx.num_queries) == (ry.num_rays, ry.num_queries)
    assert after.closest_queries - before.closest_queries == 32 * 32 * 3
    assert after.shadow_queries == before.shadow_queries
    assert after.aabb_tests[0] > before.aabb_tests[0] and after.aabb_tests[1] == before.aabb_tests[1]
    for stage in ("camera", "closest", "shade", "film"):
        k = _ffi.STAGES.index(stage)
        assert after.launches[k] - before.launches[k] == 3, stage
    for stage in ("shadow", "finish", "ring"):
        k = _ffi.STAGES.index(stage)
        assert after.launches[k] == before.launches[k], stage


def test_errors_match_the_render_call():
    lib = _ffi.load()
    t = tile_task(0, 0, 8, 8, 1, 1)
    buf = np.zeros(4 * 64)
    out = _ffi.FeaturePlanes(buf.ctypes.data_as(_ffi.c_double_p), None, None)
    dev = L.Device(0)
    try:
        assert lib.lumo_render_features(dev.ctx, C.byref(t), 1, None, C.byref(out)) == 4  # NO_SCENE
        sc, cam = built("cornell", (16, 16))
        dev.upload(sc)
        assert lib.lumo_render_features(dev.ctx, C.byref(t), 1, None, C.byref(out)) == 5  # NO_CAMERA
        dev.upload(sc, cam)
        assert lib.lumo_render_features(dev.ctx, C.byref(t), 1, None, None) == 1
        assert lib.lumo_render_features(dev.ctx, C.byref(t), 1, C.byref(_ffi.FeatureCfg(4, 0)), C.byref(out)) == 1
        big = _ffi.TileTask((0, 0), (8, 8), 0, 1, 1024, 1)
        assert lib.lumo_render_features(dev.ctx, C.byref(big), 1, C.byref(_ffi.FeatureCfg(3, 0)), C.byref(out)) == 1
        empty = _ffi.TileTask((8, 0), (8, 8), 0, 1, 1, 1)
        assert lib.lumo_render_features(dev.ctx, C.byref(empty), 1, None, C.byref(out)) == 1
        # a NULL plane is skipped: only the albedo plane is written
        assert lib.lumo_render_features(dev.ctx, C.byref(t), 1, None, C.byref(out)) == 0
        assert (buf.reshape(-1, 4)[:, 3] > 0.0).all()
    finally:
        dev.close()


# ---------------------------------------------------------------- 8. Renderer.render_features
def test_renderer_render_features():
    """Cornell at 48 x 32: the FeatureFilm equals the planes of Device.render_features over
    make_tasks, tile by tile; its shards add up to it."""
    sc = L.Scene.cornell_box()
    cam = L.Camera.cornell_box((48, 32))
    r = L.Renderer(sc, cam).samples(2).seed(SEED + 15)
    film = r.render_features()
    tasks = L.make_tasks(48, 32, 2, SEED + 15)
    dev = L.Device(0)
    try:
        dev.upload(r.scene, cam)
        planes = dev.render_features(tasks)
    finally:
        dev.close()
    want = L.FeatureFilm(48, 32)
    for t, p in zip(tasks, planes):
        want.add_tile(t, p)
    halves = [r.render_features(rank=k, world_size=2) for k in range(2)]
    for k in ("albedo_w", "normal_w", "depth_w"):
        np.testing.assert_array_equal(getattr(film, k), getattr(want, k))
        np.testing.assert_array_equal(getattr(halves[0], k) + getattr(halves[1], k), getattr(want, k))
    cov = film.coverage()
    assert ((cov >= 0.0) & (cov <= 1.0)).all() and (cov[12:20, 20:28] == 1.0).all()  # the box fills the centre
    seen = cov > 0.0
    assert np.isfinite(film.depth()).all() and (film.depth()[seen] > 0.0).all() and not film.depth()[~seen].any()
    np.testing.assert_allclose(np.linalg.norm(film.normal()[seen], axis=-1), 1.0, rtol=1e-12)
    assert not film.normal()[~seen].any() and not film.albedo()[~seen].any()
