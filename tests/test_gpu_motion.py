"""The motion feature on the GPU (DESIGN.md §4g "Motion"): the per-sample delta against tests/denoise_motion_ref.py and,
without any restatement, against a rigid translation; the plane against the reference film; the end-to-end sequence."""
import ctypes as C
import functools

import denoise_motion_ref as MR
import features_ref as FR
import numpy as np
import pytest
from test_gpu_features import SCENES, tile_task
from test_gpu_scale import _arrays
from test_gpu_wide import _small_scenes
from test_gpu_wide_refit import _moved

import lumo_amd as L
from lumo_amd import _ffi

pytestmark = pytest.mark.gpu
SEED, RES, EPS = 0x307104, (24, 20), 2.0 ** -52
TILES = {"film": (4, 2, 20, 18), "gather": (2, 0, 22, 18)}  # 256 pixels: k_motion_film; 360: the per-slot gather
NAMES = ["small_dragon", "scaled_instances"]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, camera, vertices, which of them _moved moves)"""
    make, cam = (_small_scenes()[name][0], _small_scenes()[name][2]) if name == "small_dragon" else SCENES["instances"]
    sc = make().build()
    v0 = _arrays(sc.desc())[0].copy()
    return sc, cam(RES), v0, (_moved(sc.desc())[0] != v0).any(axis=1)


def run(name, tile, v1):
    """The records and planes of one task after a mark and an update to v1, and the planes before either."""
    sc, cam, _, _ = scene(name)
    task = tile_task(*TILES[tile], 2, SEED)
    dev = L.Device(0, accel=1)
    try:
        dev.upload(sc, cam)
        still = [dev.render_features_motion([task], features=False)[0], dev.motion_mark().render_features_motion([task])[0][3]]
        dev.update_vertices(v1)
        return dict(task=task, cam=cam, still=still, g=dev.debug_features(task), mo=dev.debug_motion(task),
                    planes=dev.render_features_motion([task])[0], feat=dev.render_features([task])[0],
                    beauty=dev.render_tasks([task])[0][0])
    finally:
        dev.close()


def by_object(name, g):
    """Per object hit on a kd mesh: (its samples, the vertex indices of their triangles, its transform or None)."""
    d = scene(name)[0].desc()
    for o in np.unique(g["object"][g["kind"] == 1]):
        if d.objects[o].type == 0:
            sel, x = (g["kind"] == 1) & (g["object"] == o), d.objects[o].xform
            yield sel, _arrays(d)[1]["v"][g["prim"][sel]], np.array(d.transforms[x].m).reshape(4, 4) if x >= 0 else None


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", NAMES)
def test_delta_and_plane(name, tile):
    v0, v1 = scene(name)[2], _moved(scene(name)[0].desc())[0]
    r = run(name, tile, v1)
    g, mo, want, moving = r["g"], r["mo"], np.zeros_like(r["mo"]["delta"]), np.zeros(len(r["g"]["kind"]), dtype=bool)
    for sel, tv, m in by_object(name, g):
        want[sel] = MR.delta(mo["bary"][sel], v1[tv], v0[tv], m)
        p = MR.point(mo["bary"][sel], v1[tv])  # pins bary without restating the intersection
        np.testing.assert_array_equal(g["p"][sel], p if m is None else MR.through(m, p, 1.0))
        moving |= sel & (want != 0.0).any(axis=1)
    assert moving.any() and ((g["kind"] != 0) & ~moving).any()  # a moved mesh and a static object are in view
    assert (mo["delta"].view(np.uint64) == want.view(np.uint64)).all()
    tile_w, mag = FR.film_tile(r["task"], r["cam"].desc, g["raster"], mo["delta"], with_abs=True)
    got = r["planes"][3].reshape(tile_w.shape)
    assert (np.abs(got - tile_w) <= 1e-12 * np.concatenate([mag, tile_w[..., 3:4]], axis=-1)).all()
    np.testing.assert_array_equal(got[..., 3].ravel(), r["beauty"].reshape(-1, 4)[:, 3])
    for a, b in zip(r["planes"][:3], r["feat"]):
        np.testing.assert_array_equal(a, b)
    for plane in r["still"]:  # before a mark, and after a mark without an update
        assert not plane.reshape(-1, 4)[:, :3].any() and (plane.reshape(-1, 4)[:, 3] == got[..., 3].ravel()).all()


@pytest.mark.parametrize("name", NAMES)
def test_rigid_translation(name):
    """Every movable vertex moved by t: a kd-mesh sample has delta = -t (an instance's through its m) to within 64 eps
    of the largest coordinate involved (the local vertices', times the largest row sum of |m|): a handful of roundings
    in e / det and in two 3-term sums, and the transform's.  Every other sample has exactly 0."""
    _, _, v0, mov = scene(name)
    t = np.array([0.03, -0.02, 0.05])
    r = run(name, "film", v0 + mov[:, None] * t)
    delta, moving, big = r["mo"]["delta"], np.zeros(len(r["g"]["kind"]), dtype=bool), np.abs(v0[mov]).max() + np.abs(t).max()
    for sel, tv, m in by_object(name, r["g"]):
        assert mov[tv].all()
        err = np.abs(delta[sel] + (t if m is None else m[:3, :3] @ t)).max()
        bound = 64 * EPS * big * (1.0 if m is None else np.abs(m[:3, :3]).sum(1).max())
        print(name, "worst |delta + t|", err, "bound", bound)
        assert err <= bound
        moving |= sel
    assert moving.any() and ((r["g"]["kind"] != 0) & ~moving).any() and not delta[~moving].any()


def test_sequence_keeps_history_on_a_moving_mesh():
    """small_dragon at 32 x 32, 4 spp, a static camera, the mesh moving about a pixel per frame: with the motion plane
    at least as many pixels find their history as without it, and more on the third frame."""
    sc, _, v0, mov = scene("small_dragon")
    cam = _small_scenes()["small_dragon"][2]((32, 32))
    step = np.array([0.25 * np.abs(v0[mov]).max(), 0.0, 0.0])  # in the mesh's own space; the plane reads 0.98 pixel
    info, counts, other = {}, [], L.Device(0)
    try:
        for film, feat, _ in L.Renderer(sc, cam).samples(4).seed(SEED).render_denoised_sequence(
                [cam] * 3, vertices=[v0 + k * mov[:, None] * step for k in range(3)], info=info):
            assert (feat.motion_w[..., :3] != 0.0).any() == (len(counts) > 0)
            without = {}
            other.denoise_temporal(film, feat, cam, info=without)  # the same frames, no plane
            counts.append((info["with_history"], without["with_history"]))
    finally:
        other.close()
    print("with_history (motion, none) per frame:", counts)
    assert all(a >= b for a, b in counts) and counts[2][0] > counts[2][1]


def test_refusals_and_arguments():
    lib, task, dev = _ffi.load(), tile_task(0, 0, 8, 8, 1, 1), L.Device(0)
    buf, one, ptr = np.zeros(4 * 64), np.zeros((64, 3)), lambda a: a.ctypes.data_as(_ffi.c_double_p)
    t, planes, dump = C.byref(task), C.byref(_ffi.MotionPlanes(ptr(buf))), C.byref(_ffi.MotionDump(ptr(one), None))
    sc, cam, _, _ = scene("small_dragon")
    den = lambda ctx, c: lib.lumo_denoise_temporal_motion(  # noqa: E731
        ctx, C.byref(_ffi.DenoiseIn(8, 8, *[ptr(buf)] * 4, None)), ptr(buf), c, None, None, ptr(one), None, None)
    try:
        assert [lib.lumo_scene_motion_mark(None), lib.lumo_scene_motion_mark(dev.ctx)] == [1, 4]  # INVALID, NO_SCENE
        assert [lib.lumo_render_features_motion(dev.ctx, t, 1, None, None, planes), lib.lumo_debug_motion(dev.ctx, t, dump)] == [4, 4]
        dev.upload(sc)
        assert lib.lumo_render_features_motion(dev.ctx, t, 1, None, None, planes) == 5  # NO_CAMERA
        dev.upload(sc, cam)
        assert lib.lumo_scene_motion_mark(dev.ctx) == 0  # accel = 0: nothing can move
        bad = [lib.lumo_render_features_motion(dev.ctx, t, 1, None, None, None), lib.lumo_render_features_motion(None, t, 1, None, None, planes),
               lib.lumo_render_features_motion(dev.ctx, t, 1, C.byref(_ffi.FeatureCfg(4, 0)), None, planes),
               lib.lumo_debug_motion(dev.ctx, t, None), lib.lumo_debug_motion(dev.ctx, None, dump), den(None, C.byref(cam.desc)),
               den(dev.ctx, None), den(dev.ctx, C.byref(cam.desc))]  # the last: the camera is 24 x 20, the frame 8 x 8
        assert bad == [1] * len(bad)
        assert lib.lumo_render_features_motion(dev.ctx, t, 1, None, None, planes) == 0 and lib.lumo_debug_motion(dev.ctx, t, dump) == 0
        assert (buf.reshape(-1, 4)[:, 3] > 0.0).all() and not buf.reshape(-1, 4)[:, :3].any()
    finally:
        dev.close()
