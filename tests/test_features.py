"""Feature buffers off the GPU: the numpy reference of tests/features_ref.py pinned to the oracle,
the two entry points in the ABI, and FeatureFilm on synthetic tiles."""
import ctypes as C

import numpy as np
import pytest

import features_ref as FR
import lumo_amd as L
import oracle_ffi as O
from lumo_amd import _ffi

SEED = 0xFEA7


@pytest.fixture(scope="module")
def cornell():
    scene = L.Scene.cornell_box()
    cam = L.Camera.cornell_box((24, 24))
    return scene, cam, L.make_tasks(24, 24, 3, SEED)


def test_reference_film_matches_oracle(cornell):
    """The reference colour pipeline and film gather, fed with the oracle's per-path radiance,
    wavelengths and raster positions, give the oracle's tiles within 1e-12 Σw|c| per channel (exp and
    cosh: numpy's against lmath, a few ulp per term).  24 x 24: four tiles, 16- and 8-wide."""
    scene, cam, tasks = cornell
    assert len(tasks) == 4
    assert sorted((t.px_max[0] - t.px_min[0], t.px_max[1] - t.px_min[1]) for t in tasks) == \
        [(8, 8), (8, 16), (16, 8), (16, 16)]
    obufs, _, _ = O.render_tasks(scene.desc(), cam.desc, tasks, O.WAVEFRONT, 1)
    for t, ob in zip(tasks, obufs):
        p = O.trace_paths(scene.desc(), cam.desc, t)
        rgb = FR.color_rgb(scene.desc(), cam.desc, p["radiance"], p["lam"])
        tile, mag = FR.film_tile(t, cam.desc, p["raster"], rgb, with_abs=True)
        want = ob.reshape(tile.shape)
        assert (want[..., 3] > 0).all()
        bound = 1e-12 * np.concatenate([mag, want[..., 3:4]], axis=-1)
        err = np.abs(tile - want)
        print("max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()


def test_reference_film_clips_to_the_tile():
    """A sample near a tile edge spreads only inside the tile; its weights are the separable Gaussian's."""
    cam = L.Camera.cornell_box((32, 32))
    t = _ffi.TileTask((16, 0), (32, 16), 0, 1, 1, 1)
    tile = FR.film_tile(t, cam.desc, [(16.2, 0.7)], [(1.0, -2.0, 0.5)])
    nz = np.argwhere(tile[..., 3] != 0.0)
    assert len(nz) and nz[:, 0].max() <= 2 and nz[:, 1].max() <= 1
    fr, fs = cam.desc.filter_radius, cam.desc.filter_sigma
    w = (FR.gauss(16.2 - 16.5, fs) - FR.gauss(fr, fs)) * (FR.gauss(0.7 - 0.5, fs) - FR.gauss(fr, fs))
    assert tile[0, 0, 3] == w and tile[0, 0, 1] == -2.0 * w


def test_entry_points_exported():
    lib = _ffi.load()
    names = [n for n, _, _ in _ffi.DEVICE_API]
    for name in ("lumo_render_features", "lumo_debug_features"):
        assert name in names
        assert hasattr(lib, name)
    assert lib.lumo_abi_version() == 10  # an addition: the capability check is the symbol


def test_null_context_is_invalid():
    lib = _ffi.load()
    t = _ffi.TileTask((0, 0), (8, 8), 0, 1, 1, 1)
    out = _ffi.FeaturePlanes()
    cfg = _ffi.FeatureCfg(0, 0)
    assert lib.lumo_render_features(None, C.byref(t), 1, C.byref(cfg), C.byref(out)) == 1  # LUMO_ERR_INVALID
    assert lib.lumo_render_features(None, None, 0, None, None) == 1
    assert lib.lumo_debug_features(None, C.byref(t), C.byref(_ffi.FeatureDump())) == 1


def test_struct_layouts():
    """The ctypes mirrors of the three new structs: pointer-sized fields in the header's order."""
    assert C.sizeof(_ffi.FeaturePlanes) == 3 * C.sizeof(C.c_void_p)
    assert C.sizeof(_ffi.FeatureCfg) == 8
    assert [f[0] for f in _ffi.FeatureDump._fields_] == [
        "kind", "object", "prim", "material", "backface", "t", "p", "ng", "ns", "n", "uv", "albedo", "albedo_rgb",
        "raster", "lambda_"]
    assert C.sizeof(_ffi.FeatureDump) == 15 * C.sizeof(C.c_void_p)


def _tile(w, h, albedo, normal, t, hit, weight):
    """Planes of a w x h tile whose every pixel has one sample of the given features and weight."""
    P = w * h
    a = np.tile(np.array([*(weight * np.asarray(albedo)), weight]), P)
    n = np.tile(np.array([*(weight * np.asarray(normal)), weight]), P)
    d = np.tile(np.array([weight * t * hit, weight * hit, 0.0, weight]), P)
    return a, n, d


def test_feature_film_accumulates_and_normalises(tmp_path):
    film = L.FeatureFilm(8, 4)
    t0 = _ffi.TileTask((0, 0), (4, 4), 0, 1, 2, 1)
    t1 = _ffi.TileTask((0, 0), (4, 4), 1, 1, 2, 2)  # the tile's second batch
    film.add_tile(t0, _tile(4, 4, (0.2, 0.4, 0.6), (0.0, 0.0, 1.0), 2.0, 1.0, 0.5))
    film.add_tile(t1, _tile(4, 4, (0.6, 0.4, 0.2), (0.0, 1.0, 0.0), 4.0, 1.0, 1.5))
    # left half: two batches; right half: never written
    np.testing.assert_array_equal(film.albedo_w[:, :4, 3], 2.0)
    np.testing.assert_allclose(film.albedo()[:, :4], np.broadcast_to((0.5, 0.4, 0.3), (4, 4, 3)), rtol=1e-15)
    np.testing.assert_allclose(film.depth()[:, :4], (0.5 * 2.0 + 1.5 * 4.0) / 2.0, rtol=1e-15)
    np.testing.assert_array_equal(film.coverage()[:, :4], 1.0)
    n = film.normal()[:, :4]
    np.testing.assert_allclose(np.linalg.norm(n, axis=-1), 1.0, rtol=1e-15)
    np.testing.assert_allclose(n, np.broadcast_to(np.array((0.0, 1.5, 0.5)) / np.hypot(1.5, 0.5), (4, 4, 3)), rtol=1e-15)
    for plane in (film.albedo(), film.normal(), film.depth(), film.coverage()):
        assert np.isfinite(plane).all()
        assert (plane[:, 4:] == 0.0).all()  # an empty pixel is 0, not NaN
    film.save_albedo(tmp_path / "albedo.png")
    film.save_normal(tmp_path / "normal.png")
    from lumo_amd.image import read_png
    img = read_png(tmp_path / "normal.png")
    assert img.shape == (4, 8, 3)
    assert tuple(img[0, 7]) == (128, 128, 128)  # 0.5 n + 0.5 of an empty pixel
    assert img[0, 0, 1] > 200 and img[0, 0, 0] == 128
    assert read_png(tmp_path / "albedo.png").shape == (4, 8, 3)


def test_feature_film_partial_coverage():
    """Misses add weight with zero features: depth is over the hits only, coverage their share."""
    film = L.FeatureFilm(2, 2)
    t = _ffi.TileTask((0, 0), (2, 2), 0, 2, 2, 1)
    film.add_tile(t, _tile(2, 2, (0.8, 0.8, 0.8), (1.0, 0.0, 0.0), 3.0, 1.0, 1.0))
    film.add_tile(t, _tile(2, 2, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, 0.0, 3.0))  # a miss
    np.testing.assert_array_equal(film.depth(), 3.0)
    np.testing.assert_array_equal(film.coverage(), 0.25)
    np.testing.assert_allclose(film.albedo(), 0.2, rtol=1e-15)
    np.testing.assert_array_equal(film.normal(), np.broadcast_to((1.0, 0.0, 0.0), (2, 2, 3)))
