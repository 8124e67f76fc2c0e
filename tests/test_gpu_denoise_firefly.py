"""The firefly clamp (lumo_denoise_set_firefly) against tests/denoise_firefly_ref.py composed with the unchanged
references: equal bits for rgb and variance, and the same count of clamped pixels."""
import ctypes as C

import denoise_firefly_ref as FR
import denoise_ref as DR
import denoise_temporal_ref as TR
import numpy as np
import pytest
from test_gpu_denoise import assert_equal_bits, dev, film_of  # noqa: F401 (dev: the module's context fixture)
from test_gpu_denoise_temporal import camera

import lumo_amd as L
from lumo_amd import _ffi

pytestmark = pytest.mark.gpu

# (x, y) of the fireflies per frame size, all on hit pixels but `miss`: `pair` and `ell` are copies of their first pixel
# (equal luminances), `edge` lies either side of the depth and normal edge, `seam_x` either side of x = 127 | 128
# (two blocks), `seam_y` either side of y = 15 | 16 and 31 | 32 (two marches).  (1, 1) and (5, 3) are smaller than a
# wave and a ring, (131, 5) has two blocks in x, (67, 37) three marches in y.
SPIKES = {
    (1, 1): {},
    (5, 3): dict(alone=[(0, 0)], corner=[(4, 2)], miss=[(3, 1)]),
    (131, 5): dict(alone=[(16, 3)], pair=[(43, 0), (44, 0)], ell=[(98, 3), (99, 3), (98, 4)], corner=[(0, 4)],
                   edge=[(72, 2), (73, 4)], miss=[(100, 1)], seam_x=[(127, 1), (128, 3)]),
    (67, 37): dict(alone=[(8, 30)], pair=[(22, 5), (23, 5)], ell=[(50, 28), (51, 28), (50, 29)], corner=[(0, 0), (66, 36)],
                   edge=[(36, 25), (37, 8)], miss=[(48, 15)], seam_y=[(5, 15), (60, 16), (25, 31), (30, 32)]),
}
# R, rank, min_alike, gain; the last: a corner or border pixel never has min_alike neighbours
SETTINGS = [(2, 2, 4, 1.0), (1, 1, 1, 1.0), (3, 8, 8, 2.0), (1, 8, 8, 1.0)]
CFG = dict(iterations=2)  # the filter behind the clamp is test_gpu_denoise's subject


def spiked(size, seed=None):
    """(film, features, add_rgb) of DR.frame with SPIKES[size] injected: rgb_w's colour times 50 .. 1000."""
    planes = [np.ascontiguousarray(p) for p in DR.frame(*size, seed=size[0] if seed is None else seed)]
    for i, (name, pix) in enumerate(SPIKES[size].items()):
        for x, y in pix:
            if (x, y) != pix[0] and name in ("pair", "ell"):
                for p in planes:
                    p[y, x] = p[pix[0][1], pix[0][0]]
            else:
                planes[0][y, x, :3] *= 50.0 + 950.0 * (i % 5) / 4.0
    film, feat = film_of(planes)
    return film, feat, film.splat_scale * film.splats / film.filter_integral()


def reference(film, feat, add, setting):
    """(c', the clamped count) of the frame under `setting`."""
    return FR.clamp(film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w, add,
                    dict(zip(("radius", "rank", "min_alike", "gain"), setting)))


@pytest.fixture
def clamping(dev):  # noqa: F811
    """The module's context, with the clamp switched off again afterwards."""
    yield dev
    dev.set_firefly(None)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "R%d-rank%d-min%d-gain%g" % s)
@pytest.mark.parametrize("size", SPIKES, ids=lambda s: "%dx%d" % s)
def test_synthetic_frames(clamping, size, setting):
    film, feat, add = spiked(size)
    c1, count = reference(film, feat, add, setting)
    want = DR.denoise(FR.frame_of(c1), feat.albedo_w, feat.normal_w, feat.depth_w, None, **CFG)
    clamping.set_firefly(**dict(zip(("radius", "rank", "min_alike", "gain"), setting)))
    assert_equal_bits(clamping.denoise(film, feat, return_variance=True, **CFG), want)
    assert clamping.firefly_info()["clamped"] == count and clamping.firefly_info()["ms"] > 0.0


def test_off_is_off():
    """A context that never set the clamp and one that set it and took it back filter the raw frame."""
    film, feat, add = spiked((67, 37))
    want = DR.denoise(film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w, add, **CFG)
    d = L.Device(0)
    try:
        for _ in range(2):
            assert_equal_bits(d.denoise(film, feat, return_variance=True, **CFG), want)
            assert d.firefly_info() == {"clamped": 0, "ms": 0.0}
            d.set_firefly({})
            d.set_firefly(None)
    finally:
        d.close()


def test_temporal(clamping):
    """Two static frames and a pan on one context: each the temporal reference of the clamped frames, the first also
    Device.denoise of its input under the same setting."""
    size, S = (67, 37), None
    clamping.set_firefly()
    clamping.denoise_reset()
    for k, cam in enumerate([camera(size), camera(size), camera(size, yaw=2e-3 * 64 / size[0], shift=0.02)]):
        film, feat, add = spiked(size, seed=size[0] + 7 * k)
        c1, count = reference(film, feat, add, SETTINGS[0])
        *want, S, met = TR.denoise_temporal(S, cam, FR.frame_of(c1), feat.albedo_w, feat.normal_w, feat.depth_w, None, **CFG)
        assert_equal_bits(clamping.denoise_temporal(film, feat, cam, return_variance=True, **CFG), want)
        assert clamping.firefly_info()["clamped"] == count and (met["with_history"] > 0) == (k > 0)
        if k == 0:
            assert_equal_bits(clamping.denoise(film, feat, return_variance=True, **CFG), want)


def test_argument_errors(clamping):
    lib = _ffi.load()

    def call(ctx=clamping.ctx, **kw):
        return lib.lumo_denoise_set_firefly(ctx, C.byref(_ffi.FireflyCfg(**{**_ffi.FIREFLY_DEFAULTS, **kw})))

    bad = [dict(radius=0), dict(radius=4), dict(rank=0), dict(rank=9, min_alike=9), dict(min_alike=1), dict(min_alike=49),
           dict(reserved=1), dict(gain=0.5), dict(gain=2e6), dict(gain=float("nan")), dict(gain=float("inf")),
           dict(normal_cos_min=-1.5), dict(normal_cos_min=1.5), dict(depth_rel_max=-1.0), dict(depth_rel_max=2e6),
           dict(depth_rel_max=float("nan")), dict(ctx=None)]
    assert [call(**kw) for kw in bad] == [1] * len(bad) and call() == 0 and call(rank=8, min_alike=48, radius=3) == 0
    info = _ffi.FireflyInfo()
    assert lib.lumo_denoise_firefly_info(None, C.byref(info)) == 1 and lib.lumo_denoise_firefly_info(clamping.ctx, None) == 1
    with pytest.raises(TypeError):
        clamping.set_firefly(sigma=1.0)
