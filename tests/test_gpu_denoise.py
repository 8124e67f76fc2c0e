"""lumo_denoise against tests/denoise_ref.py: equal bits (the same IEEE operations, the same exp)."""
import ctypes as C

import denoise_ref as DR
import numpy as np
import pytest
import lumo_amd as L
from lumo_amd import _ffi

pytestmark = pytest.mark.gpu

SEED = 0xDE401500


def film_of(planes):
    """A (Film, FeatureFilm) pair holding a synthetic frame; the Film's splats give add_rgb."""
    rgb_w, albedo_w, normal_w, depth_w, add = planes
    h, w = rgb_w.shape[:2]
    film, feat = L.Film(w, h), L.FeatureFilm(w, h)
    film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w = rgb_w, albedo_w, normal_w, depth_w
    film.splats = film.splats if add is None else add
    return film, feat


def assert_equal_bits(got, want):
    for g, w, name in zip(got, want, ("rgb", "variance")):
        np.testing.assert_array_equal(g.view(np.uint64), w.view(np.uint64), err_msg=name)


# (1, 1): smaller than every footprint; (5, 3): narrower and shorter than a ring; (70, 9): one x seam
# between waves; (67, 70): x and y seams, the step-16 taps inside and outside the image
SIZES = [(1, 1), (5, 3), (70, 9), (67, 70)]
# iterations, demodulate, normal_log2_power, variance_radius, add_rgb
CFGS = [(5, 1, 7, 3, True), (1, 1, 7, 3, False), (5, 0, 0, 1, False), (1, 0, 0, 1, True), (5, 1, 0, 3, False),
        (1, 0, 7, 1, True)]


@pytest.fixture(scope="module")
def dev():
    d = L.Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "N%d-dem%d-k%d-r%d-add%d" % c)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_synthetic_frames(dev, size, cfg):
    planes = DR.frame(*size, seed=size[0])
    film, feat = film_of(planes if cfg[4] else (*planes[:4], None))
    kw = dict(zip(("iterations", "demodulate", "normal_log2_power", "variance_radius"), cfg))
    add = film.splat_scale * film.splats / film.filter_integral() if cfg[4] else None
    want = DR.denoise(film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w, add, **kw)
    assert_equal_bits(dev.denoise(film, feat, return_variance=True, **kw), want)


def test_one_context_three_calls():
    """Large, small, large on a fresh context: the kept work buffers (poisoned when new) serve all."""
    d = L.Device(0)
    try:
        out = [d.denoise(*film_of(DR.frame(w, h, seed=w)), return_variance=True) for w, h in [(67, 70), (5, 3), (67, 70)]]
    finally:
        d.close()
    assert_equal_bits(out[2], out[0])


@pytest.fixture(scope="module")
def cornell():
    r = L.Renderer(L.Scene.cornell_box(), L.Camera.cornell_box((64, 64))).samples(4).seed(SEED)
    return r, r.render_denoised()


def test_render_denoised_is_the_reference_of_its_own_frame(cornell):
    _, (film, feat, den) = cornell
    assert not film.splats.any() and (feat.coverage() > 0.0).any()
    want = DR.denoise(film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w)
    assert_equal_bits((den.rgb(),), want)
    assert den.rgb_image().shape == (64, 64, 3)


def test_the_filter_filters(cornell):
    """Against a 256-spp render of the frame the denoised 4-spp image is closer than the 4-spp one."""
    r, (film, _, den) = cornell
    truth = L.Renderer(r.scene, r.camera).samples(256).seed(SEED + 1).render().rgb()
    rmse = [float(np.sqrt(np.mean((x - truth) ** 2))) for x in (den.rgb(), film.rgb())]
    print("rmse against 256 spp: denoised %.6g, 4 spp %.6g" % tuple(rmse))
    assert rmse[0] < rmse[1]


def test_argument_errors(dev):
    planes = [np.ascontiguousarray(p) for p in DR.frame(5, 3, seed=5)[:4]]
    ptr = [p.ctypes.data_as(_ffi.c_double_p) for p in planes]
    out = np.zeros((3, 5, 3))

    def call(w=5, plane3=ptr[3], **kw):
        cfg = _ffi.DenoiseCfg(**{**_ffi.DENOISE_DEFAULTS, **kw})
        return _ffi.load().lumo_denoise(dev.ctx, C.byref(_ffi.DenoiseIn(w, 3, ptr[0], ptr[1], ptr[2], plane3, None)),
                                C.byref(cfg), out.ctypes.data_as(_ffi.c_double_p), None)

    bad = [dict(iterations=0), dict(iterations=6), dict(normal_log2_power=11), dict(w=0), dict(plane3=None),
           dict(sigma_l=float("nan"))]
    assert [call(**kw) for kw in bad] == [1] * 6 and call() == 0
    assert_equal_bits((out,), DR.denoise(*planes))
