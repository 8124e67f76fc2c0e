"""lumo_denoise_temporal against tests/denoise_temporal_ref.py: equal bits for rgb, variance and the history counts."""
import ctypes as C
import math

import denoise_ref as DR
import denoise_temporal_ref as TR
import numpy as np
import pytest
from test_gpu_denoise import assert_equal_bits, dev, film_of  # noqa: F401 (dev: the module's context fixture)

import lumo_amd as L
from lumo_amd import _ffi

pytestmark = pytest.mark.gpu

# (5, 3): smaller than a block; (70, 9): one seam in x, no box outgrows the tile; (67, 70): seams in x and y
SIZES = [(5, 3), (70, 9), (67, 70)]
# A block's box is clipped to the image, so an image of at most 768 pixels (device/denoise_temporal.h DT_CAP) is always
# staged: the least number of direct blocks under the roll, per size.  (96, 80), 3 x 10 blocks, is there for several.
MOVING = {(5, 3): 0, (70, 9): 0, (67, 70): 1, (96, 80): 2}


def camera(size, yaw=0.0, roll=0.0, shift=0.0):
    """Cornell's camera moved by `shift` along x, turned by `yaw` about y and rolled about its axis (radians)."""
    o = (278.0 + shift, 273.0, -800.0)
    b = L.Camera.cornell_box_builder().resolution(size).origin(*o)
    return b.towards(o[0] + 800.0 * math.sin(yaw), o[1], o[2] + 800.0 * math.cos(yaw)).up(math.sin(roll), math.cos(roll), 0.0).build()


def frame(size, k):
    """Frame k of a sequence: DR.frame with its own noise; odd frames have another depth in the lower left, so
    reprojection loses the history there."""
    planes = DR.frame(*size, seed=size[0] + 7 * k)
    if k % 2:
        planes[3][size[1] // 2:, :size[0] // 4, 0] *= 1.5
    return planes


def run(dev, size, cameras, **cfg):
    """The sequence on the device and in the reference, every frame compared; the reference's (state, counters) per
    frame and the device's info."""
    dev.denoise_reset()
    S, out = None, []
    for k, cam in enumerate(cameras):
        planes, info = frame(size, k), {}
        film, feat = film_of(planes)
        add = film.splat_scale * film.splats / film.filter_integral()
        *want, S, met = TR.denoise_temporal(S, cam, film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w, add, **cfg)
        got = dev.denoise_temporal(film, feat, cam, return_variance=True, info=info, **cfg)
        assert_equal_bits(got, want)
        assert (info["with_history"], info["without_history"]) == (met["with_history"], met["without_history"]), k
        out.append((S, met, info))
    return out


def test_first_frame():
    """A fresh context, a reset one and one whose frame size changed give Device.denoise's bits."""
    d = L.Device(0)

    def call(size, first):
        film, feat, info = *film_of(frame(size, 0)), {}
        got = d.denoise_temporal(film, feat, camera(size), return_variance=True, info=info)
        assert (info["with_history"] == 0) == first
        if first:
            assert_equal_bits(got, d.denoise(film, feat, return_variance=True))

    try:
        for _ in range(2):  # a fresh context, then a reset one
            call((67, 70), True)
            call((67, 70), False)
            d.denoise_reset()
        call((67, 70), True)
        call((70, 9), True)
    finally:
        d.close()


# feedback, alpha, max_history
STATIC = [(0, 0.2, 32), (1, 0.2, 32), (5, 0.2, 32), (1, 0.5, 3), (2, 0.0, 32)]


@pytest.mark.parametrize("cfg", STATIC, ids=lambda c: "fb%d-a%g-max%d" % c)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_static_camera(dev, size, cfg):
    kw = dict(zip(("feedback", "alpha", "max_history"), cfg))
    out = run(dev, size, [camera(size)] * 6, **kw)
    assert [int(S["len"].max()) for S, _, _ in out] == [min(k + 1, cfg[2]) for k in range(6)]
    assert out[0][1]["with_history"] == 0 < out[5][1]["with_history"] and out[5][1]["without_history"] > 0
    long = out[5][0]["len"] >= _ffi.TEMPORAL_DEFAULTS["min_history"]  # the temporal variance took over there
    assert long.any() == (cfg[2] >= 4) and not long.all()


@pytest.mark.parametrize("stage_lds", [1, 0])
@pytest.mark.parametrize("size", MOVING, ids=lambda s: "%dx%d" % s)
def test_moving_camera(dev, size, stage_lds):
    """Still, a pan of a pixel or two, a roll of 0.8 rad, then the camera turned away."""
    cams = [camera(size), camera(size, yaw=2e-3 * 64 / size[0], shift=0.02), camera(size, yaw=2e-3 * 64 / size[0], roll=0.8),
            camera(size, yaw=math.pi)]
    (_, _, i0), (_, pan, i1), (_, rolled, i2), (_, away, i3) = run(dev, size, cams, stage_lds=stage_lds)
    for met in (pan, rolled):
        assert 0 < met["with_history"] and 0 < met["without_history"]
    seen = {k: pan[k] + rolled[k] for k in ("outside", "miss", "normal", "depth", "fallback")}
    assert all(seen.values()), seen
    assert away["with_history"] == 0 and i3["with_history"] == 0
    if stage_lds:
        assert i1["blocks_staged"] > 0 and i1["blocks_direct"] == 0
        assert i2["blocks_direct"] >= MOVING[size] and (MOVING[size] or i2["blocks_direct"] == 0)
    else:
        assert [i["blocks_staged"] for i in (i0, i1, i2, i3)] == [0] * 4 and i1["blocks_direct"] > 0


def test_render_denoised_sequence():
    """Frame k is render_denoised's frame of seed + k with camera k, denoised on one context with frames 0 .. k - 1 as
    history; the renderer's own seed and camera are as before afterwards."""
    size, seed, S = (16, 16), 0xDE401600, None
    cams = [camera(size), camera(size, yaw=2e-3)]
    r = L.Renderer(L.Scene.cornell_box(), cams[0]).samples(2).seed(seed)
    for k, (film, feat, den) in enumerate(r.render_denoised_sequence(cams, iterations=2)):
        alone = L.Renderer(r.scene, cams[k]).samples(2).seed(seed + k).render_denoised(iterations=2)
        assert (film.pixels == alone[0].pixels).all() and (feat.depth_w == alone[1].depth_w).all()
        want, _, S, met = TR.denoise_temporal(S, cams[k], film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w, iterations=2)
        assert_equal_bits((den.rgb(),), (want,))
        assert (met["with_history"] > 0) == (k == 1) and (k == 0) == (den.rgb() == alone[2].rgb()).all()
    assert k == 1 and r._seed == seed and r.camera is cams[0]


def test_argument_errors(dev):
    planes = [np.ascontiguousarray(p) for p in DR.frame(5, 3, seed=5)[:4]]
    ptr = [p.ctypes.data_as(_ffi.c_double_p) for p in planes]
    out = np.zeros((3, 5, 3))
    ortho = L.Camera.cornell_box_builder().resolution((5, 3)).camera_type(L.CameraType.Orthographic).build()

    def call(cam=camera((5, 3)), iterations=5, **kw):
        cfg = _ffi.DenoiseCfg(**{**_ffi.DENOISE_DEFAULTS, "iterations": iterations})
        t = _ffi.TemporalCfg(**{**_ffi.TEMPORAL_DEFAULTS, **kw})
        return _ffi.load().lumo_denoise_temporal(dev.ctx, C.byref(_ffi.DenoiseIn(5, 3, *ptr, None)),
                                                 cam and C.byref(cam.desc), C.byref(cfg), C.byref(t),
                                                 out.ctypes.data_as(_ffi.c_double_p), None, None)

    bad = [dict(cam=None), dict(cam=camera((3, 5))), dict(alpha=-0.1), dict(alpha=1.5), dict(max_history=0),
           dict(max_history=1025), dict(min_history=0), dict(normal_cos_min=1.5), dict(depth_rel_max=-1.0),
           dict(feedback=-1), dict(feedback=3, iterations=2), dict(stage_lds=2), dict(alpha=float("nan")),
           dict(depth_rel_max=float("inf")), dict(iterations=0)]
    assert [call(**kw) for kw in bad] == [1] * len(bad) and call(cam=ortho) == 6
    assert dev.denoise_reset() is None and call() == 0 and _ffi.load().lumo_denoise_reset(None) == 1
    assert_equal_bits((out,), DR.denoise(*planes))
