"""lumo_denoise_temporal_motion against tests/denoise_motion_ref.py on synthetic frames: equal bits for rgb, variance
and the history counts; without a plane, and with an all-zero one, lumo_denoise_temporal's bits."""
import denoise_motion_ref as MR
import denoise_temporal_ref as TR
import numpy as np
import pytest
from test_gpu_denoise import assert_equal_bits, dev, film_of  # noqa: F401 (dev: the module's context fixture)
from test_gpu_denoise_temporal import SIZES, camera, frame

pytestmark = pytest.mark.gpu


def motion_plane(size, depth_w, cam):
    """motion_w of a constant world-space vector, three pixel widths at depth 4 along x, on the left half's hits."""
    w, h = size
    c = [TR.xf(cam.desc.camera_to_screen, 1, TR.xf(cam.desc.screen_to_raster, 1, np.array([[w / 2 + k, h / 2, 0.0]]), 1.0), 1.0)
         for k in (0, 1)]
    m = np.zeros((h, w, 4))
    m[:, :w // 2, 0] = 3.0 * 4.0 * abs(float(c[1][0, 0] / TR.length(c[1])[0] - c[0][0, 0] / TR.length(c[0])[0]))
    m[..., :3] *= depth_w[..., 1:2]
    m[..., 3] = depth_w[..., 3]
    return m


@pytest.mark.parametrize("stage_lds", [1, 0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_motion_frames(dev, size, stage_lds):
    """Four frames under a slow pan: the plane's sequence against the motion reference; no plane and a zero plane
    against denoise_temporal_ref itself."""
    cams = [camera(size, yaw=1e-3 * k * 64 / size[0]) for k in range(4)]
    outs = {}
    for how in ("plane", "none", "zero"):
        dev.denoise_reset()
        S, outs[how] = None, []
        for k, cam in enumerate(cams):
            film, feat = film_of(frame(size, k))
            args, info = (cam, film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w), {}
            add = film.splat_scale * film.splats / film.filter_integral()
            mot = motion_plane(size, feat.depth_w, cam)
            if how == "plane":
                *want, S, met = MR.denoise_temporal(S, *args, mot, add, stage_lds=stage_lds)
            else:
                *want, S, met = TR.denoise_temporal(S, *args, add, stage_lds=stage_lds)
                mot = None if how == "none" else 0.0 * mot
            got = dev.denoise_temporal(film, feat, cam, return_variance=True, info=info, motion=mot, stage_lds=stage_lds)
            assert_equal_bits(got, want)
            assert (info["with_history"], info["without_history"]) == (met["with_history"], met["without_history"]), (how, k)
            outs[how].append((want[0], met))
    assert outs["plane"][2][1]["with_history"] > 0 and outs["plane"][2][1]["without_history"] > 0
    assert any((a != b).any() for (a, _), (b, _) in zip(outs["plane"], outs["none"]))  # the plane moved something
