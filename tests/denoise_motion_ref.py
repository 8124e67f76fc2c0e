"""numpy f64 restatement of what the motion feature adds (include/lumo_amd.h "Motion"): the per-sample
delta from the dumped barycentrics, and steps 1 to 3 of lumo_denoise_temporal_motion.  The same IEEE operations in the
same order as the device; everything else is denoise_temporal_ref's."""
import denoise_temporal_ref as TR
import numpy as np
from denoise_ref import ratio


def point(bary, tri):
    """(bary.x A + bary.y B) + bary.z C per component: bary (n, 3), tri (n, 3 corners, 3)."""
    return (bary[:, 0, None] * tri[:, 0] + bary[:, 1, None] * tri[:, 1]) + bary[:, 2, None] * tri[:, 2]


def through(m, v, w):
    """xf_apply: (n, 3) vectors through the row-major 4 x 4 m with fourth component w, divided by the result's unless 0."""
    r = [((m[i, 0] * v[:, 0] + m[i, 1] * v[:, 1]) + m[i, 2] * v[:, 2]) + m[i, 3] * w for i in range(4)]
    with np.errstate(all="ignore"):
        return np.where((r[3] == 0.0)[:, None], np.stack(r[:3], -1), np.stack(r[:3], -1) / r[3][:, None])


def delta(bary, now, before, m=None):
    """The sample's delta: point(before) - point(now), an instance's through its m as a direction."""
    d = point(bary, before) - point(bary, now)
    return d if m is None else through(m, d, 0.0)


def reproject(S, cam, c, n, z, hit, m):
    """TR.reproject with P' = P + m: steps 2 and 3 restated, step 4 as there (without its bookkeeping)."""
    h, w = z.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    zero, d, p, xf, length = np.zeros((1, 1, 3)), cam.desc, S["cam"].desc, TR.xf, TR.length
    cpt = xf(d.camera_to_screen, 1, xf(d.screen_to_raster, 1, np.stack([x + 0.5, y + 0.5, 0.0 * x], -1), 1.0), 1.0)
    dr = xf(d.world_to_camera, 1, cpt / length(cpt)[..., None], 0.0)
    P = (xf(d.world_to_camera, 1, zero, 1.0) + z[..., None] * (dr / length(dr)[..., None])) + m
    cp = xf(p.world_to_camera, 0, P, 1.0)
    q = xf(p.screen_to_raster, 0, xf(p.camera_to_screen, 0, cp, 1.0), 1.0)
    u, v = q[..., 0] - 0.5, q[..., 1] - 0.5
    cand = hit & (cp[..., 2] > 0.0) & np.isfinite(q[..., 0]) & np.isfinite(q[..., 1])
    cand &= (u >= -2.0) & (u < w + 1.0) & (v >= -2.0) & (v < h + 1.0)
    u, v = np.where(cand, u, 0.0), np.where(cand, v, 0.0)
    zp = length(P - xf(p.world_to_camera, 1, zero, 1.0))

    def gather(taps, on):
        sw, s, best = np.zeros((h, w)), np.zeros((h, w, 5)), np.zeros((h, w), dtype=np.int64)
        for xt, yt, wt in taps:
            yc, xc = np.clip(yt, 0, h - 1), np.clip(xt, 0, w - 1)
            nq = S["n"][yc, xc]
            ok = on & (xt >= 0) & (xt < w) & (yt >= 0) & (yt < h) & S["hit"][yc, xc]
            ok &= (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2] >= c["normal_cos_min"]
            ok &= np.abs(S["z"][yc, xc] - zp) <= c["depth_rel_max"] * zp
            sw, s = np.where(ok, sw + wt, sw), np.where(ok[..., None], s + wt[..., None] * S["x"][yc, xc], s)
            best = np.where(ok & (S["len"][yc, xc] > best), S["len"][yc, xc], best)
        return sw, s, best

    fu, fv = np.floor(u), np.floor(v)
    x0, y0, wx, wy = fu.astype(np.int64), fv.astype(np.int64), (1.0 - (u - fu), u - fu), (1.0 - (v - fv), v - fv)
    sw, s, best = gather([(x0 + i, y0 + j, wx[i] * wy[j]) for j in range(2) for i in range(2)], cand)
    cx, cy, one = np.floor(u + 0.5).astype(np.int64), np.floor(v + 0.5).astype(np.int64), np.ones((h, w))
    first = sw > 0.0
    sw9, s9, best9 = gather([(cx + i, cy + j, one) for j in range(-1, 2) for i in range(-1, 2)], cand & ~first)
    sw, s, best = np.where(first, sw, sw9), np.where(first[..., None], s, s9), np.where(first, best, best9)
    return s / sw[..., None], best, first | (sw9 > 0.0), {}


def denoise_temporal(S, camera, rgb_w, albedo_w, normal_w, depth_w, motion_w, add_rgb=None, **cfg):
    """TR.denoise_temporal with the motion plane: step 1's m, then its own steps with the reprojection above."""
    with np.errstate(all="ignore"):
        m = ratio(motion_w[..., :3], depth_w[..., 1:2])
    plain, TR.reproject = TR.reproject, lambda *a: reproject(*a, m)
    try:
        return TR.denoise_temporal(S, camera, rgb_w, albedo_w, normal_w, depth_w, add_rgb, **cfg)
    finally:
        TR.reproject = plain
