"""numpy f64 restatement of the denoiser's firefly clamp (step 1b; include/lumo_amd.h): step 1's values
as denoise_ref.denoise computes them, the window's taps stacked with -inf where a tap is not alike, the order statistic
by np.sort.  The whole filter with the clamp is then the unchanged reference on the frame (c', 1) without add_rgb."""
import numpy as np
from denoise_ref import lum, ratio, tap

from lumo_amd import _ffi


def clamp(rgb_w, albedo_w, normal_w, depth_w, add_rgb=None, firefly=None, **cfg):
    """(c' H x W x 3, the number of pixels clamped); firefly: fields over FIREFLY_DEFAULTS, cfg: lumo_denoise_cfg's."""
    c, f = {**_ffi.DENOISE_DEFAULTS, **cfg}, {**_ffi.FIREFLY_DEFAULTS, **(firefly or {})}
    with np.errstate(all="ignore"):
        col = ratio(rgb_w[..., :3], rgb_w[..., 3:4])
        col = col if add_rgb is None else col + add_rgb
        cov, z = ratio(depth_w[..., 1], depth_w[..., 3]), ratio(depth_w[..., 0], depth_w[..., 1])
        hit = cov > 0.0
        nx, ny, nz = (normal_w[..., k] for k in range(3))
        n = ratio(normal_w[..., :3], np.sqrt((nx * nx + ny * ny) + nz * nz)[..., None])
        div = ratio(albedo_w[..., :3], albedo_w[..., 3:4]) + (1.0 - cov)[..., None]
        div = np.where(div > c["albedo_floor"], div, c["albedo_floor"]) if c["demodulate"] else np.ones_like(col)
        l, r = lum(col / div), f["radius"]
        taps, m = [], np.zeros(l.shape, dtype=np.int64)
        for dy, dx in ((dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx or dy):
            (nq, ok), zq, hq = tap(n, dx, dy), tap(z, dx, dy)[0], tap(hit, dx, dy)[0]
            d = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
            alike = ok & hq & (d >= f["normal_cos_min"]) & (np.abs(zq - z) <= f["depth_rel_max"] * z)
            taps.append(np.where(alike, tap(l, dx, dy)[0], -np.inf))
            m += alike
        b = f["gain"] * np.sort(np.stack(taps, -1), -1)[..., -f["rank"]]
        over = hit & (m >= f["min_alike"]) & (l > b)
        return col * np.where(over, b / l, 1.0)[..., None], int(over.sum())


def frame_of(c1):
    """The rgb_w of the frame (c', 1)."""
    return np.concatenate([c1, np.ones_like(c1[..., :1])], -1)
