"""numpy f64 restatement of lumo_denoise (include/lumo_amd.h): the same IEEE operations in the same
order, vectorised over pixels, a Python loop over taps in row-major order, exp from the library's lm_exp."""
import numpy as np

from lumo_amd import _ffi

B, G = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0), (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)


def lm_exp(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    _ffi.load().lumo_lmath(0, x.ctypes.data_as(_ffi.c_double_p), y.ctypes.data_as(_ffi.c_double_p), x.size)
    return y


def ratio(a, b):
    out = np.zeros(np.broadcast(a, b).shape)
    return np.divide(a, b, out=out, where=np.broadcast_to(b != 0.0, out.shape))


def lum(e):
    return (0.2126 * e[..., 0] + 0.7152 * e[..., 1]) + 0.0722 * e[..., 2]


def tap(a, ox, oy, clamped=False):
    """`a` at pixel offset (ox, oy) and where that pixel is in the image (all of it when clamped)."""
    h, w = a.shape[:2]
    ys, xs = np.arange(h) + oy, np.arange(w) + ox
    ok = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    q = a[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
    return q, (np.ones_like(ok) if clamped else ok)


def denoise(rgb_w, albedo_w, normal_w, depth_w, add_rgb=None, **cfg):
    """(rgb_out H x W x 3, variance_out H x W)."""
    c = {**_ffi.DENOISE_DEFAULTS, **cfg}
    with np.errstate(all="ignore"):
        # 1 prepare
        col = ratio(rgb_w[..., :3], rgb_w[..., 3:4])
        col = col if add_rgb is None else col + add_rgb
        cov = ratio(depth_w[..., 1], depth_w[..., 3])
        z = ratio(depth_w[..., 0], depth_w[..., 1])
        hit = cov > 0.0
        nx, ny, nz = (normal_w[..., k] for k in range(3))
        n = ratio(normal_w[..., :3], np.sqrt((nx * nx + ny * ny) + nz * nz)[..., None])
        a = ratio(albedo_w[..., :3], albedo_w[..., 3:4])
        div = a + (1.0 - cov)[..., None]
        div = np.where(div > c["albedo_floor"], div, c["albedo_floor"]) if c["demodulate"] else np.ones_like(a)
        e = col / div
        ax, ay = np.abs(tap(z, 1, 0, True)[0] - z), np.abs(tap(z, 0, 1, True)[0] - z)
        fz = np.where(ax > ay, ax, ay)
        za, zb = c["sigma_z"] * fz, c["depth_floor"] * z

        def pair(ox, oy):
            """2: (wn, dz, in the image and not a hit paired with a miss) of the tap at (ox, oy)."""
            (nq, ok), zq, hq = tap(n, ox, oy), tap(z, ox, oy)[0], tap(hit, ox, oy)[0]
            d = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
            d = np.where(d > 0.0, d, 0.0)
            for _ in range(c["normal_log2_power"]):
                d = d * d
            dz = np.abs(z - zq) / (za * np.sqrt(float(ox) * float(ox) + float(oy) * float(oy)) + zb)
            both = hit | hq
            return np.where(both, d, 1.0), np.where(both, dz, 0.0), ok & (hit == hq)

        falloff = lambda m: lm_exp(-np.where(m < 700.0, m, 700.0))  # noqa: E731

        # 3 variance
        l, r = lum(e), c["variance_radius"]
        sw, s1, s2 = (np.zeros_like(l) for _ in range(3))
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                wn, dz, ok = pair(dx, dy)
                w = np.where(ok, 1.0 if dx == dy == 0 else wn * falloff(dz), 0.0)
                lq = np.where(ok, tap(l, dx, dy)[0], 0.0)
                sw, s1, s2 = sw + w, s1 + w * lq, s2 + w * (lq * lq)
        m1, m2 = s1 / sw, s2 / sw
        var = np.where(m2 - m1 * m1 > 0.0, m2 - m1 * m1, 0.0)
        # 4 a-trous
        for i in range(c["iterations"]):
            s, l = 1 << i, lum(e)
            gv = np.zeros_like(var)
            for dy, dx in ((dy, dx) for dy in range(-1, 2) for dx in range(-1, 2)):
                gv = gv + (G[dy + 1] * G[dx + 1]) * tap(var, dx, dy, True)[0]
            lden = c["sigma_l"] * np.sqrt(gv) + c["lum_floor"]
            sw, sv, se = np.zeros_like(l), np.zeros_like(l), np.zeros_like(e)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    wn, dz, ok = pair(s * dx, s * dy)
                    h = B[dy + 2] * B[dx + 2]
                    dl = np.abs(l - tap(l, s * dx, s * dy)[0]) / lden
                    w = np.full_like(l, h) if dx == dy == 0 else np.where(ok, (h * wn) * falloff(dz + dl), 0.0)
                    eq = np.where(ok[..., None], tap(e, s * dx, s * dy)[0], 0.0)
                    vq = np.where(ok, tap(var, s * dx, s * dy)[0], 0.0)
                    sw, se, sv = sw + w, se + w[..., None] * eq, sv + (w * w) * vq
            e, var = se / sw[..., None], sv / (sw * sw)
        # 5 finish
        return e * div, var


def frame(w, h, seed):
    """(rgb_w, albedo_w, normal_w, depth_w, add_rgb): two slanted planes meeting at a depth and normal edge, a block
    of misses, a column of partial coverage, a few zero-albedo pixels, one pixel without weight, noisy colour."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    left = x < 0.55 * w
    sw = rng.uniform(0.5, 2.0, (h, w))
    cov = np.ones((h, w))
    cov[h // 3:h // 3 + max(1, h // 4), (2 * w) // 3:(2 * w) // 3 + max(1, w // 5)] = 0.0  # misses
    cov[:, w // 4] = rng.uniform(0.2, 0.8, h)                                            # a silhouette
    depth = np.where(left, 3.0 + 0.02 * x + 0.01 * y, 5.0 - 0.015 * x + 0.03 * y)
    nrm = np.where(left[..., None], (0.6, 0.0, 0.8), (-0.28, 0.0, 0.96)) * rng.uniform(0.9, 1.0, (h, w, 1))
    alb = np.where(left[..., None], (0.7, 0.3, 0.2), (0.2, 0.5, 0.8)) * np.ones((h, w, 1))
    alb[rng.integers(0, h, 3), rng.integers(0, w, 3)] = 0.0
    col = alb * rng.gamma(2.0, 0.5, (h, w, 3)) + (1.0 - cov)[..., None] * 0.3
    c3 = cov[..., None]
    planes = [np.concatenate([v * sw[..., None], sw[..., None]], axis=-1) for v in (col, alb * c3, nrm * c3)]
    planes.append(np.stack([depth * cov * sw, cov * sw, np.zeros((h, w)), sw], axis=-1))
    for p in planes:
        p[h // 2, w // 2] = 0.0  # no sample reached this pixel
    return (*planes, rng.uniform(0.0, 0.1, (h, w, 3)))
