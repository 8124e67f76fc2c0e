"""numpy f64 restatement of lumo_denoise_temporal (include/lumo_amd.h): the same IEEE operations in the
same order as the device, vectorised over pixels, Python loops over taps in row-major order."""
import numpy as np
from denoise_ref import B, G, lm_exp, lum, ratio, tap

from lumo_amd import _ffi


def xf(desc_field, inv, p, w):
    """common/vec.h xf_pt / xf_dir (w = 1 / 0) with the matrix (inv = 0) or its inverse (1) of a lumo_camera_desc field."""
    m = np.array(desc_field[inv][:]).reshape(4, 4)
    x, y, z = (np.asarray(p[..., k], dtype=np.float64) for k in range(3))
    r = [((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] * w for i in range(4)]
    out = np.stack(r[:3], axis=-1)
    return np.where((r[3] == 0.0)[..., None], out, out / r[3][..., None])


def length(a):
    return np.sqrt(np.fmax((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2], 0.0))


def reproject(S, cam, c, n, z, hit):
    """Steps 2-4: (history of e0..2, m1, m2 as H x W x 5, its length, found, what the taps met) from state S."""
    h, w = z.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    zero, d, p = np.zeros((1, 1, 3)), cam.desc, S["cam"].desc
    cpt = xf(d.camera_to_screen, 1, xf(d.screen_to_raster, 1, np.stack([x + 0.5, y + 0.5, 0.0 * x], -1), 1.0), 1.0)
    dr = xf(d.world_to_camera, 1, cpt / length(cpt)[..., None], 0.0)
    P = xf(d.world_to_camera, 1, zero, 1.0) + z[..., None] * (dr / length(dr)[..., None])
    cp = xf(p.world_to_camera, 0, P, 1.0)
    q = xf(p.screen_to_raster, 0, xf(p.camera_to_screen, 0, cp, 1.0), 1.0)
    u, v = q[..., 0] - 0.5, q[..., 1] - 0.5
    cand = hit & (cp[..., 2] > 0.0) & np.isfinite(q[..., 0]) & np.isfinite(q[..., 1])
    cand &= (u >= -2.0) & (u < w + 1.0) & (v >= -2.0) & (v < h + 1.0)
    u, v = np.where(cand, u, 0.0), np.where(cand, v, 0.0)
    zp = length(P - xf(p.world_to_camera, 1, zero, 1.0))
    met = dict(outside=0, miss=0, normal=0, depth=0)

    def gather(taps, on):
        sw, s, best = np.zeros((h, w)), np.zeros((h, w, 5)), np.zeros((h, w), dtype=np.int64)
        for xt, yt, wt in taps:
            inside = (xt >= 0) & (xt < w) & (yt >= 0) & (yt < h)
            yc, xc = np.clip(yt, 0, h - 1), np.clip(xt, 0, w - 1)
            nq = S["n"][yc, xc]
            tests = [inside, S["hit"][yc, xc], (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                     >= c["normal_cos_min"], np.abs(S["z"][yc, xc] - zp) <= c["depth_rel_max"] * zp]
            ok = on
            for name, t in zip(met, tests):  # the first test a tap fails, among the taps the definition evaluates
                met[name] += int((ok & ~t).sum())
                ok = ok & t
            sw = np.where(ok, sw + wt, sw)
            s = np.where(ok[..., None], s + wt[..., None] * S["x"][yc, xc], s)
            best = np.where(ok & (S["len"][yc, xc] > best), S["len"][yc, xc], best)
        return sw, s, best

    fu, fv = np.floor(u), np.floor(v)
    x0, y0, wx, wy = fu.astype(np.int64), fv.astype(np.int64), (1.0 - (u - fu), u - fu), (1.0 - (v - fv), v - fv)
    sw, s, best = gather([(x0 + i, y0 + j, wx[i] * wy[j]) for j in range(2) for i in range(2)], cand)
    cx, cy, one = np.floor(u + 0.5).astype(np.int64), np.floor(v + 0.5).astype(np.int64), np.ones((h, w))
    first = sw > 0.0
    sw9, s9, best9 = gather([(cx + i, cy + j, one) for j in range(-1, 2) for i in range(-1, 2)], cand & ~first)
    found = first | (sw9 > 0.0)
    met["fallback"] = int((~first & found).sum())
    sw, s, best = np.where(first, sw, sw9), np.where(first[..., None], s, s9), np.where(first, best, best9)
    return s / sw[..., None], best, found, met


def denoise_temporal(S, camera, rgb_w, albedo_w, normal_w, depth_w, add_rgb=None, **cfg):
    """One call with history S (None: a first frame): (rgb_out, variance_out, the history after it, counters)."""
    c = {**_ffi.DENOISE_DEFAULTS, **_ffi.TEMPORAL_DEFAULTS, **cfg}
    with np.errstate(all="ignore"):
        # 1 prepare (as denoise_ref.denoise)
        col = ratio(rgb_w[..., :3], rgb_w[..., 3:4])
        col = col if add_rgb is None else col + add_rgb
        cov, z = ratio(depth_w[..., 1], depth_w[..., 3]), ratio(depth_w[..., 0], depth_w[..., 1])
        hit = cov > 0.0
        nx, ny, nz = (normal_w[..., k] for k in range(3))
        n = ratio(normal_w[..., :3], np.sqrt((nx * nx + ny * ny) + nz * nz)[..., None])
        div = ratio(albedo_w[..., :3], albedo_w[..., 3:4]) + (1.0 - cov)[..., None]
        div = np.where(div > c["albedo_floor"], div, c["albedo_floor"]) if c["demodulate"] else np.ones_like(col)
        e = col / div
        ax, ay = np.abs(tap(z, 1, 0, True)[0] - z), np.abs(tap(z, 0, 1, True)[0] - z)
        za, zb = c["sigma_z"] * np.where(ax > ay, ax, ay), c["depth_floor"] * z
        # 2-5 reproject and accumulate
        l = lum(e)
        x, N, found, met = np.concatenate([e, l[..., None], (l * l)[..., None]], -1), np.ones(l.shape, dtype=np.int64), hit & False, {}
        if S is not None and S["z"].shape == z.shape:
            hist, best, found, met = reproject(S, camera, c, n, z, hit)
            N = np.where(found, np.minimum(best + 1, c["max_history"]), 1)
            a = np.where(c["alpha"] > 1.0 / N, c["alpha"], 1.0 / N)[..., None]
            x = np.where(found[..., None], (1.0 - a) * hist + a * x, x)
        e = x[..., :3]

        def pair(ox, oy):
            (nq, ok), zq, hq = tap(n, ox, oy), tap(z, ox, oy)[0], tap(hit, ox, oy)[0]
            d = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
            d = np.where(d > 0.0, d, 0.0)
            for _ in range(c["normal_log2_power"]):
                d = d * d
            dz = np.abs(z - zq) / (za * np.sqrt(float(ox) * float(ox) + float(oy) * float(oy)) + zb)
            return np.where(hit | hq, d, 1.0), np.where(hit | hq, dz, 0.0), ok & (hit == hq)

        falloff = lambda m: lm_exp(-np.where(m < 700.0, m, 700.0))  # noqa: E731
        # 6 variance: spatial from the luminance of e_acc, temporal where the history is long enough
        l, r = lum(e), c["variance_radius"]
        sw, s1, s2 = (np.zeros_like(l) for _ in range(3))
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                wn, dz, ok = pair(dx, dy)
                wt = np.where(ok, 1.0 if dx == dy == 0 else wn * falloff(dz), 0.0)
                lq = np.where(ok, tap(l, dx, dy)[0], 0.0)
                sw, s1, s2 = sw + wt, s1 + wt * lq, s2 + wt * (lq * lq)
        m1, m2 = s1 / sw, s2 / sw
        v = np.where(N >= c["min_history"], x[..., 4] - x[..., 3] * x[..., 3], m2 - m1 * m1)
        var = np.where(v > 0.0, v, 0.0)
        # 7 a-trous with the feedback tap, finish
        fed = e
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
                    b = B[dy + 2] * B[dx + 2]
                    dl = np.abs(l - tap(l, s * dx, s * dy)[0]) / lden
                    wt = np.full_like(l, b) if dx == dy == 0 else np.where(ok, (b * wn) * falloff(dz + dl), 0.0)
                    eq = np.where(ok[..., None], tap(e, s * dx, s * dy)[0], 0.0)
                    vq = np.where(ok, tap(var, s * dx, s * dy)[0], 0.0)
                    sw, se, sv = sw + wt, se + wt[..., None] * eq, sv + (wt * wt) * vq
            e, var = se / sw[..., None], sv / (sw * sw)
            fed = e if i + 1 == c["feedback"] else fed
        S = dict(x=np.concatenate([fed, x[..., 3:]], -1), len=N, n=n, z=z, hit=hit, cam=camera)
        met.update(with_history=int(found.sum()), without_history=int((~found).sum()))
        return e * div, var, S, met
