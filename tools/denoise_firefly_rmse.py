#!/usr/bin/env python3
"""Does the firefly clamp cure DESIGN.md §4e's table?  That table again, with two more columns.

Cornell 64 x 64 at 4 spp, a static camera, 8 frames with render_denoised_sequence's seeds (seed + k),
RMSE of the linear RGB against a 256-spp render of seed + 8: the temporal filter, the spatial filter
of each frame alone and the 4-spp input, then the same two filters behind the clamp at its defaults.

    python tools/denoise_firefly_rmse.py --render frames.npz   an MI355X: the frames, their feature planes, the
                                                               256-spp render; prints the device's own figures
    python tools/denoise_firefly_rmse.py --table frames.npz    no GPU: the numpy references of tests/ on those
                                                               inputs, a markdown table; [--firefly rank=3 ...]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import lumo_amd as L  # noqa: E402

SEED, FRAMES, SIZE = 0xDE401500, 8, (64, 64)
PLANES = ("rgb_w", "albedo_w", "normal_w", "depth_w")


def rmse(x, truth, keep=None):
    d = (x - truth) ** 2
    return float(np.sqrt(np.mean(d if keep is None else d[keep])))


def render(path, seed):
    cam = L.Camera.cornell_box(SIZE)
    r = L.Renderer(L.Scene.cornell_box(), cam).samples(4).seed(seed)
    truth = L.Renderer(r.scene, cam).samples(256).seed(seed + FRAMES).render().rgb()
    out = {name: [] for name in PLANES}
    for firefly in (None, {}):
        print("device, firefly =", firefly)
        for k, (film, feat, den) in enumerate(r.render_denoised_sequence([cam] * FRAMES, firefly=firefly)):
            alone = L.Device(0)
            alone.set_firefly(firefly)
            spatial = alone.denoise(film, feat)
            alone.close()
            print("  frame %d: temporal %.6f spatial %.6f input %.6f" % (k + 1, rmse(den.rgb(), truth), rmse(spatial, truth),
                                                                      rmse(film.rgb(), truth)))
            if firefly is None:
                for name, a in zip(PLANES, (film.pixels, feat.albedo_w, feat.normal_w, feat.depth_w)):
                    out[name].append(a)
    np.savez_compressed(path, truth=truth, **{k: np.stack(v) for k, v in out.items()})


def table(path, firefly, below):
    import denoise_firefly_ref as FR
    import denoise_ref as DR
    import denoise_temporal_ref as TR
    d, cam = np.load(path), L.Camera.cornell_box(SIZE)
    S = S1 = keep = None
    if below is not None:  # without the pixels within 2 of one the 256-spp render has brighter than `below`: the emitter
        bright = np.pad(d["truth"].max(-1) > below, 2)
        keep = ~np.any([bright[2 + dy:2 + dy + SIZE[1], 2 + dx:2 + dx + SIZE[0]] for dy in range(-2, 3) for dx in range(-2, 3)], 0)
        print("%d of %d pixels kept" % (keep.sum(), keep.size))
    print("| frame | temporal | spatial | 4-spp input | temporal + clamp | spatial + clamp | pixels clamped |\n|---|---|---|---|---|---|---|")
    for k in range(FRAMES):
        planes = [d[name][k] for name in PLANES]
        c1, count = FR.clamp(*planes, firefly=firefly)
        clamped = [FR.frame_of(c1), *planes[1:]]
        temporal, _, S, _ = TR.denoise_temporal(S, cam, *planes)
        temporal1, _, S1, _ = TR.denoise_temporal(S1, cam, *clamped)
        row = [temporal, DR.denoise(*planes)[0], DR.ratio(planes[0][..., :3], planes[0][..., 3:4]), temporal1,
               DR.denoise(*clamped)[0]]
        print("| %d | " % (k + 1) + " | ".join("%.6f" % rmse(x, d["truth"], keep) for x in row) + " | %d |" % count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--render", metavar="NPZ")
    ap.add_argument("--table", metavar="NPZ")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=SEED)
    ap.add_argument("--below", type=float, help="--table: leave out the pixels around those the 256-spp render has above this")
    ap.add_argument("--firefly", nargs="*", default=[], help="lumo_firefly_cfg fields over the defaults, as name=value")
    a = ap.parse_args()
    if a.render:
        render(a.render, a.seed)
    if a.table:
        table(a.table, {k: float(v) if "." in v else int(v) for k, v in (f.split("=") for f in a.firefly)}, a.below)


if __name__ == "__main__":
    main()
