#!/usr/bin/env python3
"""Time of Device.denoise on whole frames, with the defaults.

Per frame size (1024 x 1024 and 1920 x 1080): lumo's Cornell box at `--spp` as beauty and features
on one context, then the denoiser on that frame: the host-clock time of a call (it ends in a
synchronise), median of `--repeats` after a warm-up call, and one more call's split by HIP events
(lumo_denoise_cfg.stage_ms) into the upload, each kernel and the read-back.  Needs an MI355X.

    python tools/denoise_time.py [--spp 4] [--repeats 3]  ->  one JSON line per frame size"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import lumo_amd as L  # noqa: E402

SEED = 0x5EED1234


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    scene = L.Scene.cornell_box().build()
    for w, h in ((1024, 1024), (1920, 1080)):
        cam = L.Camera.cornell_box((w, h))
        dev = L.Device(0)
        dev.upload(scene, cam)
        tasks = L.make_tasks(w, h, a.spp, SEED)
        film, feat = L.Film(w, h, samples=a.spp), L.FeatureFilm(w, h)
        for t, b in zip(tasks, dev.render_tasks(tasks)[0]):
            film.add_tile(t, b)
        for t, p in zip(tasks, dev.render_features(tasks)):
            feat.add_tile(t, p)
        dev.denoise(film, feat)
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            dev.denoise(film, feat)
            ms.append((time.perf_counter() - t0) * 1e3)
        stages = []
        dev.denoise(film, feat, stage_ms=stages)
        dev.close()
        names = ["upload", "prepare", "variance"] + [f"atrous_s{1 << i}" for i in range(len(stages) - 5)] + \
                ["finish", "readback"]
        print(json.dumps({"frame": f"cornell {w}x{h}", "spp": a.spp, "call_ms": round(statistics.median(ms), 2),
                          "calls_ms": [round(x, 2) for x in ms],
                          "stage_ms": {k: round(v, 3) for k, v in zip(names, stages)}}))


if __name__ == "__main__":
    main()
