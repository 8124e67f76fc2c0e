#!/usr/bin/env python3
"""Time of the denoiser's firefly clamp on whole frames, at its defaults, beside k_dn_variance.

Per frame size (1024 x 1024 and 1920 x 1080): lumo's Cornell box at `--spp` as beauty and features on
one context, the clamp set, a warm-up call of Device.denoise, then `--repeats` calls: of each the
step's device time (lumo_firefly_info.ms: k_dn_firefly and k_dn_firefly_apply by HIP events) and
k_dn_variance's from the same call's stage_ms (it shares the staging shape); the medians, and the
host-clock time of the call with the clamp and, in the same run, without it.  Needs an MI355X.

    python tools/denoise_firefly_time.py [--spp 4] [--repeats 3]  ->  one JSON line per frame size"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import lumo_amd as L  # noqa: E402

SEED = 0x5EED1234
VARIANCE = 2  # stage_ms: upload, prepare (with the clamp when set), variance, ...


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
        out = {"frame": f"cornell {w}x{h}", "spp": a.spp}
        for name, firefly in (("off", None), ("on", {})):
            dev.set_firefly(firefly)
            dev.denoise(film, feat)
            calls, step, variance, prepare = [], [], [], []
            for _ in range(a.repeats):
                stages = []
                t0 = time.perf_counter()
                dev.denoise(film, feat, stage_ms=stages)
                calls.append((time.perf_counter() - t0) * 1e3)
                step.append(dev.firefly_info()["ms"])
                variance.append(stages[VARIANCE])
                prepare.append(stages[VARIANCE - 1])
            out[name] = {"call_ms": round(statistics.median(calls), 2), "calls_ms": [round(x, 2) for x in calls],
                         "firefly_ms": round(statistics.median(step), 3), "firefly_calls_ms": [round(x, 3) for x in step],
                         "variance_ms": round(statistics.median(variance), 3), "variance_calls_ms": [round(x, 3) for x in variance],
                         "prepare_interval_ms": round(statistics.median(prepare), 3), "clamped": dev.firefly_info()["clamped"]}
        dev.close()
        print(json.dumps(out))


if __name__ == "__main__":
    main()
