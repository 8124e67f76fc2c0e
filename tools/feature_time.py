#!/usr/bin/env python3
"""Time of a feature pass beside a beauty pass of the same frame, on one context.

C1's frame (lumo's Cornell box, 1024 x 1024) at 16 spp, rendered as beauty (Device.render_tasks)
and as features (Device.render_features) after a 1-spp warm-up of each.  Wall time is a host clock
around the call (both calls end in a device synchronise), with launch timing off; the two are
alternated, `--repeats` times each, and the medians reported as ms per pass.  One more run of each
with LUMO_OPT_TIMING on gives the per-stage device times (HIP events).  Needs an MI355X: without a
device lumo_create fails and so does this script.

    python tools/feature_time.py [--res 1024] [--spp 16] [--repeats 3]  ->  one JSON line"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import lumo_amd as L  # noqa: E402
from lumo_amd import _ffi  # noqa: E402

SEED = 0x5EED1234


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stage_ms(dev, fn):
    lib = _ffi.load()
    dev.set_option("timing", 1)
    _ffi.check(lib.lumo_stats_reset(dev.ctx), "stats_reset")
    fn()
    s = dev.stats()
    dev.set_option("timing", 0)
    return {name: round(s.kernel_ms[k], 3) for k, name in enumerate(_ffi.STAGES) if s.launches[k]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--beauty-only", action="store_true",
                    help="time the beauty render alone (the same command on a commit before the feature render)")
    a = ap.parse_args()
    scene = L.Scene.cornell_box().build()
    cam = L.Camera.cornell_box((a.res, a.res))
    dev = L.Device(0)
    dev.upload(scene, cam)
    warm = L.make_tasks(a.res, a.res, 1, SEED)
    tasks = L.make_tasks(a.res, a.res, a.spp, SEED)
    runs = {"beauty": lambda t=tasks: dev.render_tasks(t)}
    dev.render_tasks(warm)
    if not a.beauty_only:
        runs["features"] = lambda t=tasks: dev.render_features(t)
        dev.render_features(warm)
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    out = {"frame": f"cornell {a.res}x{a.res}", "spp": a.spp, "repeats": a.repeats}
    for k, fn in runs.items():
        med = statistics.median(ms[k])
        out[k] = {"ms_per_pass": round(med / a.spp, 3), "frame_ms": [round(x, 2) for x in ms[k]],
                  "stage_ms": stage_ms(dev, fn)}
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
