#!/usr/bin/env python3
"""Time of Device.denoise_temporal on whole frames, with the defaults, against Device.denoise.

Per frame size (1024 x 1024 and 1920 x 1080): lumo's Cornell box at `--spp` as beauty and features on
one context.  The host-clock time of a steady-state denoise_temporal call (the history of the same
frame and camera in place), median of `--repeats` after a warm-up call, beside Device.denoise's of the
same frame in the same run; one call's split by HIP events (lumo_temporal_info.stage_ms); and the
HIP-event time of k_dn_reproject, median of `--repeats`, staged (stage_lds = 1) against direct
(stage_lds = 0), for a static camera and for one that pans a few pixels between the calls.  Needs an
MI355X.

    python tools/denoise_temporal_time.py [--spp 4] [--repeats 3]  ->  one JSON line per frame size"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import lumo_amd as L  # noqa: E402

SEED = 0x5EED1234
REPROJECT = 2  # stage_ms: upload, prepare, reproject, ...


def clock(repeats, call):
    call()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 2), [round(x, 2) for x in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    scene = L.Scene.cornell_box().build()
    for w, h in ((1024, 1024), (1920, 1080)):
        cam = L.Camera.cornell_box((w, h))
        # the pan: the view turned about y by 3e-3 rad (4.3 pixels at 1024 wide) and back, call by call
        pans = [L.Camera.cornell_box_builder().resolution((w, h))
                .towards(278.0 + 800.0 * math.sin(k * 3e-3), 273.0, -800.0 + 800.0 * math.cos(k * 3e-3)).build() for k in (0, 1)]
        dev = L.Device(0)
        dev.upload(scene, cam)
        tasks = L.make_tasks(w, h, a.spp, SEED)
        film, feat = L.Film(w, h, samples=a.spp), L.FeatureFilm(w, h)
        for t, b in zip(tasks, dev.render_tasks(tasks)[0]):
            film.add_tile(t, b)
        for t, p in zip(tasks, dev.render_features(tasks)):
            feat.add_tile(t, p)
        spatial = clock(a.repeats, lambda: dev.denoise(film, feat))
        temporal = clock(a.repeats, lambda: dev.denoise_temporal(film, feat, cam))
        info = {}
        dev.denoise_temporal(film, feat, cam, info=info)
        n = len(info["stage_ms"]) - 8
        names = ["upload", "prepare", "reproject", "variance", "tvar", "atrous_s1", "history"]  # feedback = 1
        names += [f"atrous_s{1 << i}" for i in range(1, n)] + ["finish", "readback"]
        reproject = {}
        for motion, cams in (("static", [cam, cam]), ("pan", pans)):
            for stage_lds in (1, 0):
                ms = []
                for k in range(a.repeats + 1):
                    i = {}
                    dev.denoise_temporal(film, feat, cams[k % 2], info=i, stage_lds=stage_lds)
                    ms.append(i["stage_ms"][REPROJECT])
                reproject[f"{motion}_{'staged' if stage_lds else 'direct'}"] = {
                    "ms": round(statistics.median(ms[1:]), 3), "calls_ms": [round(x, 3) for x in ms[1:]],
                    "with_history": i["with_history"], "blocks_staged": i["blocks_staged"], "blocks_direct": i["blocks_direct"]}
        dev.close()
        print(json.dumps({"frame": f"cornell {w}x{h}", "spp": a.spp, "denoise_ms": spatial[0], "denoise_calls_ms": spatial[1],
                          "temporal_ms": temporal[0], "temporal_calls_ms": temporal[1],
                          "stage_ms": {k: round(v, 3) for k, v in zip(names, info["stage_ms"])}, "k_dn_reproject": reproject}))


if __name__ == "__main__":
    main()
