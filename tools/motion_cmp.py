#!/usr/bin/env python3
"""What the motion feature costs (DESIGN.md §4g "Motion"), on bench.py's stand-in scenes, one MI355X.

Per config, after a displacement of the movable vertices (tools/wide_refit_cmp.py's, between a motion mark and the
renders), medians of three with the launch timing on (HIP events, summed over the timed stages): lumo_render_features,
lumo_render_features_motion with and without the feature planes, the wall clock of lumo_scene_motion_mark, and the
reproject stage of lumo_denoise_temporal against lumo_denoise_temporal_motion's on the second of two frames, with the
share of k_dn_reproject's blocks that tap the history from LDS.

    python tools/motion_cmp.py [--configs c2] [--amp 0.05] [--res N]  ->  one JSON line per config"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="*", default=["c2"])
    ap.add_argument("--amp", type=float, default=0.05)
    ap.add_argument("--res", type=int, default=None)
    ap.add_argument("--max-paths", type=int, default=1 << 23)
    a = ap.parse_args()
    import lumo_amd as L
    from bench import build_config
    from lumo_amd import _ffi
    from wide_refit_cmp import SPP, moved
    for cfg in a.configs:
        scene, cam, (W, H), spp, _ = build_config(cfg, a.res, SPP[cfg])
        tasks = L.make_tasks(W, H, spp, 0x5EED)
        w, n_mov = moved(scene.desc(), a.amp)
        dev = L.Device(0, accel=1, wide_build="device", wide_cluster=32, timing=1)
        has_motion = hasattr(dev, "motion_mark")  # the parent commit: the feature render alone
        try:
            dev.upload(scene, cam)

            def device_ms(call):
                out = []
                for k in range(4):  # the first is a warm-up
                    _ffi.load().lumo_stats_reset(dev.ctx)
                    call()
                    out.append(round(sum(dev.stats().kernel_ms), 3))
                return out[1:]
            marks = []
            for _ in range(3 if has_motion else 0):
                t0 = time.perf_counter()
                dev.motion_mark()
                marks.append(round(1e3 * (time.perf_counter() - t0), 3))
            dev.update_vertices(w)
            row = {"config": cfg, "amp": a.amp, "frame": [W, H, spp], "movable": n_mov,
                   "features_ms": device_ms(lambda: dev.render_features(tasks, max_paths=a.max_paths))}
            if has_motion:
                row["mark_wall_ms"] = marks
                row["features_motion_ms"] = device_ms(lambda: dev.render_features_motion(tasks, max_paths=a.max_paths))
                row["motion_only_ms"] = device_ms(lambda: dev.render_features_motion(tasks, max_paths=a.max_paths, features=False))
                film = L.Film(W, H, samples=spp, filter_radius=cam.desc.filter_radius, filter_sigma=cam.desc.filter_sigma)
                feat = L.FeatureFilm(W, H)
                for t, b in zip(tasks, dev.render_tasks(tasks, max_paths=a.max_paths)[0]):
                    film.add_tile(t, b)
                for t, p in zip(tasks, dev.render_features_motion(tasks, max_paths=a.max_paths)):
                    feat.add_tile(t, p)
                for name, mot in (("plain", None), ("motion", feat.motion_w)):
                    ms, info = [], {}
                    for _ in range(3):
                        dev.denoise_reset()
                        dev.denoise_temporal(film, feat, cam)
                        dev.denoise_temporal(film, feat, cam, info=info, motion=mot)
                        ms.append(round(info["stage_ms"][2], 3))
                    row["reproject_ms_" + name] = ms
                    row["blocks_" + name] = [info["blocks_staged"], info["blocks_direct"]]
                    row["with_history_" + name] = info["with_history"]
            row.update({k + "_median": statistics.median(v) for k, v in row.items() if k.endswith("_ms") and v})
            print(json.dumps(row), flush=True)
        finally:
            dev.close()


if __name__ == "__main__":
    main()
