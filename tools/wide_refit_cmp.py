#!/usr/bin/env python3
"""Refit against rebuild of the wide BVH (DESIGN.md §4g "Refit"), on bench.py's stand-in scenes, one MI355X.

Per config and displacement (a share of the movable vertices' extent per axis, times a sine of the other two
coordinates; lights and objects that are no kd mesh stay): the tree of the clustered device builder is refit
by lumo_scene_update_vertices (three updates: refit_ms from HIP events, and their median), then the moved scene
is uploaded afresh (the description with the moved vertex array) and built by the same builder.  For both
trees: the SAH cost and the wall clock of a short frame (tools/wide_build_cmp.py's).  Also what a caller paid
before: the wall clock of a whole lumo_scene_upload, and the device build's share of it (build_ms).

    python tools/wide_refit_cmp.py [--configs c2 c3] [--amps 0.01 0.05 0.2] [--cluster 32] [--frames 3]
        ->  one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPP = {"c2": 4, "c3": 8, "c4": 8}
KDMESH, TRIANGLE, SPHERE = 0, 2, 3


def moved(d, amp):
    """The scene's vertex array with every vertex that only kd-mesh objects use displaced."""
    v = np.ctypeslib.as_array(d.vertices, shape=(d.num_vertices, 3))
    tv = np.ctypeslib.as_array(d.triangles, shape=(d.num_triangles,))["v"]
    used = np.zeros((2, len(v)), dtype=bool)  # by a kd-mesh object; protected
    for table, n, light in ((d.objects, d.num_objects, False), (d.lights, d.num_lights, True)):
        for o in (table[i] for i in range(n)):
            if o.type != SPHERE:
                k = 1 if o.type == TRIANGLE else o.num_tris
                used[int(light or o.type != KDMESH), tv[o.tri_base:o.tri_base + k].ravel()] = True
    mov = used[0] & ~used[1]
    p = v[mov]
    ext = p.max(0) - p.min(0)
    w = v.copy()
    w[mov] = p + amp * ext * np.sin(2.0 * np.pi / ext.max() * (p[:, [1, 2, 0]] + 2.0 * p[:, [2, 0, 1]]))
    return w, int(mov.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="*", default=["c2", "c3"], choices=sorted(SPP))
    ap.add_argument("--amps", nargs="*", type=float, default=[0.01, 0.05, 0.2])
    ap.add_argument("--cluster", type=int, default=32, metavar="RADIUS", help="the device builder's search radius (0: the LBVH)")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--max-paths", type=int, default=1 << 23)
    ap.add_argument("--res", type=int, default=None)
    a = ap.parse_args()
    import lumo_amd as L
    from bench import build_config
    from lumo_amd import _ffi
    for cfg in a.configs:
        scene, cam, (W, H), spp, wl = build_config(cfg, a.res, SPP[cfg])
        tasks = L.make_tasks(W, H, spp, 0x5EED)
        integrator = wl.get("integrator", 0)
        d = scene.desc()

        def frame_ms(dev):
            def render():
                dev.render_tasks(tasks, max_paths=a.max_paths, integrator=integrator, splats_out=[] if integrator else None)
            render()  # warm-up
            out = []
            for _ in range(a.frames):
                t0 = time.perf_counter()
                render()
                out.append(round(1e3 * (time.perf_counter() - t0), 2))
            return statistics.median(out)
        for amp in a.amps:  # one context at a time
            w, n_mov = moved(d, amp)
            d2 = _ffi.SceneDesc.from_buffer_copy(d)
            d2.vertices = w.ctypes.data_as(_ffi.c_double_p)
            dev = L.Device(0, accel=1, wide_build="device", wide_cluster=a.cluster)
            try:
                uploads, builds = [], []
                for _ in range(3):
                    t0 = time.perf_counter()
                    dev.upload(scene, cam)
                    uploads.append(round(1e3 * (time.perf_counter() - t0), 2))
                    builds.append(round(dev.wide_build_info()["build_ms"], 3))
                built = dev.wide_build_info()
                refits = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    dev.update_vertices(w)
                    refits.append((round(dev.refit_info()["refit_ms"], 3), round(1e3 * (time.perf_counter() - t0), 3)))
                info = dev.refit_info()
                refit_frame = frame_ms(dev)
                _ffi.check(_ffi.load().lumo_scene_upload(dev.ctx, C.byref(d2)), "upload of the moved scene")
                fresh = dev.wide_build_info()
                fresh_frame = frame_ms(dev)
            finally:
                dev.close()
            print(json.dumps({"config": cfg, "amp": amp, "cluster": a.cluster, "frame": [W, H, spp], "vertices": len(w),
                              "movable": n_mov, "nodes": built["nodes"], "tris": built["tris"],
                              "upload_ms": uploads, "upload_ms_median": statistics.median(uploads),
                              "build_ms": builds, "build_ms_median": statistics.median(builds),
                              "refit_ms": [r[0] for r in refits], "refit_ms_median": statistics.median(r[0] for r in refits),
                              "update_wall_ms": [r[1] for r in refits],
                              "sah_build": round(info["sah_build"], 3), "sah_refit": round(info["sah_cost"], 3),
                              "sah_fresh": round(fresh["sah_cost"], 3), "fresh_build_ms": round(fresh["build_ms"], 3),
                              "frame_ms_refit": refit_frame, "frame_ms_fresh": fresh_frame}), flush=True)


if __name__ == "__main__":
    main()
