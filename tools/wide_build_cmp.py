#!/usr/bin/env python3
"""The two builders of the wide BVH side by side, on bench.py's stand-in scenes, one MI355X.

Per config and builder ("host": binned SAH on the CPU, "device": the LBVH of device/wbvh_dev.h or, with
`--cluster RADIUS`, the clustered build of device/wbvh_ploc.h, with `--treelet PASSES` the restructuring passes
of device/wbvh_treelet.h over it; per leaf_max, radius and pass count): the build time of three
uploads (lumo_wide_build_info.build_ms: host wall clock, device HIP events) and their median, the clustering's
share of it and its iterations, the treelet passes' share, counts and objective, the SAH cost, nodes, levels, stack need, and the wall clock of a short frame
(tools/ab2.sh's: C2 at 4 spp, C3 and C4 at 8 spp; one warm-up frame, then `--frames` timed ones; one context at
a time).

    python tools/wide_build_cmp.py [--configs c2 c3 c4] [--leaf-max 8 4] [--cluster 0 8 16 32] [--treelet 0 1 2 3] [--frames 3]
        ->  one JSON line per case"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPP = {"c2": 4, "c3": 8, "c4": 8}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="*", default=["c2", "c3", "c4"], choices=sorted(SPP))
    ap.add_argument("--leaf-max", nargs="*", type=int, default=[8, 4])
    ap.add_argument("--cluster", nargs="*", type=int, default=[0], metavar="RADIUS",
                    help="device cases per search radius of the clustered builder (0: the LBVH)")
    ap.add_argument("--cluster-iters", type=int, default=None, help="lumo_wide_cluster_cfg.max_iter (default: the built-in cap)")
    ap.add_argument("--treelet", nargs="*", type=int, default=[0], metavar="PASSES",
                    help="device cases per number of treelet passes over the clustered tree (0: none)")
    ap.add_argument("--treelet-gamma", type=int, default=None, help="lumo_wide_treelet_cfg.gamma (default: the built-in value)")
    ap.add_argument("--no-host", action="store_true", help="leave the host builder's case out")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--max-paths", type=int, default=1 << 23, help="paths in flight per wavefront (bench.py's default)")
    ap.add_argument("--res", type=int, default=None, help="square frames of this size instead of the configs' own")
    a = ap.parse_args()
    import lumo_amd as L
    from bench import build_config
    for cfg in a.configs:
        scene, cam, (W, H), spp, wl = build_config(cfg, a.res, SPP[cfg])
        tasks = L.make_tasks(W, H, spp, 0x5EED)
        integrator = wl.get("integrator", 0)

        def render(dev):  # BDPT's light-tracing splats are collected and dropped
            dev.render_tasks(tasks, max_paths=a.max_paths, integrator=integrator, splats_out=[] if integrator else None)
        cases = ([] if a.no_host else [("host", 8, 0, 0)]) + [("device", m, r, p) for r in a.cluster for p in a.treelet
                                                               for m in a.leaf_max if r or not p]
        for builder, leaf_max, radius, passes in cases:  # one context at a time: a C3 context's work buffers take much of the HBM
            print(f"{cfg}: {builder} builder, leaf_max {leaf_max}, cluster radius {radius}, {passes} treelet passes", file=sys.stderr, flush=True)
            dev = L.Device(0, accel=1, wide_build=builder, leaf_max=leaf_max, wide_cluster=radius,
                           cluster_iters=a.cluster_iters, wide_treelet=passes, treelet_gamma=a.treelet_gamma)
            try:
                builds, clusters, treelets = [], [], []
                for _ in range(3):
                    dev.upload(scene, cam)
                    builds.append(dev.wide_build_info())
                    clusters.append(dev.wide_cluster_info())
                    treelets.append(dev.wide_treelet_info())
                info, how, tl = builds[-1], clusters[-1], treelets[-1]
                if tl["passes_used"] != passes:
                    raise SystemExit(f"{cfg}: asked for {passes} treelet passes, got {tl['passes_used']}")
                if how["radius_used"] != radius:
                    raise SystemExit(f"{cfg}: asked for cluster radius {radius}, got {how['radius_used']}")
                if info["builder_used"] != L._ffi.WIDE_BUILDERS[builder]:
                    raise SystemExit(f"{cfg}: asked for the {builder} builder, got {info['builder_used']}")
                render(dev)  # warm-up
                frames = []
                for _ in range(a.frames):
                    t0 = time.perf_counter()
                    render(dev)
                    frames.append(round(1e3 * (time.perf_counter() - t0), 2))
            finally:
                dev.close()
            print(json.dumps({"config": cfg, "builder": builder, "leaf_max": leaf_max, "frame": [W, H, spp],
                              "build_ms": [round(b["build_ms"], 3) for b in builds],
                              "build_ms_median": round(statistics.median(b["build_ms"] for b in builds), 3),
                              "cluster": radius, "cluster_ms": [round(c["cluster_ms"], 3) for c in clusters],
                              "iterations": [how["iterations"], how["paired_iterations"]],
                              "treelet": passes, "treelet_ms": [round(t["treelet_ms"], 3) for t in treelets],
                              "tried": tl["tried"], "replaced": tl["replaced"],
                              "area_before": tl["area_before"], "area_after": tl["area_after"],
                              "sah_cost": round(info["sah_cost"], 3),
                              **{k: info[k] for k in ("trees", "levels", "nodes", "tris", "stack")},
                              "frame_ms": frames, "frame_ms_median": statistics.median(frames)}), flush=True)


if __name__ == "__main__":
    main()
