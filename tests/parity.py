"""Helpers shared by the GPU parity tests and smoke()."""
import ctypes as C

import numpy as np

from lumo_amd import _ffi


def gpu_paths(dev, task, sampler=0):
    """lumo_debug_paths: per-path radiance / wavelengths / raster / depth of one task."""
    P = (task.px_max[0] - task.px_min[0]) * (task.px_max[1] - task.px_min[1])
    m = P * task.samples
    rad, lam, ras = np.zeros(4 * m), np.zeros(4 * m), np.zeros(2 * m)
    depth, delta = np.zeros(m, dtype=np.uint64), np.zeros(task.samples)
    dump = _ffi.PathDump(rad.ctypes.data_as(_ffi.c_double_p), lam.ctypes.data_as(_ffi.c_double_p),
                         ras.ctypes.data_as(_ffi.c_double_p), depth.ctypes.data_as(_ffi.c_uint64_p),
                         delta.ctypes.data_as(_ffi.c_double_p))
    lib = _ffi.load()
    _ffi.check(lib.lumo_debug_set_sampler(dev.ctx, int(sampler)), "debug_set_sampler")
    try:
        _ffi.check(lib.lumo_debug_paths(dev.ctx, C.byref(task), C.byref(dump)), "debug_paths")
    finally:
        lib.lumo_debug_set_sampler(dev.ctx, 0)
    return dict(radiance=rad.reshape(-1, 4), lam=lam.reshape(-1, 4), raster=ras.reshape(-1, 2), depth=depth,
                delta=delta)


def assert_paths_equal(g, o):
    """Every per-path output of lumo_debug_paths and the pass deltas against the oracle's, bit for bit."""
    for k in ("depth", "raster", "lam", "radiance", "delta"):
        np.testing.assert_array_equal(g[k], o[k], err_msg=k)


def assert_tiles_equal(bufs, res, obufs, ores, camera_rays=False):
    """Every task's tile buffer bit-equal to the oracle's and its ray and query counts the same."""
    assert len(bufs) == len(obufs)
    for i, (b, ob, r, orr) in enumerate(zip(bufs, obufs, res, ores)):
        np.testing.assert_array_equal(b, ob, err_msg=f"task {i}")
        assert (r.num_rays, r.num_queries) == (orr.num_rays, orr.num_queries), f"task {i}"
        if camera_rays:
            assert r.num_camera_rays == orr.num_camera_rays, f"task {i}"


def assert_splats_equal(sp, osp):
    """Per-task light-tracing splat lists (lumo's order) bit-equal to the oracle's."""
    assert len(sp) == len(osp)
    for i, (s, os_) in enumerate(zip(sp, osp)):
        assert len(s) == len(os_), f"task {i}"
        for k in ("x", "y", "rgb"):
            np.testing.assert_array_equal(s[k], os_[k], err_msg=f"task {i} {k}")


def stage_launches(before, after, stage):
    """Launches of a stage (a name of _ffi.STAGES) between two Device.stats() readings."""
    k = _ffi.STAGES.index(stage)
    return after.launches[k] - before.launches[k]


def oracle_threads():
    """Threads for the CPU oracle in a parity test: the cores this process may use (the affinity
    mask, capped by a cgroup v2 quota: on the GPU box os.cpu_count() is the whole machine)."""
    import math
    import os
    n = len(os.sched_getaffinity(0))
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, math.floor(int(q) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 32))


# The path-tracing kernel forms of an n_shadow == 1 scene, each chosen by the options alone (plain
# pass loop, pipeline 0): the fused bounce, the tail kernel from the first bounce (tail_below above
# the path count) and the split closest / shade / shadow kernels; "default" is the caller's device.
SCHEDULES = [("default", None, None), ("fused", 1, 0), ("tail", 1, 1 << 30), ("split", 0, 0)]
SCHEDULE_IDS = [s[0] for s in SCHEDULES]


def render_scheduled(dev, scene, cam, tasks, how, fused, tail):
    """render_tasks through schedule `how` (default: on dev), asserting that the kernel the case
    names ran: n_shadow == 1, the schedule's fused flag, tail queries only in the tail form."""
    import lumo_amd as L
    d = dev if how == "default" else L.Device(0, fused=fused, tail_below=tail, pipeline=0)
    try:
        d.upload(scene, cam)
        bufs, res = d.render_tasks(tasks)
        if how != "default":
            assert d.scene_info().n_shadow == 1
            assert d.last_schedule().fused == fused
            assert (d.stats().tail_queries > 0) == (how == "tail")
    finally:
        if d is not dev:
            d.close()
    return bufs, res
