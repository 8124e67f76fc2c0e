"""Dynamic geometry (lumo_scene_update_vertices, DESIGN.md §4g "Refit"): vertices overwritten on the device,
the wide BVH refit in place by the HIP kernels of device/wbvh_refit.h.

* An update with the unchanged vertices reproduces the tree of either builder byte for byte: the rounding
  rule, the sphere rule and the instance boxes are pinned without being restated.
* After a smooth displacement of the movable vertices the topology is the old one, every record holds the
  moved vertices and every child box is, bit for bit, the outward-rounded f32 of the exact f64 bounds of
  what lies beneath it (restated in numpy over the export, BLASes first, children before parents).
* Walks over the refit tree obey the brute-force rule of tests/test_brute.py on the moved scene, renders
  equal oracle(wide) of the moved scene.  The moved scene is a shallow copy of the description with the
  moved vertex array: the state the device is in.
* What is refused leaves the scene as it was.

refit_info's sah_build is the cost of the tree as built by the device's reduction: the device builder's own
figure exactly, the host builder's (summed per tree on the host) to rounding, 1e-12 relative here for sums
of at most a few thousand positive terms."""
import ctypes as C
import functools

import numpy as np
import pytest

import lumo_amd as L
import oracle_ffi as O
from lumo_amd import _ffi
from parity import oracle_threads
from test_brute import check_against_brute, scene, trace4
from test_gpu_brute import _joined
from test_gpu_scale import _arrays
from test_gpu_wide import BDPT, SEED, _small_scenes, _tiles_cmp
from test_wide import KDMESH, RECT, SPHERE, TRI, _leaves

pytestmark = pytest.mark.gpu
SCENES = ["cornell", "small_dragon", "scaled_instances", "zoo_translated", "spheres", "degenerate", "flat"]
BUILDERS = {"host": dict(wide_build="host"), "device": dict(wide_build="device", wide_cluster=16, wide_treelet=2)}
KEYS = ("nodes", "tv", "obj_blas", "light_blas", "obj_root", "light_root", "stack", "depth")


def _same(a, b):
    for k in KEYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def _moved(d, amp=0.05):
    """(moved vertices, description of the moved scene): every vertex that only kd-mesh objects use gets, per
    coordinate, amp x the movable vertices' extent on that axis x a sine of its other two coordinates."""
    v, tris = _arrays(d)
    used = np.zeros((2, len(v)), dtype=bool)  # by a kd-mesh object; protected
    for table, n, is_light in ((d.objects, d.num_objects, False), (d.lights, d.num_lights, True)):
        for o in (table[i] for i in range(n)):
            if o.type != SPHERE:
                k = 1 if o.type == TRI else o.num_tris
                used[int(is_light or o.type != KDMESH), tris["v"][o.tri_base:o.tri_base + k].ravel()] = True
    mov = used[0] & ~used[1]
    w = v.copy()
    p = v[mov]
    ext = p.max(0) - p.min(0) if mov.any() else np.zeros(3)
    if ext.max() > 0.0:
        w[mov] = p + amp * ext * np.sin(2.0 * np.pi / ext.max() * (p[:, [1, 2, 0]] + 2.0 * p[:, [2, 0, 1]]))
    d2 = _ffi.SceneDesc.from_buffer_copy(d)
    d2.vertices = w.ctypes.data_as(_ffi.c_double_p)
    d2._keep = (d, w)
    return w, d2


@functools.lru_cache(maxsize=None)
def _moved_scene(name):
    return _moved(scene(name)[1])


@functools.lru_cache(maxsize=None)
def _brute_moved(name, vis):
    _, o, dirs, li, _ = _joined(name, vis)
    d2 = _moved_scene(name)[1]
    return trace4(d2, o, dirs, li, O.BRUTE), trace4(d2, o, dirs, li, O.BRUTE_REV)


def _max_abs(nodes):
    valid = np.arange(4) < nodes["n"][:, None, None]
    return np.float32(max(np.abs(nodes[k])[np.broadcast_to(valid, nodes[k].shape)].max(initial=0.0) for k in ("lo", "hi")))


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", SCENES)
def test_unchanged_vertices_reproduce_the_tree(name, builder):
    sc, d, _, _ = scene(name)
    dev = L.Device(0, accel=1, **BUILDERS[builder])
    try:
        dev.upload(sc)
        a, built = dev.wide_export(), dev.wide_build_info()
        dev.update_vertices(_arrays(d)[0])
        b, info = dev.wide_export(), dev.refit_info()
    finally:
        dev.close()
    _same(a, b)
    assert (info["changed"], info["updates"]) == (0, 1) and info["refit_ms"] > 0.0
    assert info["sah_cost"] == info["sah_build"] and info["max_abs"] == _max_abs(b["nodes"])
    assert info["sah_build"] == (built["sah_cost"] if builder == "device" else pytest.approx(built["sah_cost"], rel=1e-12))


def _xf_box(m, lo, hi):
    """wbvh_build.h xf_box: the 8 corners through the row-major 4x4 m, then the pad."""
    c = np.array([[(hi if i >> a & 1 else lo)[a] for a in range(3)] for i in range(8)])
    o = ((m[:, 0] * c[:, [0]] + m[:, 1] * c[:, [1]]) + m[:, 2] * c[:, [2]]) + m[:, 3]
    q = o[:, :3] / o[:, [3]]
    pad = max(np.abs(q.min(0)).max(), np.abs(q.max(0)).max()) * 1e-9
    return q.min(0) - pad, q.max(0) + pad


def _assert_tight(acc, d2):
    """Every child box is the outward-rounded f32 of the exact f64 bounds beneath it."""
    nodes, tv = acc["nodes"], acc["tv"]
    box = np.zeros((len(nodes), 2, 3))
    tables = {}
    for root, table, blas in ((acc["obj_root"], d2.objects, acc["obj_blas"]), (acc["light_root"], d2.lights, acc["light_blas"])):
        tables.update({i: (table, blas) for i in _leaves(acc, root)[1]})

    def bounds(r, node):
        if r >= 0:
            return box[r]
        first, cnt = (~r) >> 4, (~r) & 15
        if cnt:
            p = tv[first:first + cnt, :9].reshape(-1, 3)
            return p.min(0), p.max(0)
        table, blas = tables[node]
        o = table[first]
        rad = abs(o.radius)
        lo, hi = (np.full(3, -rad), np.full(3, rad)) if o.type == SPHERE else bounds(int(blas[first]), None)
        return _xf_box(np.array(d2.transforms[o.xform].m).reshape(4, 4), lo, hi) if o.xform >= 0 else (lo, hi)
    for world in (False, True):  # an instance leaf needs its BLAS; a child has a larger index than its parent
        for i in reversed([i for i in range(len(nodes)) if (i in tables) == world]):
            kids = [bounds(int(nodes[i]["ref"][k]), i) for k in range(nodes[i]["n"])]
            for k, (lo, hi) in enumerate(kids):
                lo, hi = np.asarray(lo), np.asarray(hi)
                fl, fh = lo.astype(np.float32), hi.astype(np.float32)
                fl = np.where(fl.astype(np.float64) > lo, np.nextafter(fl, np.float32(-np.inf)), fl)
                fh = np.where(fh.astype(np.float64) < hi, np.nextafter(fh, np.float32(np.inf)), fh)
                assert nodes[i]["lo"][:, k].tobytes() == fl.astype(np.float32).tobytes(), (i, k, "lo")
                assert nodes[i]["hi"][:, k].tobytes() == fh.astype(np.float32).tobytes(), (i, k, "hi")
            box[i] = np.min([b[0] for b in kids], axis=0), np.max([b[1] for b in kids], axis=0)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", SCENES)
def test_moved_tree_is_valid_and_tight(name, builder):
    sc, d, _, _ = scene(name)
    w, d2 = _moved_scene(name)
    changed = int((w != _arrays(d)[0]).any(1).sum())
    assert changed > 0 or name == "spheres"
    dev = L.Device(0, accel=1, **BUILDERS[builder])
    try:
        dev.upload(sc)
        before = dev.wide_export()
        dev.update_vertices(w)
        acc, info = dev.wide_export(), dev.refit_info()
        dev.update_vertices(w)
        again, info2 = dev.wide_export(), dev.refit_info()
    finally:
        dev.close()
    for k in ("ref", "n"):
        assert acc["nodes"][k].tobytes() == before["nodes"][k].tobytes(), k
    assert all(np.array_equal(acc[k], before[k]) for k in KEYS[2:] + ("tri", "obj"))
    v2, tris = _arrays(d2)
    np.testing.assert_array_equal(acc["tv"][:, :9].reshape(-1, 3, 3), v2[tris["v"][acc["tri"]]])
    _assert_tight(acc, d2)
    assert (info["changed"], info["updates"], info["max_abs"]) == (changed, 1, _max_abs(acc["nodes"]))
    _same(acc, again)
    assert (info2["changed"], info2["updates"], info2["sah_cost"]) == (0, 2, info["sah_cost"])
    print(f"{name}/{builder}: sah_cost {info['sah_build']:.3f} -> {info['sah_cost']:.3f}, refit {info['refit_ms']:.3f} ms")


@pytest.mark.parametrize("name,builder,opts", [(n, b, {}) for n in SCENES for b in BUILDERS] +
                         [("small_dragon", "device", dict(top_staging=1, top_kb=8))])
def test_walks_on_the_refit_tree_equal_brute(name, builder, opts):
    sc = scene(name)[0]
    dev = L.Device(0, accel=1, **BUILDERS[builder], **opts)
    try:
        dev.upload(sc)
        info = dev.scene_info()
        assert info.accel == 1 and (name != "cornell" or info.lds_bytes > 0)
        assert not opts or 0 < info.top_wide_nodes < info.wide_nodes  # the staged prefix cuts the tree
        dev.update_vertices(_moved_scene(name)[0])
        for vis in (False, True):
            fams, o, dirs, li, bounds = _joined(name, vis)
            g = dev.trace(o, dirs, li)
            brute, rev = _brute_moved(name, vis)
            if vis:  # lumo_trace reports no triangle for a visibility query; the oracle's is -1
                g = g[:3] + (brute[3],)
            for k, f in enumerate(fams):
                s = slice(bounds[k], bounds[k + 1])
                share = check_against_brute(*[tuple(a[s] for a in x) for x in (g, brute, rev)], what=f"{name}/{f}")
                print(f"{name}/{f}: excused share {share:g}")
    finally:
        dev.close()


@pytest.mark.parametrize("name,integrator,fused", [("small_dragon", 0, 1), ("small_dragon", 0, 0), ("cornell", 0, -1),
                                                   ("cornell", BDPT, -1)])
def test_renders_before_and_after_equal_oracle(name, integrator, fused):
    make, _, camera = _small_scenes()[name]
    sc, cam = make().build(), camera((32, 32))
    tasks = L.make_tasks(32, 32, 4, SEED)
    w, d2 = _moved(sc.desc())
    dev = L.Device(0, accel=1, fused=fused, **BUILDERS["device"])
    try:
        dev.upload(sc, cam)
        for desc in (sc.desc(), d2):  # the original scene, then the same context after the update
            if desc is d2:
                dev.update_vertices(w)
                assert dev.refit_info()["changed"] > 0
            sp, osp = ([], []) if integrator else (None, None)
            bufs, res = dev.render_tasks(tasks, integrator=integrator, splats_out=sp)
            assert fused < 0 or dev.last_schedule().fused == fused
            obufs, ores, _ = O.render_tasks(desc, cam.desc, tasks, O.WAVEFRONT, oracle_threads(), integrator=integrator,
                                            splats_out=osp, accel=1)
            _tiles_cmp(bufs, res, obufs, ores, sp=sp, osp=osp)
    finally:
        dev.close()


def test_refusals_and_arguments():
    lib, info = _ffi.load(), _ffi.RefitInfo()
    sc, d, _, _ = scene("cornell")
    v = _arrays(d)[0]
    dev, lumo = L.Device(0, accel=1), L.Device(0)

    def update(ctx, first, xyz):
        a = np.ascontiguousarray(xyz, dtype=np.float64)
        return lib.lumo_scene_update_vertices(ctx, first, len(a), a.ctypes.data_as(_ffi.c_double_p))

    def protected(desc, tri):  # moving one vertex of the triangle is refused, its present value is accepted
        pv, pt = _arrays(desc)
        i = int(pt["v"][tri][0])
        assert update(dev.ctx, i, pv[i:i + 1] + 1.0) == 6 and update(dev.ctx, i, pv[i:i + 1]) == 0
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            dev.update_vertices(pv[i:i + 1] * 2.0 + 1.0, first=i)
    try:
        assert update(dev.ctx, 0, v) == 4 and lib.lumo_scene_refit_info(dev.ctx, C.byref(info)) == 4  # LUMO_ERR_NO_SCENE
        rs, rd = scene("spheres")[:2]  # its floor is a Rectangle object
        dev.upload(rs)
        before = dev.wide_export()
        protected(rd, next(rd.objects[i] for i in range(rd.num_objects) if rd.objects[i].type == RECT).tri_base)
        _same(before, dev.wide_export())
        dev.upload(sc)
        lumo.upload(sc)
        before = dev.wide_export()
        protected(d, d.lights[0].tri_base)  # Cornell's light
        moved = _moved_scene("cornell")[0].copy()
        moved[len(v) // 2, 1] = np.nan
        assert update(dev.ctx, 0, moved) == 1 and update(dev.ctx, 0, np.where(np.isnan(moved), np.inf, moved)) == 1
        assert update(dev.ctx, 1, v) == 1 and update(dev.ctx, -1, v[:1]) == 1 and update(dev.ctx, len(v), v[:1]) == 1
        assert lib.lumo_scene_update_vertices(dev.ctx, 0, -1, v.ctypes.data_as(_ffi.c_double_p)) == 1
        assert lib.lumo_scene_update_vertices(dev.ctx, 0, 1, None) == 1 and update(None, 0, v) == 1
        assert lib.lumo_scene_refit_info(dev.ctx, None) == 1 and lib.lumo_scene_refit_info(None, C.byref(info)) == 1
        assert update(lumo.ctx, 0, v) == 6  # accel = 0: kd-trees and object BVHs cannot be refit
        _same(before, dev.wide_export())
        assert dev.refit_info()["changed"] == 0 and dev.refit_info()["updates"] == 1  # the accepted one above
    finally:
        dev.close()
        lumo.close()
