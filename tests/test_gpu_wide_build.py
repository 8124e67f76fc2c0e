"""The device builder of the wide BVH (lumo_scene_set_wide_build): an LBVH built by the HIP
kernels of device/wbvh_dev.h in the node format the walks already read.

* Structure of the exported tree, against the scene itself: every node once, 2 to 4 children, every triangle
  once with its object, every box around what it holds (exactly, in f64), level-major indices, the stack need
  restated in numpy, two uploads byte for byte the same.  The host builder's export equals the oracle's.
* Walks over the device-built tree obey the brute-force rule of tests/test_brute.py: any valid tree with
  outward-rounded boxes gives brute force's answer, so the reference does not depend on the builder.  The SAH
  tree measures an excused share of 0; another tree may keep the other of two tied hits, so the bound here
  is the rule's own cap.
* Renders on the device-built tree equal oracle(wide) bit for bit (no two triangles of one tree tie in these
  scenes); the traversal counters belong to the tree and are not compared.
* The fallback to the host builder, and the arguments."""
import ctypes as C
import functools

import numpy as np
import pytest

import lumo_amd as L
import oracle_ffi as O
from lumo_amd import _ffi
from parity import oracle_threads
from test_brute import SPHERE, _object_points, check_against_brute, scene, trace4
from test_gpu_brute import _joined
from test_gpu_scale import _arrays, _closest_rays
from test_gpu_wide import BDPT, SEED, _small_scenes, _tiles_cmp, _trace_cmp
from test_wide import NAMES, NONE, _box, _leaves

pytestmark = pytest.mark.gpu
SCENES = ["cornell", "small_dragon", "spheres", "lights_only", "concentric", "degenerate", "flat", "zoo_translated",
          "scaled_instances", "stadium"]
assert set(SCENES) <= set(NAMES)


def _device(**kw):
    return L.Device(0, accel=1, wide_build="device", **kw)


def _stack_need(acc, blas_nodes, blas_roots):
    """wbvh_build.h's rule: a node needs n - 1 + its largest child need, an instance leaf 1 + the deepest BLAS
    need; BLASes first.  Children have larger indices, so one reverse sweep per pass."""
    nodes, need = acc["nodes"], np.zeros(len(acc["nodes"]), dtype=int)

    def ref_need(r, world, bn):
        if r == NONE:
            return 0
        return need[r] if r >= 0 else (1 + bn if world and (~r) & 15 == 0 else 0)
    bn = 0
    for world in (False, True):
        for i in reversed(range(len(nodes))):
            if (i in blas_nodes) != world:
                need[i] = nodes[i]["n"] - 1 + max(ref_need(int(r), world, bn) for r in nodes[i]["ref"][:nodes[i]["n"]])
        if not world:
            bn = max([ref_need(b, False, 0) for b in blas_roots], default=0)
    return max(ref_need(acc["obj_root"], True, bn), ref_need(acc["light_root"], True, bn))


@pytest.mark.parametrize("name", SCENES)
def test_device_tree_structure(name):
    sc, d, _, _ = scene(name)
    dev = _device()
    try:
        dev.upload(sc)
        acc, info = dev.wide_export(), dev.wide_build_info()
        dev.upload(sc)
        again = dev.wide_export()
    finally:
        dev.close()
    assert acc["ok"] and (info["builder_asked"], info["builder_used"]) == (1, 1)
    for k in ("nodes", "tv", "obj_blas", "light_blas"):  # reproducible
        assert acc[k].tobytes() == again[k].tobytes(), k
    assert [acc[k] for k in ("obj_root", "light_root", "stack", "depth")] == \
           [again[k] for k in ("obj_root", "light_root", "stack", "depth")]
    nodes, tv = acc["nodes"], acc["tv"]
    assert (info["nodes"], info["tris"], info["build_ms"] > 0.0) == (len(nodes), len(tv), True)
    vtx, tris = _arrays(d)
    objs = np.ctypeslib.as_array(d.objects, shape=(d.num_objects,)) if d.num_objects else []
    lights = np.ctypeslib.as_array(d.lights, shape=(d.num_lights,))

    def leaf_points(r):  # the records of a triangle leaf: they hold the scene's vertices, at most 8
        first, cnt = (~r) >> 4, (~r) & 15
        assert 1 <= cnt <= 8
        for j in range(first, first + cnt):
            np.testing.assert_array_equal(tv[j, :9].reshape(3, 3), vtx[tris["v"][acc["tri"][j]]])
        return tv[first:first + cnt, :9].reshape(-1, 3)

    def inside(node, k, p):
        if node is not None:
            lo, hi = _box(nodes[node], k)
            assert (p >= lo).all() and (p <= hi).all(), (name, node, k)
    reached, blas_nodes = [], set()
    for root, table, blas in ((acc["obj_root"], objs, acc["obj_blas"]), (acc["light_root"], lights, acc["light_blas"])):
        leaves, seen = _leaves(acc, root)  # asserts: a tree, 2 to 4 children
        reached += sorted(seen)
        got = {}
        for node, k, r in leaves:
            first, cnt = (~r) >> 4, (~r) & 15
            if cnt:
                inside(node, k, leaf_points(r))
                for j in range(first, first + cnt):
                    assert int(acc["tri"][j]) not in got, "a triangle in two leaves"
                    got[int(acc["tri"][j])] = int(acc["obj"][j])
                continue
            o = table[first]  # object leaf: a sphere (centre +- radius on each axis), or an instance
            assert o["type"] == SPHERE or o["xform"] >= 0
            if o["type"] == SPHERE:
                c = _object_points(d, o).mean(0)
                inside(node, k, np.array([c + s * float(o["radius"]) * e for e in np.eye(3) for s in (-1, 1)]))
                continue
            inside(node, k, _object_points(d, o))
            bl, bseen = _leaves(acc, int(blas[first]))
            blas_nodes |= bseen
            for bn, bk, br in bl:
                inside(bn, bk, leaf_points(br))
            n = 1 if o["type"] == 2 else int(o["num_tris"])
            held = sorted(int(acc["tri"][((~br) >> 4) + j]) for _, _, br in bl for j in range((~br) & 15))
            assert held == list(range(o["tri_base"], o["tri_base"] + n))
        want = {t: i for i, o in enumerate(table) if o["xform"] < 0 and o["type"] != SPHERE
                for t in range(o["tri_base"], o["tri_base"] + (1 if o["type"] == 2 else o["num_tris"]))}
        assert got == want
    assert sorted(reached + sorted(blas_nodes)) == list(range(len(nodes))), "a node unreached, or reached twice"
    blas_roots = sorted({int(b) for b in list(acc["obj_blas"]) + list(acc["light_blas"])} - {NONE})
    # level-major: breadth-first from all the roots, the levels are contiguous index ranges in order
    level, frontier, depth = np.full(len(nodes), -1), [r for r in [acc["obj_root"], acc["light_root"]] + blas_roots if r >= 0], 0
    while frontier:
        level[frontier] = depth
        nxt = []
        for i in frontier:
            nd = nodes[i]
            for k in range(nd["n"]):
                r = int(nd["ref"][k])
                if r >= 0:
                    assert r > i
                    nxt.append(r)
                    lo, hi = _box(nd, k)  # the child node's boxes lie inside the parent's box for it
                    for j in range(nodes[r]["n"]):
                        clo, chi = _box(nodes[r], j)
                        assert (clo >= lo).all() and (chi <= hi).all()
        frontier, depth = nxt, depth + 1
    assert (np.diff(level) >= 0).all() and (level >= 0).all()
    assert info["levels"] == depth == (acc["depth"] + 1 if len(nodes) else 0)
    assert _stack_need(acc, blas_nodes, blas_roots) == info["stack"] == acc["stack"] <= 64


def test_host_builder_export_equals_oracle():
    sc, d, _, _ = scene("small_dragon")
    dev = L.Device(0, accel=1)
    try:
        dev.upload(sc)
        acc, info = dev.wide_export(), dev.wide_build_info()
    finally:
        dev.close()
    ref = O.wide_export(d)
    assert (info["builder_asked"], info["builder_used"]) == (0, 0) and info["sah_cost"] > 0.0 and info["build_ms"] > 0.0
    for k in ("nodes", "tv", "obj_blas", "light_blas"):
        assert acc[k].tobytes() == ref[k].tobytes(), k
    assert all(acc[k] == ref[k] for k in ("ok", "stack", "depth", "obj_root", "light_root"))


@functools.lru_cache(maxsize=None)
def _brute(name, vis):
    _, o, dirs, li, _ = _joined(name, vis)
    d = scene(name)[1]
    return trace4(d, o, dirs, li, O.BRUTE), trace4(d, o, dirs, li, O.BRUTE_REV)


@pytest.mark.parametrize("name,opts", [(n, {}) for n in SCENES] + [("small_dragon", dict(top_staging=1, top_kb=8))],
                         ids=SCENES + ["small_dragon-top8"])
def test_device_tree_walks_equal_brute(name, opts):
    sc = scene(name)[0]
    dev = _device(**opts)
    try:
        dev.upload(sc)
        assert dev.wide_build_info()["builder_used"] == 1 and dev.scene_info().accel == 1
        if opts:  # the staged prefix cuts the tree
            assert 0 < dev.scene_info().top_wide_nodes < dev.scene_info().wide_nodes
        if name == "cornell":
            assert dev.scene_info().lds_bytes > 0
        for vis in (False, True):
            fams, o, dirs, li, bounds = _joined(name, vis)
            g = dev.trace(o, dirs, li)
            brute, rev = _brute(name, vis)
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
def test_device_tree_renders_equal_oracle(name, integrator, fused):
    make, _, camera = _small_scenes()[name]
    sc, cam = make().build(), camera((32, 32))
    tasks = L.make_tasks(32, 32, 4, SEED)
    sp, osp = ([], []) if integrator else (None, None)
    dev = _device(fused=fused)
    try:
        dev.upload(sc, cam)
        assert dev.wide_build_info()["builder_used"] == 1
        bufs, res = dev.render_tasks(tasks, integrator=integrator, splats_out=sp)
        assert fused < 0 or dev.last_schedule().fused == fused
    finally:
        dev.close()
    obufs, ores, _ = O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads(), integrator=integrator,
                                    splats_out=osp, accel=1)
    _tiles_cmp(bufs, res, obufs, ores, sp=sp, osp=osp)


def test_fallback_and_arguments():
    lib, info = _ffi.load(), _ffi.WideBuildInfo()
    sc, d, eye, _ = scene("small_dragon")
    dev = _device(stack_limit=2)
    try:
        assert lib.lumo_scene_wide_build_info(dev.ctx, C.byref(info)) == 4  # LUMO_ERR_NO_SCENE
        assert lib.lumo_debug_wide_export(dev.ctx, (C.c_int64 * 8)(), None, None, None, None) == 4
        assert lib.lumo_scene_set_wide_build(None, None) == 1 and lib.lumo_scene_wide_build_info(dev.ctx, None) == 1
        for bad in (dict(builder=2), dict(builder=-1), dict(leaf_max=0), dict(leaf_max=9), dict(stack_limit=0),
                    dict(stack_limit=65), dict(reserved=1)):  # refused: stack_limit = 2 stays
            cfg = _ffi.WideBuildCfg(**{**_ffi.WIDE_BUILD_DEFAULTS, "builder": 1, **bad})
            assert lib.lumo_scene_set_wide_build(dev.ctx, C.byref(cfg)) == 1, bad
        with pytest.raises(ValueError):
            dev.set_wide_build("gpu")
        o, dirs = _closest_rays(d, eye, 1 << 14, 5)
        _trace_cmp(dev, sc, o, dirs)  # uploads; the host tree: oracle(wide) bit for bit, counters included
        got = dev.wide_build_info()
        assert (got["builder_asked"], got["builder_used"]) == (1, 0) and got["stack"] > 2
    finally:
        dev.close()
