"""GPU parity of every kernel form and schedule in the wide accel mode (LUMO_OPT_ACCEL 1).

On the device the wide mode is stack class 0: an eighth instantiation of every traversal launcher of
launch.h, with its own walk (dscene.h wide_walk), its own TOP layout (upload.hip: the object records
and a breadth-first prefix of the wide nodes) and its own branches in the fused bounce and in the BDPT
visibility.  bench.py times C2, C3 and C4 in this mode.  tests/test_gpu_wide.py holds the walks to the
oracle at the default options; this module runs the forms and schedules the lumo-mode tests run for
classes 4-64 (test_kernel_variants, test_bounce_modes_small_dragon, test_top_staging_budgets,
test_split_pipeline_passes_in_flight, test_split_merged_passes, tests/test_gpu_options.py and
tests/test_gpu_bdpt.py) with accel = 1.  tests/wide_matrix.py lists which test runs which launcher in
which staging form.

Bar: BIT-EXACT against the f64 oracle run with accel = 1 (oracle.cpp wide_walk, written independently
of the kernels): tile buffers, per-task num_rays / num_queries / num_camera_rays, the frame's closest /
shadow query totals, splat lists, and for lumo_trace t / kind / object / triangle and the three
traversal counters.  No tolerance anywhere.  Each case also asserts, from lumo_scene_info,
lumo_last_schedule, lumo_stats and the launch counts, that the form it names is the one that ran.
Schedule cases take a throw-away device (poisoned buffers, conftest); kernel-form cases share the
module's device and put its options back."""
import functools

import numpy as np
import pytest

import lumo_amd as L
import oracle_ffi as O
from lumo_amd import scenes
from lumo_amd.procedural import torus_knot_tube
from parity import (assert_paths_equal, assert_splats_equal, assert_tiles_equal, gpu_paths, oracle_threads,
                    stage_launches)
from scenes import DeepLightScene, default_camera, light_kd_depth, texture_zoo
from test_gpu_options import (_assert_query_totals, _caustics, _cornell, _crowded_cornell, _device, _mid_bistro,
                              _options, _render_counted)
from test_gpu_scale import _closest_rays, _visibility_rays
from test_gpu_wide import _trace_cmp

pytestmark = pytest.mark.gpu
SEED = 0x5EED1234
BDPT = L.Integrator.BDPathTrace
NODE_BYTES = 128  # wbvh.h Node


@pytest.fixture(scope="module")
def dev():
    d = L.Device(0, accel=1)
    assert d.option("accel") == 1
    yield d
    d.close()


# ---------------------------------------------------------------------------- scenes and oracle results (accel = 1)
@functools.lru_cache(maxsize=None)
def _small_dragon():
    return scenes.dragon(torus_knot_tube(300, 12)).build()


@functools.lru_cache(maxsize=None)
def _texture_zoo():
    return texture_zoo().build()


def _scene(name, res):
    if name == "cornell":
        return _cornell(), L.Camera.cornell_box(res)
    if name == "small_dragon":
        return _small_dragon(), scenes.default_camera(res)
    if name == "mid_bistro":
        return _mid_bistro(), scenes.bistro_camera(res)
    if name == "caustics":
        return _caustics(), scenes.caustics_camera(res)
    assert name == "texture_zoo"
    return _texture_zoo(), default_camera(res)


@functools.lru_cache(maxsize=None)
def _frame(name, res, spp, seed=SEED, first=None):
    """Scene, camera, tasks (the first `first` of the frame's) and the oracle's tiles, results and
    counters on the wide structures."""
    sc, cam = _scene(name, res)
    tasks = L.make_tasks(res[0], res[1], spp, seed)
    if first is not None:
        tasks = list(tasks)[:first]
    return (sc, cam, tasks) + O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads(), accel=1)


@functools.lru_cache(maxsize=None)
def _paths(name, res, spp, task):
    sc, cam = _scene(name, res)
    return O.trace_paths(sc.desc(), cam.desc, L.make_tasks(res[0], res[1], spp, SEED)[task], accel=1)


@functools.lru_cache(maxsize=None)
def _bdpt_frame(name, res, spp, seed):
    sc, cam = _scene(name, res)
    tasks = L.make_tasks(res[0], res[1], spp, seed)
    osp = []
    obufs, ores, _ = O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads(), integrator=BDPT,
                                    splats_out=osp, accel=1)
    assert sum(len(s) for s in osp) > 0
    return sc, cam, tasks, obufs, ores, osp


def _wide(info):
    """The uploaded scene walks the wide structures through the class-0 kernels."""
    assert (info.accel, info.stack_class) == (1, 0) and info.wide_nodes > 0, (info.accel, info.stack_class)
    return info


def _trace_equal(d, rays, want, lights=None):
    """lumo_trace against oracle answers computed once: t, kind, object, triangle (closest hits) and
    the traversal counters (child boxes, nodes, triangles)."""
    before = d.stats()
    g = d.trace(rays[0], rays[1], lights)
    after = d.stats()
    t, kind, obj, prim, cnt = want
    np.testing.assert_array_equal(g[0], t)
    np.testing.assert_array_equal(g[1], kind)
    np.testing.assert_array_equal(g[2], obj)
    if lights is None:
        np.testing.assert_array_equal(g[3], prim)
    k = 0 if lights is None else 1
    got = [after.aabb_tests[k] - before.aabb_tests[k], after.kd_nodes[k] - before.kd_nodes[k],
           after.tri_tests[k] - before.tri_tests[k]]
    assert got == [cnt.aabb_tests, cnt.kd_nodes, cnt.tri_tests]


# ---------------------------------------------------------------------------- 1. class-0 kernel variants
VARIANT = {"cornell": ((48, 40), 8), "small_dragon": ((48, 32), 8)}


@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", ["cornell", "small_dragon"])
def test_wide_kernel_variants(dev, name, lds, full):
    """test_kernel_variants for class 0 (accel = 1): LDS staging on / off x lean / forced full kernels.
    Cornell staged runs the fused bounce with the wide trees in LDS; with lds_staging 0 its packed
    scene stays in HBM and, being small enough to stage, has no TOP set either: the plain forms of
    k_closest_q / k_shade / k_shadow_q.  The small dragon (instanced: BLAS markers on the walk stack)
    exceeds 48 KiB and walks through the TOP forms.  Per-path parity of one task, then six tiles."""
    res, spp = VARIANT[name]
    sc, cam, tasks, obufs, ores, cnt = _frame(name, res, spp, first=6)
    with _options(dev, lds_staging=lds, full_kernels=full) as d:
        d.upload(sc, cam)
        info = _wide(d.scene_info())
        assert (info.lds_bytes > 0) == (lds == 1 and name == "cornell"), info.lds_bytes
        assert info.full_kernels == (1 if (full or name == "small_dragon") else 0)
        assert (info.top_wide_nodes > 0) == (name == "small_dragon"), info.top_wide_nodes
        assert_paths_equal(gpu_paths(d, tasks[1]), _paths(name, res, spp, 1))
        bufs, res_, before, after = _render_counted(d, tasks)
        assert d.last_schedule().fused == (1 if info.lds_bytes > 0 else 0)
    assert_tiles_equal(bufs, res_, obufs, ores)
    _assert_query_totals(before, after, cnt)


@pytest.mark.parametrize("tail", [0, 1 << 18])
def test_wide_split_kernels_staged(dev, tail):
    """Cornell staged in LDS with fused = 0: k_closest_q / k_shade / k_shadow_q reading the wide trees
    from the staged scene (the split pipeline, n_shadow 1), without and with the tail kernel (accel 1)."""
    sc, cam, tasks, obufs, ores, cnt = _frame("cornell", (48, 40), 8, first=6)
    with _options(dev, fused=0, tail_below=tail) as d:
        d.upload(sc, cam)
        info = _wide(d.scene_info())
        assert info.lds_bytes > 0 and info.n_shadow == 1
        bufs, res, before, after = _render_counted(d, tasks)
        assert d.last_schedule().fused == 0
        assert (after.tail_queries > before.tail_queries) == (tail > 0)
        assert stage_launches(before, after, "shadow") > 0
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


# ---------------------------------------------------------------------------- 2. bounce forms off LDS
@pytest.mark.parametrize("fused,tail,pipe", [(1, 0, 0), (1, 300, 0), (0, 1 << 30, 0), (1, 0, 1), (1, 0, 2), (1, 0, 3),
                                             (0, 0, 1), (0, 1 << 18, 1)])
def test_wide_bounce_modes_small_dragon(dev, fused, tail, pipe):
    """test_bounce_modes_small_dragon with accel = 1: the fused bounce and the tail kernel walking an
    instanced glass mesh from HBM (feature class 1, no LDS staging), in the pass loop, with the
    mid-pass hand-over to the tail kernel and on 1-3 head streams.  Paths and tiles equal the oracle's;
    tail queries grow exactly where a tail kernel is entered: below tail_below live paths, and at the
    end of every pass of the fused pipeline."""
    sc, cam, tasks, obufs, ores, cnt = _frame("small_dragon", (48, 32), 8, first=6)
    with _options(dev, fused=fused, tail_below=tail, pipeline=pipe) as d:
        d.upload(sc, cam)
        info = _wide(d.scene_info())
        assert info.lds_bytes == 0 and info.n_shadow == 1 and info.full_kernels == 1
        assert_paths_equal(gpu_paths(d, tasks[1]), _paths("small_dragon", (48, 32), 8, 1))
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
        assert sch.fused == fused
        if fused and pipe:
            assert (sch.schedule, sch.head_streams) == (1, pipe)
        entered = tail > 0 or (fused == 1 and pipe > 0)
        assert (after.tail_queries > before.tail_queries) == entered, after.tail_queries - before.tail_queries
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


# ---------------------------------------------------------------------------- 3. fused pipeline, staged
STAGED = {  # case -> (scene, resolution, passes, options besides accel / pipeline 3 / tail_below 300)
    "threads256": ("cornell", (48, 40), 9, dict(merge_passes=1)),
    "threads64_dyn": ("cornell", (48, 40), 9, dict(merge_passes=1, bounce_threads=64, dyn_fetch=1)),
    "merge3": ("cornell", (48, 40), 9, dict(merge_passes=3)),
    "merge3_ragged": ("cornell", (48, 40), 10, dict(merge_passes=3)),  # a last unit of one pass
    "texture_zoo": ("texture_zoo", (48, 32), 8, dict(merge_passes=1, fused=1)),
}


@pytest.mark.parametrize("case", list(STAGED))
def test_wide_fused_pipeline_staged(case):
    """render_pipelined in the wide mode (accel = 1): 3 head streams, the tail kernel below 300 live
    paths and at the end of every pass, on Cornell staged in LDS at 256 threads, at 64 threads with
    blocks fetching from a counter, with merged units of 3 passes (nine passes: three whole units; ten:
    a last unit of one pass), and the texture zoo (feature class 2, walk_hit_record's STK == 0 branch)
    through fused = 1."""
    name, res, spp, opts = STAGED[case]
    sc, cam, tasks, obufs, ores, cnt = _frame(name, res, spp)
    d = _device(accel=1, pipeline=3, tail_below=300, **opts)
    try:
        d.upload(sc, cam)
        info = _wide(d.scene_info())
        if name == "cornell":
            assert info.lds_bytes > 0 and info.full_kernels == 0
        else:
            assert info.full_kernels == 2
        bufs, res_, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
    finally:
        d.close()
    assert (sch.schedule, sch.fused, sch.head_streams, sch.merged_passes) == (1, 1, 3, opts["merge_passes"])
    assert after.tail_queries > before.tail_queries
    assert stage_launches(before, after, "resolve") == spp  # one tail kernel per pass
    assert_tiles_equal(bufs, res_, obufs, ores)
    _assert_query_totals(before, after, cnt)


# ---------------------------------------------------------------------------- 4. TOP prefix edges
@functools.lru_cache(maxsize=None)
def _bistro_rays():
    """test_top_staging_budgets' ray sets on mid_bistro and the oracle's wide answers and counters."""
    desc = _mid_bistro().desc()
    o, d = _closest_rays(desc, (-16.0, 5.0, -1.0), 1 << 17, 21)
    vo, vd, li = _visibility_rays(desc, 1 << 17, 22)
    return ((o, d), O.trace(desc, o, d, accel=1, with_prim=True)), \
           ((vo, vd), li, O.trace(desc, vo, vd, li, accel=1, with_prim=True))


@functools.lru_cache(maxsize=None)
def _smallest_top_kb():
    """The smallest top_kb, stepping upward from 5, at which mid_bistro gets a TOP set in wide mode
    (upload.hip: a budget of at least 4096 B after the kernels' 256 B, holding the object records and
    16 nodes)."""
    d = L.Device(0, accel=1)
    try:
        for kb in range(5, 161):
            d.set_option("top_kb", kb)
            d.upload(_mid_bistro())
            if d.scene_info().top_bytes > 0:
                return kb
    finally:
        d.close()
    raise AssertionError("no top_kb up to 160 gives mid_bistro a TOP set in wide mode")


@pytest.mark.parametrize("budget", ["smallest", "below", 20, None, "off"])
def test_wide_top_prefix_edges(budget):
    """The wide walk reads node i from LDS when i < top_wide_nodes and from HBM otherwise (accel = 1).
    mid_bistro with the smallest budget that stages anything (the prefix cuts the top levels), one KiB
    less (no TOP set: the plain HBM kernels), 20 KiB, the default budget (the CU's LDS) and
    top_staging 0: 2^17 closest rays and 2^17 visibility rays with their counters, then six tiles."""
    kb = {"smallest": _smallest_top_kb(), "below": _smallest_top_kb() - 1, "off": None}.get(budget, budget)
    opts = {"top_staging": 0 if budget == "off" else 1}
    if kb is not None:
        opts["top_kb"] = kb
    sc, cam, tasks, obufs, ores, cnt = _frame("mid_bistro", (64, 48), 9)
    (rays, want), (vrays, li, vwant) = _bistro_rays()
    d = _device(accel=1, **opts)
    try:
        d.upload(sc, cam)
        info = _wide(d.scene_info())
        assert info.lds_bytes == 0 and info.n_shadow > 1
        if budget in ("below", "off"):
            assert info.top_bytes == 0 and info.top_wide_nodes == 0
        else:
            assert info.top_bytes > 0 and 0 < info.top_wide_nodes <= info.wide_nodes
            cap = (kb if kb is not None else d.option("top_kb")) * 1024 - 256
            assert info.top_bytes <= cap
            # as many nodes as the budget holds beside the object records (16-B aligned), or the whole tree
            records = info.top_bytes - NODE_BYTES * info.top_wide_nodes
            assert info.top_wide_nodes == min(info.wide_nodes, (cap - records) // NODE_BYTES)
        if budget == "smallest":
            assert 0 < info.top_wide_nodes < info.wide_nodes
        print(f"top_kb {kb}: {info.top_wide_nodes} of {info.wide_nodes} wide nodes in {info.top_bytes} B of LDS")
        _trace_equal(d, rays, want)
        _trace_equal(d, vrays, vwant, li)
        sub = list(tasks)[:6]
        bufs, res, before, after = _render_counted(d, sub)
        assert d.last_schedule().fused == 0
    finally:
        d.close()
    assert_tiles_equal(bufs, res, obufs[:6], list(ores)[:6])


def test_wide_whole_tree_in_top():
    """The whole wide tree in the TOP prefix (top_wide_nodes == wide_nodes, so i < top_wnodes holds for
    every node and no walk reads a node from HBM): the first _crowded_cornell(n) that is no longer
    LDS-staged in wide mode (accel = 1), found as test_bounce_threads_decide_the_schedule finds its
    last staged one.  Rays with counters, then tiles through the split kernels' TOP forms."""
    stage_max = 48 * 1024
    cam = L.Camera.cornell_box((48, 40))
    tasks = L.make_tasks(48, 40, 8, SEED)
    d = L.Device(0, accel=1)
    try:
        d.upload(_cornell(), cam)
        base = _wide(d.scene_info()).lds_bytes
        d.upload(_crowded_cornell(8), cam)
        per = (d.scene_info().lds_bytes - base) / 8.0  # staged bytes per rectangle
        assert base > 0 and per > 0
        n = max(1, int((stage_max - base) / per) - 8)
        for n in range(n, n + 80):  # the first that is not staged
            sc = _crowded_cornell(n)
            d.upload(sc, cam)
            if d.scene_info().lds_bytes == 0:
                break
        else:
            raise AssertionError("every crowded Cornell tried is still LDS-staged")
        d.upload(_crowded_cornell(n - 1), cam)
        assert stage_max - 1024 < d.scene_info().lds_bytes <= stage_max  # n is the first: n - 1 is staged
        o, dd = _closest_rays(sc.desc(), (278.0, 273.0, -800.0), 1 << 16, 41)
        _trace_cmp(d, sc, o, dd)
        info = _wide(d.scene_info())
        assert info.lds_bytes == 0 and info.top_bytes > 0 and info.n_shadow == 1
        assert info.top_wide_nodes == info.wide_nodes
        print(f"crowded Cornell {n}: {info.wide_nodes} wide nodes, all in {info.top_bytes} B of LDS")
        o, dd, li = _visibility_rays(sc.desc(), 1 << 16, 42)
        _trace_cmp(d, sc, o, dd, li)
        d.upload(sc, cam)
        bufs, res, before, after = _render_counted(d, tasks)
        assert d.last_schedule().fused == 0
    finally:
        d.close()
    obufs, ores, cnt = O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads(), accel=1)
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


def test_wide_top_cut_in_blas():
    """The small dragon at top_kb = 8 (accel = 1): the breadth-first prefix holds the world trees and
    ends among the levels of the instanced mesh's BLAS, so a walk crosses between LDS and HBM nodes
    below a BLAS marker."""
    sc, cam, tasks, obufs, ores, cnt = _frame("small_dragon", (48, 32), 8, first=6)
    d = _device(accel=1, top_kb=8)
    try:
        desc = sc.desc()
        o, dd = _closest_rays(desc, (0.0, 0.0, 0.0), 1 << 16, 31)
        _trace_cmp(d, sc, o, dd)
        info = _wide(d.scene_info())
        assert info.lds_bytes == 0 and 0 < info.top_wide_nodes < info.wide_nodes
        acc = O.wide_export(desc)
        blas = [int(b) for b in list(acc["obj_blas"]) + list(acc["light_blas"]) if b >= 0]
        assert blas and min(blas) < info.top_wide_nodes  # a BLAS root is staged, its tree is not
        print(f"small dragon, top_kb 8: {info.top_wide_nodes} of {info.wide_nodes} wide nodes, BLAS roots {blas}")
        o, dd, li = _visibility_rays(desc, 1 << 16, 32)
        _trace_cmp(d, sc, o, dd, li)
        d.upload(sc, cam)
        bufs, res, before, after = _render_counted(d, tasks)
    finally:
        d.close()
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


# ---------------------------------------------------------------------------- 5. split pipeline in the bench's shape
@pytest.mark.parametrize("scene,k,groups,merge", [("mid_bistro", 1, 1, 1), ("mid_bistro", 4, 2, 1), ("mid_bistro", 4, 4, 1),
                                                   ("mid_bistro", 4, 2, 8), ("small_dragon", 2, 2, 4)])
def test_wide_split_pipeline(scene, k, groups, merge):
    """render_split_pipelined in the wide mode (accel = 1), as bench.py runs C3 and C2: mid_bistro
    (n_shadow > 1, TOP-staged) sequential, with 4 units in flight in 2 and in 4 task groups, with merged
    units of 8 passes (9 passes: a ragged last unit), and the small dragon (n_shadow 1) with 2 units of
    4 merged passes and the tail kernel below 300 live paths.  Tiles, counts and the frame's query
    totals equal the oracle's."""
    sc, cam, tasks, obufs, ores, cnt = _frame(scene, (64, 48), 9)
    opts = dict(tail_below=300) if scene == "small_dragon" else {}
    d = _device(accel=1, split_pipe=k, split_groups=groups, merge_passes=merge, **opts)
    try:
        d.upload(sc, cam)
        info = _wide(d.scene_info())
        assert info.lds_bytes == 0 and info.top_wide_nodes > 0
        assert (info.n_shadow > 1) == (scene == "mid_bistro")
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
    finally:
        d.close()
    want = (0, 1, 1, 1) if k == 1 else (2, k, min(groups, k), merge)
    assert (sch.schedule, sch.units_in_flight, sch.task_groups, sch.merged_passes) == want
    assert sch.fused == 0
    assert (after.tail_queries > before.tail_queries) == (scene == "small_dragon")
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


# ---------------------------------------------------------------------------- 6. BDPT
def _bdpt_render(d, tasks, **kw):
    sp = []
    before = d.stats()
    bufs, res = d.render_tasks(tasks, integrator=BDPT, splats_out=sp, **kw)
    return bufs, res, sp, before, d.stats()


@pytest.mark.parametrize("tail", [0, 300])
@pytest.mark.parametrize("name,res,spp", [("caustics", (40, 24), 4), ("cornell", (32, 32), 6)])
def test_wide_bdpt_walk_forms(dev, name, res, spp, tail):
    """test_bdpt_tiles_and_splats with accel = 1 away from the default walk tail: bdpt_tail 0 sends every
    walk bounce through k_closest + k_bdpt_step (no k_bdpt_tail launch: the only resolve-stage launches
    are the re-run and the fold of each pass), 300 hands over to k_bdpt_tail below 300 live subpaths.
    Cornell is LDS-staged in wide mode (the LDS forms of every BDPT traversal kernel); caustics.rs with
    its two instanced meshes is not (their plain forms, the visibility reading the TOP prefix)."""
    sc, cam, tasks, obufs, ores, osp = _bdpt_frame(name, res, spp, 0x5EED)
    with _options(dev, bdpt_tail=tail) as d:
        d.upload(sc, cam)
        info = _wide(d.scene_info())
        assert (info.lds_bytes > 0) == (name == "cornell") and (info.top_wide_nodes > 0) == (name == "caustics")
        bufs, rr, sp, before, after = _bdpt_render(d, tasks)
    passes = stage_launches(before, after, "camera")  # one per group and pass
    assert passes >= spp
    assert stage_launches(before, after, "closest") > 0
    assert stage_launches(before, after, "shade") == stage_launches(before, after, "closest")  # k_bdpt_step
    if tail == 0:
        assert stage_launches(before, after, "resolve") == 2 * passes
    else:
        assert stage_launches(before, after, "resolve") > 2 * passes
    assert stage_launches(before, after, "bd_vis") > 0
    assert_tiles_equal(bufs, rr, obufs, ores, camera_rays=True)
    assert_splats_equal(sp, osp)


@pytest.mark.parametrize("top", [0, 1])
def test_wide_bdpt_top_visibility(dev, top):
    """test_bdpt_top_visibility_matches_oracle with accel = 1.  Its caustics scene is LDS-staged in wide
    mode, so the scene here is the small dragon, which is not: the (b)-item visibility reads the TOP
    prefix of the wide nodes from LDS (bdpt_top 1) or every node from HBM (bdpt_top 0), and the walks,
    the re-runs and the (a)-item traces run their plain forms."""
    sc, cam, tasks, obufs, ores, osp = _bdpt_frame("small_dragon", (48, 32), 4, 0x70B)
    with _options(dev, bdpt_top=top) as d:
        d.upload(sc, cam)
        info = _wide(d.scene_info())
        assert info.lds_bytes == 0 and info.top_bytes > 0 and info.top_wide_nodes > 0
        bufs, rr, sp, before, after = _bdpt_render(d, tasks)
    assert stage_launches(before, after, "bd_vis") > 0 and stage_launches(before, after, "bd_trace_a") > 0
    assert_tiles_equal(bufs, rr, obufs, ores, camera_rays=True)
    assert_splats_equal(sp, osp)


@pytest.mark.parametrize("groups", [1, 3, 4])
@pytest.mark.parametrize("film", [0, 1], ids=["lists", "splat_film"])
def test_wide_bdpt_task_groups(groups, film):
    """test_bdpt_task_groups with accel = 1: caustics.rs in 1, 3 and 4 task groups, 5 passes, re-runs
    with max_vertices 6; splats as per-task lists (lumo's order) and summed into a film on the device
    (the order of that sum is unspecified: equal to the sequential sum of the exact lists to rounding,
    the bound of test_bdpt_splat_film_matches_lists)."""
    sc, cam, tasks, obufs, ores, osp = _bdpt_frame("caustics", (48, 32), 5, 0x6B0)
    d = _device(accel=1, bdpt_groups=groups)
    try:
        d.upload(sc, cam)
        _wide(d.scene_info())
        sp = []
        if film:
            dfilm = np.zeros((32, 48, 3))
            bufs, rr = d.render_tasks(tasks, integrator=BDPT, splat_film=dfilm, max_vertices=6)
        else:
            bufs, rr = d.render_tasks(tasks, integrator=BDPT, splats_out=sp, max_vertices=6)
        sch = d.last_schedule()
    finally:
        d.close()
    assert (sch.schedule, sch.task_groups) == ((3, groups) if groups > 1 else (0, 1))
    assert_tiles_equal(bufs, rr, obufs, ores, camera_rays=True)
    if film:
        seq = L.Film(48, 32, samples=5)
        for t, ob, s in zip(tasks, obufs, osp):
            seq.add_tile(t, ob, s)
        assert seq.splats.any()
        np.testing.assert_allclose(dfilm, seq.splats, rtol=1e-12, atol=1e-300)
    else:
        assert_splats_equal(sp, osp)


@pytest.mark.parametrize("name", ["caustics", "cornell"])
def test_wide_bdpt_long_subpaths_are_rerun(dev, name):
    """test_bdpt_long_subpaths_are_rerun with accel = 1: max_vertices = 3 sends almost every sample
    through k_bdpt_redo, walking the wide trees from HBM (caustics.rs, the lumo-mode test's scene) and
    staged in LDS (Cornell); nothing may change."""
    sc, cam, tasks, obufs, ores, osp = _bdpt_frame(name, (16, 16), 4, 77)
    dev.upload(sc, cam)
    assert (_wide(dev.scene_info()).lds_bytes > 0) == (name == "cornell")
    bufs, rr, sp, before, after = _bdpt_render(dev, tasks, max_vertices=3)
    assert_tiles_equal(bufs, rr, obufs, ores, camera_rays=True)
    assert_splats_equal(sp, osp)
    # the same frame with room for every subpath: the same results
    bufs, rr, sp, before, after = _bdpt_render(dev, tasks)
    assert_tiles_equal(bufs, rr, obufs, ores, camera_rays=True)
    assert_splats_equal(sp, osp)


@pytest.mark.parametrize("mode", [1, 2])
def test_wide_bdpt_walk_ray_sort(mode):
    """test_bdpt_walk_ray_sort with accel = 1: the walks' queues counting-sorted ahead of k_closest
    (bdpt_tail 0: no walk tail), caustics.rs at 320x208 in 2 task groups of 33 280 slots (the sort
    minimum is 32 768 rays), 1 pass."""
    sc, cam, tasks, obufs, ores, osp = _bdpt_frame("caustics", (320, 208), 1, 0x50A7)
    d = _device(accel=1, ray_sort=mode, bdpt_tail=0)
    try:
        d.upload(sc, cam)
        _wide(d.scene_info())
        bufs, rr, sp, before, after = _bdpt_render(d, tasks)
        assert d.last_schedule().schedule == 3
        assert after.sorted_bounces > before.sorted_bounces  # the sorted walk ran
    finally:
        d.close()
    assert_tiles_equal(bufs, rr, obufs, ores, camera_rays=True)
    assert_splats_equal(sp, osp)


# ---------------------------------------------------------------------------- 7. refusal and its boundary
def test_wide_refusal_and_boundary():
    """A device that asked for accel = 1 and a light kd tree at and past wbvh::LIGHT_KD_STACK (16
    levels; tests/scenes.py DeepLightScene, tests/test_wide.py test_light_kd_depth_limit): 16 levels is
    the last accepted depth and walks the wide trees, the sampled light's own kd walk pushing up to 15
    far sides on its 16-entry stack; 17 levels is refused, so the scene runs on lumo's structures with a kd stack
    class of its own; Cornell uploaded next on the same device is wide again (no state of the refusal
    stays), and with the option set to 0 and a re-upload it is lumo's."""
    cam = L.Camera.builder().origin(0.0, 0.5, 4.0).towards(0.0, 0.3, 0.0).resolution((48, 32)).build()
    tasks = L.make_tasks(48, 32, 8, SEED)
    ccam = L.Camera.cornell_box((48, 40))
    ctasks = L.make_tasks(48, 40, 8, SEED)

    def tiles(d, sc, cam, tasks, accel):
        d.upload(sc, cam)
        bufs, res, before, after = _render_counted(d, tasks)
        obufs, ores, cnt = O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads(), accel=accel)
        assert_tiles_equal(bufs, res, obufs, ores)
        _assert_query_totals(before, after, cnt)

    d = _device(accel=1)
    try:
        last = DeepLightScene(16)
        assert light_kd_depth(last.desc()) == 16
        o, dd = _closest_rays(last.desc(), (0.0, 0.5, 4.0), 1 << 15, 51)
        g = _trace_cmp(d, last, o, dd)  # asserts accel == 1
        assert np.mean(g[1] > 0) > 0.1  # a floor, a knot and a lamp in a large box of bounds
        o, dd, li = _visibility_rays(last.desc(), 1 << 15, 52)
        _trace_cmp(d, last, o, dd, li)
        _wide(d.scene_info())
        tiles(d, last, cam, tasks, 1)

        refused = DeepLightScene(17)
        assert light_kd_depth(refused.desc()) == 17
        d.upload(refused, cam)
        info = d.scene_info()
        assert info.accel == 0 and info.stack_class > 0 and info.wide_nodes == 0 and info.top_wide_nodes == 0
        assert d.option("accel") == 1  # the request stands
        tiles(d, refused, cam, tasks, 0)

        d.upload(_cornell(), ccam)
        info = _wide(d.scene_info())
        assert info.lds_bytes > 0
        tiles(d, _cornell(), ccam, ctasks, 1)

        d.set_option("accel", 0)
        d.upload(_cornell(), ccam)
        info = d.scene_info()
        assert info.accel == 0 and info.stack_class == 4 and info.wide_nodes == 0
        tiles(d, _cornell(), ccam, ctasks, 0)
    finally:
        d.close()
