"""GPU parity of the execution options' forms that no other module launches (tests/option_matrix.py
lists which test renders with which value): the fused bounce at 64 and 128 threads per block, explicit
tail-stream bounces (odd counts, merged units, more than the longest path), the film ahead of the
ring, the tail stream's priority and its re-creation, the snapshot ring at its shallowest and deepest,
TOP kernels on grids of 1 and 3 blocks, tiles larger than a block through every schedule, pixel
filters other than the default, and every option's documented range.

Bar: BIT-EXACT against the f64 oracle (tile buffers, per-task ray and query counts, the frame's
closest / shadow query totals where the neighbouring tests of the same schedule check them).  Each
case also asserts, from the option read back, lumo_last_schedule, lumo_scene_info and the launch
counts, that the form it names is the one that ran.  The session's buffers are poisoned (conftest):
the cases about a schedule (streams, sets, events, snapshot slots) each take a throw-away device, so
every buffer they touch starts as NaN / -1; the cases about a kernel form or a filter share the
module's device and put its options back (a context costs over a second late in a long session)."""
import contextlib
import functools

import numpy as np
import pytest

import lumo_amd as L
import oracle_ffi as O
from lumo_amd import _ffi, scenes
from option_matrix import OPTION_MATRIX
from parity import (assert_paths_equal, assert_splats_equal, assert_tiles_equal, gpu_paths, oracle_threads,
                    stage_launches)

pytestmark = pytest.mark.gpu
SEED = 0x5EED1234
BDPT = L.Integrator.BDPathTrace
PARK_BYTES = (12 + 9) * 8  # pt.h PARK_DOUBLES doubles of LDS per thread of the fused bounce
RR_DEPTH = 5               # path_trace.rs:60: the automatic head count of a pass below 2^21 slots


# ---------------------------------------------------------------------------- scenes and oracle results
@functools.lru_cache(maxsize=None)
def _cornell():
    return L.Scene.cornell_box()


@functools.lru_cache(maxsize=None)
def _mid_bistro():
    from lumo_amd.procedural import bistro_standin
    return scenes.bistro(bistro_standin(groups=48, lamps=160, n=8)).build()


@functools.lru_cache(maxsize=None)
def _caustics():
    return scenes.caustics().build()


def _oracle(sc, cam, tasks, **kw):
    obufs, ores, cnt = O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads(), **kw)
    return obufs, ores, cnt


@functools.lru_cache(maxsize=None)
def _cornell_frame(spp=24, res=(48, 40), accel=0):
    """Cornell 48x40 at 24 spp (test_gpu_parity's bounce-mode frame): scene, camera, tasks, oracle."""
    sc, cam = _cornell(), L.Camera.cornell_box(res)
    tasks = L.make_tasks(res[0], res[1], spp, SEED)
    return (sc, cam, tasks) + _oracle(sc, cam, tasks, accel=accel)


@functools.lru_cache(maxsize=None)
def _cornell_paths(spp):
    sc, cam, tasks = _cornell_frame(spp)[:3]
    return O.trace_paths(sc.desc(), cam.desc, tasks[4])


@functools.lru_cache(maxsize=None)
def _texture_zoo_frame():
    """The texture zoo 64x48 at 16 spp (test_gpu_textures' frame; feature class 2)."""
    from scenes import default_camera, texture_zoo
    sc, cam = texture_zoo().build(), default_camera((64, 48))
    tasks = L.make_tasks(64, 48, 16, 0x7E47)
    return (sc, cam, tasks) + _oracle(sc, cam, tasks)


@functools.lru_cache(maxsize=None)
def _bistro_frame():
    """mid_bistro 64x48 at 9 spp (test_gpu_scale's split-pipeline frame; n_shadow > 1, TOP-staged)."""
    sc, cam = _mid_bistro(), scenes.bistro_camera((64, 48))
    tasks = L.make_tasks(64, 48, 9, SEED)
    return (sc, cam, tasks) + _oracle(sc, cam, tasks)


def _large_tasks(spp):
    """Two 32x48 tasks covering a 64x48 frame, as test_large_tiles_match_oracle builds them."""
    seeds = [t.seed for t in L.make_tasks(64, 48, spp, SEED)]
    return (_ffi.TileTask * 2)(*[_ffi.TileTask((32 * i, 0), (32 * i + 32, 48), 0, spp, spp, seeds[i]) for i in range(2)])


@functools.lru_cache(maxsize=None)
def _large_frame(which):
    if which == "cornell":
        sc, cam = _cornell(), L.Camera.cornell_box((64, 48))
    else:
        sc, cam = _mid_bistro(), scenes.bistro_camera((64, 48))
    tasks = _large_tasks(12)
    return (sc, cam, tasks) + _oracle(sc, cam, tasks)


@functools.lru_cache(maxsize=None)
def _bdpt_frame(res, spp, seed):
    """caustics.rs at the sizes test_gpu_bdpt uses: tiles and per-task splat lists of the oracle."""
    sc, cam = _caustics(), scenes.caustics_camera(res)
    tasks = L.make_tasks(res[0], res[1], spp, seed)
    osp = []
    obufs, ores, _ = _oracle(sc, cam, tasks, integrator=BDPT, splats_out=osp)
    assert sum(len(s) for s in osp) > 0
    return sc, cam, tasks, obufs, ores, osp


def _set(dev, **opts):
    """Set the options and assert that each reads back."""
    for k, v in opts.items():
        dev.set_option(k, v)
        assert dev.option(k) == v, k
    return dev


def _device(**opts):
    d = L.Device(0, **opts)
    for k, v in opts.items():
        assert d.option(k) == v, k
    return d


@contextlib.contextmanager
def _options(dev, **opts):
    """The options set on a live device (each read back) and put back afterwards."""
    start = {k: dev.option(k) for k in opts}
    try:
        yield _set(dev, **opts)
    finally:
        for k, v in start.items():
            dev.set_option(k, v)


@pytest.fixture(scope="module")
def dev():
    d = L.Device(0)
    yield d
    d.close()


def _render_counted(d, tasks, **kw):
    before = d.stats()
    bufs, res = d.render_tasks(tasks, **kw)
    return bufs, res, before, d.stats()


def _assert_query_totals(before, after, cnt):
    assert after.closest_queries - before.closest_queries == cnt.closest_queries
    assert after.shadow_queries - before.shadow_queries == cnt.shadow_queries


# ---------------------------------------------------------------------------- 1. fused bounce at 64 / 128 threads
# form -> (frame, options besides the plain fused pass loop, what lumo_scene_info must show)
FORMS = {
    "lds_lean": ("cornell", {}, lambda i: i.lds_bytes > 0 and i.full_kernels == 0 and i.accel == 0),
    "lds_full": ("cornell", {"full_kernels": 1}, lambda i: i.lds_bytes > 0 and i.full_kernels == 1),
    "not_staged": ("cornell", {"lds_staging": 0}, lambda i: i.lds_bytes == 0 and i.full_kernels == 0),
    "textured": ("texture_zoo", {}, lambda i: i.full_kernels == 2),
    "wide": ("cornell_wide", {"accel": 1}, lambda i: i.accel == 1 and i.lds_bytes > 0),
    "lds_lean_dyn": ("cornell", {"dyn_fetch": 1}, lambda i: i.lds_bytes > 0 and i.full_kernels == 0),
    "lds_lean_grid5": ("cornell", {"lds_grid": 5}, lambda i: i.lds_bytes > 0 and i.full_kernels == 0),
}


def _frame(name):
    if name == "texture_zoo":
        return _texture_zoo_frame()
    return _cornell_frame(accel=1 if name == "cornell_wide" else 0)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("threads", [64, 128])
def test_fused_bounce_threads(dev, threads, form):
    """k_bounce_q<.., TAIL = false> at 64 and 128 threads per block (bounce_threads), on the plain pass
    loop with no tail kernel, so every bounce of every path runs in the narrow blocks: the parked NEE
    records at k * nt + threadIdx.x behind the staged scene, block_slot's scan over nt / 64 waves, the
    grid of BLOCK / nt times as many blocks.  LDS-staged lean and full kernels, the scene in HBM, the
    textured class, the wide accel; the lean form also with blocks fetching from a counter and with a
    grid of 5 (x BLOCK / nt) blocks, each striding many times."""
    frame, extra, shows = FORMS[form]
    sc, cam, tasks, obufs, ores, cnt = _frame(frame)
    with _options(dev, bounce_threads=threads, pipeline=0, fused=1, tail_below=0, **extra) as d:
        d.upload(sc, cam)  # the upload options among them take effect here
        info = d.scene_info()
        assert info.n_shadow == 1 and shows(info), (info.lds_bytes, info.full_kernels, info.accel)
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
        assert (sch.schedule, sch.fused) == (0, 1)
        assert after.tail_queries == before.tail_queries  # no path left the narrow bounce kernel
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


@pytest.mark.parametrize("threads", [64, 128])
def test_bounce_threads_with_tail_mid_pass(threads):
    """The default pipeline (3 head streams) with the narrow bounce and the tail entered below 300
    live paths: the 256-thread tail kernel and the bounce_threads-wide bounce share every pass, on the
    head streams and (tail_bounces, automatic 2) on the tail stream."""
    sc, cam, tasks, obufs, ores, cnt = _cornell_frame()
    d = _device(bounce_threads=threads, pipeline=3, tail_below=300, merge_passes=1)
    try:
        d.upload(sc, cam)
        assert d.scene_info().lds_bytes > 0
        assert_paths_equal(gpu_paths(d, tasks[4]), _cornell_paths(24))
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
        assert (sch.schedule, sch.fused, sch.head_streams, sch.merged_passes, sch.tail_bounces) == (1, 1, 3, 1, 2)
        assert stage_launches(before, after, "closest") == (RR_DEPTH + 2) * 24
        assert after.tail_queries > before.tail_queries
    finally:
        d.close()
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


def _crowded_cornell(extra):
    """The Cornell box with `extra` more small rectangles on its floor: a larger staged scene."""
    sc = L.Scene.cornell_box()
    grey = L.Material.lambertian(L.Spectrum.from_rgb(0.5, 0.5, 0.5))
    for k in range(extra):
        x, z = 30.0 + 25.0 * (k % 20), 30.0 + 25.0 * (k // 20)
        sc.add_rectangle((x, 1.0 + (k % 7), z), (x + 20.0, 1.0 + (k % 7), z), (x + 20.0, 1.0 + (k % 7), z + 20.0), grey)
    return sc.build()


def test_bounce_threads_decide_the_schedule():
    """fused = -1 takes the fused bounce when the scene is staged and, with the parked records of a block
    (PARK_DOUBLES * 8 * threads bytes), fits the LDS one block may allocate.  On MI355X a block may
    allocate the CU's whole 160 KiB, and a staged scene is at most 48 KiB (LUMO_OPT_LDS_STAGING), so the
    two together reach at most 90 KiB: no scene runs fused at 64 threads and unfused at 256.  What does
    decide the schedule here is the staging limit.  So: Cornell plus as many rectangles as keep it
    staged (within 1 KiB of 48 KiB) runs the fused bounce at 256, 128 and 64 threads, the 256-thread
    blocks with 90 KiB of dynamic LDS, the most any launch of this kernel asks for; one rectangle more
    and the scene is not staged and runs three kernels per bounce.  All equal the oracle."""
    block_lds, stage_max = 160 * 1024, 48 * 1024
    assert stage_max + PARK_BYTES * 256 <= block_lds  # the window of sizes between the two limits is empty
    d = L.Device(0, pipeline=0)
    try:
        cam = L.Camera.cornell_box((48, 40))
        tasks = L.make_tasks(48, 40, 8, SEED)
        d.upload(_cornell(), cam)
        base = d.scene_info().lds_bytes
        d.upload(_crowded_cornell(40), cam)
        per = (d.scene_info().lds_bytes - base) / 40.0  # staged bytes per rectangle
        assert base > 0 and per > 0
        n = int((stage_max - base) / per) + 4
        while n > 0:  # the most rectangles that stay staged
            sc = _crowded_cornell(n)
            d.upload(sc, cam)
            if d.scene_info().lds_bytes > 0:
                break
            n -= 1
        info = d.scene_info()
        assert stage_max - 1024 < info.lds_bytes <= stage_max and info.n_shadow == 1, info.lds_bytes
        obufs, ores, cnt = _oracle(sc, cam, tasks)
        for threads in (256, 128, 64):
            _set(d, bounce_threads=threads, fused=-1)
            bufs, res, before, after = _render_counted(d, tasks)
            assert (d.last_schedule().schedule, d.last_schedule().fused) == (0, 1), threads
            assert_tiles_equal(bufs, res, obufs, ores)
            _assert_query_totals(before, after, cnt)
        sc = _crowded_cornell(n + 1)
        d.upload(sc, cam)
        assert d.scene_info().lds_bytes == 0 and d.scene_info().n_shadow == 1
        obufs, ores, cnt = _oracle(sc, cam, tasks)
        bufs, res, before, after = _render_counted(d, tasks)
        assert (d.last_schedule().schedule, d.last_schedule().fused) == (0, 0)
        assert_tiles_equal(bufs, res, obufs, ores)
        _assert_query_totals(before, after, cnt)
    finally:
        d.close()


# ---------------------------------------------------------------------------- 2. tail-stream bounces
TAIL_CASES = [(bb, merge, 24, heads) for bb in (0, 1, 3, 16) for merge in (1, 3) for heads in (0, 4)] + [(1, 3, 25, 0)]


@pytest.mark.parametrize("bb,merge,spp,heads", TAIL_CASES)
def test_tail_bounces(bb, merge, spp, heads):
    """render_pipelined with an explicit number of fused bounces per pass on the tail stream: none, an
    odd count (the ping-pong queues change roles before the tail kernel), 3, and 16 (more than most
    paths live: launches on an empty queue), with one-pass units and with merged units of 3 passes
    (per-pass queue segments and counters; 25 passes: a last unit of one pass), after 5 (automatic)
    or 4 head bounces.  Paths with their per-pass delta, tiles, counts and query totals equal the
    oracle's; the closest-stage launches are the head bounces of every unit and bb per pass."""
    sc, cam, tasks, obufs, ores, cnt = _cornell_frame(spp)
    d = _device(tail_bounces=bb, merge_passes=merge, heads=heads)
    try:
        d.upload(sc, cam)
        assert_paths_equal(gpu_paths(d, tasks[4]), _cornell_paths(spp))
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
    finally:
        d.close()
    want_heads = min(heads or RR_DEPTH, RR_DEPTH) if merge > 1 else (heads or RR_DEPTH)
    assert (sch.schedule, sch.fused, sch.merged_passes, sch.head_bounces, sch.tail_bounces) == (1, 1, merge, want_heads, bb)
    units = -(-spp // merge)
    assert stage_launches(before, after, "closest") == want_heads * units + bb * spp
    assert stage_launches(before, after, "resolve") == spp  # one tail kernel per pass
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


# ---------------------------------------------------------------------------- 3. film before the ring; tail priority
@pytest.mark.parametrize("pipe", [3, 2])
@pytest.mark.parametrize("merge", [1, 3])
def test_film_first(merge, pipe):
    """film_first = 1: with 3 head streams the film shares the tail stream and k_finish_film moves ahead
    of the unit's last k_ring; with 2 the film has a stream of its own and the option changes nothing.
    16x16 tiles, one-pass and merged units: one film launch per unit and one ring per pass either way."""
    sc, cam, tasks, obufs, ores, cnt = _cornell_frame()
    d = _device(film_first=1, pipeline=pipe, merge_passes=merge)
    try:
        d.upload(sc, cam)
        assert_paths_equal(gpu_paths(d, tasks[4]), _cornell_paths(24))
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
    finally:
        d.close()
    assert (sch.schedule, sch.head_streams, sch.merged_passes) == (1, pipe, merge)
    assert stage_launches(before, after, "film") == -(-24 // merge)
    assert stage_launches(before, after, "ring") == 24
    assert stage_launches(before, after, "finish") == 0  # the fused per-tile film, not k_finish + k_film
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


def test_tail_priority():
    """tail_priority = 1 from creation, then switched on a live context between renders (0 -> 1 -> 0:
    lumo_set_option destroys and recreates the tail stream each time): every render of the same tasks
    equals the oracle's, so all equal each other."""
    sc, cam, tasks, obufs, ores, cnt = _cornell_frame()
    d = _device(tail_priority=1)
    try:
        d.upload(sc, cam)
        bufs, res, before, after = _render_counted(d, tasks)
        assert d.last_schedule().schedule == 1
        assert_tiles_equal(bufs, res, obufs, ores)
        _assert_query_totals(before, after, cnt)
    finally:
        d.close()
    d = L.Device(0)
    try:
        d.upload(sc, cam)
        for v in (0, 1, 0):
            _set(d, tail_priority=v)
            bufs, res, before, after = _render_counted(d, tasks)
            assert d.last_schedule().schedule == 1
            assert_tiles_equal(bufs, res, obufs, ores)
            _assert_query_totals(before, after, cnt)
    finally:
        d.close()


# ---------------------------------------------------------------------------- 4. snapshot ring depth
@pytest.mark.parametrize("where", ["fused_loop", "split_loop", "split_pipeline", "bdpt_groups"])
@pytest.mark.parametrize("ahead", [1, 15])
def test_bounce_ahead(ahead, where):
    """bounce_ahead at its lowest and highest value in each scheduler that sizes its pinned snapshot
    ring by it: the sequential loop with fused bounces (Cornell) and with three kernels per bounce
    (mid_bistro, n_shadow > 1), render_split_pipelined (4 units in 2 task groups) and the BDPT task
    groups (2 groups, lists)."""
    if where == "bdpt_groups":
        sc, cam, tasks, obufs, ores, osp = _bdpt_frame((48, 32), 5, 0x6B0)
        d = _device(bounce_ahead=ahead, bdpt_groups=2)
        try:
            d.upload(sc, cam)
            sp = []
            bufs, res = d.render_tasks(tasks, integrator=BDPT, splats_out=sp, max_vertices=6)
            sch = d.last_schedule()
        finally:
            d.close()
        assert (sch.schedule, sch.task_groups) == (3, 2)
        assert_tiles_equal(bufs, res, obufs, ores, camera_rays=True)
        assert_splats_equal(sp, osp)
        return
    if where == "fused_loop":
        frame, opts, want = _cornell_frame(), dict(pipeline=0), (0, 1, 1)
    elif where == "split_loop":
        frame, opts, want = _bistro_frame(), dict(pipeline=0), (0, 0, 1)
    else:
        frame, opts, want = _bistro_frame(), dict(split_pipe=4, split_groups=2, merge_passes=1), (2, 0, 4)
    sc, cam, tasks, obufs, ores, cnt = frame
    d = _device(bounce_ahead=ahead, **opts)
    try:
        d.upload(sc, cam)
        assert (d.scene_info().n_shadow > 1) == (where != "fused_loop")
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
    finally:
        d.close()
    assert (sch.schedule, sch.fused, sch.units_in_flight) == want
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


@functools.lru_cache(maxsize=None)
def _cornell_300():
    sc, cam = _cornell(), L.Camera.cornell_box((40, 24))
    tasks = L.make_tasks(40, 24, 300, SEED)
    return (sc, cam, tasks) + _oracle(sc, cam, tasks)


def test_bounce_ahead_many_passes():
    """300 passes of the sequential loop with bounce_ahead 15 (test_multi_batch_tiles_match_oracle's
    frame): each pass leaves up to 15 bounces enqueued past its last live one, and the next pass
    records the same snapshot slots and events again."""
    sc, cam, tasks, obufs, ores, cnt = _cornell_300()
    d = _device(bounce_ahead=15, pipeline=0)
    try:
        d.upload(sc, cam)
        bufs, res, before, after = _render_counted(d, tasks)
        assert (d.last_schedule().schedule, d.last_schedule().fused) == (0, 1)
    finally:
        d.close()
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


# ---------------------------------------------------------------------------- 5. TOP kernels striding
@functools.lru_cache(maxsize=None)
def _bistro_rays():
    """test_top_staging_budgets' ray sets on mid_bistro and the oracle's answers and counters."""
    from test_gpu_scale import _closest_rays, _visibility_rays
    desc = _mid_bistro().desc()
    o, d = _closest_rays(desc, (-16.0, 5.0, -1.0), 1 << 17, 21)
    vo, vd, li = _visibility_rays(desc, 1 << 17, 22)
    return (o, d, O.trace(desc, o, d)), (vo, vd, li, O.trace(desc, vo, vd, li))


@pytest.mark.parametrize("grid", [1, 3])
def test_top_grid_trace(dev, grid):
    """k_trace's TOP form on a grid of 1 and of 3 blocks of 1 024 threads: 2^17 rays, so every thread
    goes round its grid-stride loop 43 to 128 times (the default grid of 128 blocks: once).  Closest
    hits and light visibility, with the traversal counters."""
    (o, dd, ref), (vo, vd, li, vref) = _bistro_rays()
    with _options(dev, top_grid=grid) as d:
        d.upload(_mid_bistro())
        info = d.scene_info()
        assert info.top_bytes > 0 and info.lds_bytes == 0
        for k, (ro, rd, lights, want) in enumerate(((o, dd, None, ref), (vo, vd, li, vref))):
            before = d.stats()
            g = d.trace(ro, rd, lights)
            after = d.stats()
            t, kind, obj, cnt = want
            np.testing.assert_array_equal(g[0], t)
            np.testing.assert_array_equal(g[1], kind)
            np.testing.assert_array_equal(g[2], obj)
            got = [after.aabb_tests[k] - before.aabb_tests[k], after.kd_nodes[k] - before.kd_nodes[k],
                   after.tri_tests[k] - before.tri_tests[k]]
            assert got == [cnt.aabb_tests, cnt.kd_nodes, cnt.tri_tests]


@pytest.mark.parametrize("grid", [1, 3])
def test_top_grid_render(dev, grid):
    """k_closest_q and k_shadow_q in their TOP forms on 1 and 3 blocks: mid_bistro 64x48 at 9 spp holds
    3 072 paths and several times as many visibility queries per bounce, so the blocks stride."""
    sc, cam, tasks, obufs, ores, cnt = _bistro_frame()
    with _options(dev, top_grid=grid) as d:
        d.upload(sc, cam)
        info = d.scene_info()
        assert info.top_bytes > 0 and info.lds_bytes == 0 and info.n_shadow > 1
        bufs, res, before, after = _render_counted(d, tasks)
        assert d.last_schedule().fused == 0
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


@pytest.mark.parametrize("grid", [1, 3])
def test_top_grid_bdpt(dev, grid):
    """k_bdpt_vis reading the TOP set from LDS (bdpt_top = 1) on 1 and 3 blocks: the caustics scene of
    test_bdpt_top_visibility_matches_oracle."""
    sc, cam, tasks, obufs, ores, osp = _bdpt_frame((48, 32), 4, 0x70B)
    with _options(dev, top_grid=grid, bdpt_top=1) as d:
        d.upload(sc, cam)
        info = d.scene_info()
        assert info.lds_bytes == 0 and info.top_bytes > 0 and info.top_kd_nodes > 0
        sp = []
        bufs, res = d.render_tasks(tasks, integrator=BDPT, splats_out=sp)
    assert_tiles_equal(bufs, res, obufs, ores, camera_rays=True)
    assert_splats_equal(sp, osp)


# ---------------------------------------------------------------------------- 6. large tiles through every schedule
@pytest.mark.parametrize("pipe,merge", [(0, 1), (1, 1), (1, 3), (3, 1), (3, 3)])
def test_large_tiles_fused_schedules(pipe, merge):
    """Two 32x48 tasks (more pixels than a block: k_finish + k_film per pass on the tail stream, the
    film event recorded there) at 12 spp through the sequential loop and render_pipelined with 1 and 3
    head streams, one-pass and merged units: 12 or 4 units over 2 or 4 sets, so every set is reused."""
    sc, cam, tasks, obufs, ores, cnt = _large_frame("cornell")
    d = _device(pipeline=pipe, merge_passes=merge)
    try:
        d.upload(sc, cam)
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
    finally:
        d.close()
    if pipe == 0:
        assert (sch.schedule, sch.fused) == (0, 1)
    else:
        assert (sch.schedule, sch.fused, sch.head_streams, sch.merged_passes) == (1, 1, pipe, merge)
    assert stage_launches(before, after, "finish") == 12 and stage_launches(before, after, "film") == 12
    for b in bufs:
        assert b.shape == (4 * 32 * 48,)
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


@pytest.mark.parametrize("merge", [1, 3])
def test_large_tiles_split_pipeline(merge):
    """The same two 32x48 tasks on mid_bistro through render_split_pipelined: 4 units in flight in 2
    task groups (one task each), one-pass and merged units."""
    sc, cam, tasks, obufs, ores, cnt = _large_frame("bistro")
    d = _device(split_pipe=4, split_groups=2, merge_passes=merge)
    try:
        d.upload(sc, cam)
        assert d.scene_info().n_shadow > 1
        bufs, res, before, after = _render_counted(d, tasks)
        sch = d.last_schedule()
    finally:
        d.close()
    assert (sch.schedule, sch.units_in_flight, sch.task_groups, sch.merged_passes) == (2, 4, 2, merge)
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)


def test_large_tiles_bdpt_groups():
    """The two 32x48 tasks on Cornell through the BDPT task groups, one task per group, at 2 spp: each
    group's film is k_finish + k_film per pass on the group's stream, over the group's slots of the
    render's whole per-slot view.  Tiles, counts and per-task splat lists equal the oracle's."""
    sc, cam, tasks = _cornell(), L.Camera.cornell_box((64, 48)), _large_tasks(2)
    osp = []
    obufs, ores, _ = _oracle(sc, cam, tasks, integrator=BDPT, splats_out=osp)
    d = _device(bdpt_groups=2)
    try:
        d.upload(sc, cam)
        sp = []
        bufs, res, before, after = _render_counted(d, tasks, integrator=BDPT, splats_out=sp, max_vertices=6)
        sch = d.last_schedule()
    finally:
        d.close()
    assert (sch.schedule, sch.task_groups) == (3, 2)
    # k_finish once per group and pass, as the camera (the wrapper renders again if a splat list was short)
    cameras = stage_launches(before, after, "camera")
    assert cameras >= 2 * 2 and stage_launches(before, after, "finish") == cameras
    assert_tiles_equal(bufs, res, obufs, ores, camera_rays=True)
    assert_splats_equal(sp, osp)


# ---------------------------------------------------------------------------- 7. pixel filter footprints
FILTERS = [(1.5, 0.2), (1.0, 0.5), (0.6, 0.375), (1.5, 3.0)]


def _filter_camera(radius, sigma):
    return L.Camera.cornell_box_builder().resolution((40, 24)).filter(radius, sigma).build()


@functools.lru_cache(maxsize=None)
def _filter_frame(radius, sigma, form):
    """Cornell 40x24 at 9 spp (ragged right and bottom tiles) under a Gaussian (radius, sigma) filter."""
    sc, cam = _cornell(), _filter_camera(radius, sigma)
    assert (cam.desc.filter_radius, cam.desc.filter_sigma) == (radius, sigma)
    tasks = L.make_tasks(40, 24, 9, SEED)
    if form == "large_tile":  # one task of 960 pixels
        tasks = (_ffi.TileTask * 1)(_ffi.TileTask((0, 0), (40, 24), 0, 9, 9, tasks[0].seed))
    if form == "bdpt":
        osp = []
        obufs, ores, _ = _oracle(sc, cam, tasks, integrator=BDPT, splats_out=osp)
        assert sum(len(s) for s in osp) > 0
        return sc, cam, tasks, obufs, ores, osp
    return (sc, cam, tasks) + _oracle(sc, cam, tasks)


@pytest.mark.parametrize("form", ["tile_film", "large_tile"])
@pytest.mark.parametrize("radius,sigma", FILTERS)
def test_pixel_filter(dev, radius, sigma, form):
    """gauss(., sigma) - gauss(radius, sigma) over the 3x3 footprint with a narrow and a wide sigma and
    radii from just above 0.5 to 1.5: k_finish_film (16x16 tiles) and k_finish + k_film (one 40x24 task)."""
    sc, cam, tasks, obufs, ores, cnt = _filter_frame(radius, sigma, form)
    dev.upload(sc, cam)
    bufs, res, before, after = _render_counted(dev, tasks)
    assert stage_launches(before, after, "finish") == (9 if form == "large_tile" else 0)
    assert_tiles_equal(bufs, res, obufs, ores)
    _assert_query_totals(before, after, cnt)
    default = _filter_frame(1.5, 0.375, form)[3]
    assert not np.array_equal(np.concatenate(obufs), np.concatenate(default))  # the filter matters


@pytest.mark.parametrize("radius,sigma", FILTERS)
def test_pixel_filter_bdpt(dev, radius, sigma):
    """BDPT under the same filters: the tiles, the light-tracing taps as per-task lists (k_bdpt_taps,
    bit-exact in lumo's order) and summed into a splat film (the order of that sum is unspecified, as
    lumo's tile completion order: equal to the sequential sum of the exact lists to rounding, the
    bound of test_bdpt_splat_film_matches_lists)."""
    sc, cam, tasks, obufs, ores, osp = _filter_frame(radius, sigma, "bdpt")
    dev.upload(sc, cam)
    sp = []
    bufs, res = dev.render_tasks(tasks, integrator=BDPT, splats_out=sp)
    assert_tiles_equal(bufs, res, obufs, ores, camera_rays=True)
    assert_splats_equal(sp, osp)
    film = np.zeros((24, 40, 3))
    bufs2, res2 = dev.render_tasks(tasks, integrator=BDPT, splat_film=film)
    assert_tiles_equal(bufs2, res2, obufs, ores, camera_rays=True)
    seq = L.Film(40, 24, samples=9, filter_radius=radius, filter_sigma=sigma)
    for t, ob, s in zip(tasks, obufs, osp):
        seq.add_tile(t, ob, s)
    assert seq.splats.any()
    np.testing.assert_allclose(film, seq.splats, rtol=1e-12, atol=1e-300)


def test_pixel_filter_refusals(dev):
    """Radii outside (0.5, 1.5] need another footprint than 3x3: UNSUPPORTED at lumo_camera_set, and the
    context keeps the camera it had.  A zero or NaN radius or sigma is INVALID, at the builder and at
    lumo_camera_set."""
    sc, cam, tasks, obufs, ores, cnt = _filter_frame(1.0, 0.5, "tile_film")
    dev.upload(sc, cam)
    for radius in (0.5, 1.51):
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            dev.upload(sc, _filter_camera(radius, 0.375))
    for radius, sigma in ((0.0, 0.375), (float("nan"), 0.375), (1.5, 0.0), (1.5, float("nan"))):
        with pytest.raises(RuntimeError, match="INVALID"):
            _filter_camera(radius, sigma)
        bad = _filter_camera(1.5, 0.375)
        bad.desc.filter_radius, bad.desc.filter_sigma = radius, sigma
        with pytest.raises(RuntimeError, match="INVALID"):
            dev.upload(sc, bad)
    bufs, res = dev.render_tasks(tasks)  # still the (1.0, 0.5) camera
    assert_tiles_equal(bufs, res, obufs, ores)


# ---------------------------------------------------------------------------- 8. option ranges as documented
def test_option_ranges_as_documented():
    """Every row of tests/option_matrix.py on a device: the documented lowest and highest value are
    accepted and read back, one below and one above are INVALID and leave the value alone, as is a
    value inside the range that is not one of a listed set.  top_kb's upper bound is the device's LDS
    per CU in KiB, which is also its default."""
    d = L.Device(0)
    try:
        assert list(OPTION_MATRIX) == list(_ffi.OPTIONS)
        for name, row in OPTION_MATRIX.items():
            start = d.option(name)
            if row.default is not None and name != "poison":  # the session's LUMO_POISON
                assert start == row.default, name
            hi = row.hi if row.hi is not None else start
            try:
                for v in (row.lo, hi):
                    d.set_option(name, v)
                    assert d.option(name) == v, (name, v)
                bad = [row.lo - 1, hi + 1]
                if row.values is not None:
                    bad += [v for v in range(row.lo, hi + 1) if v not in row.values][:3]
                    for v in row.values:
                        d.set_option(name, v)
                        assert d.option(name) == v, (name, v)
                for v in bad:
                    kept = d.option(name)
                    with pytest.raises(RuntimeError, match="INVALID"):
                        d.set_option(name, v)
                    assert d.option(name) == kept, (name, v)
            finally:
                d.set_option(name, start)
            assert d.option(name) == start
    finally:
        d.close()
