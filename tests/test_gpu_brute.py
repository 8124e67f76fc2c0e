"""The HIP traversal kernels on the adversarial ray families of tests/rays.py.

* Wide mode: lumo_trace over every family, on every scene of test_wide.NAMES (the builder's edge
  scenes included), equals the oracle's wide walk bit for bit (t / kind / object / triangle and the
  three traversal counters, test_gpu_wide._trace_cmp) and obeys the brute-force rule of
  tests/test_brute.py: equal to a reference that tests every primitive with no structure.
* Lumo mode: the same rays through lumo's kd and BVH kernels equal the oracle's restatement bit for
  bit, counters included.  Zero and -0.0 direction components, origins on split planes and
  directions below the f32 range of 1 / d reach these kernels nowhere else in the suite.
* Both k_trace forms: TOP staging off / on with the staged prefix cutting the tree, and the
  whole-in-LDS path.
* Axis-parallel primary rays through the render kernels: an orthographic camera looking exactly
  along an axis, path traced in both accel modes through the fused and the split bounce schedules.

A mismatch here with tests/test_brute.py green is a kernel bug."""
import functools

import numpy as np
import pytest

import lumo_amd as L
import oracle_ffi as O
import rays
import test_brute as B
from parity import oracle_threads
from scenes import material_zoo
from test_gpu_scale import _trace_cmp as _trace_cmp_lumo
from test_gpu_wide import _tiles_cmp, _trace_cmp
from test_wide import NAMES

pytestmark = pytest.mark.gpu
SEED = 0x1DE


@pytest.fixture(scope="module")
def devs():
    d = {"lumo": L.Device(0), "wide": L.Device(0, accel=1)}
    yield d
    for x in d.values():
        x.close()


@functools.lru_cache(maxsize=None)
def _families(name):
    """Every family of the scene: list of (family, origins, directions, lights or None)."""
    return [(f,) + B.family_rays(name, f) for f in rays.CLOSEST + rays.VISIBILITY]


def _joined(name, vis):
    fam = [x for x in _families(name) if (x[3] is not None) == vis]
    o, d = np.concatenate([x[1] for x in fam]), np.concatenate([x[2] for x in fam])
    li = np.concatenate([x[3] for x in fam]) if vis else None
    bounds = np.cumsum([0] + [len(x[1]) for x in fam])
    return [x[0] for x in fam], o, d, li, bounds


@pytest.mark.parametrize("mode", ["wide", "lumo"])
@pytest.mark.parametrize("name", NAMES)
def test_trace_adversarial_rays(devs, name, mode):
    sc, desc, _, _ = B.scene(name)
    for vis in (False, True):
        fams, o, d, li, bounds = _joined(name, vis)
        if name == "cornell":  # staged whole in LDS: the other k_trace form (TOP staging: below)
            devs[mode].upload(sc)
            assert devs[mode].scene_info().lds_bytes > 0
        if mode == "lumo":
            _trace_cmp_lumo(devs["lumo"], sc, o, d, li)
            continue
        g = _trace_cmp(devs["wide"], sc, o, d, li)
        brute, rev = B.trace4(desc, o, d, li, O.BRUTE), B.trace4(desc, o, d, li, O.BRUTE_REV)
        if vis:  # lumo_trace reports no triangle for a visibility query; the oracle's is -1
            g = g[:3] + (brute[3],)
        for k, f in enumerate(fams):
            s = slice(bounds[k], bounds[k + 1])
            cut = [tuple(a[s] for a in x) for x in (g, brute, rev)]
            assert B.check_against_brute(*cut, what=f"{name}/{f}") == 0.0


@pytest.mark.parametrize("mode", ["wide", "lumo"])
@pytest.mark.parametrize("top", [0, 1])
def test_trace_top_staging_forms(mode, top):
    """k_trace with TOP staging off and on, the 8 KiB budget cutting the staged prefix inside the
    tree, on the small bistro stand-in."""
    sc, _, _, _ = B.scene("bistro_small")
    dev = L.Device(0, accel=int(mode == "wide"), top_staging=top, top_kb=8)
    try:
        cmp = _trace_cmp if mode == "wide" else _trace_cmp_lumo
        for vis in (False, True):
            _, o, d, li, _ = _joined("bistro_small", vis)
            cmp(dev, sc, o, d, li)
        info, desc = dev.scene_info(), sc.desc()
        assert info.lds_bytes == 0 and (info.top_bytes > 0) == bool(top)
        if top and mode == "wide":
            assert 0 < info.top_wide_nodes < info.wide_nodes
        elif top:  # the objects' BVH fits the budget; the cut falls inside the lights' BVH
            staged = info.top_object_nodes + info.top_light_nodes
            assert 0 < staged < desc.num_object_nodes + desc.num_light_nodes
    finally:
        dev.close()


def _axis_camera(which, res):
    """An orthographic camera whose rays all run exactly along +-z."""
    if which == "cornell":  # the box opens towards -z (cornell_box.rs): looking along +z into it
        b = L.Camera.builder().origin(278.0, 273.0, -800.0).towards(278.0, 273.0, 0.0)
    else:  # the zoo's box is centred at (0, 0, -1): looking along -z
        b = L.Camera.builder().origin(0.0, 0.0, 0.0).towards(0.0, 0.0, -1.0)
    return b.camera_type(L.CameraType.Orthographic).resolution(res).build()


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "split"])
@pytest.mark.parametrize("accel", [0, 1], ids=["lumo", "wide"])
@pytest.mark.parametrize("which", ["cornell", "zoo"])
def test_axis_parallel_primary_rays_render(which, accel, fused):
    """32 x 32 @ 4 spp path traced with every primary ray exactly axis-parallel (two direction
    components +-0): tiles and counts equal the oracle's in both accel modes, through the fused
    bounce kernel and the split schedule."""
    sc = L.Scene.cornell_box() if which == "cornell" else material_zoo()
    sc.build()
    cam = _axis_camera(which, (32, 32))
    c2w = np.array(cam.desc.world_to_camera[1]).reshape(4, 4)
    axis = c2w[:3, :3] @ np.array([0.0, 0.0, 1.0])
    assert sorted(np.abs(axis)) == [0.0, 0.0, 1.0]
    tasks = L.make_tasks(32, 32, 4, SEED)
    dev = L.Device(0, accel=accel, fused=fused)
    try:
        dev.upload(sc, cam)
        assert dev.scene_info().accel == accel
        bufs, res = dev.render_tasks(tasks)
        assert dev.last_schedule().fused == fused
    finally:
        dev.close()
    obufs, ores, _ = O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads(), accel=accel)
    _tiles_cmp(bufs, res, obufs, ores)
    assert sum(float(b.sum()) for b in obufs) > 0.0
