"""What the reuse of walk values in lumo's kd / BVH kernels newly puts at risk (DESIGN.md §4 "Walk
reuse": a leaf's slab interval handed to its object's kd walk, the winner's acceptance and hit
record taken from the walk's own triangle test).

* Marked leaves beside unmarked ones: the upload marks a BVH leaf whose single un-instanced kd
  mesh / rectangle has the leaf's box; instances, spheres, single triangles and leaves of several
  objects keep the separate slab test.  One scene holds all of them.
* A light behind a light: the sampled light's t - EPSILON bounds the lights' any-hit walk, which
  meets the sampled light again; rays through the diagonal shared by a rectangle's two triangles;
  origins so far away that t - EPSILON == t.
* The same scene through the fused, tail and split render kernels, in both feature classes.  The
  reuse runs in lumo_trace (tests 1 and 2) and in the lean fused and tail kernels (test 3, "lean");
  the split schedule and the full-feature kernels keep lumo's calls and stand beside them here.

Everything is compared with the oracle bit for bit, traversal counters included.  The oracle's
lumo walk reports no triangle (oracle_ffi.trace: -1), so the GPU's triangle index is compared with
the brute-force reference wherever that reference is order-free and agrees on (t, kind, object),
by the rule of tests/test_brute.py.  A visibility query reports no triangle on either side
(lumo_trace writes -1, as the oracle does), so there is none to compare there.

What these tests cannot see: whether the device marked any leaf.  The mark lives in the device's
own node array and no stat or info field exposes it (the C ABI is pinned), so _leaf_kinds below
restates the upload's rule on the host description.  Were the upload never to mark a leaf, every
walk would take the unmarked path and these tests would still pass; that the marked path runs
shows only in the instruction counts of the profiled kernels."""
import functools

import numpy as np
import pytest

import lumo_amd as L
import oracle_ffi as O
import rays
import test_brute as B
from lumo_amd import named_spectrum as NS
from parity import oracle_threads
from scenes import cube_mesh
from test_gpu_scale import _trace_cmp as _trace_cmp_lumo
from test_gpu_wide import _tiles_cmp

pytestmark = pytest.mark.gpu
SEED = 0x1DE
KDMESH, RECT, TRI, SPHERE = 0, 1, 2, 3
N_RAYS = 1 << 13


def _grey():
    return L.Material.lambertian(L.Spectrum.from_rgb(0.5, 0.5, 0.5))


def _white():
    return L.Material.light(NS("WHITE"))


def _table(desc, lights=False):
    t, n = (desc.lights, desc.num_lights) if lights else (desc.objects, desc.num_objects)
    return np.ctypeslib.as_array(t, shape=(n,))


# ------------------------------------------------------------------ 1. marked beside unmarked leaves
@functools.lru_cache(maxsize=None)
def _mixed():
    """A plain mesh, a rectangle, an instanced mesh (rotated, non-uniformly scaled: its world box
    is not its kd box), a sphere, two concentric cubes (equal box centres, dyadic coordinates: no
    SAH plane separates them, bvh/node.rs sah_partition), a triangle light and a rectangle light."""
    s = L.Scene()
    s.add_rectangle((-2.0, 0.0, 2.0), (-2.0, 0.0, -2.0), (2.0, 0.0, -2.0), _grey())
    v, f = cube_mesh((-1.0, 0.4, 0.3), 0.7, rot_y=0.4)
    s.add_mesh(v, f, _grey())
    v, f = cube_mesh((0.0, 0.0, 0.0), 0.5)
    s.add_mesh(v, f, _grey()).scale(1.0, 0.5, 2.0).rotate_y(0.6).rotate_x(-0.3).translate(1.0, 0.6, -0.5)
    s.add_sphere(0.3, _grey()).translate(0.2, 0.3, 1.0)
    for size in (0.25, 0.5):
        v, f = cube_mesh((0.5, 0.5, -1.5), size)
        s.add_mesh(v, f, _grey())
    s.add_mesh(np.array([(-1.5, 2.0, -0.5), (-0.5, 2.0, -0.5), (-1.0, 2.0, 0.5)]), [(0, 1, 2)], _white(), light=True)
    s.add_rectangle((0.25, 2.0, 0.5), (0.25, 2.0, -0.5), (1.25, 2.0, -0.5), _white(), light=True)
    s.build()
    d = s.desc()
    return s, d, rays.Geometry(d)


def _leaf_kinds(desc):
    """Per BVH leaf of the objects' and the lights' tree: 'same' (what the upload marks: one
    un-instanced kd mesh / rectangle whose kd boundary is bitwise the leaf's box), else 'multi',
    'instance', 'sphere', 'triangle' or 'other_box'."""
    out = []
    for nodes, n, items, table in ((desc.object_nodes, desc.num_object_nodes, desc.object_items, _table(desc)),
                                   (desc.light_nodes, desc.num_light_nodes, desc.light_items, _table(desc, True))):
        for i in range(n):
            nd = nodes[i]
            if nd.count == 0:
                continue
            if nd.count > 1:
                out.append("multi")
                continue
            o = table[items[nd.first]]
            if o["type"] == SPHERE:  # placed by an instance transform of its own
                out.append("sphere")
            elif o["xform"] >= 0:
                out.append("instance")
            elif o["type"] == TRI:
                out.append("triangle")
            else:
                same = (np.array(nd.bmin[:]).tobytes() == o["bmin"].tobytes() and
                        np.array(nd.bmax[:]).tobytes() == o["bmax"].tobytes())
                out.append("same" if same else "other_box")
    return out


def test_mixed_scene_has_every_leaf_kind():
    """The scene's leaves as built on the host: marked leaves, and beside them every kind the mark
    excludes.  The concentric cubes share one leaf: lumo's builder does produce a multi-object
    leaf (both land on one side of every SAH split until the Morton fallback stops at
    MAX_LEAF_SIZE)."""
    kinds = set(_leaf_kinds(_mixed()[1]))
    assert {"same", "multi", "instance", "sphere", "triangle"} <= kinds, kinds


@pytest.fixture(scope="module")
def dev():
    d = L.Device(0)
    yield d
    d.close()


def _closest_cmp(dev, sc, desc, o, d, what):
    g = _trace_cmp_lumo(dev, sc, o, d)  # t, kind, object and the three counters equal the oracle's
    brute, rev = B.trace4(desc, o, d, None, O.BRUTE), B.trace4(desc, o, d, None, O.BRUTE_REV)
    ids = (B.same_hit(g, brute) & B.same_hit(brute, rev) & (brute[2] == rev[2]) & (brute[3] == rev[3]) &
           (g[2] == brute[2]) & (g[1] != 0))
    assert ids.mean() > 0.2, (what, ids.mean())  # the comparison below is not vacuous
    np.testing.assert_array_equal(g[3][ids], brute[3][ids], err_msg=what + " triangle")


@pytest.mark.parametrize("family", ["generic", "surface", "at_edge_mid", "far"])
def test_mixed_scene_closest(dev, family):
    sc, desc, geom = _mixed()
    o, d = rays.closest(desc, (0.0, 1.0, 4.0), family, N_RAYS, SEED, geom)
    _closest_cmp(dev, sc, desc, o, d, family)


@pytest.mark.parametrize("family", ["vis_generic", "vis_surface", "vis_far"])
def test_mixed_scene_visibility(dev, family):
    sc, desc, geom = _mixed()
    o, d, li = rays.visibility(desc, family, N_RAYS, SEED, geom)
    assert set(np.unique(li)) == {0, 1}  # both the triangle light and the rectangle light are sampled
    g = _trace_cmp_lumo(dev, sc, o, d, li)
    assert 0 < (g[1] == 2).mean() < 1  # visible and not, both present


# ------------------------------------------------------------------ 2. a light behind a light
FAR_Y, NEAR_Y = 2.0, 1.9


def _stacked(fx):
    """Over a floor rectangle: a rectangle light at y = 2 (x, z in [-1, 1]), a smaller one 0.1
    below it covering part of it (its edge at x = 1/32 passes just beside the centre of the farther
    light, so rays towards that centre are hidden from one side only), and a third light beside
    them: a triangle light (fx: also an instanced cube on the floor; feature class 1) or a
    rectangle light (only kd meshes, rectangles and Lambertian / light materials: feature class
    0).  3 lights: n_shadow = 1."""
    s = L.Scene()
    s.add_rectangle((-2.0, 0.0, 2.0), (-2.0, 0.0, -2.0), (2.0, 0.0, -2.0), _grey())
    if fx:
        box = s.add_mesh(*cube_mesh((0.0, 0.0, 0.0), 0.5), _grey())
        box.scale(1.0, 0.5, 1.5).rotate_y(0.5).translate(-1.25, 0.25, 1.0)
    else:
        s.add_mesh(*cube_mesh((-1.25, 0.25, 1.0), 0.5), _grey())
    s.add_rectangle((-1.0, FAR_Y, 1.0), (-1.0, FAR_Y, -1.0), (1.0, FAR_Y, -1.0), _white(), light=True)
    s.add_rectangle((-1.0, NEAR_Y, 0.5), (-1.0, NEAR_Y, -0.5), (0.03125, NEAR_Y, -0.5), _white(), light=True)
    if fx:
        s.add_mesh(np.array([(1.5, 2.0, -0.5), (2.0, 2.0, -0.5), (1.75, 2.0, 0.5)]), [(0, 1, 2)], _white(), light=True)
    else:
        s.add_rectangle((1.5, 2.0, 0.5), (1.5, 2.0, -0.5), (2.0, 2.0, -0.5), _white(), light=True)
    s.build()
    return s


@functools.lru_cache(maxsize=None)
def _stacked_rays():
    """(scene, desc, far light, near set, far set), each set (origins, directions, lights).
    Near set: from floor points towards uniform points of the farther light, a quarter of them
    towards the midpoint of its diagonal (0, 2, 0), where both of its triangles are hit at equal
    t.  Far set: the same targets seen from 2^22 .. 2^23 away, from below the floor's plane at so
    shallow an angle that the line meets that plane outside the floor (the floor would hide every
    light from straight below); there t - EPSILON == t (EPSILON = 1e-10 < ulp(2^22) / 2)."""
    sc = _stacked(True)
    desc = sc.desc()
    lights = _table(desc, True)
    far = [i for i in range(desc.num_lights) if lights[i]["type"] == RECT and
           tuple(lights[i]["origin"]) == (-1.0, FAR_Y, -1.0)]
    assert len(far) == 1 and desc.num_lights == 3
    rng = np.random.default_rng(SEED)
    n = N_RAYS
    tgt = np.stack([rng.uniform(-1.0, 1.0, n), np.full(n, FAR_Y), rng.uniform(-1.0, 1.0, n)], 1)
    tgt[: n // 4] = (0.0, FAR_Y, 0.0)
    o = np.stack([rng.uniform(-2.0, 2.0, n), np.zeros(n), rng.uniform(-2.0, 2.0, n)], 1)
    d = tgt - o
    li = np.full(n, far[0], dtype=np.int32)
    near = (o, d / np.linalg.norm(d, axis=1, keepdims=True), li)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    uy = rng.uniform(0.05, 0.4, n)
    u = np.stack([np.sqrt(1.0 - uy * uy) * np.cos(phi), -uy, np.sqrt(1.0 - uy * uy) * np.sin(phi)], 1)
    o2 = tgt + u * rng.uniform(2.0 ** 22, 2.0 ** 23, (n, 1))
    d2 = tgt - o2
    return sc, desc, far[0], near, (o2, d2 / np.linalg.norm(d2, axis=1, keepdims=True), li)


def test_light_behind_light_ray_sets():
    """From the oracle's answers alone: the near set holds occluded and visible rays (at least
    10 % each, so the GPU comparison cannot pass on one outcome), the far set's hits are where
    t - EPSILON == t and both outcomes occur there too."""
    _, desc, _, near, far = _stacked_rays()
    t, kind, _, _ = O.trace(desc, *near)
    vis = (kind == 2).mean()
    assert 0.1 <= vis <= 0.9, vis
    t, kind, _, _ = O.trace(desc, *far)
    hit = kind == 2
    assert hit.any() and not hit.all()
    assert (t[hit] >= 2.0 ** 22).all() and (t[hit] - 1e-10 == t[hit]).all()


@pytest.mark.parametrize("which", ["near", "far"])
def test_light_behind_light(dev, which):
    sc, desc, _, near, far = _stacked_rays()
    o, d, li = near if which == "near" else far
    _trace_cmp_lumo(dev, sc, o, d, li)


# ------------------------------------------------------------------ 3. the same through the render kernels
@pytest.mark.parametrize("how,fused,tail", [("fused", 1, 0), ("tail", 1, 1 << 30), ("split", 0, 0)])
@pytest.mark.parametrize("fx", [0, 1], ids=["lean", "full"])
def test_stacked_lights_render(fx, how, fused, tail):
    """32 x 32 @ 4 spp of the stacked-lights scene in lumo mode through the fused bounce kernel,
    the tail kernel from the first bounce (tail_below above the path count) and the split
    schedule (each with the plain pass loop, pipeline 0, so that the options alone choose the
    kernels): tiles and counts equal the oracle's."""
    sc = _stacked(bool(fx))
    cam = L.Camera.builder().origin(0.0, 0.9, 3.5).towards(0.0, 1.0, 0.0).resolution((32, 32)).build()
    tasks = L.make_tasks(32, 32, 4, SEED)
    dev = L.Device(0, accel=0, fused=fused, tail_below=tail, pipeline=0)
    try:
        dev.upload(sc, cam)
        info = dev.scene_info()
        assert info.accel == 0 and info.lds_bytes > 0 and info.full_kernels == fx and info.n_shadow == 1
        bufs, res = dev.render_tasks(tasks)
        assert dev.last_schedule().fused == fused
        assert (dev.stats().tail_queries > 0) == (how == "tail")  # bounces past the first run by the tail kernel
    finally:
        dev.close()
    obufs, ores, _ = O.render_tasks(sc.desc(), cam.desc, tasks, O.WAVEFRONT, oracle_threads())
    _tiles_cmp(bufs, res, obufs, ores)
    assert sum(float(b.sum()) for b in obufs) > 0.0
