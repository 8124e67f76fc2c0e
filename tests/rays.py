"""Adversarial ray families for the traversal tests (tests/test_brute.py, tests/test_gpu_brute.py).

The generic ray sets (test_gpu_scale._closest_rays / _visibility_rays) draw Gaussian directions and
points inside the bounds; these families add the inputs where a slab test yields inf, -inf and
0 * inf, where a kd walk compares against NaN split distances and where a conservative f32 box
test needs its margin: zero direction components (both signs of zero), rays through vertices,
along box planes and edges, origins on surfaces and far outside the scene, and direction components
below the f32 range of 1 / d.

Every family is deterministic from (scene desc, eye, n, seed).  All directions are finite and
non-zero: no NaN, inf or zero-vector input.  Directions are unit length up to rounding (the `tiny`
family's are exactly one +-1 component plus components too small to change the norm).
"""
import numpy as np

from test_gpu_scale import _arrays, _closest_rays, _visibility_rays

TRI, SPHERE = 2, 3
CLOSEST = ["generic", "axis", "axis_thru_vertex", "planar", "at_vertex", "at_edge_mid", "far", "tiny", "surface"]
VISIBILITY = ["vis_generic", "vis_surface", "vis_far", "vis_light_features"]
TINY = np.array([1e-20, 1e-30, 1e-33, 1e-36, 1e-38, 3e-39, 1e-300, 5e-324])


def world_triangles(desc):
    """(T, 3, 3) world-space corners of every triangle of every object and light (instances moved by
    their transform), and for each the index of the triangle light it is (-1 if none)."""
    v, tris = _arrays(desc)
    out, light = [], []
    for table, n, is_light in ((desc.objects, desc.num_objects, False), (desc.lights, desc.num_lights, True)):
        objs = np.ctypeslib.as_array(table, shape=(n,)) if n else []
        for i, o in enumerate(objs):
            if o["type"] == SPHERE:
                continue
            k = 1 if o["type"] == TRI else int(o["num_tris"])
            p = v[tris["v"][o["tri_base"]:o["tri_base"] + k]]
            if o["xform"] >= 0:
                m = np.array(desc.transforms[int(o["xform"])].m).reshape(4, 4)
                p = p @ m[:3, :3].T + m[:3, 3]
            out.append(p)
            light.append(np.full(k, i if is_light and o["type"] == TRI else -1))
    if not out:
        return np.zeros((0, 3, 3)), np.zeros(0, dtype=np.int64)
    return np.concatenate(out), np.concatenate(light)


def _sphere_bounds(desc):
    pts = []
    for table, n in ((desc.objects, desc.num_objects), (desc.lights, desc.num_lights)):
        for o in (np.ctypeslib.as_array(table, shape=(n,)) if n else []):
            if o["type"] == SPHERE and o["radius"] < 1e6:  # not the environment sphere
                c = np.zeros(3)
                if o["xform"] >= 0:
                    c = np.array(desc.transforms[int(o["xform"])].m).reshape(4, 4)[:3, 3]
                r = float(o["radius"])
                pts += [c - r, c + r]
    return pts


class Geometry:
    """What the families draw from: the world-space triangles, their distinct corners and edge
    midpoints and the bounds of everything finite in the scene."""

    def __init__(self, desc):
        self.tri, self.tri_light = world_triangles(desc)
        pts = [self.tri.reshape(-1, 3)] if len(self.tri) else []
        sb = _sphere_bounds(desc)
        if sb:
            pts.append(np.array(sb))
        allp = np.concatenate(pts)
        self.lo, self.hi = allp.min(0), allp.max(0)
        self.extent = float(np.max(self.hi - self.lo))
        # a scene of spheres only: the corners of the spheres' boxes stand in for vertices
        self.vert = self.tri.reshape(-1, 3) if len(self.tri) else np.array(sb)
        if len(self.tri):
            self.edge_mid = 0.5 * (self.tri + np.roll(self.tri, -1, axis=1)).reshape(-1, 3)
        else:
            self.edge_mid = 0.5 * (self.vert + np.roll(self.vert, -1, axis=0))

    def inside(self, rng, n):
        return rng.uniform(self.lo, self.hi, size=(n, 3))

    def surface(self, rng, n):
        """Barycentric points of random triangles: corners, edges (one weight 0) and interiors."""
        if not len(self.tri):
            return self.vert[rng.integers(0, len(self.vert), n)]
        t = self.tri[rng.integers(0, len(self.tri), n)]
        w = rng.dirichlet((1.0, 1.0, 1.0), size=n)
        w[: n // 4, 0] = 0.0  # on an edge
        w[: n // 8] = np.eye(3)[rng.integers(0, 3, n // 8)]  # on a corner
        w /= w.sum(1, keepdims=True)
        return np.einsum("nk,nkc->nc", w, t)


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _aim(o, tgt, spare):
    """Origins and unit directions towards tgt; an origin that is its own target takes the spare one."""
    same = (o == tgt).all(axis=1)
    o = np.where(same[:, None], spare, o)
    assert not (o == tgt).all(axis=1).any()
    return o, _unit(tgt - o)


def _axis_dirs(rng, n):
    """+-e_k exactly, the two zero components with random signs of zero."""
    k = rng.integers(0, 3, n)
    d = np.where(rng.integers(0, 2, (n, 3)) == 1, 0.0, -0.0)
    d[np.arange(n), k] = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
    return d, k


def _outside_origins(g, rng, n, eye):
    """The eye for a third of the rays; for the rest points up to one extent outside the bounds:
    strictly outside along one axis at least, so no origin is the vertex it aims at."""
    side = rng.integers(0, 2, (n, 3)) == 1
    off = rng.uniform(0.0, g.extent, (n, 3)) * (rng.integers(0, 3, (n, 3)) > 0)
    k = rng.integers(0, 3, n)
    off[np.arange(n), k] = rng.uniform(1.0 / 64.0, 1.0, n) * g.extent
    o = np.where(side, g.hi + off, g.lo - off)
    o[: n // 3] = np.asarray(eye, dtype=np.float64)
    return o


def _far_origins(g, rng, n):
    """Origins 1e2 .. 1e6 extents from the bounds' centre, log-uniform (not farther: beyond ~1e8
    extents sphere_hit's error interval makes the accepted sphere depend on the visiting order)."""
    dist = g.extent * 10.0 ** rng.uniform(2.0, 6.0, (n, 1))
    return 0.5 * (g.lo + g.hi) + dist * _unit(rng.normal(size=(n, 3)))


def closest(desc, eye, family, n, seed, geom=None):
    """(origins, directions) of one closest-hit family."""
    g = geom or Geometry(desc)
    rng = np.random.default_rng([seed, CLOSEST.index(family)])
    if family == "generic":
        return _closest_rays(desc, eye, n, seed)
    if family == "axis":
        return g.inside(rng, n), _axis_dirs(rng, n)[0]
    if family == "axis_thru_vertex":
        d, k = _axis_dirs(rng, n)
        o = g.vert[rng.integers(0, len(g.vert), n)].copy()
        o[np.arange(n), k] = g.inside(rng, n)[np.arange(n), k]
        return o, d
    if family == "planar":
        d = rng.normal(size=(n, 3))
        d[np.arange(n), rng.integers(0, 3, n)] = np.where(rng.integers(0, 2, n) == 1, 0.0, -0.0)
        o = g.inside(rng, n)
        # the second half: every coordinate from some vertex, so the rays lie in box planes
        h = n // 2
        o[h:] = np.stack([g.vert[rng.integers(0, len(g.vert), n - h), c] for c in range(3)], 1)
        return o, _unit(d)
    if family in ("at_vertex", "at_edge_mid"):
        pts = g.vert if family == "at_vertex" else g.edge_mid
        o = _outside_origins(g, rng, n, eye)
        return _aim(o, pts[rng.integers(0, len(pts), n)], g.hi + g.extent)
    if family == "far":
        o = _far_origins(g, rng, n)
        tgt = g.inside(rng, n)
        tgt[n // 2:] = g.surface(rng, n - n // 2)  # half at the surfaces (a sparse scene is mostly empty)
        return o, _unit(tgt - o)
    if family == "tiny":
        d = TINY[rng.integers(0, len(TINY), (n, 3))] * np.where(rng.integers(0, 2, (n, 3)) == 1, 1.0, -1.0)
        d[np.arange(n), rng.integers(0, 3, n)] = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
        o = g.inside(rng, n)
        h = n // 2  # half through vertex coordinates
        o[h:] = np.stack([g.vert[rng.integers(0, len(g.vert), n - h), c] for c in range(3)], 1)
        return o, d
    if family == "surface":
        return g.surface(rng, n), _unit(rng.normal(size=(n, 3)))
    raise KeyError(family)


def visibility(desc, family, n, seed, geom=None):
    """(origins, directions, light indices) of one visibility family."""
    g = geom or Geometry(desc)
    rng = np.random.default_rng([seed, 100 + VISIBILITY.index(family)])
    o, d, li = _visibility_rays(desc, n, seed)
    if family == "vis_generic":
        return o, d, li
    if family in ("vis_surface", "vis_far"):
        # the same targets (a point one unit along the generic ray's direction is on the line to the
        # light's point), seen from origins on surfaces / far away
        lights = np.ctypeslib.as_array(desc.lights, shape=(desc.num_lights,))
        aimed = lights["type"][li] != SPHERE
        tgt = _light_points(desc, g, rng, li)
        o2 = g.surface(rng, n) if family == "vis_surface" else _far_origins(g, rng, n)
        d2 = np.where(aimed[:, None], tgt - o2, rng.normal(size=(n, 3)))
        return o2, _unit(d2), li
    if family == "vis_light_features":
        # the corners and edge midpoints of triangle lights; scenes without any keep the generic rays
        idx = np.nonzero(g.tri_light >= 0)[0]
        if not len(idx):
            return o, d, li
        pick = idx[rng.integers(0, len(idx), n)]
        t = g.tri[pick]
        feat = np.concatenate([t, 0.5 * (t + np.roll(t, -1, axis=1))], axis=1)  # (n, 6, 3)
        tgt = feat[np.arange(n), rng.integers(0, 6, n)]
        o2 = g.inside(rng, n)
        h = n // 2
        o2[h:] = g.surface(rng, n - h)
        o2, d2 = _aim(o2, tgt, g.lo - g.extent)
        return o2, d2, g.tri_light[pick].astype(np.int32)
    raise KeyError(family)


def _light_points(desc, g, rng, li):
    """A random point of each ray's light (triangle and rectangle lights; spheres: unused)."""
    v, tris = _arrays(desc)
    lights = np.ctypeslib.as_array(desc.lights, shape=(desc.num_lights,))
    n = len(li)
    p = np.zeros((n, 3))
    for i in np.unique(li):
        L = lights[i]
        if L["type"] == SPHERE:
            continue
        k = 1 if L["type"] == TRI else int(L["num_tris"])
        c = v[tris["v"][L["tri_base"]:L["tri_base"] + k]]
        if L["xform"] >= 0:
            m = np.array(desc.transforms[int(L["xform"])].m).reshape(4, 4)
            c = c @ m[:3, :3].T + m[:3, 3]
        sel = np.nonzero(li == i)[0]
        t = c[rng.integers(0, k, len(sel))]
        w = rng.dirichlet((1.0, 1.0, 1.0), size=len(sel))
        p[sel] = np.einsum("nk,nkc->nc", w, t)
    return p
