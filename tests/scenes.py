"""Small test scenes built through lumo_amd's builder API (shared by CPU and GPU tests)."""
import numpy as np

import lumo_amd as L
from lumo_amd import named_spectrum as NS


def cube_mesh(center, size, rot_y=0.0):
    """Axis-aligned cube (optionally rotated about y) as 6 quads with outward winding."""
    h = size / 2.0
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], dtype=float)
    c, s = np.cos(rot_y), np.sin(rot_y)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    v = v @ R.T + np.asarray(center, dtype=float)
    # vertex index = 4*ix + 2*iy + iz
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, faces


def material_zoo():
    """empty_box (dragon.rs colours) with one cube per microfacet material kind."""
    s = L.Scene.empty_box(L.Spectrum.from_srgb(242, 242, 242), L.Material.diffuse(NS("RED")),
                          L.Material.diffuse(NS("GREEN")))
    mats = [L.Material.metal(L.Spectrum.from_srgb(230, 180, 90), 0.3, 1.5, 3.0),
            L.Material.mirror(),
            L.Material.glass(),
            L.Material.transparent(NS("MAGENTA"), 0.03, 1.5),
            L.Material.transparent(NS("CYAN"), 0.2, 1.7),
            L.Material.lambertian(L.Spectrum.from_rgb(0.3, 0.5, 0.7))]
    pos = [(-0.6, -0.55, -1.5), (0.0, -0.55, -1.6), (0.6, -0.55, -1.5), (-0.45, -0.55, -0.9), (0.45, -0.55, -0.9),
           (0.0, 0.2, -1.3)]
    for i, (m, p) in enumerate(zip(mats, pos)):
        v, f = cube_mesh(p, 0.45, rot_y=0.3 * i)
        s.add_mesh(v, f, m)
    return s


def default_camera(res):
    """Camera::builder().build() at resolution `res` (camera/builder.rs defaults)."""
    return L.Camera.builder().resolution(res).build()


def cube_obj(center, size, rot_y=0.0, uv_scale=2.0):
    """The cube of cube_mesh as .obj text with per-face texture coordinates (0..uv_scale, so the
    uvs wrap, hit.rs:61-68)."""
    v, faces = cube_mesh(center, size, rot_y)
    lines = [f"v {float(x)!r} {float(y)!r} {float(z)!r}" for x, y, z in v]
    s = uv_scale
    lines += [f"vt 0 0", f"vt {s!r} 0", f"vt {s!r} {s!r}", f"vt 0 {s!r}"]
    lines += ["f " + " ".join(f"{i + 1}/{k + 1}" for k, i in enumerate(f)) for f in faces]
    return ("\n".join(lines) + "\n").encode()


def texture_zoo(seed=7):
    """empty_box with every texture kind (texture.rs): checkerboard of marble / Mandelbrot and an
    image on the walls, image kd + bump map, image ks (metal), checkerboard tf (dielectric), a
    marble sphere, an image-textured light and a Radiance HDR environment map."""
    from imgdata import hdr_bytes, random_png
    rng = np.random.default_rng(seed)
    img = L.Texture.image(random_png(rng, 13, 9, 2, 8)[0])
    pal = L.Texture.image(random_png(rng, 8, 8, 3, 4)[0])
    bump = L.NormalMap(random_png(rng, 6, 5, 2, 8)[0])
    marble = L.Texture.marble(1234, L.Spectrum.from_rgb(0.8, 0.75, 0.7))
    checker = L.Texture.checkerboard(marble, L.Texture.mandelbrot(), 6.0)
    s = L.Scene.empty_box(L.Spectrum.from_srgb(242, 242, 242), L.Material.diffuse(checker), L.Material.diffuse(img))
    objs = [(L.Material.microfacet(0.4, 1.5, 0.0, False, False, pal, L.Spectrum.from_rgb(1, 1, 1),
                                   L.Spectrum.black(), bump_map=bump), (-0.55, -0.55, -1.5)),
            (L.Material.metal(img, 0.25, 1.5, 3.0), (0.55, -0.55, -1.5)),
            (L.Material.transparent(L.Texture.checkerboard(L.Spectrum.from_rgb(0.9, 0.6, 0.6),
                                                           L.Spectrum.from_rgb(0.6, 0.9, 0.9), 3.0), 0.2, 1.5),
             (0.0, -0.55, -1.0))]
    for i, (m, p) in enumerate(objs):
        s.add_obj(cube_obj(p, 0.45, rot_y=0.4 * i), m)
    s.add_sphere(0.2, L.Material.diffuse(marble)).translate(0.0, 0.25, -1.6)
    s.add_rectangle([-0.25, 0.79, -1.4], [0.25, 0.79, -1.4], [0.25, 0.79, -0.9],
                    L.Material.light(L.Texture.image(random_png(rng, 4, 4, 6, 8)[0]), scale=4.0), light=True)
    px = rng.integers(0, 256, size=(8 * 4, 4))
    px[:, 3] = rng.integers(126, 131, size=32)
    s.set_environment_map(L.Texture.hdr(hdr_bytes(8, 4, px)), 0.5)
    return s


def textured_obj_zip(path):
    """A zip with an .obj (textured cube, floor, emissive quad), its .mtl using map_Kd (named
    with a backslash and other case), map_Bump and map_Ke, and the PNGs; returns `path`."""
    import io
    import zipfile

    from imgdata import random_png
    rng = np.random.default_rng(4)
    files = {"t/kd.png": random_png(rng, 9, 7, 2, 8)[0], "t/bump.png": random_png(rng, 5, 5, 2, 8)[0],
             "t/lamp.png": random_png(rng, 3, 3, 6, 8)[0]}
    obj = cube_obj((0.0, -0.3, -1.5), 0.6, 0.5).decode().replace("f ", "usemtl box\nf ", 1)
    nv = 8
    obj += ("v -0.3 0.7 -1.8\nv 0.3 0.7 -1.8\nv 0.3 0.7 -1.2\nv -0.3 0.7 -1.2\n"
            f"usemtl lamp\nf {nv + 1}/1 {nv + 2}/2 {nv + 3}/3 {nv + 4}/4\n")
    obj += ("v -5 -0.6 -5\nv 5 -0.6 -5\nv 5 -0.6 5\nv -5 -0.6 5\n"
            f"usemtl box\nf {nv + 8}/1 {nv + 7}/2 {nv + 6}/3 {nv + 5}/4\n")
    mtl = (b"newmtl box\nKd 0.8 0.8 0.8\nNs 200\nmap_Kd T\\KD.png\nmap_Bump t/bump.png\n"
           b"newmtl lamp\nKe 1 1 1\nmap_Ke t/lamp.png\n")
    bio = io.BytesIO()
    with zipfile.ZipFile(bio, "w") as z:
        z.writestr("scene.obj", "mtllib scene.mtl\n" + obj)
        z.writestr("scene.mtl", mtl)
        for n, b in files.items():
            z.writestr(n, b)
    path.write_bytes(bio.getvalue())
    return path


# ---- builder edge scenes (tests/test_wide.py NAMES, tests/test_brute.py): each a few hundred
# triangles at most, each aimed at one branch of the wide builder (wbvh_build.h)
def _grey():
    return L.Material.lambertian(L.Spectrum.from_rgb(0.5, 0.5, 0.5))


def _lamp(s, y=3.0, half=0.25):
    """Two triangle lights (a quad) above the origin, facing down."""
    v = np.array([(-half, y, -half), (half, y, -half), (half, y, half), (-half, y, half)], dtype=float)
    s.add_mesh(v, [(0, 1, 2, 3)], L.Material.light(NS("WHITE")), light=True)


def concentric_triangles():
    """Coplanar triangles (plane y = 0) whose boxes share one centre: 20 around the origin and 16
    around (3, 0, 0), with dyadic sizes so the box centres coincide exactly.  No SAH bin separates
    centres that coincide, so after the split between the two groups the builder halves the lists
    (count / 2): 20 -> 10 -> leaves of 5, 16 -> leaves of 8 = LEAF_MAX."""
    v, f = [], []
    for cx, n in ((0.0, 20), (3.0, 16)):
        for k in range(n):
            h = 0.25 + 0.125 * k
            f.append(tuple(range(len(v), len(v) + 3)))
            v += [(cx - h, 0.0, -h), (cx + h, 0.0, -h), (cx, 0.0, h)]
    s = L.Scene()
    s.add_mesh(np.array(v), f, _grey())
    _lamp(s)
    return s


def degenerate_mesh():
    """A small knot with every fifth triangle duplicated, plus zero-area triangles: two corners
    equal, three corners equal, three corners collinear."""
    from lumo_amd.procedural import torus_knot_tube
    v, q = torus_knot_tube(16, 4)
    q = np.asarray(q)
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    f += f[::5]
    n = len(v)
    v = np.concatenate([v, [(0.0, 0.0, 0.0), (0.5, 0.25, -0.5), (1.0, 0.5, -1.0)]])
    f += [(0, 0, 1), (2, 2, 2), (n, n + 1, n + 2), (n, n + 2, n + 1), (5, 9, 5)]
    s = L.Scene()
    s.add_mesh(v, f, _grey())
    _lamp(s)
    return s


def flat_mesh(n=9):
    """An n x n grid of quads in the plane y = 0.25 (exact in f32, so outward rounding keeps the
    boxes flat) with irregular spacing: every box of the objects' tree has zero height."""
    rng = np.random.default_rng(3)
    x = np.cumsum(rng.uniform(0.05, 0.4, n + 1)) - 1.0
    z = np.cumsum(rng.uniform(0.05, 0.4, n + 1)) - 1.0
    v = np.array([(xi, 0.25, zi) for xi in x for zi in z])
    f = [(i * (n + 1) + j, i * (n + 1) + j + 1, (i + 1) * (n + 1) + j + 1, (i + 1) * (n + 1) + j)
         for i in range(n) for j in range(n)]
    s = L.Scene()
    s.add_mesh(v, f, _grey())
    _lamp(s)
    return s


ZOO_SHIFT = (1e4 + 0.1, -1e4 - 0.3, 1e4 + 0.7)


def translated_zoo(shift=ZOO_SHIFT):
    """The material zoo's triangles re-added as plain meshes at shifted coordinates: the vertices
    are no f32 values and the outward rounding of the f32 boxes (~1e-3 at 1e4) is as large as the
    gaps between the cubes and the floor."""
    from rays import world_triangles
    d = material_zoo().build().desc()
    tri, light = world_triangles(d)
    tri = tri + np.asarray(shift)
    s = L.Scene()
    for sel, is_light in ((light < 0, False), (light >= 0, True)):
        t = tri[sel]
        v = t.reshape(-1, 3)
        f = np.arange(len(v)).reshape(-1, 3)
        if not len(t):  # the zoo's light is a rectangle: keep a lamp under the roof instead
            continue
        s.add_mesh(v, [tuple(r) for r in f], L.Material.light(NS("WHITE")) if is_light else _grey(), light=is_light)
    if not (light >= 0).any():
        h, y = 0.2, 0.75
        v = np.array([(-h, y, -1 - h), (h, y, -1 - h), (h, y, -1 + h), (-h, y, -1 + h)]) + np.asarray(shift)
        s.add_mesh(v, [(0, 1, 2, 3)], L.Material.light(NS("WHITE")), light=True)
    return s


def scaled_instances():
    """One mesh instanced twice: scale (1e-3, 1, 1e3), a rotation and a translation of 1e4 (the
    instance's world box is padded by 1e-9 of its magnitude, wbvh_build.h xf_box), and scale 1."""
    from lumo_amd.procedural import torus_knot_tube
    v, f = torus_knot_tube(40, 5)
    s = L.Scene()
    s.add_mesh(v, f, _grey()).scale(1e-3, 1.0, 1e3).rotate_y(0.7).rotate_x(-0.2).translate(1e4, 0.5, -1e4)
    s.add_mesh(v, f, _grey()).scale_uniform(1.0).rotate_z(0.3).translate(1e4 + 2.0, 0.0, -1e4 + 1.0)
    v = np.array([(-1.0, 5.0, -1.0), (1.0, 5.0, -1.0), (1.0, 5.0, 1.0), (-1.0, 5.0, 1.0)]) + (1e4, 0.0, -1e4)
    s.add_mesh(v, [(0, 1, 2, 3)], L.Material.light(NS("WHITE")), light=True)
    return s


def sphere_field(n=40):
    """Spheres only (n objects, one sphere light): both trees hold object leaves and nothing else."""
    rng = np.random.default_rng(11)
    s = L.Scene()
    for c, r in zip(rng.uniform(-2.0, 2.0, (n, 3)), rng.uniform(0.1, 0.6, n)):
        s.add_sphere(float(r), _grey()).translate(*c)
    s.add_sphere(0.4, L.Material.light(NS("WHITE")), light=True).translate(0.0, 3.5, 0.0)
    return s


def stadium():
    """A teapot in a stadium: a 2-triangle floor of size 1e4 and a 200-triangle knot of size 1 on it.
    The floor falls by 1e-4 per unit of x, so its box is not flat: lumo's kd walk clips hits at a flat
    leaf's exit (test_wide.py), which on an axis-aligned floor of this size loses 8 % of the generic
    rays and would say nothing about the wide builder."""
    from lumo_amd.procedural import torus_knot_tube
    v, f = torus_knot_tube(25, 4)
    v = (v - v.min(0)) / (v.max(0) - v.min(0)).max()
    s = L.Scene()
    h, dy = 5e3, 0.5
    s.add_mesh(np.array([(-h, dy, -h), (h, -dy, -h), (h, -dy, h), (-h, dy, h)]), [(0, 3, 2, 1)], _grey())
    s.add_mesh(v + (0.3, 0.0, -0.2), f, _grey())
    _lamp(s, y=4.0)
    return s


# ---- light kd trees at the wide accel's depth limit (wbvh.h LIGHT_KD_STACK; tests/test_wide.py,
# tests/test_gpu_wide_forms.py)
def light_kd_depth(desc):
    """Deepest level of a light's kd tree, the root counted as level 1 (0: no light has a tree), over
    the lights wbvh::build looks at: kd meshes and rectangles with a root."""
    deepest = 0
    for i in range(desc.num_lights):
        o = desc.lights[i]
        if o.type not in (0, 1) or o.kd_root < 0:  # LUMO_OBJ_KDMESH, LUMO_OBJ_RECTANGLE
            continue
        stack = [(o.kd_root, 1)]
        while stack:
            k, level = stack.pop()
            if k < 0 or k >= desc.num_kd_nodes:
                continue
            deepest = max(deepest, level)
            if not desc.kd_nodes[k].leaf:
                stack += [(k + 1, level + 1), (desc.kd_nodes[k].right, level + 1)]
    return deepest


def knot_light_scene(n, m):
    """A torus_knot_tube(n, m) mesh added as a light.  The builder turns a light mesh into one triangle
    light per face (Scene::add_mesh), so no light of such a scene has a kd tree, whatever n and m."""
    from lumo_amd.procedural import torus_knot_tube
    v, f = torus_knot_tube(n, m)
    s = L.Scene()
    s.add_mesh(v, f, L.Material.light(L.Spectrum.from_rgb(1.0, 0.8, 0.6), scale=0.5), light=True)
    return s


class DeepLightScene:
    """A floor, a small grey knot and one tilted rectangle light whose kd tree is `levels` deep.

    The only lights with a kd tree are rectangles (two triangles, one or two levels), so the depth
    comes from the scene description, not from the builder: the description of the built scene is
    copied with the light's tree re-rooted under a chain of interior nodes.  Chain node j splits the
    light's box at a plane inside it (x and z in turn); its left child is the next chain node (the
    last one's: a copy of the original tree) and its right child another copy of the original tree.
    Both triangles stay reachable on either side of every plane, as triangles that straddle a kd
    split are, so it is a valid kd tree of the same rectangle and rays that cross the planes push
    the far side.  upload() and the oracle take it as any scene (desc())."""

    def __init__(self, levels):
        import ctypes as C

        from lumo_amd import _ffi
        from lumo_amd.procedural import torus_knot_tube
        s = L.Scene()
        s.add_rectangle((-3, -1, -3), (3, -1, -3), (3, -1, 3), _grey())
        v, f = torus_knot_tube(25, 4)
        s.add_mesh(0.5 * (v - v.mean(0)) / np.abs(v - v.mean(0)).max() + (0.2, -0.4, 0.1), f, _grey())
        s.add_rectangle((-0.5, 2.0, -0.5), (0.5, 2.3, -0.5), (0.5, 2.3, 0.5), L.Material.light(NS("WHITE")), light=True)
        self._base = s.build()
        d = self._base.desc()
        assert d.num_lights == 1 and d.lights[0].type == 1 and d.lights[0].kd_root >= 0
        own = light_kd_depth(d)
        assert 1 <= own <= levels
        nodes = [d.kd_nodes[i] for i in range(d.num_kd_nodes)]

        def copy_tree(i):  # lumo's layout: the left child follows its parent
            src = d.kd_nodes[i]
            at = len(nodes)
            nodes.append(_ffi.KdNode(src.point, src.axis, src.right, src.leaf, src.first, src.count, 0))
            if not src.leaf:
                assert copy_tree(i + 1) == at + 1
                nodes[at].right = copy_tree(src.right)
            return at

        old_root = d.lights[0].kd_root
        chain = levels - own
        lo, hi = d.lights[0].bmin, d.lights[0].bmax
        first = len(nodes)
        for j in range(chain):
            axis = (0, 2)[j % 2]
            point = lo[axis] + (hi[axis] - lo[axis]) * (j + 1) / (chain + 1)
            nodes.append(_ffi.KdNode(point, axis, -1, 0, 0, 0, 0))
        root = copy_tree(old_root)  # follows the last chain node: its left child
        assert chain == 0 or root == first + chain
        for j in range(chain):
            nodes[first + j].right = copy_tree(old_root)
        self._nodes = (_ffi.KdNode * len(nodes))(*nodes)
        self._lights = (_ffi.Object * 1)()
        C.memmove(self._lights, d.lights, C.sizeof(_ffi.Object))
        self._lights[0].kd_root = first if chain else root
        self._desc = _ffi.SceneDesc()
        C.memmove(C.byref(self._desc), C.byref(d), C.sizeof(_ffi.SceneDesc))
        self._desc.kd_nodes, self._desc.num_kd_nodes = self._nodes, len(nodes)
        self._desc.lights = self._lights

    def build(self):
        return self

    def desc(self):
        return self._desc


EDGE_SCENES = {"concentric": (concentric_triangles, (0.3, 2.0, 1.0)), "degenerate": (degenerate_mesh, (0.0, 0.5, 4.0)),
               "flat": (flat_mesh, (0.2, 2.0, 0.5)),
               "zoo_translated": (translated_zoo, ZOO_SHIFT),
               "scaled_instances": (scaled_instances, (1e4 + 1.0, 1.0, -1e4 + 6.0)),
               "sphere_field": (sphere_field, (0.0, 0.3, 6.0)), "stadium": (stadium, (3.0, 1.5, 2.0))}
