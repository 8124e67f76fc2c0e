"""The clustered device builder of the wide BVH (lumo_scene_set_wide_cluster): PLOC in place of
the LBVH's radix tree.  The yardsticks are tests/test_gpu_wide_build.py's, which never depended on the builder
(the tree against the scene, two uploads byte for byte; walks against brute force; renders against
oracle(wide)): its `_device` is pointed at the clustered builder and its test functions run as they are.  What
is new here: the forced pairing phase, the tree's SAH cost against the LBVH's, and the interface."""
import ctypes as C

import pytest

import lumo_amd as L
import test_gpu_wide_build as B
from lumo_amd import _ffi
from test_brute import scene

pytestmark = pytest.mark.gpu
# more than 256 + r primitives (tile and halo boundaries); small BLAS trees within one tile, trees of 1 and 2;
# every key equal and the boxes nested (all ties); zero half-areas (two); object leaves interleaved
EDGE = ["small_dragon", "scaled_instances", "concentric", "flat", "degenerate", "spheres"]


def _clustered(monkeypatch, radius, iters=None):
    monkeypatch.setattr(B, "_device", lambda **kw: L.Device(0, accel=1, wide_build="device", wide_cluster=radius,
                                                            cluster_iters=iters, **kw))


def _cases(test):
    return test.pytestmark[0].args[1]


@pytest.mark.parametrize("name,radius", [(n, 16) for n in B.SCENES] + [(n, r) for r in (1, 64) for n in EDGE])
def test_clustered_tree_structure(monkeypatch, name, radius):
    _clustered(monkeypatch, radius)
    B.test_device_tree_structure(name)


@pytest.mark.parametrize("name", ["small_dragon", "concentric"])
def test_forced_pairing(monkeypatch, name):
    _clustered(monkeypatch, 16, iters=1)
    B.test_device_tree_structure(name)
    dev = B._device()
    try:
        dev.upload(scene(name)[0])
        info = dev.wide_cluster_info()
    finally:
        dev.close()
    assert (info["radius_used"], info["iterations"]) == (16, 1) and info["paired_iterations"] > 0


@pytest.mark.parametrize("name,opts", _cases(B.test_device_tree_walks_equal_brute),
                         ids=B.SCENES + ["small_dragon-top8"])
def test_clustered_tree_walks_equal_brute(monkeypatch, name, opts):
    _clustered(monkeypatch, 16)
    B.test_device_tree_walks_equal_brute(name, opts)  # the rule's own cap, 1e-3; prints the excused share


@pytest.mark.parametrize("name,integrator,fused", _cases(B.test_device_tree_renders_equal_oracle))
def test_clustered_tree_renders_equal_oracle(monkeypatch, name, integrator, fused):
    _clustered(monkeypatch, 16)
    B.test_device_tree_renders_equal_oracle(name, integrator, fused)


def test_quality_and_interface():
    lib, info, sc = _ffi.load(), _ffi.WideClusterInfo(), scene("small_dragon")[0]

    def build(dev):
        try:
            dev.upload(sc)
            return dev.wide_export(), dev.wide_build_info(), dev.wide_cluster_info()
        finally:
            dev.close()
    dev = L.Device(0, accel=1, wide_build="device", wide_cluster=16)
    assert lib.lumo_scene_wide_cluster_info(dev.ctx, C.byref(info)) == 4  # LUMO_ERR_NO_SCENE
    assert lib.lumo_scene_set_wide_cluster(None, None) == 1 and lib.lumo_scene_wide_cluster_info(None, C.byref(info)) == 1
    for bad in (dict(radius=-1), dict(radius=65), dict(max_iter=-1), dict(max_iter=4097), dict(reserved=(0, 1)),
                dict(reserved=(1, 0))):  # refused: radius 16 stays
        assert lib.lumo_scene_set_wide_cluster(dev.ctx, C.byref(_ffi.WideClusterCfg(**{"radius": 8, **bad}))) == 1, bad
    _, ploc, how = build(dev)
    plain, lbvh, how_plain = build(L.Device(0, accel=1, wide_build="device"))
    zero, _, how_zero = build(L.Device(0, accel=1, wide_build="device", wide_cluster=0))
    _, host, how_host = build(L.Device(0, accel=1, wide_build="host", wide_cluster=16))
    assert (ploc["builder_used"], how["radius_used"]) == (1, 16) and how["iterations"] > 0 and how["cluster_ms"] > 0.0
    assert how["cluster_ms"] < ploc["build_ms"]
    print(f"sah_cost: radius 16 {ploc['sah_cost']:.3f}, LBVH {lbvh['sah_cost']:.3f}, host {host['sah_cost']:.3f}; "
          f"{how['iterations']} + {how['paired_iterations']} iterations")
    assert ploc["sah_cost"] < lbvh["sah_cost"]  # the same leaf_max, no margin
    assert how_plain["radius_used"] == how_zero["radius_used"] == 0 == how_zero["iterations"]
    for k in ("nodes", "tv", "obj_blas", "light_blas"):
        assert zero[k].tobytes() == plain[k].tobytes(), k
    assert (host["builder_used"], how_host["radius_used"]) == (0, 0)
