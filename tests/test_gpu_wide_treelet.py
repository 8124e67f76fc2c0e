"""Treelet restructuring of the clustered device builder's tree (lumo_scene_set_wide_treelet).
The yardsticks are tests/test_gpu_wide_build.py's, which never depended on the builder: its `_device` is pointed
at the clustered builder (radius 16) with the passes on and its test functions run as they are.  What is new
here: the binary objective before and after, the counts, and the interface."""
import ctypes as C

import pytest

import lumo_amd as L
import test_gpu_wide_build as B
from lumo_amd import _ffi
from test_brute import scene

pytestmark = pytest.mark.gpu
# many waves and treelets stacked over passes; object leaves inside treelets and BLASes of about 7 primitives;
# every area comparison a tie; zero areas, nothing strictly better (two); trees of 1 and 2, never qualifying
EDGE = ["small_dragon", "scaled_instances", "concentric", "flat", "degenerate", "spheres"]


def _treelets(monkeypatch, passes, gamma=7):
    monkeypatch.setattr(B, "_device", lambda **kw: L.Device(0, accel=1, wide_build="device", wide_cluster=16,
                                                            wide_treelet=passes, treelet_gamma=gamma, **kw))


def _cases(test):
    return test.pytestmark[0].args[1]


@pytest.mark.parametrize("name,passes,gamma", [(n, 2, 7) for n in B.SCENES] + [(n, p, 7) for p in (1, 3) for n in EDGE] +
                         [("small_dragon", 2, 64)])  # gamma 64: only upper nodes qualify
def test_treelet_tree_structure(monkeypatch, name, passes, gamma):
    _treelets(monkeypatch, passes, gamma)
    B.test_device_tree_structure(name)


@pytest.mark.parametrize("name,opts", _cases(B.test_device_tree_walks_equal_brute),
                         ids=B.SCENES + ["small_dragon-top8"])
def test_treelet_tree_walks_equal_brute(monkeypatch, name, opts):
    _treelets(monkeypatch, 2)
    B.test_device_tree_walks_equal_brute(name, opts)  # the rule's own cap, 1e-3; prints the excused share


@pytest.mark.parametrize("name,integrator,fused", _cases(B.test_device_tree_renders_equal_oracle))
def test_treelet_tree_renders_equal_oracle(monkeypatch, name, integrator, fused):
    _treelets(monkeypatch, 2)
    B.test_device_tree_renders_equal_oracle(name, integrator, fused)


def test_quality_and_interface():
    lib, info, sc = _ffi.load(), _ffi.WideTreeletInfo(), scene("small_dragon")[0]

    def build(dev):
        try:
            dev.upload(sc)
            return dev.wide_export(), dev.wide_build_info(), dev.wide_treelet_info()
        finally:
            dev.close()
    dev = L.Device(0, accel=1, wide_build="device", wide_cluster=16, wide_treelet=2)
    assert lib.lumo_scene_wide_treelet_info(dev.ctx, C.byref(info)) == 4  # LUMO_ERR_NO_SCENE
    assert lib.lumo_scene_set_wide_treelet(None, None) == 1 and lib.lumo_scene_wide_treelet_info(None, C.byref(info)) == 1
    for bad in [dict(passes=-1), dict(passes=9), dict(gamma=(1 << 20) + 1), dict(reserved=(0, 1)), dict(reserved=(1, 0))] + \
            [dict(gamma=g) for g in range(1, 7)]:  # refused: 2 passes stay
        assert lib.lumo_scene_set_wide_treelet(dev.ctx, C.byref(_ffi.WideTreeletCfg(**{"passes": 1, **bad}))) == 1, bad
    _, tree, how = build(dev)
    zero, ploc, how_zero = build(L.Device(0, accel=1, wide_build="device", wide_cluster=16, wide_treelet=0))
    plain, _, how_plain = build(L.Device(0, accel=1, wide_build="device", wide_cluster=16))
    _, lbvh, how_lbvh = build(L.Device(0, accel=1, wide_build="device", wide_treelet=2))
    _, host, how_host = build(L.Device(0, accel=1, wide_build="host", wide_cluster=16, wide_treelet=2))
    print(f"sah_cost: host {host['sah_cost']:.3f}, LBVH {lbvh['sah_cost']:.3f}, PLOC {ploc['sah_cost']:.3f}, "
          f"PLOC + treelets {tree['sah_cost']:.3f}; {how}")
    assert how["passes_used"] == 2 and how["tried"] >= how["replaced"] > 0 and how["treelet_ms"] > 0.0
    assert how["treelet_ms"] < tree["build_ms"]
    assert tree["sah_cost"] < ploc["sah_cost"]  # the wide tree's cost follows the binary objective here: no margin
    assert how["area_after"] < how["area_before"]  # by construction once a treelet was replaced: no margin
    assert how["area_before"] == how_zero["area_after"] == how_zero["area_before"]  # the clustered tree's, bit for bit
    assert (how_zero["passes_used"], how_zero["tried"], how_zero["treelet_ms"]) == (0, 0, 0.0) and how_plain == how_zero
    for k in ("nodes", "tv", "obj_blas", "light_blas"):
        assert zero[k].tobytes() == plain[k].tobytes(), k
    for inert, used in ((how_lbvh, lbvh), (how_host, host)):  # radius 0; the host builder
        assert not any(inert.values()) and used["builder_used"] == (1 if inert is how_lbvh else 0)
