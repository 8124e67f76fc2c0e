"""bench.py's command line: a plain run reports the headline only, `--full` adds what else the
benchmark measures, and `--dump-outputs DIR` writes the last timed frame's outputs (the tile
buffers and per-task counters the render call returned), identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
SMALL = ["--gpus", "1", "--res", "48", "--spp", "4"]  # 9 tiles, one batch


def _oracle_frame(res):
    import bench
    import lumo_amd as L
    import oracle_ffi as O
    scene, cam = L.Scene.cornell_box(), L.Camera.cornell_box((res, res))
    tasks = L.make_tasks(res, res, 2, bench.SEED)
    bufs, results, _ = O.render_tasks(scene.build().desc(), cam.desc, tasks, O.WAVEFRONT, 2)
    return tasks, bufs, results


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_whole_frame(tmp_path):
    """Under the budget every tile buffer is written, in task order, with every task's counters."""
    import bench
    tasks, bufs, results = _oracle_frame(40)  # 9 tiles, the last row and column 8 pixels wide
    half = len(tasks) // 2  # two render calls of one frame (the dynamic schedule's chunks)
    bench.dump_outputs(str(tmp_path), [(tasks[:half], bufs[:half], results[:half]),
                                       (tasks[half:], bufs[half:], results[half:])], None, 0, 1)
    d = _load(tmp_path)
    assert sorted(d) == ["counters", "rgb_w", "rgb_w_tasks"]
    assert all(a.dtype == np.float64 for a in d.values())
    np.testing.assert_array_equal(d["rgb_w_tasks"], np.arange(len(tasks)))
    np.testing.assert_array_equal(d["rgb_w"], np.concatenate(bufs))
    np.testing.assert_array_equal(d["counters"], [(r.num_camera_rays, r.num_rays, r.num_queries) for r in results])


def test_dump_outputs_keeps_to_its_budget(tmp_path, monkeypatch):
    """Over the budget: a sample of the tile buffers (and of the splat film's pixels) that is the
    same on every call, the files together below the budget."""
    import bench
    tasks, bufs, results = _oracle_frame(40)
    splats = np.arange(40 * 40 * 3, dtype=np.float64).reshape(40, 40, 3)
    monkeypatch.setattr(bench, "DUMP_BYTES", 20000)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for p in dirs:
        bench.dump_outputs(str(p), [(tasks, bufs, results)], splats, 0, 1)
    a, b = _load(dirs[0]), _load(dirs[1])
    assert sum(os.path.getsize(dirs[0] / n) for n in os.listdir(dirs[0])) <= 20000
    assert sorted(a) == ["counters", "rgb_w", "rgb_w_tasks", "splat_film", "splat_film_pixels"]
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    pick = a["rgb_w_tasks"].astype(int)
    assert 0 < len(pick) < len(tasks) and (np.diff(pick) > 0).all()
    np.testing.assert_array_equal(a["rgb_w"], np.concatenate([bufs[i] for i in pick]))
    assert len(a["counters"]) == len(tasks)
    px = a["splat_film_pixels"].astype(int)
    assert 0 < len(px) < 40 * 40
    np.testing.assert_array_equal(a["splat_film"], splats.reshape(-1, 3)[px])


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_repeat(tmp_path):
    """A plain run times --steps frames and nothing else; its dumped outputs are the oracle's
    (C1 renders bit-exact) and the same on a second run."""
    import bench
    import lumo_amd as L
    import oracle_ffi as O
    a, err = _bench(*SMALL, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    b, _ = _bench(*SMALL, "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "b"))
    for k in HEADLINE:
        assert k in a, k
    assert (a["steps"], a["warmup"], b["steps"], b["warmup"]) == (3, 1, 1, 0)
    assert a["metric"] == "Mrays/s" and a["unit"] == "Mrays/s" and a["higher_is_better"] is True and a["dtype"] == "f64"
    assert a["value"] > 0 and a["ms_per_step"] > 0
    assert a["cpu_baseline"] is None and not {"c2", "c3", "c4_share"} & set(a)
    assert "cpu baseline" not in err and "c3:" not in err
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(da) == ["counters", "rgb_w", "rgb_w_tasks"]
    for k in da:
        assert da[k].dtype == np.float64
        np.testing.assert_array_equal(da[k], db[k])
    scene, cam, (w, h), spp, _ = bench.build_config("c1", 48, 4)
    tasks = L.make_tasks(w, h, spp, bench.SEED)
    bufs, results, _ = O.render_tasks(scene.desc(), cam.desc, tasks, O.WAVEFRONT, 4)
    np.testing.assert_array_equal(da["rgb_w"], np.concatenate(bufs))
    np.testing.assert_array_equal(da["counters"][:, 0], [r.num_camera_rays for r in results])
    assert a["queries_per_step"] == da["counters"][:, 2].sum()


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline():
    """--full goes on to the CPU baseline (the further frames switched off here: they take minutes)."""
    d, err = _bench(*SMALL, "--steps", "1", "--warmup", "0", "--full", "--bistro-frames", "0", "--dragon-frames", "0",
                    "--c4-share", "")
    for k in HEADLINE:
        assert k in d, k
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["unit"] == "Mrays/s"
    assert "cpu baseline" in err
