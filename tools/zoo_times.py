"""Frame times of the kernels no bench configuration runs: the tests' material zoo (feature class 1)
and texture zoo (class 2), n_shadow = 1, at 512 x 384 @ 64 spp through the fused, tail (tail_below
above the path count) and split schedules, each with pipeline 0.  Per schedule one warm-up frame,
then the median of three frames in ms.  Prints one JSON line; LUMO_AMD_LIB picks the library, as
for tools/ab2.sh.  Usage (repo root): LUMO_AMD_LIB=lumo_amd/var/liblumo_amd_<name>.so python tools/zoo_times.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lumo_amd as L  # noqa: E402
from scenes import default_camera, material_zoo, texture_zoo  # noqa: E402

W, H, SPP = 512, 384, 64
out = {}
for name, sc in (("material", material_zoo()), ("texture", texture_zoo().build())):
    cam = default_camera((W, H))
    tasks = L.make_tasks(W, H, SPP, 0xD1CE)
    for how, fused, tail in (("fused", 1, 0), ("tail", 1, 1 << 30), ("split", 0, 0)):
        d = L.Device(0, fused=fused, tail_below=tail, pipeline=0)
        try:
            d.upload(sc, cam)
            d.render_tasks(tasks)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                d.render_tasks(tasks)
                ts.append((time.perf_counter() - t0) * 1e3)
            out[f"{name}_{how}"] = round(sorted(ts)[1], 2)
        finally:
            d.close()
print(json.dumps(out))
