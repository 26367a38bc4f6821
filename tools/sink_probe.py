#!/usr/bin/env python
"""tools/sink_probe.py — what deleting by region costs, to be run once on the MI355X.  bench.py's config 2 scene
(10^6 particles in the open tank) after 30 steps; the particles below a horizontal plane, about 1 % of them, are deleted.  Median of
REPS repetitions, each on a world rebuilt and stepped afresh, host wall clock around calls that return when their work is done:
  (a) the way before this call existed: salva_hip_get_fluid, a numpy mask, salva_hip_delete_particles;
  (b) salva_hip_delete_particles_in_region with the same half-space;
  (c) the same call with a half-space that matches nothing;
  (d) the next step without and with one registered sink that matches nothing.
Writes one JSON line to profiles/sink_probe.json and prints it.  Usage: python tools/sink_probe.py [--side 100] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from salva_amd import _lib, regions  # noqa: E402

DT, G = 1.0 / 200.0, (0.0, -9.81, 0.0)
FP, U8P = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def stepped_world(fluid, shell, steps):
    w, f = bench.make_world(fluid, shell, 0)
    for _ in range(steps):
        w.step(DT, G)
    return w, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    fluid, shell = bench.build_scene(args.side)
    n = len(fluid)
    pos, vel = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)

    w, f = stepped_world(fluid, shell, args.steps)  # where the plane lies: the first percentile of the heights after the steps
    _lib.check(w._L.salva_hip_get_fluid(w._h, 0, pos.ctypes.data_as(FP), vel.ctypes.data_as(FP)))
    y0 = float(np.percentile(pos[:, 1], 1.0))
    del w, f
    plane = regions.HalfSpace([0.0, y0, 0.0], [0.0, 1.0, 0.0])
    nowhere = regions.HalfSpace([0.0, float(pos[:, 1].min()) - 10.0, 0.0], [0.0, 1.0, 0.0])

    times = {k: [] for k in ("a_get_mask_delete", "b_region_call", "c_region_call_no_match", "d_step_plain", "d_step_with_idle_sink")}
    deleted = {}
    for _ in range(args.reps):
        w, f = stepped_world(fluid, shell, args.steps)
        t = time.perf_counter()
        _lib.check(w._L.salva_hip_get_fluid(w._h, 0, pos.ctypes.data_as(FP), vel.ctypes.data_as(FP)))
        mask = (pos[:, 1] <= np.float32(y0)).astype(np.uint8)
        kept = w._L.salva_hip_delete_particles(w._h, 0, mask.ctypes.data_as(U8P))
        times["a_get_mask_delete"].append(time.perf_counter() - t)
        deleted["a"] = n - int(kept)
        del w, f

        for key, region in (("b_region_call", plane), ("c_region_call_no_match", nowhere)):
            w, f = stepped_world(fluid, shell, args.steps)
            r = region._struct(w)
            t = time.perf_counter()
            k = w._L.salva_hip_delete_particles_in_region(w._h, C.byref(r), 0, None)
            times[key].append(time.perf_counter() - t)
            deleted[key[0]] = int(k)
            del w, f

        for key, sink in (("d_step_plain", False), ("d_step_with_idle_sink", True)):
            w, f = stepped_world(fluid, shell, args.steps)
            if sink:
                w.add_sink(nowhere, f)
            g = (C.c_float * 3)(*G)
            st = _lib.StepStats()
            t = time.perf_counter()
            _lib.check(w._L.salva_hip_step(w._h, DT, g, C.byref(st)))
            times[key].append(time.perf_counter() - t)
            del w, f

    assert deleted["a"] == deleted["b"] and deleted["c"] == 0, deleted
    out = {"tool": "tools/sink_probe.py", "particles": n, "steps_before": args.steps, "reps": args.reps, "plane_y": y0,
           "deleted": deleted["b"], "deleted_share": deleted["b"] / n,
           "median_ms": {k: round(1e3 * float(np.median(v)), 4) for k, v in times.items()},
           "min_ms": {k: round(1e3 * float(np.min(v)), 4) for k, v in times.items()},
           "max_ms": {k: round(1e3 * float(np.max(v)), 4) for k, v in times.items()}}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sink_probe.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
