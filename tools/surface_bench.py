#!/usr/bin/env python
"""tools/surface_bench.py — what extracting the fluid's surface costs, to be run once on the MI355X.  bench.py's
config 2 scene (10^6 particles in the open tank) after 100 steps; the lattice is LiquidWorld.surface_lattice's - the fluid's box from
salva_hip_get_fluid_bounds grown by h - at spacing 2r and r.  Per spacing, alternating within the one run, outputs in device memory:
  whole           salva_hip_extract_surface, fraction = 0.5, vertices and triangles (the fill call: evaluation, classification, totals,
                  scans, emission)
  whole_normals   the same with normals (adds the evaluator's points path on the vertices and the normalisation)
  count_only      out == NULL: evaluation, classification and totals
  evaluate_*      salva_hip_evaluate_fields_lattice of the same lattice with the density alone - the parent commit's code and the
                  yardstick - and with the fraction alone, which is what the extraction evaluates
`passes_ms` = whole - evaluate_fraction (means): what the streaming passes over the nodes add to the evaluation they follow.

Clock: the host's, around calls that return when their results are complete (the calls end with a wait for the world's stream, which
is not exposed: device events cannot bracket the work).  3 warm-up and 20 timed repetitions; mean, standard deviation, min, max in ms.
Writes one JSON line to profiles/surface_bench.json and prints it.
Usage: python tools/surface_bench.py [--side 100] [--steps 100] [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DT, G = 1.0 / 200.0, (0.0, -9.81, 0.0)


def stats(ms):
    a = np.asarray(ms)
    return {"mean": round(float(a.mean()), 4), "std": round(float(a.std(ddof=1)), 4), "min": round(float(a.min()), 4), "max": round(float(a.max()), 4)}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    fluid, shell = bench.build_scene(args.side)
    w, _ = bench.make_world(fluid, shell, 0)
    for _ in range(args.steps):
        w.step(DT, G)
    r = np.float32(bench.R)
    dev = torch.device("cuda:0")
    rows = []
    for label, spacing in (("2r", 2 * r), ("r", r)):
        origin, dims = w.surface_lattice(spacing)
        nodes = dims[0] * dims[1] * dims[2]
        nv, nt = w.extract_surface_device(origin, spacing, dims)
        mesh = {k: torch.zeros(3 * max(n, 1), dtype=torch.int32 if k == "triangles" else torch.float32, device=dev)
                for k, n in (("vertices", nv), ("normals", nv), ("triangles", nt))}
        field = torch.zeros(nodes, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        room = dict(vertices=mesh["vertices"].data_ptr(), triangles=mesh["triangles"].data_ptr(), vertex_capacity=nv, triangle_capacity=nt)
        calls = {
            "whole": lambda: w.extract_surface_device(origin, spacing, dims, **room),
            "whole_normals": lambda: w.extract_surface_device(origin, spacing, dims, normals=mesh["normals"].data_ptr(), **room),
            "count_only": lambda: w.extract_surface_device(origin, spacing, dims),
            "evaluate_density": lambda: w.evaluate_lattice_device(origin, spacing, dims, density=field.data_ptr()),
            "evaluate_fraction": lambda: w.evaluate_lattice_device(origin, spacing, dims, fraction=field.data_ptr()),
        }
        times = {name: [] for name in calls}
        for k in range(args.warmup + args.reps):
            for name, call in calls.items():  # the calls alternate
                t = time.perf_counter()
                call()
                if k >= args.warmup:
                    times[name].append(1e3 * (time.perf_counter() - t))
        row = {"spacing": label, "origin": [float(v) for v in origin], "dims": list(dims), "nodes": nodes, "vertices": nv, "triangles": nt,
               **{name + "_ms": stats(v) for name, v in times.items()}}
        row["passes_ms"] = round(row["whole_ms"]["mean"] - row["evaluate_fraction_ms"]["mean"], 4)
        rows.append(row)
        del mesh, field
    out = {"tool": "tools/surface_bench.py", "particles": len(fluid), "steps_before": args.steps, "reps": args.reps, "warmup": args.warmup,
           "clock": "host, around calls that end with a stream wait", "field": "fraction", "iso": 0.5, "lattices": rows}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "surface_bench.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
