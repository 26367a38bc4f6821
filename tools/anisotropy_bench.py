#!/usr/bin/env python
"""tools/anisotropy_bench.py — what the anisotropic kernels cost, to be run once on the MI355X.  The protocol of
tools/surface_bench.py: bench.py's config 2 scene (10^6 particles in the open tank) after 100 steps, LiquidWorld.surface_lattice at
spacing 2r and r, outputs in device memory, the calls alternating within the one run:
  moments            salva_hip_compute_anisotropy of every particle (centres, metrics, counts): the table over the fluid's box, the
                     neighbour sums over 2h, the eigen-decompositions, the packing
  aniso_lattice      salva_hip_evaluate_fields_anisotropic_lattice, fraction alone: the moments of the particles that can matter, the
                     table on the centres, the sums
  aniso_whole        salva_hip_extract_surface_anisotropic, fraction = 0.5, vertices and triangles
  aniso_whole_normals  the same with normals (a second anisotropic evaluation, on the vertices)
  iso_lattice, iso_whole, iso_whole_normals   the isotropic calls of DESIGN.md §20 / §21 on the same lattice: the yardstick
Clock: the host's, around calls that return when their results are complete.  3 warm-up and 20 timed repetitions; mean, standard
deviation, min, max in ms.  Writes one JSON line to profiles/anisotropy_bench.json and prints it.
Usage: python tools/anisotropy_bench.py [--side 100] [--steps 100] [--reps 20]"""
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

    from salva_amd import Anisotropy

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
    prm = Anisotropy()
    n = w.anisotropy_device(prm)
    per_row = {k: torch.zeros(width * max(n, 1), dtype=torch.int32 if k == "count" else torch.float32, device=dev)
               for k, width in (("centres", 3), ("metric", 6), ("count", 1))}
    rows = []
    for label, spacing in (("2r", 2 * r), ("r", r)):
        origin, dims = w.surface_lattice(spacing)
        nodes = dims[0] * dims[1] * dims[2]
        sizes = {"iso": w.extract_surface_device(origin, spacing, dims), "aniso": w.extract_surface_device(origin, spacing, dims, anisotropy=prm)}
        nv, nt = max(sizes["iso"][0], sizes["aniso"][0]), max(sizes["iso"][1], sizes["aniso"][1])
        mesh = {k: torch.zeros(3 * max(m, 1), dtype=torch.int32 if k == "triangles" else torch.float32, device=dev)
                for k, m in (("vertices", nv), ("normals", nv), ("triangles", nt))}
        field = torch.zeros(nodes, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        room = dict(vertices=mesh["vertices"].data_ptr(), triangles=mesh["triangles"].data_ptr(), vertex_capacity=nv, triangle_capacity=nt)
        normals = mesh["normals"].data_ptr()
        calls = {
            "moments": lambda: w.anisotropy_device(prm, row_capacity=n, **{k: b.data_ptr() for k, b in per_row.items()}),
            "aniso_lattice": lambda: w.evaluate_lattice_device(origin, spacing, dims, anisotropy=prm, fraction=field.data_ptr()),
            "iso_lattice": lambda: w.evaluate_lattice_device(origin, spacing, dims, fraction=field.data_ptr()),
            "aniso_whole": lambda: w.extract_surface_device(origin, spacing, dims, anisotropy=prm, **room),
            "iso_whole": lambda: w.extract_surface_device(origin, spacing, dims, **room),
            "aniso_whole_normals": lambda: w.extract_surface_device(origin, spacing, dims, anisotropy=prm, normals=normals, **room),
            "iso_whole_normals": lambda: w.extract_surface_device(origin, spacing, dims, normals=normals, **room),
        }
        times = {name: [] for name in calls}
        for k in range(args.warmup + args.reps):
            for name, call in calls.items():  # the calls alternate
                t = time.perf_counter()
                call()
                if k >= args.warmup:
                    times[name].append(1e3 * (time.perf_counter() - t))
        rows.append({"spacing": label, "origin": [float(v) for v in origin], "dims": list(dims), "nodes": nodes,
                     "iso_mesh": list(sizes["iso"]), "aniso_mesh": list(sizes["aniso"]), **{name + "_ms": stats(v) for name, v in times.items()}})
        del mesh, field
    count = per_row["count"].cpu().numpy()
    out = {"tool": "tools/anisotropy_bench.py", "particles": len(fluid), "rows": n, "neighbours_mean": round(float(count.mean()), 2),
           "neighbours_max": int(count.max()), "steps_before": args.steps, "reps": args.reps, "warmup": args.warmup,
           "clock": "host, around calls that end with a stream wait", "field": "fraction", "iso": 0.5, "lattices": rows}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "anisotropy_bench.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
