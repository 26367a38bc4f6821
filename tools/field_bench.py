#!/usr/bin/env python
"""tools/field_bench.py — what evaluating SPH fields on a lattice costs, to be run once on the MI355X.  bench.py's
config 2 scene (10^6 particles in the open tank) after 100 steps; the lattice covers the fluid's box at spacing r, 2r, h/2, h and 2h.
Two worlds hold the same state, one created with SALVA_HIP_FIELD_ARM=points and one with =lattice (the switch is read when a world is
created), and their evaluations alternate within the one run: warm-up first, then REPS repetitions of the five-field and of the
density-only evaluation per arm and spacing, outputs in device memory.

Clock: the host's, around calls that return when their results are complete (SALVA_HIP_FIELD_OUT_ON_DEVICE: the call ends with a
wait for the world's stream).  The world's stream is not exposed, so device events cannot bracket the work; the figures therefore
include the launches and the one wait, about what a caller pays.  Reported: mean, standard deviation, min and max in ms.

Also timed, for scale: salva_hip_get_fluid of all particles — what a user of the parent commit paid for the same information BEFORE
doing the neighbour sums on the host, which are not included.

Writes one JSON line to profiles/field_bench.json and prints it.  `crossover`: the largest measured spacing / h at which the brick arm
is faster than the lane-per-point arm by more than the larger of the two standard deviations (five fields).
Usage: python tools/field_bench.py [--side 100] [--steps 100] [--reps 20]"""
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
from salva_amd import _lib  # noqa: E402

DT, G = 1.0 / 200.0, (0.0, -9.81, 0.0)
FP = C.POINTER(C.c_float)
FIELDS = (("density", 1), ("fraction", 1), ("velocity", 3), ("gradient", 3), ("count", 1))


def world_with_arm(arm, fluid, shell, steps):
    os.environ["SALVA_HIP_FIELD_ARM"] = arm
    w, f = bench.make_world(fluid, shell, 0)
    os.environ.pop("SALVA_HIP_FIELD_ARM")
    for _ in range(steps):
        w.step(DT, G)
    return w, f


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
    n = len(fluid)
    worlds = {arm: world_with_arm(arm, fluid, shell, args.steps) for arm in ("points", "lattice")}
    pos, vel = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    w0 = worlds["points"][0]
    download = []
    for k in range(args.warmup + args.reps):
        t = time.perf_counter()
        _lib.check(w0._L.salva_hip_get_fluid(w0._h, 0, pos.ctypes.data_as(FP), vel.ctypes.data_as(FP)))
        if k >= args.warmup:
            download.append(1e3 * (time.perf_counter() - t))
    r, h = np.float32(bench.R), np.float32(bench.R) * np.float32(4.0)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    dev = torch.device("cuda:0")
    rows = []
    for label, spacing in (("r", r), ("2r", 2 * r), ("h/2", h / 2), ("h", h), ("2h", 2 * h)):
        dims = tuple(int(np.floor((hi[a] - lo[a]) / spacing)) + 1 for a in range(3))
        nodes = dims[0] * dims[1] * dims[2]
        bufs = {k: torch.zeros(nodes * width, dtype=torch.int32 if k == "count" else torch.float32, device=dev) for k, width in FIELDS}
        torch.cuda.synchronize()
        sets = {"five": {k: b.data_ptr() for k, b in bufs.items()}, "density": {"density": bufs["density"].data_ptr()}}
        times = {(arm, s): [] for arm in worlds for s in sets}
        for k in range(args.warmup + args.reps):
            for s, addresses in sets.items():
                for arm, (w, _) in worlds.items():  # the arms alternate
                    t = time.perf_counter()
                    w.evaluate_lattice_device(lo, spacing, dims, **addresses)
                    if k >= args.warmup:
                        times[(arm, s)].append(1e3 * (time.perf_counter() - t))
        inside = int((bufs["count"] > 0).sum().item())
        rows.append({"spacing": label, "spacing_over_h": round(float(spacing / h), 4), "dims": dims, "nodes": nodes, "nodes_in_support": inside,
                     **{f"{arm}_{s}_ms": stats(v) for (arm, s), v in times.items()}})
        del bufs
    crossover = 0.0
    for row in rows:
        b, p = row["lattice_five_ms"], row["points_five_ms"]
        if b["mean"] + max(b["std"], p["std"]) < p["mean"]:
            crossover = max(crossover, row["spacing_over_h"])
    out = {"tool": "tools/field_bench.py", "particles": n, "steps_before": args.steps, "reps": args.reps, "warmup": args.warmup,
           "clock": "host, around calls that end with a stream wait", "lattices": rows, "crossover_spacing_over_h": crossover,
           "get_fluid_ms": stats(download), "get_fluid_note": "the download only: the host-side neighbour sums are not included"}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "field_bench.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
