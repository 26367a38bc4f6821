#!/usr/bin/env python
"""tools/diffuse_bench.py — what the potentials of diffuse particles cost, to be run once on the MI355X.  The protocol
of tools/anisotropy_bench.py: bench.py's config 2 scene (10^6 particles in the open tank) after 100 steps, outputs in device memory, the
calls alternating within the one run:
  potentials         salva_hip_diffuse_potentials, all five outputs: the table over the fluid's box, both passes, the packing
  no_crest           the same without wave_crest: one pass
  count_only         count alone: the table and the walk without a sum
  fields_at_particles  salva_hip_evaluate_fields at the particles' own positions, count and velocity: the yardstick of DESIGN.md §20 -
                     the same 27 cells of width h per place
  update_1e5, update_1e6  salva_hip_update_diffuse of a set held at 10^5 and at 10^6 diffuse particles (seeded on the fluid's own
                     particles; no emission and no ageing in the timed calls, so that the set keeps its size): the table, the
                     evaluator at the diffuse particles, advection, the scan and the compaction, both passes of the potentials, the
                     emission's count, scan and placement, one read-back of the counters
  host_path          what the calls replace: salva_hip_get_fluid of positions and velocities into host memory
  host_path_1e5, host_path_1e6  the same and the upload of a diffuse set of that size (salva_hip_add_diffuse from host memory; the
                     host's neighbour sums are not included, which flatters the host)
Clock: the host's, around calls that return when their results are complete.  3 warm-up and 20 timed repetitions; mean, standard
deviation, min, max in ms.  Writes one JSON line to profiles/diffuse_bench.json and prints it.
Usage: python tools/diffuse_bench.py [--side 100] [--steps 100] [--reps 20]"""
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

DT, G = 1.0 / 200.0, (0.0, -9.81, 0.0)
WIDTH = dict(trapped_air=1, wave_crest=1, energy=1, normal=3, count=1)


def stats(ms):
    a = np.asarray(ms)
    return {"mean": round(float(a.mean()), 4), "std": round(float(a.std(ddof=1)), 4), "min": round(float(a.min()), 4), "max": round(float(a.max()), 4)}


def main():
    import torch

    from salva_amd import Diffuse, _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    fluid, shell = bench.build_scene(args.side)
    w, f = bench.make_world(fluid, shell, 0)
    for _ in range(args.steps):
        w.step(DT, G)
    dev = torch.device("cuda:0")
    prm = Diffuse()
    n = w.diffuse_potentials_device(prm)
    bufs = {k: torch.zeros(width * max(n, 1), dtype=torch.int32 if k == "count" else torch.float32, device=dev) for k, width in WIDTH.items()}
    ptr = {k: b.data_ptr() for k, b in bufs.items()}
    points = torch.from_numpy(np.ascontiguousarray(f.positions, np.float32)).to(dev).contiguous()
    velocity = torch.zeros(3 * max(n, 1), dtype=torch.float32, device=dev)
    host_x, host_v = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    fp = C.POINTER(C.c_float)
    torch.cuda.synchronize()
    calls = {
        "potentials": lambda: w.diffuse_potentials_device(prm, row_capacity=n, **ptr),
        "no_crest": lambda: w.diffuse_potentials_device(prm, row_capacity=n, **{k: v for k, v in ptr.items() if k != "wave_crest"}),
        "count_only": lambda: w.diffuse_potentials_device(prm, row_capacity=n, count=ptr["count"]),
        "fields_at_particles": lambda: w.evaluate_fields_device(points.data_ptr(), n, count=ptr["count"], velocity=velocity.data_ptr()),
        "host_path": lambda: _lib.check(w._L.salva_hip_get_fluid(w._h, f._slot, host_x.ctypes.data_as(fp), host_v.ctypes.data_as(fp))),
    }
    # the sets: seeded on fluid particles.  Rates 0: nothing is emitted; n_spray = n_bubble = 0 makes a bubble of every particle inside
    # the fluid, and with k_b = 0 and k_d = 1 it is carried along; no kill box: nothing is removed.  The sets keep their size.
    keep = Diffuse(k_ta=0.0, k_wc=0.0, n_spray=0, n_bubble=0, k_d=1.0, k_b=0.0)
    seeds = np.ascontiguousarray(f.positions, np.float32)
    sets = {}
    for label, size in (("1e5", 100000), ("1e6", 1000000)):
        size = min(size, n)
        pick = np.linspace(0, n - 1, size).astype(np.int64)
        ds = w.create_diffuse(size, keep)
        ds.add(seeds[pick], np.zeros((size, 3), np.float32), 1.0e9)
        sets[label] = (ds, size, seeds[pick].copy(), np.zeros((size, 3), np.float32))
        calls["update_" + label] = (lambda d=ds: d.update(DT))
    scratch = w.create_diffuse(1000000)

    def host_path(size, x, v):
        _lib.check(w._L.salva_hip_get_fluid(w._h, f._slot, host_x.ctypes.data_as(fp), host_v.ctypes.data_as(fp)))
        scratch.clear()
        scratch.add(x, v)

    for label, (ds, size, x, v) in sets.items():
        calls["host_path_" + label] = (lambda size=size, x=x, v=v: host_path(size, x, v))
    times = {name: [] for name in calls}
    for k in range(args.warmup + args.reps):
        for name, call in calls.items():  # the calls alternate
            t = time.perf_counter()
            call()
            if k >= args.warmup:
                times[name].append(1e3 * (time.perf_counter() - t))
    w.diffuse_potentials_device(prm, row_capacity=n, **ptr)
    got = {k: b.cpu().numpy() for k, b in bufs.items()}
    has_normal = (got["normal"].reshape(-1, 3) != 0).any(axis=1)
    out = {"tool": "tools/diffuse_bench.py", "particles": len(fluid), "rows": n, "neighbours_mean": round(float(got["count"].mean()), 2),
           "neighbours_max": int(got["count"].max()), "with_normal": int(has_normal.sum()), "with_crest": int((got["wave_crest"] > 0).sum()),
           "trapped_air_mean": round(float(got["trapped_air"].mean()), 4), "energy_mean": round(float(got["energy"].mean()), 6),
           "set_sizes": {label: len(ds) for label, (ds, _, _, _) in sets.items()}, "steps_before": args.steps, "reps": args.reps,
           "warmup": args.warmup, "clock": "host, around calls that end with a stream wait",
           **{name + "_ms": stats(v) for name, v in times.items()}}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "diffuse_bench.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
