#!/usr/bin/env python
"""tools/raycast_bench.py — what casting rays at the fluid costs, to be run once on the MI355X.  bench.py's config 2
scene (10^6 particles in the open tank) after 100 steps, §20's protocol: outputs in device memory, warm-up first, then REPS
repetitions, the arms alternating within the one run, mean +- standard deviation, the host's clock around calls that return when
their results are complete (SALVA_HIP_RAY_OUT_ON_DEVICE: the call ends with a wait for the world's stream).

Arms: a 1920 x 1080 camera looking down on the tank and one looking along it, each asking for the first hit only, + normal,
+ thickness; 2 x 10^6 random rays from a list in device memory (origins in the fluid's box grown by half its size, aimed at points
in the box), first hit + normal; and a call with one ray, which is the build of the call's own table (box reduction, keys, scan,
sort) plus one lane's walk - the floor under every call.  Every call builds its table: it is part of each figure.
Then, untimed, the mean and the maximum number of particles a ray's walk put to the exact cast (salva_hip_count_ray_candidates), for
the first-hit walk and for the thickness walk of each set of rays.

Also timed, for scale: salva_hip_get_fluid of all particles — what a user of the parent commit paid BEFORE any host-side
acceleration structure or cast.

Writes one JSON line to --out (profiles/raycast_bench.json) and prints it.
Usage: python tools/raycast_bench.py [--side 100] [--steps 100] [--reps 20]"""
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
OUTPUTS = (("t", 1), ("fluid", 1), ("index", 1), ("normal", 3), ("thickness", 1))
SETS = {"first_hit": ("t", "fluid", "index"), "plus_normal": ("t", "fluid", "index", "normal"),
        "plus_thickness": ("t", "fluid", "index", "normal", "thickness")}


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
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_bench.json"))
    args = ap.parse_args()
    fluid, shell = bench.build_scene(args.side)
    n = len(fluid)
    w, _ = bench.make_world(fluid, shell, 0)
    for _ in range(args.steps):
        w.step(DT, G)
    pos, vel = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    download = []
    for k in range(args.warmup + args.reps):
        t = time.perf_counter()
        _lib.check(w._L.salva_hip_get_fluid(w._h, 0, pos.ctypes.data_as(FP), vel.ctypes.data_as(FP)))
        if k >= args.warmup:
            download.append(1e3 * (time.perf_counter() - t))
    lo, hi = pos.min(axis=0).astype(np.float64), pos.max(axis=0).astype(np.float64)
    mid, size = 0.5 * (lo + hi), hi - lo
    # looking down -y from two units above the fluid: where the frustum meets the fluid's top (t = 2) it spans the box in x (right) and
    # z (up) and a tenth more; looking along +x from two units in front of it, likewise
    cams = {
        "down": {"origin": [mid[0], hi[1] + 2.0, mid[2]], "forward": [0.0, -1.0, 0.0], "right": [0.275 * size[0], 0.0, 0.0], "up": [0.0, 0.0, 0.275 * size[2]]},
        "along": {"origin": [lo[0] - 2.0, mid[1], mid[2]], "forward": [1.0, 0.0, 0.0], "right": [0.0, 0.0, 0.275 * size[2]], "up": [0.0, 0.275 * size[1], 0.0]},
    }
    for c in cams.values():
        c["width"], c["height"] = 1920, 1080
    dev = torch.device("cuda:0")
    m_cam, m_list = 1920 * 1080, args.rays
    room = max(m_cam, m_list)
    bufs = {k: torch.zeros(room * width, dtype=torch.int32 if k in ("fluid", "index") else torch.float32, device=dev) for k, width in OUTPUTS}
    rng = np.random.default_rng(1)
    origins = rng.uniform(lo - 0.5 * size, hi + 0.5 * size, (m_list, 3))
    directions = rng.uniform(lo, hi, (m_list, 3)) - origins
    d_o, d_d = (torch.from_numpy(a.astype(np.float32)).to(dev).contiguous() for a in (origins, directions))
    torch.cuda.synchronize()

    def addresses(names):
        return {k: bufs[k].data_ptr() for k in names}

    arms = {}
    for cname, cam in cams.items():
        for sname, names in SETS.items():
            arms[f"camera_{cname}_{sname}"] = (lambda cam=cam, names=names: w.cast_camera_device(cam, **addresses(names)))
    arms["list_plus_normal"] = lambda: w.cast_rays_device(d_o.data_ptr(), d_d.data_ptr(), m_list, **addresses(SETS["plus_normal"]))
    arms["one_ray_table_build"] = lambda: w.cast_rays_device(d_o.data_ptr(), d_d.data_ptr(), 1, **addresses(SETS["first_hit"]))
    times = {k: [] for k in arms}
    for k in range(args.warmup + args.reps):
        for name, call in arms.items():  # the arms alternate
            t = time.perf_counter()
            call()
            if k >= args.warmup:
                times[name].append(1e3 * (time.perf_counter() - t))
    hits = {}
    for cname, cam in cams.items():
        w.cast_camera_device(cam, **addresses(SETS["plus_thickness"]))
        hits[cname] = {"hits": int((bufs["fluid"][:m_cam] != -1).sum().item()), "mean_thickness": float(bufs["thickness"][:m_cam].mean().item())}
    w.cast_rays_device(d_o.data_ptr(), d_d.data_ptr(), m_list, **addresses(SETS["first_hit"]))
    hits["list"] = {"hits": int((bufs["fluid"][:m_list] != -1).sum().item())}
    # candidates put to the exact cast per ray (salva_hip_count_ray_candidates), reduced on the device
    tested = torch.zeros(room, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    candidates = {}
    for walk, thick in (("first_hit_walk", False), ("thickness_walk", True)):
        for cname, cam in cams.items():
            w.count_ray_candidates_device(tested.data_ptr(), camera=cam, thickness_walk=thick)
            v = tested[:m_cam].to(torch.float64)
            candidates[f"camera_{cname}_{walk}"] = {"mean": round(float(v.mean().item()), 2), "max": int(v.max().item())}
        w.count_ray_candidates_device(tested.data_ptr(), d_o.data_ptr(), d_d.data_ptr(), m_list, thickness_walk=thick)
        v = tested[:m_list].to(torch.float64)
        candidates[f"list_{walk}"] = {"mean": round(float(v.mean().item()), 2), "max": int(v.max().item())}
    out = {"tool": "tools/raycast_bench.py", "particles": n, "steps_before": args.steps, "reps": args.reps, "warmup": args.warmup,
           "clock": "host, around calls that end with a stream wait", "radius": float(bench.R), "camera_rays": m_cam, "list_rays": m_list,
           "box": [[round(float(v), 4) for v in lo], [round(float(v), 4) for v in hi]], "ms": {k: stats(v) for k, v in times.items()}, "seen": hits,
           "candidates_tested_per_ray": candidates,
           "get_fluid_ms": stats(download), "get_fluid_note": "the download only: no host-side acceleration structure or cast included"}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
