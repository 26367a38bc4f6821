#!/usr/bin/env python
"""tools/vorticity_probe.py — what a VorticityConfinement entry costs per step, to be run once on the MI355X.

bench.py's config 2 scene (side^3 particles in the open tank, DFSPH + XSPH) in three worlds of the same build, stepped side by side:
  without     the scene as bench.py steps it
  curl_only   + VorticityConfinement(0): pass 1 alone (k_vorticity_curl)
  confine     + VorticityConfinement(strength): both passes
After `--settle` steps taken by all three, `--rounds` rounds of `--steps` steps each, the worlds alternating within a round; the clock
is the host's around steps that end in the step's own read-back of its statistics (a step returns when its last kernel has finished).
Per world: mean, standard deviation, min and max of the per-round ms per step; the differences to `without` are the entry's cost, and
the spread of `without` against itself is what a difference has to exceed.  The algorithmic bytes of a pass — per particle: two float4
in (position + mass, velocity; or position + volume, omega), one float4 out (omega; or the acceleration, read and written: two), the
list's dwords not counted — over the kernel time a profile reports give its share of the HBM roofline; this probe reports step times only.
Writes one JSON line to profiles/vorticity_probe.json and prints it.
Usage: python tools/vorticity_probe.py [--side 100] [--settle 20] [--steps 20] [--rounds 5] [--strength 0.05]"""
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
    return {"mean": round(float(a.mean()), 4), "std": round(float(a.std(ddof=1)), 4) if len(a) > 1 else 0.0, "min": round(float(a.min()), 4),
            "max": round(float(a.max()), 4)}


def main():
    import torch

    from salva_amd import VorticityConfinement

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--settle", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--strength", type=float, default=0.05)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vorticity_probe.py needs an MI355X: there is no CPU path to measure")
    fluid, shell = bench.build_scene(args.side)
    worlds = {}
    for name, extra in (("without", []), ("curl_only", [VorticityConfinement(0.0)]), ("confine", [VorticityConfinement(args.strength)])):
        w, f = bench.make_world(fluid, shell, 0)
        f.nonpressure_forces.extend(extra)
        worlds[name] = w
    for _ in range(args.settle):
        for w in worlds.values():
            w.step(DT, G)
    ms = {name: [] for name in worlds}
    for _ in range(args.rounds):
        for name, w in worlds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                w.step(DT, G)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    out = {"particles": int(len(fluid)), "settle": args.settle, "steps_per_round": args.steps, "rounds": args.rounds, "strength": args.strength,
           "ms_per_step": {name: stats(v) for name, v in ms.items()}}
    base = out["ms_per_step"]["without"]["mean"]
    out["cost_ms_per_step"] = {name: round(out["ms_per_step"][name]["mean"] - base, 4) for name in ("curl_only", "confine")}
    # what the two passes move at the least, per step (one substep per step): 48 + 64 bytes per particle
    out["algorithmic_bytes_per_step"] = {"curl": 48 * int(len(fluid)), "confine": 64 * int(len(fluid))}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vorticity_probe.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
