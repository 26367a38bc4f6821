"""tools/elastic_bench.py — one JSON line for Becker2009Elasticity at 10^6 particles: a 100 x 100 x 100 elastic block (E = 5e5,
nu = 0.3, nonlinear strain, with XSPHViscosity(0.5, 1.0)) resting on a sampled floor, ms per step with and without the force
(same scene, 5 warm-up + 20 timed steps), the rotation / stress pass and the force pass on their own (salva_hip_time_kernel 7 and 8)
and their fraction of the algorithmic byte model of DESIGN.md §12 at 8 TB/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import salva_amd  # noqa: E402
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, XSPHViscosity, scenes  # noqa: E402

R = 0.025
DT = 1.0 / 200.0
HBM = 8.0e12


def run(side, elastic, warmup, steps):
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    p = scenes.cube_fluid_positions(side, side, side, R).astype(np.float32)
    p[:, 1] -= p[:, 1].min() - np.float32(2 * R)
    f = Fluid(p, R, 1000.0)
    if elastic:
        f.nonpressure_forces.append(salva_amd.Becker2009Elasticity(5e5, 0.3, True))
    f.nonpressure_forces.append(XSPHViscosity(0.5, 1.0))
    w.add_fluid(f)
    half = side * R + 4 * R
    n_floor = int(2 * half / (2 * R)) + 1
    w.add_boundary(Boundary(scenes.plane_lattice(n_floor, n_floor, 0.0, R, -half, -half, layers=2)))
    for _ in range(warmup):
        w.step(DT, (0.0, -9.81, 0.0))
    t0 = time.perf_counter()
    for _ in range(steps):
        w.step(DT, (0.0, -9.81, 0.0))
    ms = (time.perf_counter() - t0) * 1e3 / steps
    out = {"ms_per_step": ms, "n": len(p)}
    if elastic:
        st = w.elasticity_state(f)
        k = st["ncontacts0"] / len(p)
        t7 = float(w._L.salva_hip_time_kernel(w._h, 7, 20))
        t8 = float(w._L.salva_hip_time_kernel(w._h, 8, 20))
        n = len(p)
        b7 = n * (4 * k + 164)
        b8 = n * (4 * k + 148) + n * 28
        out.update({"K": k, "rot_stress_us": t7, "forces_us": t8, "rot_stress_model_us": b7 / HBM * 1e6, "forces_model_us": b8 / HBM * 1e6,
                    "rot_stress_frac": b7 / HBM * 1e6 / t7, "forces_frac": b8 / HBM * 1e6 / t8})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    with_f = run(a.side, True, a.warmup, a.steps)
    without = run(a.side, False, a.warmup, a.steps)
    print(json.dumps({"bench": "elastic", "n": with_f["n"], "ms_per_step_with": with_f["ms_per_step"],
                      "ms_per_step_without": without["ms_per_step"], **{k: v for k, v in with_f.items() if k not in ("n", "ms_per_step")}}))


if __name__ == "__main__":
    main()
