#!/usr/bin/env python
"""tools/sampling_bench.py [--out FILE] — what volume-sampling a shape into a fluid costs on the device, next to what
replaces it without the sampler: a numpy build of the same points plus salva_hip_add_particles.

Shapes: a cuboid of ~8 x 10^6 points and a ball of ~10^6 at r = 0.005.  Every timed call ends in a synchronisation of the world's
stream (the entry points return when the device work is done), so a host clock around the call is the call's time; each figure is
the median of `reps` calls, each on a fresh world, after one untimed warm-up call.  The algorithmic bytes stated next to the times are
the bit lattice's words (4 B each) plus 16 B per sample written (12 B for packed xyz)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from salva_amd import DFSPHSolver, Fluid, LiquidWorld, _lib  # noqa: E402
from salva_amd.coupling import make_shape  # noqa: E402

F = np.float32
R = 0.005
FP = C.POINTER(C.c_float)


def numpy_points(shape):
    """The lattice points inside the shape, vectorised (what a user without the sampler writes): same spacing and origin."""
    s = F(2 * R)
    if shape[0] == "cuboid":
        ext = np.asarray(shape[1], F)
    else:
        ext = np.full(3, shape[1], F)
    origin = (-ext - s) + s / F(2)
    n = np.ceil((2 * ext + 1.5 * s) / s).astype(int)
    ax = [origin[a] + np.arange(n[a], dtype=F) * s for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    if shape[0] == "cuboid":
        m = (np.abs(x) <= ext[0]) & (np.abs(y) <= ext[1]) & (np.abs(z) <= ext[2])
    else:
        m = x * x + y * y + z * z <= ext[0] * ext[0]
    return np.stack([x[m], y[m], z[m]], axis=1).astype(F)


def fresh():
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    f = w.add_fluid(Fluid(np.zeros((1, 3), F), R, 1000.0))
    w.sync_to_device()
    return w, f


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        ts.append(fn())
    return {"median_ms": float(np.median(ts)) * 1e3, "all_ms": [t * 1e3 for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sampling_bench.json")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    res = {"particle_radius": R, "reps": a.reps, "clock": "host clock around calls that end in a stream synchronise", "shapes": {}}
    t0, q0 = np.zeros(3, F), np.array([0, 0, 0, 1], F)
    for name, shape in (("cuboid_8m", ("cuboid", (0.9975, 0.9975, 0.9975))), ("ball_1m", ("ball", 0.62))):
        s = make_shape(shape)
        counts = {}

        def device_add():
            w, f = fresh()
            t = time.perf_counter()
            k = w._L.salva_hip_add_particles_sampled(w._h, 0, C.byref(s), t0.ctypes.data_as(FP), q0.ctypes.data_as(FP), 1, None)
            dt = time.perf_counter() - t
            assert k > 0, k
            counts["device"] = int(k)
            return dt

        def device_download():
            w, f = fresh()
            n = counts["device"]
            out = np.empty((n, 3), F)
            t = time.perf_counter()
            k = w._L.salva_hip_sample_shape(w._h, C.byref(s), R, 1, n, out.ctypes.data_as(FP))
            dt = time.perf_counter() - t
            assert k == n
            return dt

        def device_count_only():
            w, f = fresh()
            t = time.perf_counter()
            k = w._L.salva_hip_sample_shape(w._h, C.byref(s), R, 1, 0, None)
            dt = time.perf_counter() - t
            assert k == counts["device"]
            return dt

        def host_build_and_add():
            w, f = fresh()
            t = time.perf_counter()
            pts = numpy_points(shape)
            tb = time.perf_counter()
            _lib.check(w._L.salva_hip_add_particles(w._h, 0, len(pts), pts.ctypes.data_as(FP), None))
            te = time.perf_counter()
            counts["numpy"] = len(pts)
            counts.setdefault("numpy_build_s", []).append(tb - t)
            counts.setdefault("upload_add_s", []).append(te - tb)
            return te - t

        r = {"add_particles_sampled": timed(device_add, a.reps)}
        r["sample_shape_count_only"] = timed(device_count_only, a.reps)
        r["sample_shape_with_download"] = timed(device_download, a.reps)
        r["numpy_build_plus_add_particles"] = timed(host_build_and_add, a.reps)
        r["numpy_build_plus_add_particles"]["numpy_build_median_ms"] = float(np.median(counts["numpy_build_s"][1:])) * 1e3
        r["numpy_build_plus_add_particles"]["upload_add_median_ms"] = float(np.median(counts["upload_add_s"][1:])) * 1e3
        n = counts["device"]
        w, f = fresh()
        r["samples"], r["numpy_points"] = n, counts["numpy"]
        side = int(round((n if shape[0] == "cuboid" else 0) ** (1 / 3))) if shape[0] == "cuboid" else None
        r["cube_side"] = side
        res["shapes"][name] = r
        print(name, json.dumps(r))
    # lattice words: filled in from the line counts (N = ceil(2 ext / s + 1.5) per axis, rows padded to 32)
    for name, ext in (("cuboid_8m", 0.9975), ("ball_1m", 0.62)):
        N = int(np.ceil(2 * ext / (2 * R) + 1.5))
        words = N * N * ((N + 31) // 32)
        r = res["shapes"][name]
        r["lattice_lines_per_axis"], r["lattice_words"] = N, words
        r["algorithmic_bytes_float4"] = 4 * words + 16 * r["samples"]
        r["algorithmic_bytes_xyz"] = 4 * words + 12 * r["samples"]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
