#!/usr/bin/env python
"""Set-up time of ray-sampling a compound (DESIGN.md §17 "Ray sampling"): salva_hip_sample_compound against salva_hip_sample_host_shape
with the two callbacks in C++ running the same `__host__ __device__` casts on the host (tools/compound_ray_arm.hip, built on first
use) — what a binding did for a parry `Compound` before the device path.  The scene is the open box of five slabs of
examples/compound3.cpp at the bench radius r = 0.025, outer half width 4 h (tools/coupling_bench.py box_parts), sampled on the
surface and in the volume.  One session, the host clock around whole calls (count call + fill call, as every mirror makes them);
the two arms must give the same points.

  python tools/compound_sampling_bench.py --out profiles/compound_sampling_bench.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from coupling_bench import H, R, box_parts  # noqa: E402
from salva_amd import DFSPHSolver, LiquidWorld, _lib, sampling  # noqa: E402

F = np.float32
FP = C.POINTER(C.c_float)


def ray_arm():
    so, src = os.path.join(HERE, "libcompound_ray_arm.so"), os.path.join(HERE, "compound_ray_arm.hip")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "--offload-arch=gfx950", "-I" + _lib.CSRC, src, "-o", so, "-L" + _lib.CSRC, "-lsalva_hip", "-Wl,-rpath,$ORIGIN/../salva_amd/csrc"])
    lib = C.CDLL(so)
    lib.ray_arm_create.restype = C.c_void_p
    lib.ray_arm_create.argtypes = [C.POINTER(_lib.CompoundPart), C.c_uint32]
    lib.ray_arm_destroy.argtypes = [C.c_void_p]
    return lib


def sample_twice(call):
    """The count call and the fill call -> (points, seconds)."""
    t0 = time.perf_counter()
    n = call(0, None)
    if n < 0:
        _lib.check(int(n))
    pts = np.zeros((n, 3), F)
    m = call(n, pts.ctypes.data_as(FP))
    t1 = time.perf_counter()
    assert m == n
    return pts, t1 - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    parts = box_parts(4 * H)
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    comp = sampling.Compound(parts)
    h = comp.handle(w)
    arr = (_lib.CompoundPart * len(parts))()
    for k, (s, t, q) in enumerate(comp.parts):
        arr[k].kind = s.kind
        arr[k].params[:] = list(s.params)
        arr[k].translation[:] = [float(x) for x in t]
        arr[k].rotation_ijkw[:] = [float(x) for x in q]
    lib = ray_arm()
    user = lib.ray_arm_create(arr, len(parts))
    shape = _lib.HostRayShape(user, C.cast(lib.ray_arm_aabb, _lib.HOST_AABB_FN), C.cast(lib.ray_arm_cast, _lib.HOST_CAST_FN))
    result = {"scene": "open box of five slabs, outer half width 4 h", "particle_radius": R, "repeats": a.repeats, "clock": "host, count call + fill call"}
    for mode, name in ((_lib.SAMPLE_SURFACE, "surface"), (_lib.SAMPLE_VOLUME, "volume")):
        def device(cap, out, mode=mode):
            return w._L.salva_hip_sample_compound(w._h, h, R, mode, cap, out)

        def host(cap, out, mode=mode):
            return w._L.salva_hip_sample_host_shape(w._h, C.byref(shape), R, mode, cap, out)

        times = {"device": [], "host_arm": []}
        for rep in range(a.repeats + 2):  # (two warm-up rounds: buffers grow, code objects load)
            pd, td = sample_twice(device)
            ph, th = sample_twice(host)
            assert len(pd) == len(ph) and np.array_equal(pd.view(np.uint32), ph.view(np.uint32)), "the two arms disagree"
            if rep >= 2:
                times["device"].append(td)
                times["host_arm"].append(th)
        result[name] = {"points": int(len(pd)),
                        "device_ms": {"median": round(1e3 * float(np.median(times["device"])), 4), "min": round(1e3 * min(times["device"]), 4)},
                        "host_arm_ms": {"median": round(1e3 * float(np.median(times["host_arm"])), 4), "min": round(1e3 * min(times["host_arm"]), 4)}}
    lib.ray_arm_destroy(user)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
