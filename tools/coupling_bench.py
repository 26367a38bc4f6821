"""tools/coupling_bench.py — what the rigid-body coupling loop costs with K dynamically sampled colliders in 10^6 particles.

The bench scene of config 2 (bench.py: a 100^3 block in an open tank, XSPH, DFSPH) with K ball colliders of radius 4 h on a lattice
inside the fluid, K in {1, 16, 128}; the fluid particles that would start inside a ball are left out (`n` is reported).  Every ball
hangs on a dynamic body that is far too heavy to move, so that each step runs the full loop of a rapier user: poses in
(`update_boundaries`), the step, wrenches out (`transmit_forces`) — which ends in a stream wait; the host clock runs around 20 such
steps after 5 warm-up steps, three runs (fresh worlds) per K.

  python tools/coupling_bench.py --out profiles/dcs_batch_bench.json --label batched
  SALVA_HIP_NO_DCS_BATCH=1 python tools/coupling_bench.py --single --label per-collider ...

`--single` drives the loop through the single-collider entry points (salva_hip_update_boundary_pose / _get_boundary_wrench), which
is also what works on a library without the batched ones.  Results are appended to the JSON file under `label`.

`--shape compound` puts a five-part compound (an open box of five cuboid slabs) of the same extent in place of every
ball; `--host` registers it through the host arm instead, with the two callbacks in C++ (tools/compound_host_arm.hip, built on first
use): what such a collider cost before compounds had device code.

  python tools/coupling_bench.py --shape compound --out profiles/compound_bench.json --label device
  python tools/coupling_bench.py --shape compound --host --out profiles/compound_bench.json --label host-arm
  SALVA_HIP_NO_DCS_BATCH=1 python tools/coupling_bench.py --shape compound --out profiles/compound_bench.json --label device-unbatched
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, XSPHViscosity, _lib, sampling, scenes  # noqa: E402
from salva_amd.coupling import ColliderCouplingSet, DynamicContactSampling, HostShapeSampling, RigidBody  # noqa: E402

R = 0.025
H = 4 * R
DT = 1.0 / 200.0
GRAVITY = (0.0, -9.81, 0.0)
F = np.float32


class SingleCallSet(ColliderCouplingSet):
    """One pose call and one wrench call per collider."""

    def update_boundaries(self, world):
        if not all(e.uploaded for e in self.entries.values()):
            super().update_boundaries(world)
        for e in self.entries.values():
            _lib.check(world._L.salva_hip_update_boundary_pose(world._h, e.boundary._slot, C.byref(e.body.pose())))

    def transmit_forces(self, world, dt):
        fp = C.POINTER(C.c_float)
        for e in self.entries.values():
            b = e.boundary
            if not b.wants_forces or b.num_particles() == 0:
                continue
            com = e.body.center_of_mass()
            f, t = np.zeros(3, F), np.zeros(3, F)
            _lib.check(world._L.salva_hip_get_boundary_wrench(world._h, b._slot, com.ctypes.data_as(fp), f.ctypes.data_as(fp), t.ctypes.data_as(fp)))
            e.body.apply_impulse(f * F(dt))
            e.body.apply_torque_impulse(t * F(dt))


def box_parts(half):
    """An open box of five cuboid slabs with outer half width `half`: a floor and four walls."""
    wall, hh, q = 0.15 * half, 0.6 * half, (0.0, 0.0, 0.0, 1.0)
    return [(("cuboid", (half, wall, half)), (0.0, -hh, 0.0), q),
            (("cuboid", (wall, hh, half)), (-(half - wall), wall, 0.0), q), (("cuboid", (wall, hh, half)), (half - wall, wall, 0.0), q),
            (("cuboid", (half, hh, wall)), (0.0, wall, -(half - wall)), q), (("cuboid", (half, hh, wall)), (0.0, wall, half - wall), q)]


class CompoundHostArm(HostShapeSampling):
    """The host arm over the C++ callbacks of tools/compound_host_arm.hip (no Python in the step).  The C++ side keeps the pose it was
    created with, where the device arm takes the body's pose every step: the bodies of this bench are too heavy to move."""
    _plugin = None

    @classmethod
    def library(cls):
        if cls._plugin is None:
            here = os.path.dirname(os.path.abspath(__file__))
            so, src = os.path.join(here, "libcompound_host_arm.so"), os.path.join(here, "compound_host_arm.hip")
            if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
                subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                       "--offload-arch=gfx950", "-I" + _lib.CSRC, src, "-o", so, "-L" + _lib.CSRC, "-lsalva_hip", "-Wl,-rpath,$ORIGIN/../salva_amd/csrc"])
            cls._plugin = C.CDLL(so)
            cls._plugin.arm_create.restype = C.c_void_p
            cls._plugin.arm_create.argtypes = [C.POINTER(_lib.CompoundPart), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        return cls._plugin

    def __init__(self, parts, body):
        from salva_amd.coupling import make_shape

        lib = self.library()
        arr = (_lib.CompoundPart * len(parts))()
        for k, (shape, t, q) in enumerate(parts):
            s = make_shape(shape)
            arr[k].kind = s.kind
            arr[k].params[:] = list(s.params)
            arr[k].translation[:] = t
            arr[k].rotation_ijkw[:] = q
        self._error = None
        self._user = lib.arm_create(arr, len(parts), (C.c_float * 3)(*body.translation), (C.c_float * 4)(*body.rotation))
        self.shape = _lib.HostShape(C.cast(lib.arm_aabb, _lib.HOST_AABB_FN), C.cast(lib.arm_project, _lib.HOST_PROJECT_FN), self._user)


def ball_centres(k, lo, hi):
    m = int(np.ceil(k ** (1.0 / 3.0) - 1e-9))
    g = (np.arange(m) + 0.5) / m
    c = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:k]
    return (lo + c * (hi - lo)).astype(F)


def run(side, k, single, warmup, steps, shape="ball", host=False):
    fluid, shell = scenes.tank(side, side, side, R)
    fluid = scenes.jitter(fluid, 0.1 * R, seed=42)
    centres = ball_centres(k, fluid.min(axis=0), fluid.max(axis=0))
    radius = 4 * H
    keep = np.ones(len(fluid), bool)
    for c in centres:
        if shape == "ball":
            keep &= ((fluid - c) ** 2).sum(axis=1) > (radius + R) ** 2
        else:  # the box's own box, cavity included: the fluid runs into it
            keep &= (np.abs(fluid - c) > np.array([radius, 0.75 * radius, radius]) + R).any(axis=1)
    fluid = np.ascontiguousarray(fluid[keep])
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    f = Fluid(fluid, R, 1000.0)
    f.nonpressure_forces.append(XSPHViscosity(0.5, 0.0))
    w.add_fluid(f)
    w.add_boundary(Boundary(shell))
    coupling = SingleCallSet() if single else ColliderCouplingSet()
    for j, c in enumerate(centres):
        body = RigidBody(translation=c, mass=1e12, principal_inertia=F([1e12, 1e12, 1e12]))
        if shape == "ball":
            method = DynamicContactSampling(("ball", radius))
        elif host:
            method = CompoundHostArm(box_parts(radius), body)
        else:
            method = DynamicContactSampling(sampling.Compound(box_parts(radius)))
        coupling.register_coupling(w.add_boundary(Boundary(np.zeros((0, 3), F))), j, body, method)
    for _ in range(warmup):
        w.step_with_coupling(DT, GRAVITY, coupling)
    t0 = time.perf_counter()
    for _ in range(steps):
        w.step_with_coupling(DT, GRAVITY, coupling)  # (ends in transmit_forces: a stream wait)
    ms = (time.perf_counter() - t0) * 1e3 / steps
    out = {"ms_per_step": ms, "n": int(len(fluid)), "boundary_rows": int(sum(e.boundary.num_particles() for e in coupling.entries.values()))}
    if hasattr(w._L, "salva_hip_get_dcs_stats"):
        s = (C.c_uint64 * 4)()
        _lib.check(w._L.salva_hip_get_dcs_stats(w._h, s))
        out["dcs_passes"], out["dcs_waits"], out["dcs_batched"], out["dcs_records"] = (int(x) for x in s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--colliders", type=int, nargs="+", default=[1, 16, 128])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--single", action="store_true", help="the single-collider entry points, one call per collider")
    ap.add_argument("--shape", choices=["ball", "compound"], default="ball")
    ap.add_argument("--host", action="store_true", help="--shape compound through the host arm with C++ callbacks")
    ap.add_argument("--label", default="run")
    ap.add_argument("--out", default=os.path.join("profiles", "dcs_batch_bench.json"))
    a = ap.parse_args()
    res = {"side": a.side, "warmup": a.warmup, "steps": a.steps, "single_entry_points": a.single, "shape": a.shape, "host_arm": a.host,
           "no_dcs_batch": os.environ.get("SALVA_HIP_NO_DCS_BATCH") is not None, "by_colliders": {}}
    for k in a.colliders:
        runs = [run(a.side, k, a.single, a.warmup, a.steps, a.shape, a.host) for _ in range(a.runs)]
        res["by_colliders"][str(k)] = {"ms_per_step": [round(r["ms_per_step"], 4) for r in runs], **{x: runs[-1][x] for x in runs[-1] if x != "ms_per_step"}}
        print(a.label, "K", k, res["by_colliders"][str(k)], flush=True)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc[a.label] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
