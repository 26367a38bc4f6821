"""tools/device_force_bench.py — what a user-defined force costs on the device (SALVA_HIP_FORCE_DEVICE).

The bench scene of config 2 (bench.py: a jittered side^3 block in an open tank, DFSPH, dt = 1/200) with XSPH viscosity (0.5, 0) done
  builtin        by the built-in kernel, as bench.py runs it
  builtin_bare   by the built-in kernel with SALVA_HIP_NO_CHAIN=1 and speculation off, and (builtin_bare_all) with the deferred list
                 check and the pre-enqueued grid off as well: what a world with a user's force gives up, measured on the built-in force
  device         by df3_xsph of examples/libdevice_forces3.so as a device force over the contact tables
  host           by the same formula through the host arm (SALVA_HIP_FORCE_CUSTOM, vectorised numpy), at --host-side
For each arm: ms per step (median of the timed steps after the warm-up) and the device-force statistics of the last step; for the
device arm also the table build and df3_xsph on their own, from HIP events recorded on the world's stream by marker forces around
them, and, as a stand-in for one k_xsph pass, the difference builtin - (the same world without a force).  Writes one JSON document to
profiles/device_force_bench.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from salva_amd import Boundary, DeviceForce, DFSPHSolver, Fluid, LiquidWorld, NonPressureForce, PluginForce, XSPHViscosity, _lib, scenes  # noqa: E402

R = 0.025
DT = 1.0 / 200.0
GRAVITY = (0.0, -9.81, 0.0)
PLUGIN = os.path.join(ROOT, "examples", "libdevice_forces3.so")
ALL = _lib.DEVICE_NEEDS_FF | _lib.DEVICE_NEEDS_FB | _lib.DEVICE_NEEDS_KERNEL
BARE = {"SALVA_HIP_NO_CHAIN": "1", "SALVA_HIP_NO_SPECULATION": "1"}
BARE_ALL = dict(BARE, SALVA_HIP_NO_DEFER_LISTS="1", SALVA_HIP_NO_PREGRID="1")


class HostXSPH(NonPressureForce):
    """XSPHViscosity::solve over the exported contact lists, vectorised: the host arm's cost is the transfers, not this arithmetic"""

    def __init__(self, fc):
        self.fc = np.float32(fc)

    def solve(self, timestep, h, ff, fb, fluid, boundaries, densities):
        off, jm, j = ff.offsets.astype(np.int64), ff.j_model, ff.j.astype(np.int64)
        rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
        keep = jm[:len(rows)] == ff.i_model
        rows, j = rows[keep], j[:len(keep)][keep]
        d = fluid.positions[rows] - fluid.positions[j]
        q = np.sqrt((d * d).sum(1)) / np.float32(h)
        wgt = np.float32(8.0 / np.pi) / np.float32(h) ** 3 * np.where(q <= 0.5, 1 + 6 * (q ** 3 - q ** 2), 2 * np.clip(1 - q, 0, None) ** 3)
        s = self.fc * wgt * fluid.volumes[j] * np.float32(fluid.density0) / densities[j]
        dv = (fluid.velocities[j] - fluid.velocities[rows]) * s[:, None]
        for k in range(3):
            fluid.accelerations[:, k] += np.bincount(rows, weights=dv[:, k], minlength=len(off) - 1).astype(np.float32) * np.float32(timestep.inv_dt())


class HipEvents:
    """hipEvent pairs on the world's stream, through the HIP runtime the library itself is linked to"""

    def __init__(self, count):
        self.hip = C.CDLL("libamdhip64.so")
        self.ev = [C.c_void_p() for _ in range(count)]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def record(self, k, stream):
        assert self.hip.hipEventRecord(self.ev[k], C.c_void_p(stream)) == 0

    def ms(self, a, b):
        out = C.c_float(0)
        assert self.hip.hipEventSynchronize(self.ev[b]) == 0 and self.hip.hipEventElapsedTime(C.byref(out), self.ev[a], self.ev[b]) == 0
        return float(out.value)


class Marker(DeviceForce):
    def __init__(self, events, k, needs):
        super().__init__(needs)
        self.events, self.k = events, k

    def solve_device(self, view):
        self.events.record(self.k, view.stream)
        return 0


class TimedPlugin(PluginForce):
    def __init__(self, events, k, *a):
        super().__init__(*a)
        self.events, self.k = events, k

    def solve_device(self, view):
        rc = super().solve_device(view)
        self.events.record(self.k, view.stream)
        return rc


def make_world(side, forces, env):
    old = {k: os.environ.pop(k, None) for k in BARE_ALL}
    os.environ.update(env)
    try:
        w = LiquidWorld(DFSPHSolver(), R, 2.0)  # (a world reads its switches when it is created)
    finally:
        for k in BARE_ALL:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    fluid, shell = scenes.tank(side, side, side, R)
    f = Fluid(scenes.jitter(fluid, 0.1 * R, seed=42), R, 1000.0)
    f.nonpressure_forces += forces
    w.add_fluid(f)
    w.add_boundary(Boundary(shell))
    return w, f


def run(side, forces, env, warmup, steps, events=None):
    w, f = make_world(side, forces, env)
    for _ in range(warmup):
        w.step(DT, GRAVITY)
    times, build, xsph = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        st = w.step(DT, GRAVITY)
        times.append((time.perf_counter() - t0) * 1e3)
        if events:
            build.append(events.ms(0, 1))
            xsph.append(events.ms(1, 2))
    c = w.counters
    out = {"n": f.num_particles(), "ms_per_step": statistics.median(times), "ms_min": min(times), "iters": [st.n_divergence_iters, st.n_pressure_iters],
           "contacts_per_particle": float(st.reserved[3]), "device_force_stats": list(w.device_force_stats()),
           "chained_passes": int(c.chained_passes), "pregrid_adopted": int(c.pregrid_adopted)}
    if events:
        out["table_build_ms"], out["df3_xsph_ms"] = statistics.median(build), statistics.median(xsph)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--host-side", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_force_bench.json"))
    a = ap.parse_args()
    res = {"bench": "device_force", "side": a.side, "host_side": a.host_side, "warmup": a.warmup, "steps": a.steps, "arms": {}}
    arms = res["arms"]
    arms["no_force"] = run(a.side, [], {}, a.warmup, a.steps)
    arms["builtin"] = run(a.side, [XSPHViscosity(0.5, 0.0)], {}, a.warmup, a.steps)
    arms["builtin_bare"] = run(a.side, [XSPHViscosity(0.5, 0.0)], BARE, a.warmup, a.steps)
    arms["builtin_bare_all"] = run(a.side, [XSPHViscosity(0.5, 0.0)], BARE_ALL, a.warmup, a.steps)
    arms["device"] = run(a.side, [PluginForce(PLUGIN, "df3_xsph", ALL, [0.5, 0.0])], {}, a.warmup, a.steps)
    ev = HipEvents(3)
    arms["device_timed"] = run(a.side, [Marker(ev, 0, 0), Marker(ev, 1, ALL), TimedPlugin(ev, 2, PLUGIN, "df3_xsph", ALL, [0.5, 0.0])], {}, a.warmup, a.steps, ev)
    arms["host_small"] = run(a.host_side, [HostXSPH(0.5)], {}, 2, max(a.steps // 4, 3))
    arms["device_small"] = run(a.host_side, [PluginForce(PLUGIN, "df3_xsph", ALL, [0.5, 0.0])], {}, 2, max(a.steps // 4, 3))
    arms["builtin_small"] = run(a.host_side, [XSPHViscosity(0.5, 0.0)], {}, 2, max(a.steps // 4, 3))
    res["builtin_minus_no_force_ms"] = arms["builtin"]["ms_per_step"] - arms["no_force"]["ms_per_step"]
    res["device_vs_builtin_bare"] = arms["device"]["ms_per_step"] / arms["builtin_bare"]["ms_per_step"]
    res["bare_vs_builtin"] = arms["builtin_bare"]["ms_per_step"] / arms["builtin"]["ms_per_step"]
    n, st = arms["device"]["n"], arms["device"]["device_force_stats"]
    res["table_bytes_per_particle"] = st[2] / n
    text = json.dumps(res, indent=1)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
