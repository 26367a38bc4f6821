"""Every built-in NonPressureForce kernel by itself: k_xsph, k_artificial_viscosity, k_akinci_* (and the _one_fluid variants),
k_he2014_*, k_wcsph_tension (salva_amd/csrc/forces.hip) and the k_visc_* family (visc.hip).

World::run_forces runs a fluid's forces in list order, and a SALVA_HIP_FORCE_DEVICE entry is called at its place in the list with
the accumulated accelerations in its view.  A reader in front of a built-in force and one behind it therefore give that force's own
accelerations (acc behind - acc in front) and its own boundary reactions (the difference of bforce_fx), and the second reader's
view holds the inputs the kernel saw.  tests/force_reading.py evaluates the same force from those inputs in float64; the scenes
and the case matrix are tests/force_cases.py, the bounds come from tests/test_force_reading_cpu.py, which checks this harness
against the CPU oracle without a GPU.

The other GPU tests see these kernels only through positions and velocities after the pressure solve, at 1e-4 * vref per step:
3 to 60 mm/s^2 of acceleration error per step pass there, against forces of 3 to 60 m/s^2."""

import numpy as np
import pytest

import force_cases as FC
from force_reading import Reading, Snapshot
from test_force_reading_cpu import F32_FLOOR, REACTIONS
from salva_amd import (Akinci2013SurfaceTension, ArtificialViscosity, Boundary, DeviceForce, DFSPHSolver, DFSPHViscosity, Fluid,
                       He2014SurfaceTension, LiquidWorld, WCSPHSurfaceTension, XSPHViscosity, _lib)
from parity import KERNELS

pytestmark = pytest.mark.gpu


class Probe(DeviceForce):
    """copies the view to the host inside the callback"""

    def __init__(self, world, needs):
        super().__init__(needs)
        self.world, self.snaps = world, []

    def solve_device(self, v):
        rd, n, nb = self.world.device_view_read, int(v.n), int(v.nb)
        s = dict(n=n, nb=nb, dt=float(v.dt), inv_dt=float(v.inv_dt), h=float(v.h), scale=float(v.bforce_scale), needs=int(v.needs))
        for name, dtype, width in (("posm", np.float32, 4), ("vel", np.float32, 4), ("acc", np.float32, 4)):
            s[name] = rd(getattr(v, name), dtype, width * n).reshape(-1, width)
        s["rho"], s["model"], s["id"] = rd(v.rho, np.float32, n), rd(v.model, np.uint32, n), rd(v.id, np.uint32, n)
        s["rho0"] = rd(v.rho0, np.float32, int(v.nfluids))
        s["bposv"], s["bvel"] = rd(v.bposv, np.float32, 4 * nb).reshape(-1, 4), rd(v.bvel, np.float32, 4 * nb).reshape(-1, 4)
        s["bid"] = rd(v.bid, np.uint32, nb)
        # k_bforce_fold (world_step.hip) decodes the unsigned 64-bit sums as two's complement: (double)(long long)f * (1 / scale)
        s["bfx"] = rd(v.bforce_fx, np.uint64, 3 * nb).view(np.int64).reshape(-1, 3) if v.bforce_fx else None
        for k in ("ff", "fb"):
            s[k + "_off"] = rd(getattr(v, k + "_off"), np.uint64, n + 1) if getattr(v, k + "_off") else None
        self.snaps.append(s)
        return 0


def _mirror_force(d):
    if d[0] == "xsph":
        return XSPHViscosity(d[1], d[2])
    if d[0] == "artificial":
        f = ArtificialViscosity(d[1], d[2])
        f.alpha, f.beta, f.speed_of_sound = d[3], d[4], d[5]
        return f
    if d[0] == "akinci2013":
        return Akinci2013SurfaceTension(d[1], d[2])
    if d[0] == "he2014":
        return He2014SurfaceTension(d[1], d[2])
    if d[0] == "wcsph":
        return WCSPHSurfaceTension(d[1], 0.0)
    assert d[0] == "dfsph_viscosity"
    f = DFSPHViscosity(d[1])
    f.min_viscosity_iter, f.max_viscosity_iter, f.max_viscosity_error = int(d[2]), int(d[3]), d[4]
    return f


def run_device(case):
    """The scene through the Python mirror, a Probe in front of and behind every built-in force of the target fluid (the first one
    asks for nothing, the others for both contact tables), every boundary with wants_forces.  Returns the probes' snapshots per step
    and, per step, the iteration count of each DFSPHViscosity."""
    sc = FC.SCENES[case.scene]()
    w = LiquidWorld(DFSPHSolver(KERNELS[case.kernels[0]][1], KERNELS[case.kernels[1]][1]), FC.R, 2.0)
    probes, forces = [], []
    for g, fl in enumerate(sc["fluids"]):
        f = Fluid(fl["pos"], FC.R, fl["density0"])
        f.velocities = fl["vel"]
        if fl["vol"] is not None:
            f.volumes = fl["vol"]
        if g == case.target:
            probes.append(Probe(w, 0))
            f.nonpressure_forces.append(probes[-1])
            for d in case.forces:
                forces.append(_mirror_force(d))
                probes.append(Probe(w, _lib.DEVICE_NEEDS_FF | _lib.DEVICE_NEEDS_FB))
                f.nonpressure_forces += [forces[-1], probes[-1]]
        w.add_fluid(f)
    if sc["floor"] is not None:
        b = Boundary(sc["floor"][0], wants_forces=True)
        b.velocities = sc["floor"][1]
        w.add_boundary(b)
    iters = []
    for _ in range(FC.NSTEPS):
        w.step(FC.DT, FC.GRAVITY)
        iters.append([getattr(f, "num_iterations", None) for f in forces])
    assert all(len(p.snaps) == FC.NSTEPS for p in probes)
    return [[p.snaps[step] for p in probes] for step in range(FC.NSTEPS)], iters


def _snapshot(case, before, after):
    """what the kernel saw: the state in the view behind the force, the accelerations in the view in front of it"""
    return Snapshot(after["posm"][:, :3], after["vel"][:, :3], after["posm"][:, 3], after["rho"], after["model"], after["rho0"],
                    before["acc"][:, :3], after["bposv"][:, :3], after["bvel"][:, :3], after["bposv"][:, 3],
                    np.ascontiguousarray(after["bvel"][:, 3]).view(np.uint32), after["h"], case.kernels, after["dt"], after["inv_dt"])


@pytest.mark.parametrize("case_id", [c.id for c in FC.CASES])
def test_force_by_itself(case_id):
    """Per case, at steps 2 and 3: the force's own accelerations against the float64 reading of the same inputs within
    max(1e-5, 4 x the case's CPU f32 floor) of the field's largest magnitude (1e-5: the project's bound for neighbour sums; the 4
    allows for the device's order of summation and its approximate divisions); other fluids' accelerations bit-identical; the
    boundary reactions of XSPH, Akinci and He2014 within the same relative bound plus one fixed-point quantum per contributing
    contact, ArtificialViscosity's non-zero exactly where a fluid contact approaches (golden_scenes.py:30-33: its values depend on
    the contact order), nothing from the others; the contact tables' row lengths against the reading's contact masks.  At step 1
    XSPH and DFSPHViscosity add exactly nothing.  DFSPHViscosity runs its fixed number of iterations."""
    case = FC.BY_ID[case_id]
    steps, iters = run_device(case)
    bound = max(1e-5, 4 * F32_FLOOR[case_id])
    for step in range(FC.NSTEPS):
        for k, d in enumerate(case.forces):
            before, after = steps[step][k], steps[step][k + 1]
            assert np.array_equal(before["id"], after["id"]) and np.array_equal(np.sort(after["id"]), np.arange(after["n"]))
            own = after["model"] == case.target
            assert own.sum() == len(FC.SCENES[case.scene]()["fluids"][case.target]["pos"])
            a0, a1 = before["acc"][:, :3], after["acc"][:, :3]
            assert np.array_equal(a0[~own].view(np.uint32), a1[~own].view(np.uint32)), "a fluid's force touched another fluid's particles"
            if d[0] == "dfsph_viscosity":
                assert iters[step][k] == int(d[2]) == int(d[3]), iters
            if step == 0:
                if d[0] in ("xsph", "dfsph_viscosity"):
                    assert before["inv_dt"] == 0.0 and np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), "step 1: inv_dt = 0"
                continue
            if case.scene == "A2":  # r = 0: zero gradient, zero unit vector
                twins = after["posm"][np.argsort(after["id"])[[(4 * 9 + 4) * 9 + 4, after["n"] - 1]], :3].astype(np.float64)
                print("%s step %d: the coincident pair is %.1e apart" % (case_id, step + 1, np.sqrt(((twins[0] - twins[1]) ** 2).sum())))
                assert np.sqrt(((twins[0] - twins[1]) ** 2).sum()) <= float(np.finfo(np.float32).eps)
            rd = Reading(_snapshot(case, before, after))
            # the lists the kernel walked are the reading's contact masks: a difference below is the force's, not the lists'
            assert np.array_equal(np.diff(after["ff_off"].astype(np.int64)), rd.ff_counts()), "fluid contact lists"
            assert np.array_equal(np.diff(after["fb_off"].astype(np.int64)), rd.fb_counts()), "boundary contact lists"
            ref, ref_reaction = rd.force(case.target, d)
            got = a1.astype(np.float64) - a0.astype(np.float64)
            top = np.abs(ref).max()
            dev = np.abs(got - ref).max(axis=1)
            worst = int(np.argmax(dev))
            err = dev[worst] / top
            print("%s step %d %s: max |a| = %.4g, device - reading = %.2e of it (bound %.1e; CPU f32 floor %.2e), at particle %d of the "
                  "host order" % (case_id, step + 1, d[0], top, err, bound, F32_FLOOR[case_id], after["id"][worst]))
            assert top > 0 and err <= bound
            if after["bfx"] is None:
                assert after["nb"] == 0
                continue
            # rows of bforce_fx are in host order, bid maps a sorted boundary particle to its row
            fx = (after["bfx"] - before["bfx"])[after["bid"]]
            reaction = fx.astype(np.float64) / after["scale"]
            touching = rd.full[3] & own[:, None]
            if d[0] in REACTIONS and d[2] != 0.0:
                rtop = np.abs(ref_reaction).max()
                quanta = touching.sum(axis=0)[:, None] / after["scale"]
                excess = np.abs(reaction - ref_reaction) - quanta
                print("    reaction: max |f| = %.4g, device - reading = %.2e of it, %d particles" % (
                    rtop, np.abs(reaction - ref_reaction).max() / rtop, int(fx.any(axis=1).sum())))
                assert rtop > 0 and (excess <= bound * rtop).all()
            elif d[0] == "artificial" and d[2] != 0.0:
                approaching = (rd.approaching(case.target)[1][0]).any(axis=0)
                print("    reaction on %d boundary particles, an approaching contact on %d" % (int(fx.any(axis=1).sum()), int(approaching.sum())))
                assert approaching.sum() >= 30 and np.array_equal(fx.any(axis=1), approaching)
            else:
                assert not fx.any(), "a force without a boundary arm left a reaction"
