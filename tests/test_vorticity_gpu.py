"""Vorticity confinement on the device (salva_amd/csrc/vorticity.hip) against tests/vorticity_reading.py, the numpy
reading of the header's contract, inside the bounds that reading derives per row.

The force by itself is seen with the Probe pattern of tests/test_forces_isolated_gpu.py: a DeviceForce reader in front of the entry and
one behind it give the force's own accelerations and the state the kernels saw.  The scenes are the 730- and 810-particle scenes of
tests/force_cases.py: the smallest with more than one tile per axis, partly filled outer tiles, a stray particle, a coincident pair
and a two-fluid interface."""
import os
import re
import subprocess

import numpy as np
import pytest

import force_cases as FC
import test_dist_gpu as TD
import vorticity_reading as VR
from force_reading import Reading
from parity import KERNELS
from salva_amd import Boundary, DFSPHSolver, Fluid, IISPHSolver, LiquidWorld, VorticityConfinement, XSPHViscosity, _lib, scenes
from test_forces_isolated_gpu import Probe, _snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, KAPPA = 0.1, 0.05
BOTH = _lib.DEVICE_NEEDS_FF | _lib.DEVICE_NEEDS_FB


def _world(scene, kernels, solver, entries):
    """the scene through the Python mirror; entries[g] = the force list of fluid g as a function of the world"""
    sc = FC.SCENES[scene]()
    make = IISPHSolver if solver == "iisph" else DFSPHSolver
    w = LiquidWorld(make(KERNELS[kernels[0]][1], KERNELS[kernels[1]][1]), FC.R, 2.0)
    fluids = []
    for g, fl in enumerate(sc["fluids"]):
        f = Fluid(fl["pos"], FC.R, fl["density0"])
        f.velocities = fl["vel"]
        if fl["vol"] is not None:
            f.volumes = fl["vol"]
        f.nonpressure_forces += entries.get(g, lambda w: [])(w)
        w.add_fluid(f)
        fluids.append(f)
    if sc["floor"] is not None:
        b = Boundary(sc["floor"][0], wants_forces=True)
        b.velocities = sc["floor"][1]
        w.add_boundary(b)
    return w, fluids


def _sorted_field(field, snap, offset, own):
    """the fluid's host-order field in the order of the probe's rows (zero on the other fluids' rows)"""
    out = np.zeros((snap["n"], 3))
    out[own] = field[snap["id"][own] - offset]
    return out


def _worst(dev, bound):
    assert (dev[bound == 0] == 0).all()
    return float((dev[bound > 0] / bound[bound > 0]).max())


CASES = {
    "A": ("A", 0, ("cubic", "cubic"), "dfsph"),
    "A2": ("A2", 0, ("cubic", "cubic"), "dfsph"),
    "B0": ("B", 0, ("cubic", "cubic"), "dfsph"),
    "B1": ("B", 1, ("cubic", "cubic"), "dfsph"),
    "B0p": ("B", 0, ("poly6", "spiky"), "dfsph"),
    "B1p": ("B", 1, ("poly6", "spiky"), "dfsph"),
    "A-iisph": ("A", 0, ("cubic", "cubic"), "iisph"),
}


def _probed_run(scene, target, kernels, solver, strength, kappa=KAPPA):
    """per step: (snapshot in front, snapshot behind, the field in host order)"""
    probes = []

    def entries(w):
        probes.extend([Probe(w, 0), Probe(w, BOTH)])
        return [probes[0], VorticityConfinement(strength, kappa), probes[1]]

    w, fluids = _world(scene, kernels, solver, {target: entries})
    fields = []
    for _ in range(FC.NSTEPS):
        w.step(FC.DT, FC.GRAVITY)
        fields.append(w.vorticity(fluids[target]))
    assert all(len(p.snaps) == FC.NSTEPS for p in probes)
    offset = sum(f.num_particles() for f in fluids[:target])
    return [(probes[0].snaps[k], probes[1].snaps[k], fields[k]) for k in range(FC.NSTEPS)], offset


@pytest.mark.parametrize("case_id", list(CASES))
def test_the_force_by_itself(case_id):
    """At steps 2 and 3, row by row: acc behind - acc in front against the f64 reading of the snapshot behind inside its bound on the
    acceleration; the field against the reading's omega inside its bound; the acceleration again against the reading fed the device's
    own omega, whose bound then holds pass 2 and the force alone.  The other fluid's accelerations and every bforce_fx are bit-identical
    front to back; the lists the kernels walked are the reading's contact masks."""
    scene, target, kernels, solver = CASES[case_id]
    case = FC.Case(case_id, scene, kernels, target, ())
    steps, offset = _probed_run(scene, target, kernels, solver, EPS)
    for step in FC.COMPARED:
        before, after, field = steps[step]
        assert np.array_equal(before["id"], after["id"]) and np.array_equal(np.sort(after["id"]), np.arange(after["n"]))
        own = after["model"] == target
        assert own.sum() == len(field) == len(FC.SCENES[scene]()["fluids"][target]["pos"])
        a0, a1 = before["acc"][:, :3], after["acc"][:, :3]
        assert np.array_equal(a0[~own].view(np.uint32), a1[~own].view(np.uint32)), "the force touched another fluid's particles"
        assert after["bfx"] is not None and np.array_equal(before["bfx"], after["bfx"]), "a force without a boundary arm left a reaction"
        if scene == "A2":  # r = 0: zero gradient
            twins = after["posm"][np.argsort(after["id"])[[(4 * 9 + 4) * 9 + 4, after["n"] - 1]], :3].astype(np.float64)
            assert np.sqrt(((twins[0] - twins[1]) ** 2).sum()) <= float(np.finfo(np.float32).eps)
        snap = _snapshot(case, before, after)
        assert np.array_equal(np.diff(after["ff_off"].astype(np.int64)), Reading(snap).ff_counts()), "fluid contact lists"
        rd = VR.read(snap, target, EPS, KAPPA)
        got = a1.astype(np.float64) - a0.astype(np.float64)
        omega = _sorted_field(field, after, offset, own)
        fed = VR.read(snap, target, EPS, KAPPA, omega=omega)
        f_acc = _worst(np.abs(got - rd.acc).max(axis=1), rd.b_acc)
        f_om = _worst(np.abs(omega - rd.omega).max(axis=1), rd.b_omega)
        f_fed = _worst(np.abs(got - fed.acc).max(axis=1), fed.b_acc)
        top = np.abs(rd.acc).max()
        print("%s step %d: max |omega| %.3g, max |a| %.3g; device - reading as a fraction of the row's bound: omega %.3f, a %.3f, a from the "
              "device's own omega %.3f (median bounds on a: %.1e and %.1e of max |a|)" % (
                  case_id, step + 1, rd.n.max(), top, f_om, f_acc, f_fed, np.median(rd.b_acc[own]) / top, np.median(fed.b_acc[own]) / top))
        assert top > 0 and f_om <= 1.0 and f_acc <= 1.0 and f_fed <= 1.0
        # the stray particle, alone in its tile: nothing
        stray = after["id"] == (len(field) - (2 if scene == "A2" else 1)) + offset
        if scene in ("A", "A2"):
            assert stray.sum() == 1 and not got[stray].any() and not omega[stray].any()


def test_zero_strength_reads_the_vorticity_and_adds_nothing():
    """eps = 0: pass 1 only.  Accelerations bit-identical front to back, the field still the reading's omega."""
    case = FC.Case("A-eps0", "A", ("cubic", "cubic"), 0, ())
    steps, offset = _probed_run("A", 0, ("cubic", "cubic"), "dfsph", 0.0)
    for step in range(FC.NSTEPS):
        before, after, field = steps[step]
        assert np.array_equal(before["acc"].view(np.uint32), after["acc"].view(np.uint32))
        assert np.array_equal(before["bfx"], after["bfx"])
        if step not in FC.COMPARED:
            continue
        own = after["model"] == 0
        rd = VR.read(_snapshot(case, before, after), 0, 0.0, KAPPA)
        f_om = _worst(np.abs(_sorted_field(field, after, offset, own) - rd.omega).max(axis=1), rd.b_omega)
        print("eps = 0, step %d: max |omega| %.3g, device - reading = %.3f of the bound" % (step + 1, rd.n.max(), f_om))
        assert rd.n.max() > 1 and not rd.acc.any() and f_om <= 1.0


def test_a_world_without_the_entry_is_untouched():
    """A twin that never had the entry, a world whose eps = 0 entry is removed after two steps and a world whose entry was uploaded
    (a step of dt = 0 runs no substep) and removed again step to the same bits."""
    def make(extra):
        w, fluids = _world("A", ("cubic", "cubic"), "dfsph", {0: lambda w: [XSPHViscosity(0.5, 0.3)] + extra})
        return w, fluids[0]

    worlds = [make([]), make([VorticityConfinement(0.0)]), make([VorticityConfinement(EPS)])]
    for w, _ in worlds:
        w.step(0.0, FC.GRAVITY)
    worlds[2][1].nonpressure_forces.pop()
    for step in range(4):
        if step == 2:
            worlds[1][1].nonpressure_forces.pop()
        for w, _ in worlds:
            w.step(FC.DT, FC.GRAVITY)
        for _, f in worlds[1:]:
            assert np.array_equal(f.positions.view(np.uint32), worlds[0][1].positions.view(np.uint32)), step
            assert np.array_equal(f.velocities.view(np.uint32), worlds[0][1].velocities.view(np.uint32)), step
    for w, f in worlds:  # (and the entry is gone: the field says so)
        with pytest.raises(_lib.SalvaHipError, match="no VorticityConfinement entry"):
            w.vorticity(f)


def test_two_fluids_that_both_carry_the_force():
    """scene B, an entry on either fluid (different strengths): each field is its own fluid's"""
    probes = []

    def last(w):
        probes.append(Probe(w, BOTH))
        return [VorticityConfinement(2 * EPS, 0.0), probes[0]]

    w, fluids = _world("B", ("cubic", "cubic"), "dfsph", {0: lambda w: [VorticityConfinement(EPS)], 1: last})
    case = FC.Case("B-both", "B", ("cubic", "cubic"), 1, ())
    for _ in range(2):
        w.step(FC.DT, FC.GRAVITY)
    s = probes[0].snaps[-1]
    snap = _snapshot(case, s, s)
    offset = 0
    for g, f in enumerate(fluids):
        own = s["model"] == g
        rd = VR.read(snap, g, EPS, KAPPA)
        field = w.vorticity(f)
        frac = _worst(np.abs(_sorted_field(field, s, offset, own) - rd.omega).max(axis=1), rd.b_omega)
        print("fluid %d: max |omega| %.3g, device - reading = %.3f of the bound" % (g, rd.n.max(), frac))
        assert len(field) == own.sum() == 405 and rd.n.max() > 1 and frac <= 1.0
        offset += f.num_particles()


def test_slabs_match_single_domain(hip_lib):
    """Two loopback slabs against the undivided world for 8 steps, two fluids: omega of the outer ghost plane is refreshed between
    the passes.  The bounds are tests/test_dist_gpu.py's for forces with a dependent pass."""
    TD.FORCES["make"] = lambda: [VorticityConfinement(0.05)]
    try:
        pos, vel, bpos = TD.make_scene()
        nsteps = 8
        ref_p, ref_v, _ = TD.run_single(pos, vel, bpos, nsteps, True)
        got_p, got_v, _, seen, _, _ = TD.run_slabs(pos, vel, bpos, nsteps, 2, True)
        TD.FORCES["make"] = lambda: []
        bare_p, bare_v, _ = TD.run_single(pos, vel, bpos, nsteps, True)
    finally:
        TD.FORCES["make"] = lambda: [XSPHViscosity(0.5, 0.0)]
    assert (seen == 1).all() and np.isfinite(got_p).all()
    dp, dv = np.abs(got_p - ref_p).max(), np.abs(got_v - ref_v).max()
    print("slabs - single domain: %.2e h, %.2e m/s; the force itself moved the velocities by %.2e m/s" % (dp / TD.H, dv, np.abs(ref_v - bare_v).max()))
    assert dp < 2e-4 * TD.H and dv < 5e-3
    assert np.abs(ref_v - bare_v).max() > 5e-3  # (the run would pass without the force otherwise)


def _desc(kind, *p):
    d = _lib.ForceDesc()
    d.kind = kind
    for k, v in enumerate(p):
        d.p[k] = v
    return d


K = _lib.FORCE_VORTICITY_CONFINEMENT
REFUSED = {
    "strength nan": [_desc(K, np.nan, KAPPA)], "strength inf": [_desc(K, np.inf, KAPPA)], "strength negative": [_desc(K, -0.1, KAPPA)],
    "kappa nan": [_desc(K, EPS, np.nan)], "kappa inf": [_desc(K, EPS, np.inf)], "kappa negative": [_desc(K, EPS, -0.05)],
    "p2": [_desc(K, EPS, KAPPA, 1.0)], "p3": [_desc(K, EPS, KAPPA, 0.0, 1.0)], "p4": [_desc(K, EPS, KAPPA, 0.0, 0.0, -1.0)],
    "p5": [_desc(K, EPS, KAPPA, 0.0, 0.0, 0.0, 1e-30)], "p6": [_desc(K, EPS, KAPPA, 0.0, 0.0, 0.0, 0.0, np.nan)],
    "two entries": [_desc(K, EPS, KAPPA), _desc(_lib.FORCE_XSPH, 0.5, 0.0), _desc(K, 0.0, KAPPA)],
}


def test_refusals_leave_the_list_in_place_and_the_world_steppable():
    """every refusal of salva_hip_set_fluid_forces for this kind: E_INVALID, the previous list stays (its field is still there after
    the next step, and the step is the one a twin that was never asked takes); then the field's two errors"""
    w, (f,) = _world("A", ("cubic", "cubic"), "dfsph", {0: lambda w: [VorticityConfinement(EPS)]})
    twin, (ft,) = _world("A", ("cubic", "cubic"), "dfsph", {0: lambda w: [VorticityConfinement(EPS)]})
    w.step(FC.DT, FC.GRAVITY); twin.step(FC.DT, FC.GRAVITY)
    for name, descs in REFUSED.items():
        arr = (_lib.ForceDesc * len(descs))(*descs)
        rc = w._L.salva_hip_set_fluid_forces(w._h, f._slot, arr, len(descs))
        assert rc == _lib.E_INVALID, name
        assert "VorticityConfinement" in w._L.salva_hip_last_error().decode(), name
        w.step(FC.DT, FC.GRAVITY); twin.step(FC.DT, FC.GRAVITY)
        assert np.array_equal(f.positions.view(np.uint32), ft.positions.view(np.uint32)), name
        assert np.array_equal(w.vorticity(f).view(np.uint32), twin.vorticity(ft).view(np.uint32)), name
    assert np.abs(w.vorticity(f)).max() > 1
    # a kind beyond the last one is still unknown
    assert w._L.salva_hip_set_fluid_forces(w._h, f._slot, (_lib.ForceDesc * 1)(_desc(K + 1, 0.0)), 1) == _lib.E_INVALID
    # not right after a step: the same list set again — what the buffer holds is no longer this list's
    ok = (_lib.ForceDesc * 1)(_desc(K, EPS, KAPPA))
    assert w._L.salva_hip_set_fluid_forces(w._h, f._slot, ok, 1) == _lib.OK
    with pytest.raises(_lib.SalvaHipError, match="only available right after a step") as e:
        w.vorticity(f)
    assert e.value.code == _lib.E_INVALID
    w.step(FC.DT, FC.GRAVITY)
    assert np.abs(w.vorticity(f)).max() > 1
    # no entry
    f.nonpressure_forces.clear()
    w.step(FC.DT, FC.GRAVITY)
    with pytest.raises(_lib.SalvaHipError, match="no VorticityConfinement entry") as e:
        w.vorticity(f)
    assert e.value.code == _lib.E_INVALID
    assert len(w.densities(f)) == f.num_particles()  # (the other scratch fields are there)


# ---------------------------------------------------------------------------------------------------- the example's scene
def vorticity3(nsteps=50, strength=0.1, n=12):
    """What examples/vorticity3.cpp computes, through the Python mirror: the enstrophy sum m |omega|^2 of the last step"""
    pos = scenes.cube_fluid_positions(n, n, n, FC.R)
    f = Fluid(pos, FC.R, 1000.0)
    f.velocities = VR.lamb_oseen(pos, (0.0, 0.0), 0.5, 0.1).astype(np.float32)
    f.nonpressure_forces += [XSPHViscosity(0.5, 0.0), VorticityConfinement(strength)]
    w = LiquidWorld(DFSPHSolver(), FC.R, 2.0)
    w.add_fluid(f)
    for _ in range(nsteps):
        w.step(1.0 / 200.0, (0.0, 0.0, 0.0))
    mass = float(np.float32(f.volumes[0])) * float(np.float32(1000.0))
    return VR.enstrophy(np.full(len(pos), mass), w.vorticity(f))


@pytest.fixture(scope="module")
def enstrophies():
    return vorticity3(50, 0.1), vorticity3(50, 0.0)


def test_the_force_keeps_enstrophy(enstrophies):
    """12^3 particles, a Lamb-Oseen column, 50 steps without gravity: more enstrophy is left with the force than without.  Only the
    direction is asserted."""
    kept, lost = enstrophies
    print("enstrophy after 50 steps: %.6g with eps = 0.1, %.6g with eps = 0" % (kept, lost))
    assert np.isfinite(kept) and lost > 0 and kept > lost


def test_cpp_example_matches_the_python_mirror(enstrophies):
    """examples/vorticity3.cpp through include/salva_hip.hpp: the same scene, the same two numbers (the initial velocities are formed
    in double and rounded once on both sides; the printed figures carry nine digits)"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "vorticity3"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "vorticity3")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    m = re.search(r"enstrophy with the force: ([0-9.e+-]+); without: ([0-9.e+-]+)", r.stdout)
    assert m and "1728 particles, 50 steps" in r.stdout
    assert float(m.group(1)) == pytest.approx(enstrophies[0], rel=1e-6) and float(m.group(2)) == pytest.approx(enstrophies[1], rel=1e-6)
