"""The harness of tests/test_forces_isolated_gpu.py checked without a GPU: for every case of tests/force_cases.py the CPU oracle's
f64 build runs with a recording custom force in front of and behind the built-in force; the probe's positions, velocities and
densities and the oracle's volumes and boundary volumes go into tests/force_reading.py, and what the reading makes of them has to
be the oracle's `accelerations after - accelerations before` — both are f64, only the order of summation differs.  The same runs
measure how far the oracle's f32 build is from its f64 build (the noise floor the device is held to) and check that the scenes
exercise every term of every force.  CPU only."""
import functools

import numpy as np
import pytest

import force_cases as FC
from force_reading import Reading

# max over steps 2 and 3 and over the case's forces of  max |da_f32 - da_f64| / max |da_f64|,  da = the force's own accelerations
# (accelerations behind the force - accelerations in front of it) in the oracle's f32 and f64 builds.  Produced by
#     PYTHONPATH=. python tests/test_force_reading_cpu.py
# from the repository root; test_f32_floor holds the table to what it measures, within a factor of 2 either way.
F32_FLOOR = {
    "A-xsph": 5.77e-07,
    "A-xsph-fluid": 5.77e-07,
    "A-xsph-boundary": 8.72e-07,
    "A-artificial": 2.10e-06,
    "A-artificial-fluid": 2.10e-06,
    "A-artificial-boundary": 8.99e-07,
    "A-akinci": 1.49e-06,
    "A-akinci-fluid": 9.66e-07,
    "A-akinci-boundary": 1.82e-05,
    "A-he2014": 1.75e-06,
    "A-he2014-fluid": 2.22e-06,
    "A-he2014-boundary": 7.48e-06,
    "A-wcsph": 1.34e-06,
    "B1-xsph": 1.92e-06,
    "B1-xsph-fluid": 1.97e-06,
    "B1-xsph-boundary": 8.17e-07,
    "B1-artificial": 4.41e-06,
    "B1-artificial-fluid": 4.40e-06,
    "B1-artificial-boundary": 9.02e-07,
    "B1-akinci": 1.95e-06,
    "B1-akinci-fluid": 1.57e-06,
    "B1-akinci-boundary": 1.83e-05,
    "B1-he2014": 7.91e-07,
    "B1-he2014-fluid": 8.13e-07,
    "B1-he2014-boundary": 4.31e-06,
    "B1-wcsph": 1.70e-06,
    "B0-xsph": 9.03e-07,
    "B0-xsph-fluid": 8.79e-07,
    "B0-xsph-boundary": 9.01e-07,
    "B0-artificial": 1.94e-06,
    "B0-artificial-fluid": 1.94e-06,
    "B0-artificial-boundary": 5.37e-07,
    "B0-akinci": 2.12e-06,
    "B0-akinci-fluid": 8.03e-07,
    "B0-akinci-boundary": 3.78e-06,
    "B0-he2014": 1.46e-06,
    "B0-he2014-fluid": 1.45e-06,
    "B0-he2014-boundary": 7.46e-06,
    "B0-wcsph": 1.51e-06,
    "B1p-akinci": 1.12e-05,
    "B1p-akinci-fluid": 1.81e-06,
    "B1p-akinci-boundary": 5.42e-06,
    "B1p-he2014": 9.29e-07,
    "B1p-he2014-fluid": 1.08e-06,
    "B1p-he2014-boundary": 3.96e-06,
    "B1p-artificial": 5.27e-06,
    "B1p-artificial-fluid": 5.64e-06,
    "B1p-artificial-boundary": 8.44e-07,
    "B0p-akinci": 1.85e-06,
    "B0p-akinci-fluid": 1.09e-06,
    "B0p-akinci-boundary": 6.24e-06,
    "B0p-he2014": 1.14e-06,
    "B0p-he2014-fluid": 1.14e-06,
    "B0p-he2014-boundary": 4.38e-06,
    "B0p-artificial": 1.80e-06,
    "B0p-artificial-fluid": 1.84e-06,
    "B0p-artificial-boundary": 7.86e-07,
    "A2-xsph+akinci": 3.10e-06,
    "V-visc1": 3.29e-06,
    "V-visc3": 2.03e-06,
}

REACTIONS = ("xsph", "akinci2013", "he2014")  # forces whose boundary reaction is a plain sum over contacts (golden_scenes.py:30-33)


@functools.lru_cache(maxsize=None)
def _runs(case_id):
    """(scene, f64 records, f32 records, DFSPHViscosity's iteration counts) — once per case"""
    case = FC.BY_ID[case_id]
    sc, s64, visc = FC.run_oracle(case, True)
    _, s32, _ = FC.run_oracle(case, False)
    return sc, s64, s32, visc


@functools.lru_cache(maxsize=2)  # (a Reading holds dense pair tables: tens of megabytes)
def _reading(case_id, step, k):
    # the state behind the force is the state in front of it, but for the accelerations: the probe in front has them
    sc, s64, _, _ = _runs(case_id)
    return Reading(FC.oracle_snapshot(FC.BY_ID[case_id], sc, s64[step][k]), f32_contacts=False)


def _rows(rd, case):
    return rd.s.model == case.target


def measured_floor(case_id):
    case = FC.BY_ID[case_id]
    _, s64, s32, _ = _runs(case_id)
    worst = 0.0
    for step in FC.COMPARED:
        for k in range(len(case.forces)):
            d64 = s64[step][k + 1]["acc"] - s64[step][k]["acc"]
            d32 = s32[step][k + 1]["acc"] - s32[step][k]["acc"]
            worst = max(worst, float(np.abs(d32 - d64).max() / np.abs(d64).max()))
    return worst


@pytest.mark.parametrize("case_id", [c.id for c in FC.CASES])
def test_reading_equals_the_oracle(case_id):
    """1e-9 of the field's largest magnitude, accelerations and (XSPH, Akinci, He2014) boundary reactions, at steps 2 and 3; at
    step 1 XSPH and DFSPHViscosity add exactly nothing in the oracle (inv_dt = 0)."""
    case = FC.BY_ID[case_id]
    sc, s64, _, visc = _runs(case_id)
    for step in FC.COMPARED:
        for k, d in enumerate(case.forces):
            before, after = s64[step][k], s64[step][k + 1]
            rd = _reading(case_id, step, k)
            acc, reaction = rd.force(case.target, d)
            mine = after["acc"] - before["acc"]
            err = np.abs(acc[_rows(rd, case)] - mine).max() / np.abs(mine).max()
            print("%s step %d %s: max |a| = %.4g, reading - oracle = %.2e of it" % (case_id, step + 1, d[0], np.abs(mine).max(), err))
            assert np.abs(mine).max() > 0 and err < 1e-9
            assert not acc[~_rows(rd, case)].any()
            if d[0] in REACTIONS and sc["floor"] is not None:
                theirs = after["bforce"] - before["bforce"]
                if d[2] == 0.0:
                    assert not theirs.any() and not reaction.any()
                else:
                    rerr = np.abs(reaction - theirs).max() / np.abs(theirs).max()
                    print("    reaction: max |f| = %.4g, reading - oracle = %.2e of it" % (np.abs(theirs).max(), rerr))
                    assert rerr < 1e-9
    for k, d in enumerate(case.forces):
        if d[0] in ("xsph", "dfsph_viscosity"):
            assert np.array_equal(s64[0][k + 1]["acc"], s64[0][k]["acc"])
        if d[0] == "dfsph_viscosity":
            assert visc[k] == int(d[2]) == int(d[3])


@pytest.mark.parametrize("case_id", [c.id for c in FC.CASES])
def test_f32_floor(case_id):
    got = measured_floor(case_id)
    print("%s: f32 build - f64 build = %.2e (table: %.2e)" % (case_id, got, F32_FLOOR[case_id]))
    assert F32_FLOOR[case_id] / 2 <= got <= F32_FLOOR[case_id] * 2


@pytest.mark.parametrize("case_id", [c.id for c in FC.CASES])
def test_the_inputs_exercise_every_term(case_id):
    """On the reading alone, at steps 2 and 3: every separately switchable term that is on reaches 1 % of the force's largest
    acceleration (fluid arm, boundary arm, Akinci's curvature part, ArtificialViscosity's beta part and its alpha part); a quarter
    of the fluid's contact pairs approach and a quarter recede — for ArtificialViscosity, which is the force that asks, also among
    the fluid contacts alone and among the boundary contacts alone, whichever arms are on; each boundary arm acts on 30 particles
    or more."""
    case = FC.BY_ID[case_id]
    sc = _runs(case_id)[0]
    for step, k in [(step, k) for step in FC.COMPARED for k in range(len(case.forces))]:
        rd, d = _reading(case_id, step, k), case.forces[k]
        own = _rows(rd, case)
        full = rd.force(case.target, d)[0]
        top = np.abs(full).max()
        share = lambda a: float(np.abs(a).max() / top)
        report = {}
        if d[0] in FC.TWO_ARMS:
            if d[1] != 0.0:
                report["fluid arm"] = share(rd.force(case.target, d[:2] + (0.0,) + d[3:])[0])
            if d[2] != 0.0:
                arm = rd.force(case.target, d[:1] + (0.0,) + d[2:])[0]
                report["boundary arm"] = share(arm)
                touched = int((np.abs(arm[own]).sum(axis=1) > 0).sum())
                assert touched >= 30, f"step {step + 1}: the boundary arm acts on {touched} particles"
        if d[0] == "akinci2013" and d[1] != 0.0:
            report["curvature"] = share(rd.akinci_curvature(case.target, float(np.float32(d[1]))))
            report["cohesion"] = share(rd.force(case.target, d[:2] + (0.0,))[0] - rd.akinci_curvature(case.target, float(np.float32(d[1]))))
        if d[0] == "artificial":
            no_beta = rd.force(case.target, d[:4] + (0.0,) + d[5:])[0]
            report["alpha"], report["beta"] = share(no_beta), share(full - no_beta)
        (fa, fr), (ba, br) = rd.approaching(case.target)
        pairs = {"": (fa.sum() + ba.sum(), fr.sum() + br.sum())}
        if d[0] == "artificial":  # the one force that asks which way a pair is moving: each of its arms by itself as well
            if d[1] != 0.0:
                pairs[" fluid"] = (fa.sum(), fr.sum())
            if d[2] != 0.0:
                pairs[" boundary"] = (ba.sum(), br.sum())
        for name, (na, nr) in pairs.items():
            report["approaching%s contacts" % name], report["receding%s contacts" % name] = na / (na + nr), nr / (na + nr)
        print("%s step %d %s:" % (case_id, step + 1, d[0]), ", ".join("%s %.3f" % kv for kv in report.items()))
        for name, value in report.items():
            assert value >= (0.25 if "contacts" in name else 0.01), f"step {step + 1}: {name} = {value:.4f}"
    if case.scene == "A2":
        # the two particles are still one point when the forces look at them (the same sums move them)
        x = _reading(case_id, FC.COMPARED[-1], 0).s.x
        assert np.sqrt(((x[-1] - x[(4 * 9 + 4) * 9 + 4]) ** 2).sum()) <= 1e-12


if __name__ == "__main__":
    print("F32_FLOOR = {")
    for c in FC.CASES:
        print('    "%s": %.2e,' % (c.id, measured_floor(c.id)))
    print("}")
