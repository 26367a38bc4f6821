"""The bounds of tests/test_elasticity_isolated_gpu.py, taken from the reference and not from the device.  For every case of
tests/elasticity_cases.py the numpy reading of Becker2009Elasticity (tests/elasticity_reading.py) runs the case's steps twice from
the inputs the device will see: in float64, and as an f32 replay in which every sum, product, division, square root, sine and
cosine rounds to f32.  Their distance is the noise floor the device is held to (ELASTIC_F32_FLOOR); the same runs decide which
steps may be compared with the reading at all, and check that the cases exercise what they claim.  CPU only."""
import numpy as np
import pytest

import elasticity_cases as EC

FIELDS = ("R", "F", "stress", "acc")
MARGIN = 1.4  # committed = MARGIN x measured: the test allows measured <= committed <= 2 x measured

# Per case, over its compared steps, fluids and entries: max |f32 replay - float64 reading| of the rotations (absolute), of F
# (grad_tr), of the stress and of the accelerations, the last three as a fraction of the field's largest float64 magnitude (of the
# stretched twin's at the same angle where the step is rigid).  The accelerations are those of the force pass by itself: both
# precisions start from the f32 replay's R, F and stress, as the device's force kernel is compared from the device's own.
# Produced by
#     PYTHONPATH=. python tests/test_elasticity_reading_cpu.py
# from the repository root (MARGIN x what it measures); test_f32_floor holds the table to the measurement.
ELASTIC_F32_FLOOR = {
    "rigid-lin": {"R": 6.47e-07, "F": 4.03e-06, "stress": 4.94e-06, "acc": 9.59e-13},
    "sheared-lin": {"R": 5.03e-07, "F": 4.77e-06, "stress": 1.85e-05, "acc": 4.67e-07},
    "stretched-lin": {"R": 5.14e-07, "F": 3.11e-06, "stress": 4.23e-06, "acc": 6.61e-07},
    "rigid-nl": {"R": 6.47e-07, "F": 4.03e-06, "stress": 5.70e-06, "acc": 1.09e-12},
    "sheared-nl": {"R": 5.03e-07, "F": 4.77e-06, "stress": 2.34e-05, "acc": 4.70e-07},
    "stretched-nl": {"R": 5.14e-07, "F": 3.11e-06, "stress": 5.01e-06, "acc": 7.12e-07},
    "stretched-poly6-spiky": {"R": 5.16e-07, "F": 3.69e-06, "stress": 4.90e-06, "acc": 5.05e-07},
    "accumulated": {"R": 5.60e-07, "F": 3.84e-06, "stress": 4.70e-06, "acc": 8.33e-07},
    "sheet": {"R": 5.47e-07, "F": 3.66e-06, "stress": 2.94e-06, "acc": 1.15e-11},
    "sheet-flat": {"R": 6.14e-07, "F": 2.88e-06, "stress": 2.65e-06, "acc": 7.57e-12},
    "rod": {"R": 1.07e-06, "F": 1.10e-05, "stress": 7.84e-06, "acc": 1.63e-10},
    "sheet-flat-negative-den": {"R": 7.45e-07, "F": 3.63e-06, "stress": 3.34e-06, "acc": 6.67e-12},
    "n255": {"R": 6.05e-07, "F": 2.90e-06, "stress": 4.00e-06, "acc": 7.93e-13},
    "n256": {"R": 6.05e-07, "F": 2.92e-06, "stress": 4.00e-06, "acc": 7.53e-13},
    "n257": {"R": 6.05e-07, "F": 2.93e-06, "stress": 4.00e-06, "acc": 3.73e-12},
    "volumes": {"R": 4.90e-07, "F": 2.99e-06, "stress": 5.33e-06, "acc": 5.91e-07},
    "behind": {"R": 5.84e-07, "F": 3.74e-06, "stress": 5.01e-06, "acc": 6.57e-07},
    "two-entries": {"R": 5.14e-07, "F": 2.70e-06, "stress": 5.01e-06, "acc": 6.57e-07},
    "cold-rigid": {"R": 5.30e-07, "F": 2.83e-06, "stress": 3.36e-06, "acc": 1.09e-12},
    "cold-sheared": {"R": 5.30e-07, "F": 2.83e-06, "stress": 3.36e-06, "acc": 1.09e-12},
    "rod-90": {"R": 1.09e-06, "F": 5.20e-06, "stress": 5.05e-06, "acc": 9.87e-11},
    "inverted": {"R": 5.30e-07, "F": 2.83e-06, "stress": 3.36e-06, "acc": 1.09e-12},
    "single": {"R": 5.30e-07, "F": 2.83e-06, "stress": 3.36e-06, "acc": 1.09e-12},
    "coincident": {"R": 5.30e-07, "F": 2.83e-06, "stress": 3.23e-06, "acc": 7.22e-13},
}

ADMIT_R_FLOOR = 2e-6  # a step is compared with the reading only if the two precisions agree on R to this ...
ADMIT_DEN = 0.1       # ... and |sum_c R_c . A_c| never falls below this fraction of its converged value (the divisor of every update)
DIVERGING = ("cold-rigid", "cold-sheared", "rod-90")  # cases whose uncompared steps are uncompared because they fail that


def measured_floor(case_id):
    units = EC.compared(case_id)
    return {k: max(u["floor"][k] for u in units) for k in FIELDS}


def _label(case, u):
    st = case.steps[u["step"]]
    return "%s fluid %d entry %d step %d (%s, %g deg, %s)" % (case.id, u["fluid"], u["entry"], u["step"] + 1, st.D, st.angle, st.warm)


@pytest.mark.parametrize("case_id", [c.id for c in EC.CASES])
def test_f32_floor(case_id):
    got, table = measured_floor(case_id), ELASTIC_F32_FLOOR[case_id]
    print("%s: f32 replay - float64 reading = %s (table: %s)" % (
        case_id, ", ".join("%s %.2e" % (k, got[k]) for k in FIELDS), ", ".join("%.2e" % table[k] for k in FIELDS)))
    for k in FIELDS:
        assert got[k] <= table[k] <= 2 * got[k], k


@pytest.mark.parametrize("case_id", [c.id for c in EC.CASES])
def test_compared_steps_are_well_conditioned(case_id):
    """What admits a step to the comparison with the reading: the f32 replay and the float64 reading agree on R to 2e-6, and the
    divisor of the extraction's update stays above a tenth of its converged value in every iteration, for every particle.  The
    uncompared steps of the cold starts beyond 90 degrees and of the rod at 90 degrees fail one of the two — which is why they are
    held to invariants only."""
    case = EC.BY_ID[case_id]
    assert EC.compared(case_id)
    for u in EC.cpu_units(case_id):
        ok = u["floor"]["R"] <= ADMIT_R_FLOOR and u["den_ratio"] >= ADMIT_DEN
        print("%s: R floor %.2e, den ratio %.3f" % (_label(case, u), u["floor"]["R"], u["den_ratio"]))
        if case.steps[u["step"]].compare:
            assert ok
        elif case_id in DIVERGING:
            assert not ok


@pytest.mark.parametrize("case_id", [c.id for c in EC.CASES])
def test_the_cases_exercise_what_they_claim(case_id):
    """On the float64 reading.  Rigid steps: R is the applied rotation Q within the case's floor plus what R still lacks after its
    20 iterations (nothing, where they converge) — not for the rod, whose A_pq has rank one and leaves the turn about the rod
    open; F and the stress vanish against the stretched twin's (1 %).  Stretched and sheared steps: the largest acceleration is at
    least 1 m/s^2 and the nonlinear term F sigma d reaches 1 % of the force.  "sheet-flat-negative-den": sum_c R_c . A_c is negative
    for every particle when the extraction starts."""
    case = EC.BY_ID[case_id]
    for u in EC.compared(case_id):
        step = case.steps[u["step"]]
        name = case.fluids[u["fluid"]][0]
        if EC.is_rigid(step):
            print("%s: |R20 - Q| = %.2e, |R20 - R420| = %.2e, F %.2e of %.2e, stress %.2e of %.2e" % (
                _label(case, u), u["R_minus_Q"], u["R_short"], u["own"]["F"], u["scale"]["F"], u["own"]["stress"], u["scale"]["stress"]))
            if name != "rod":
                assert u["R_minus_Q"] <= ELASTIC_F32_FLOOR[case_id]["R"] + u["R_short"]
            assert u["own"]["F"] <= 0.01 * u["scale"]["F"] and u["own"]["stress"] <= 0.01 * u["scale"]["stress"]
            if case_id == "sheet-flat-negative-den":  # every particle's first update divides by |a negative number|
                assert u["den_first"] < 0
        else:
            print("%s: max |a| = %.4g, nonlinear share %.3f" % (_label(case, u), u["own"]["acc"], u.get("nonlinear_share", float("nan"))))
            assert u["own"]["acc"] >= 1.0
            if case.nonlinear:
                assert u["nonlinear_share"] >= 0.01


def test_the_replay_stays_in_f32():
    """a float64 operand anywhere would silently widen the replay: every array it hands out is f32, and it differs from float64"""
    case = EC.BY_ID["stretched-nl"]
    e, m = EC.reading(case, "block", 5e5)
    p = EC.positions(case, case.steps[0], "block")
    c, a = EC.evaluate(e, p, m, EC.warm_start(case.steps[0], len(m), None), np.float32)
    assert all(x.dtype == np.float32 for x in (c.A_pq, c.rotations, c.grad_tr, c.stress, c._g, a))
    c64, a64 = EC.evaluate(e, p, m, EC.warm_start(case.steps[0], len(m), None), np.float64)
    assert a64.dtype == np.float64 and 0 < np.abs(a - a64).max() < 1e-3 * np.abs(a64).max()


def test_extractions_with_nothing_to_do_hand_the_warm_start_back():
    """the inverted body (A_pq symmetric, w = 0 at once) and the one-particle fluid (A_pq = 0): the f32 replay returns the warm start
    bit for bit, as the device is asked to; the single particle's F, stress and acceleration are exactly zero"""
    for case_id in EC.UNCHANGED:
        u = next(u for u in EC.cpu_units(case_id) if u["fluid"] == 0 and u["step"] == 0)
        assert u["unchanged32"], case_id
    u = EC.cpu_units("single")[0]
    assert u["n"] == 1 and u["own"] == {"F": 0.0, "stress": 0.0, "acc": 0.0}


if __name__ == "__main__":
    print("ELASTIC_F32_FLOOR = {")
    for c in EC.CASES:
        print('    "%s": {%s},' % (c.id, ", ".join('"%s": %.2e' % (k, MARGIN * v) for k, v in measured_floor(c.id).items())))
    print("}")
