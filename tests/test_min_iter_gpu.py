"""Minimum iteration counts above 1 (world_step.hip World::SolveTest).

A convergence test of an iteration below `min_iter` cannot end the solve (`err <= tol && i >= min`), so it is not launched: the
next test that is launched counts it (`skipped`, handed to k_finalize_error / k_decide).  Every other scene of the suite runs with
`min_pressure_iter = min_divergence_iter = 1`, where that rule only ever skips iteration 0.  Here both minima are 3 — and, in the
second case, so are both maxima: the last test of the only batch is then also the `max_iter` test.

Waited batches, chained batches (with their continuations) and speculative applies must report the same counts and errors, bit
for bit, and the plain run's counts are held against the CPU oracle the way test_parity_gpu.compare holds its small scenes'."""
import numpy as np
import pytest

from parity import DT, GRAVITY
from test_chain_gpu import PLAIN, _drop_scene, _run, _same_state

pytestmark = pytest.mark.gpu
NSTEPS = 40
CASES = {
    "min3": dict(min_divergence_iter=3, min_pressure_iter=3),
    "min3_max3": dict(min_divergence_iter=3, min_pressure_iter=3, max_divergence_iter=3, max_pressure_iter=3),
}


def _scene(case):
    sc = _drop_scene(16, lift=0.1)
    sc.solver_params.update(CASES[case])
    return sc


@pytest.mark.parametrize("case", sorted(CASES))
def test_tests_below_min_iter_are_counted_by_the_next_one(case):
    w0, f0, t0 = _run(PLAIN, NSTEPS, scene=_scene(case))
    others = [_run(env, NSTEPS, scene=_scene(case)) for env in ({}, {"SALVA_HIP_NO_SPEC_APPLY": "1"})]
    iters = np.asarray([t[:2] for t in t0], dtype=np.int64)
    print(case, "iterations (divergence, pressure) per step:", iters.tolist())
    for w, f, t in others:
        assert t == t0  # iteration counts, contacts AND the errors the solves stopped at, bit for bit
        _same_state(w, f, w0, f0)
    assert (iters >= 3).all(), iters.tolist()
    if case == "min3_max3":
        assert (iters == 3).all(), iters.tolist()
    o = _scene(case).make_oracle(threads=4)
    ref = []
    for _ in range(NSTEPS):
        so = o.step(DT, GRAVITY)
        ref.append([so.n_div_iters, so.n_press_iters])
    ri = np.asarray(ref, dtype=np.int64)
    print(case, "oracle:", ri.tolist())
    assert (np.abs(iters - ri) <= 1).all(), f"{case}: iteration counts {iters.tolist()} vs {ri.tolist()}"

