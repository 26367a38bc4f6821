"""The conditions test_dcs_cloud_gpu.py rests on, checked on the CPU oracle (dcs_cloud.py holds the clouds, the classifier and the
callbacks):

1. Branch floors: around every shape the cloud puts emitting particles into every branch of its projection, pushes particles out
   of it and has particles rejected by `depth > reach` after both box tests — so "the device equals the oracle" is a statement
   about every branch.
2. A third reading: the f32 numpy callbacks (the host-shape arm's view of the shapes) applied to the predicted positions give the
   oracle's emitted points bit for bit and the same inside flags.
3. The degenerate points (exact borders between branches) come out of the oracle where the parry rules put them.
"""
import numpy as np
import pytest

import dcs_cloud as D

F = np.float32

_runs = {}


def _run(name, oracle_lib):
    """(collider, positions, velocities, predicted positions, the oracle's step) for one shape's cloud, computed once."""
    if name not in _runs:
        c = D.collider(name)
        pos, vel = D.cloud([c])
        _runs[name] = (c, pos, vel, D.predicted(pos, vel), D.run_oracle([c], pos, vel))
        for a in _runs[name][1:4]:
            a.setflags(write=False)
    return _runs[name]


@pytest.mark.parametrize("name", D.COLLIDERS)
def test_the_cloud_fills_every_branch(oracle_lib, name):
    c, pos, vel, pred, arm = _run(name, oracle_lib)
    assert 3000 < len(pos) < 9000, len(pos)
    src = arm.sources[0]
    labels, inside, near = D.classify(c, pred)
    emitted = np.zeros(len(pos), bool)
    emitted[src] = True
    counts = {b: int((labels[src] == b).sum()) for b in D.BRANCHES[c.kind]}
    assert set(labels[src]) <= set(counts), set(labels[src]) - set(counts)
    short = {b: k for b, k in counts.items() if k < 8}
    assert not short, f"{name}: branches with fewer than 8 emitting particles: {short} (all: {counts})"
    # the push-out branch: the oracle moved exactly the particles the classifier finds inside (but for those within rounding of the surface)
    moved = (arm.pushed_positions != pos).any(1)
    depth = np.linalg.norm(pred.astype(np.float64) - near, axis=1)
    clear = depth > 1e-5
    assert (moved == (inside & emitted))[clear].all(), f"{name}: {(moved != (inside & emitted))[clear].sum()} particles pushed or not against the classifier"
    assert moved.sum() >= 30, f"{name}: only {moved.sum()} particles were pushed out"
    # the rejection: passed the cell range and the box, outside, farther than the reach
    in_cells, in_box = D.box_tests(c, pos, pred)
    rejected = in_cells & in_box & ~emitted
    wrong = rejected & (inside | (depth <= D.REACH - 1e-5))
    assert not wrong.any(), f"{name}: {wrong.sum()} particles within reach did not emit, in branches {sorted(set(labels[wrong]))}"
    wrong = emitted & ~inside & (depth > D.REACH + 1e-5)
    assert not wrong.any(), f"{name}: {wrong.sum()} particles beyond the reach emitted, in branches {sorted(set(labels[wrong]))}"
    assert rejected.sum() >= 30, f"{name}: only {rejected.sum()} particles were rejected by depth > reach"
    # the emitted points lie where the classifier puts the nearest surface point; the velocity there is the body's
    off = np.abs(arm.points[0] - near[src]).max(1)
    k = off.argmax()
    assert off[k] < 2e-6, f"{name}: particle {src[k]} in branch '{labels[src[k]]}' is projected {off[k]:.2e} from its nearest surface point"
    want_v = c.body.linvel + np.cross(c.body.angvel.astype(np.float64), arm.points[0] - c.body.center_of_mass())
    assert np.abs(arm.velocities[0] - want_v).max() < 2e-5 and np.abs(arm.velocities[0]).max() > 0.1


@pytest.mark.parametrize("name", D.COLLIDERS)
def test_the_callbacks_are_a_third_reading_of_the_oracle(oracle_lib, name):
    c, pos, vel, pred, arm = _run(name, oracle_lib)
    src = arm.sources[0]
    aabb, project = D.callbacks(c)
    lo, hi = aabb()
    ext = D.half_extent(c)
    assert np.abs(lo - (c.body.translation - ext)).max() < 1e-6 and np.abs(hi - (c.body.translation + ext)).max() < 1e-6, f"{name}: the callback's box"
    points, inside = project(np.array(pred[src]))
    assert np.array_equal(points, arm.points[0]), D.first_difference(c, pred, src, points, arm.points[0], "projections (callback vs oracle)")
    moved = (arm.pushed_positions != pos).any(1)[src]
    assert np.array_equal(inside, moved), D.first_difference(c, pred, src, np.asarray(inside), moved, "inside flags (callback vs oracle)")


def test_two_overlapping_colliders_depend_on_their_order(oracle_lib):
    """The scene of the GPU test of two colliders in one pass: particles pushed by the first are seen by the second where the push left them."""
    cs = D.overlapping_pair()
    pos, vel = D.cloud(cs)
    a, b = D.run_oracle(cs, pos, vel), D.run_oracle(cs[::-1], pos, vel)
    both = np.intersect1d(a.sources[0], a.sources[1])
    assert len(both) > 100
    pushed_a, pushed_b = (a.pushed_positions != pos).any(1), (b.pushed_positions != pos).any(1)
    assert pushed_a.sum() > 100 and (a.pushed_positions != b.pushed_positions).any(1).sum() >= 1


@pytest.mark.parametrize("case", D.DEGENERATE, ids=[c[0].replace(" ", "_") for c in D.DEGENERATE])
def test_degenerate_points_in_the_oracle(oracle_lib, case):
    c, pos, vel, want = D.degenerate_world(case)
    arm = D.run_oracle([c], pos, vel)
    assert np.array_equal(arm.sources[0], np.arange(len(pos))), f"{c.name}: emitted {arm.sources[0]}"
    for k, (what, _, _) in enumerate(case[2]):
        assert np.isfinite(arm.points[0][k]).all() and np.isfinite(arm.pushed_positions[k]).all(), (c.name, what)
        if want[k] is not None:
            assert np.array_equal(arm.points[0][k], want[k]), f"{c.name}, {what}: projected to {arm.points[0][k]}, expected {want[k]}"
    # the third reading agrees here too
    points, _ = D.callbacks(c)[1](pos.copy())
    assert np.array_equal(points, arm.points[0]), (c.name, points, arm.points[0])
    assert np.isfinite(arm.positions_after).all() and np.isfinite(arm.velocities[0]).all()
