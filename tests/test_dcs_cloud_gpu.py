"""ColliderSampling::DynamicContactSampling on the device (dcs.hip) in every projection branch of each shape.

The clouds of dcs_cloud.py surround a rotated ball, cuboid, capsule, tall cylinder and flat cylinder on moving bodies;
test_dcs_cloud_cpu.py asserts that the oracle's step over them puts emitting particles into every branch — the cuboid's six inner
faces, outer faces, edges and corners, the capsule's ends and barrel, the cylinder's caps, side and rims — pushes particles out and
rejects particles beyond the reach.  Here the device has to produce the same step bit for bit: the built-in shapes against the
oracle, two colliders in one pass in both orders, the host-shape arm against the built-in shapes, a folded grid against the
unfolded one, and the exact points on the borders between the branches.
"""
import numpy as np
import pytest

import dcs_cloud as D

pytestmark = pytest.mark.gpu

F = np.float32
DT = 1.0 / 200.0


def _same_emission(colliders, pred, a, b, who):
    for k, c in enumerate(colliders):
        assert len(a.sources[k]) == len(b.sources[k]) and np.array_equal(a.sources[k], b.sources[k]), \
            f"{c.name}: {who} sampled {len(a.sources[k])} vs {len(b.sources[k])} particles; only on one side: {np.setxor1d(a.sources[k], b.sources[k])[:8]}"
        ids = a.sources[k]
        assert np.array_equal(a.points[k], b.points[k]), D.first_difference(c, pred, ids, a.points[k], b.points[k], f"projections ({who})")
        assert np.array_equal(a.velocities[k], b.velocities[k]), D.first_difference(c, pred, ids, a.velocities[k], b.velocities[k], f"velocities at the point ({who})")


def _device_equals_oracle(colliders, pos, vel, solver):
    pred = D.predicted(pos, vel)
    o = D.run_oracle(colliders, pos, vel, solver)
    g = D.HipWorld(colliders, pos, vel, solver).step(DT)
    _same_emission(colliders, pred, o, g, "oracle vs device")
    for k, c in enumerate(colliders):
        assert len(o.sources[k]) > 8
        if np.abs(c.body.linvel).max() > 0:
            assert np.abs(o.velocities[k]).max() > 0.1  # the body moves
    # the pushed-out fluid, as the first force of the step saw it
    ids = np.arange(len(pos))
    first = colliders[0]
    assert np.array_equal(o.pushed_positions, g.pushed_positions), D.first_difference(first, pred, ids, o.pushed_positions, g.pushed_positions, "pushed positions")
    if solver == "iisph":
        # IISPH calls the forces before anything else of the solver ran: the probe sees the velocities as the push-out left them
        assert (o.probe_velocities != vel).any(), "no velocity was cut"
        assert np.array_equal(o.probe_velocities, g.probe_velocities), D.first_difference(first, pred, ids, o.probe_velocities, g.probe_velocities, "pushed velocities")
    # DFSPH calls them after its divergence solve (dfsph_solver.rs:667-708), on both sides: what the probe sees there carries the
    # solver's rounding.  The velocities after the step are compared instead, by the convention of test_first_step_is_bit_exact.
    vref = max(float(np.abs(o.velocities_after).max()), 2 * D.R / DT * 1e-2)
    dv = float(np.abs(g.velocities_after - o.velocities_after).max()) / vref
    dx = float(np.abs(g.positions_after - o.positions_after).max()) / D.R
    print(f"{[c.name for c in colliders]} {solver}: after the step positions differ by {dx:.2e} r, velocities by {dv:.2e} v_ref")
    if solver == "dfsph":
        assert dx < 1e-4 and dv < 1e-4, f"after the step positions differ by {dx:.2e} r, velocities by {dv:.2e} v_ref"
    # the contact search ran from the stale cells with the emitted points: identical contact sets
    assert g.ncontacts == o.ncontacts
    assert np.array_equal(g.counts, o.counts) and np.array_equal(g.boundary_counts, o.boundary_counts)
    return o


@pytest.mark.parametrize("name,solver", [(n, s) for s in ("dfsph", "iisph") for n in D.COLLIDERS])
def test_device_arm_equals_the_oracle_in_every_branch(name, solver):
    c = D.collider(name)
    pos, vel = D.cloud([c])
    _device_equals_oracle([c], pos, vel, solver)


def test_two_overlapping_colliders_in_one_pass():
    """A particle pushed by one collider is seen by the next collider of the same pass where the push left it (and still under the cell
    it was inserted in).  Cuboid then capsule, and the same world with the two registered the other way round."""
    pos, vel = D.cloud(D.overlapping_pair())
    a = _device_equals_oracle(D.overlapping_pair(), pos, vel, "iisph")
    b = _device_equals_oracle(D.overlapping_pair()[::-1], pos, vel, "iisph")
    assert (a.pushed_positions != b.pushed_positions).any(1).sum() >= 1, "the scene does not depend on the colliders' order"


@pytest.mark.parametrize("name", ["capsule", "tall_cylinder", "flat_cylinder"])
def test_host_arm_equals_the_device_arm(name):
    """test_host_shape_gpu.py's comparison for the two shapes it does not run: the callbacks of dcs_cloud.py against the built-in
    shapes (kinematic bodies, as that test explains)."""
    ca, cb = D.collider(name), D.collider(name)
    pos, vel = D.cloud([ca])
    wa, wb = D.HipWorld([ca], pos, vel), D.HipWorld([cb], pos, vel, host=True)
    for step in range(3):
        pred = D.predicted(np.array(wa.fluid.positions, F), np.array(wa.fluid.velocities, F), D.DT_PREV if step == 0 else DT)
        a, b = wa.step(DT), wb.step(DT)
        assert len(a.sources[0]) > (50 if step == 0 else 0)
        _same_emission([ca], pred, a, b, f"step {step}, built-in vs host shape")
        assert np.array_equal(a.positions_after, b.positions_after), f"step {step}: fluid positions differ"
        assert np.array_equal(a.velocities_after, b.velocities_after), f"step {step}: fluid velocities differ"


STRAYS = F([[0.1, -40.0, 0.05], [30.0, 0.4, -0.2]])  # far below, far aside: the cell box is long in x and y, both fold


def _fold_runs(monkeypatch, capfd, make, nsteps=3):
    """The same world without a fold and on a forced torus of 8 cells per axis: (colliders as first posed, positions, predictions,
    steps unfolded, steps folded, fold periods of every pass of the folded run)."""
    def run(env):
        for k in ("SALVA_HIP_NO_FOLD", "SALVA_HIP_FOLD_CELLS", "SALVA_HIP_TILE_TRACE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cs, pos, vel = make()
        pos, vel = np.concatenate([pos, STRAYS]), np.concatenate([vel, np.zeros((2, 3), F)])
        w = D.HipWorld(cs, pos, vel)
        capfd.readouterr()
        steps = [w.step(DT) for _ in range(nsteps)]
        return pos, D.predicted(pos, vel), steps, D.fold_periods(capfd.readouterr().err)

    pos, pred, ref, _ = run({"SALVA_HIP_NO_FOLD": "1"})
    _, _, got, periods = run({"SALVA_HIP_FOLD_CELLS": "8", "SALVA_HIP_TILE_TRACE": "1"})
    cs = make()[0]  # (for the messages: the poses of the first step)
    for step, (a, b) in enumerate(zip(ref, got)):
        _same_emission(cs, pred, a, b, f"step {step}, unfolded vs folded")
        assert np.array_equal(a.pushed_positions, b.pushed_positions), f"step {step}: pushed positions differ"
        assert np.array_equal(a.probe_velocities, b.probe_velocities), f"step {step}: velocities at the first force differ"
        assert a.ncontacts == b.ncontacts, (step, a.ncontacts, b.ncontacts)
    return cs, pos, pred, ref, got, periods


@pytest.mark.parametrize("name", ["cuboid", "tall_cylinder"])
def test_a_fold_given_up_after_the_push_outs_is_run_again_from_the_unpushed_particles(monkeypatch, capfd, name):
    """The whole cloud is wider than a torus of 8 cells on every axis: the first pass finds the fluid piled onto itself from its tile
    totals — AFTER the push-outs — the world loosens the fold to 32 cells and runs the substep again.  It has to start from the
    particles as they were before the first attempt pushed them, or the points of the second attempt lie a few ulps aside (how this
    test failed before World::substep kept them).  Every pass that is compared here runs on the 32-cell torus, whose seams do
    not cut through the cloud: the seam is test_a_seam_through_the_shape's."""
    def make():
        c = D.collider(name)
        return ([c],) + D.cloud([c])

    cs, pos, pred, ref, got, periods = _fold_runs(monkeypatch, capfd, make)
    assert len(ref[0].sources[0]) > 1000
    # the first attempt of step 0 on the 8-cell torus, discarded; its repeat and every later pass on the loosened one
    assert len(periods) == 4 and periods[0] == (8, 8, 8), periods
    assert all(p[0] == 32 and p[1] == 32 for p in periods[1:]), periods


@pytest.mark.parametrize("which", ["cuboid", "tall_cylinder", "cuboid+capsule"])
def test_a_seam_through_the_shape(monkeypatch, capfd, which):
    """A torus of 8 cells that HOLDS (dcs_cloud.slab_cloud: the cloud cut down to a bar along the axis on which the posed shape's
    loosened box is wider than 8 cells): every compared pass runs on it, its seam cuts through that box, and particles of more than
    one image of the same keys emit — dcs_unfold has to pick the image from the particle's position.  With two colliders the second
    sees particles the first has pushed into the cell below the one their key names: the image is the NEAREST one (d + period / 2),
    not the one below.
    ONE step is compared, and all of it: this torus wraps the fluid onto itself, so the solver's tiles hold other particles and its
    sums run in another order than on the unfolded grid — only the first step starts from identical particles on both (the second
    step's divergence solve was seen to differ in the last bit of a velocity; the arm's own outputs were still equal there).  Three
    steps on a fold that does not overlap itself are the test above."""
    def make():
        cs = D.overlapping_pair() if which == "cuboid+capsule" else [D.collider(which)]
        pos, vel, _ = D.slab_cloud(cs)
        return cs, pos, vel

    cs, pos, pred, ref, got, periods = _fold_runs(monkeypatch, capfd, make, nsteps=1)
    axis = D.slab_cloud(cs)[2]
    assert 2 * (D.half_extent(cs[0])[axis] + D.REACH) > 8 * D.H
    assert len(periods) == 1 and all(p[axis] == 8 for p in periods), f"the 8-cell fold did not hold: {periods}"
    # the images of the emitting particles along that axis (the grid's origin is the lowest cell of the box over all particles)
    cell = np.floor(pos[:, axis].astype(np.float64) / np.float64(F(D.H))).astype(int)
    image = (cell - cell.min()) // 8
    for k, c in enumerate(cs):
        n = np.bincount(image[ref[0].sources[k]] - image[ref[0].sources[k]].min())
        assert len(n) >= 2 and np.sort(n)[-2] >= 50, f"{c.name}: emitting particles per image {n}"
    if len(cs) == 2:
        # pushed by the first collider alone (the oracle's step with it) into a lower cell, and then sampled by the second
        _, p0, v0 = make()
        alone = D.run_oracle(cs[:1], p0, v0)
        lower = (np.floor(alone.pushed_positions.astype(np.float64) / np.float64(F(D.H))) < np.floor(p0.astype(np.float64) / np.float64(F(D.H)))).any(1)
        assert np.isin(np.nonzero(lower)[0], ref[0].sources[1]).sum() >= 5


@pytest.mark.parametrize("case", D.DEGENERATE, ids=[c[0].replace(" ", "_") for c in D.DEGENERATE])
def test_degenerate_points(case):
    """Exact points on the borders between the branches (dcs_cloud.DEGENERATE; none at a ball's centre, see there)."""
    c, pos, vel, want = D.degenerate_world(case)
    o = D.run_oracle([c], pos, vel)
    g = D.HipWorld([c], pos, vel).step(DT)
    _same_emission([c], pos, o, g, "oracle vs device")
    assert np.array_equal(g.sources[0], np.arange(len(pos)))
    for k, (what, _, _) in enumerate(case[2]):
        if want[k] is not None:
            assert np.array_equal(g.points[0][k], want[k]), f"{c.name}, {what}: projected to {g.points[0][k]}, expected {want[k]}"
    assert np.array_equal(o.pushed_positions, g.pushed_positions), (o.pushed_positions, g.pushed_positions)
    for a in (g.points[0], g.velocities[0], g.pushed_positions, g.probe_velocities, g.positions_after, g.velocities_after):
        assert np.isfinite(a).all(), c.name
