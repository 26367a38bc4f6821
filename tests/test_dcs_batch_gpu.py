"""Batched DynamicContactSampling (dcs.hip "batched runs"): runs of device-shape colliders sampled in ONE pass over
the fluid, and the batched pose / wrench entry points, each against the per-collider path they replace — bit for bit, rows in row
order, nothing sorted before it is compared.  SALVA_HIP_NO_DCS_BATCH=1 (read when a world is created) gives the per-collider world.

The record buffer of the batched pass is sized optimistically and grown on demand; test_record_buffer_growth starts it at one
record (SALVA_HIP_DCSB_CAP0=1).  The scene is tests/dcs_batch_scene.py.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dcs_batch_scene as S
from parity import DT, GRAVITY, max_norm_diff
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, _lib, scenes
from salva_amd.coupling import ColliderCouplingSet, DynamicContactSampling, FluidsPipeline, HostShapeSampling, RigidBody, StaticSampling
from test_host_shape_gpu import cuboid_callbacks

pytestmark = pytest.mark.gpu

F = np.float32
R = S.R
FP = C.POINTER(C.c_float)
U32P = C.POINTER(C.c_uint32)
BLOCK = 256  # common.h


def _world(monkeypatch, batch, *args, env=None, **kw):
    """A world with (batch) or without the batched pass; further switches in `env`.  The switches are read at creation."""
    for k in ("SALVA_HIP_NO_DCS_BATCH", "SALVA_HIP_DCSB_CAP0", "SALVA_HIP_NO_FOLD", "SALVA_HIP_FOLD_CELLS"):
        monkeypatch.delenv(k, raising=False)
    if not batch:
        monkeypatch.setenv("SALVA_HIP_NO_DCS_BATCH", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    out = S.hip_world(*args, **kw)
    for k in ("SALVA_HIP_NO_DCS_BATCH", "SALVA_HIP_DCSB_CAP0", "SALVA_HIP_NO_FOLD", "SALVA_HIP_FOLD_CELLS"):
        monkeypatch.delenv(k, raising=False)
    return out


def _state(w, st, h, bounds, static, probe):
    """Everything the arm produces in one step, as it lies in memory."""
    out = {"ncontacts": int(st.ncontacts), "fluid_pos": np.array(h.positions, F), "fluid_vel": np.array(h.velocities, F),
           "cc": np.array(w.contact_counts(h)), "ccb": np.array(w.contact_counts(h, True))}
    if probe is not None:
        out["pushed"] = probe.positions.copy()
    for k, b in enumerate(bounds):
        out[f"b{k}_n"] = b.num_particles()
        out[f"b{k}_pos"] = np.array(b.positions, F).reshape(-1, 3)
        out[f"b{k}_vel"] = np.array(b.velocities, F).reshape(-1, 3)
        fs, idx = b.sources()
        out[f"b{k}_src_fluid"], out[f"b{k}_src"] = fs, idx
    if static is not None:
        pos, vel = w._boundary_particles(static)
        out["static_pos"], out["static_vel"] = np.array(pos, F), np.array(vel, F)
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        same = np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
        assert same, f"{what}: {k} differs between the batched and the per-collider world"


def _run_pair(monkeypatch, pos, vel, make_cols, nsteps, env=None, static_after=2, move=S.move):
    """The same scene in a batched and in a per-collider world -> their states per step, their stats per step, the worlds."""
    sides = []
    for batch in (True, False):
        cols, probe = make_cols(), S.Probe()
        w, h, bounds, static, c = _world(monkeypatch, batch, pos, vel, cols, env=env, static_after=static_after, probe=probe)
        states, stats = [], []
        for step in range(nsteps):
            st = w.step_with_coupling(DT, GRAVITY, c)
            states.append(_state(w, st, h, bounds, static, probe))
            stats.append(S.dcs_stats(w))
            move(cols, step)
        sides.append((states, stats, w))
    for step in range(nsteps):
        _assert_same(sides[0][0][step], sides[1][0][step], f"step {step}")
    return sides


def test_batch_equals_the_per_collider_path_bit_for_bit(monkeypatch):
    pos, vel = S.fluid()
    (sb, stats_b, _), (sp, stats_p, _) = _run_pair(monkeypatch, pos, vel, S.colliders, 3)
    # ---- what keeps the comparison from being vacuous, established on the per-collider world
    rows = [[s[f"b{k}_n"] for k in range(6)] for s in sp]
    print("rows per collider and step (per-collider world):", rows, "stats batched", stats_b, "per collider", stats_p)
    assert min(rows[0]) > 20, rows[0]
    assert any(0 in r for r in rows), rows  # the cylinder has left in the third step
    assert np.array_equal(sp[0]["static_pos"], S.static_points()) and not sp[0]["static_vel"].any()
    # collider k moved particle i iff the pushed positions of the worlds with the first k and the first k - 1 colliders differ there
    movers, prev = np.zeros(len(pos), int), pos
    for k in range(1, 7):
        probe = S.Probe()
        w, _, _, _, c = _world(monkeypatch, False, pos, vel, S.colliders()[:k], static_after=-1, probe=probe)
        w.step_with_coupling(DT, GRAVITY, c)
        movers += np.abs(probe.positions - prev).max(axis=1) > 0
        prev = probe.positions
    assert np.array_equal(prev, sp[0]["pushed"])  # (the static boundary changes nothing in the sampling pass)
    assert (movers >= 2).sum() >= 10, f"{(movers >= 2).sum()} particles were moved by two colliders"
    # the batched world went through the batch, the other did not
    assert all(s[2] == 6 for s in stats_b) and all(s[2] == 0 for s in stats_p)


def test_batch_first_step_is_bit_exact_against_the_oracle(monkeypatch):
    """Five analytic colliders (the mesh as the cuboid it is), ball / cuboid and capsule / cylinder overlapping; asserted as
    test_dynamic_sampling_gpu.py::test_first_step_is_bit_exact asserts its two."""
    pos, vel = S.fluid()
    cols = [(n, ("cuboid", S.MESH_HE) if s == "mesh" else s, b) for n, s, b in S.colliders() if s != "heightfield"]
    oprobe, gprobe = [], S.Probe()
    o, f = S.oracle_world(pos, vel, cols, oprobe)
    w, h, bounds, _, c = _world(monkeypatch, True, pos, vel, cols, static_after=-1, probe=gprobe)
    so = o.step(DT, GRAVITY)
    st = w.step_with_coupling(DT, GRAVITY, c)
    assert S.dcs_stats(w)[2] == 5
    for b in range(5):
        n = o.boundary_len(b)
        assert n > 50 and bounds[b].num_particles() == n, f"boundary {b}: {bounds[b].num_particles()} points vs {n}"
        of, op = o.boundary_sources(b)
        order = np.lexsort((op, of))
        gf, gp = bounds[b].sources()
        gorder = np.lexsort((gp, gf))
        assert np.array_equal(op[order], gp[gorder]), f"boundary {b}: different fluid particles were sampled"
        po, pg = o.boundary_vec(b, "positions").astype(F)[order], bounds[b].positions[gorder]
        vo, vg = o.boundary_vec(b, "velocities").astype(F)[order], bounds[b].velocities[gorder]
        assert np.array_equal(po, pg), f"boundary {b}: projections differ by {np.abs(po - pg).max():.3e}"
        assert np.array_equal(vo, vg), f"boundary {b}: velocity_at_point differs by {np.abs(vo - vg).max():.3e}"
        assert np.abs(vo).max() > 0.1
    assert len(oprobe) == 1 and gprobe.positions is not None
    moved = np.abs(oprobe[0] - pos).max(axis=1) > 0
    assert moved.sum() > 20, "the scene did not exercise the push-out branch"
    assert np.array_equal(oprobe[0], gprobe.positions), f"pushed positions differ by {np.abs(oprobe[0] - gprobe.positions).max():.3e}"
    assert int(st.ncontacts) == int(so.ncontacts)
    assert np.array_equal(w.contact_counts(h), o.contact_counts(f))
    assert np.array_equal(w.contact_counts(h, True), o.contact_counts(f, True))
    d = max_norm_diff(h.positions, o.fluid_vec(f, "positions")) / R
    vref = max(float(np.abs(o.fluid_vec(f, "velocities")).max()), 2 * R / DT * 1e-2)
    dv = max_norm_diff(h.velocities, o.fluid_vec(f, "velocities")) / vref
    assert d < 1e-4 and dv < 1e-4, f"after the first step positions differ by {d:.2e} r, velocities by {dv:.2e} v_ref"


def _ball(t, v=(0.0, 0.0, 0.0)):
    return RigidBody(translation=F(t), linvel=F(v), angvel=F([0.5, 1.0, -0.5]), dynamic=False)


HOST_HE = (0.12, 0.10, 0.14)


def _host_cols(pattern):
    """Balls (b) and one host-shape cuboid (h) that all overlap around the middle of the block."""
    spots = [(-0.10, 0.30, -0.05), (0.06, 0.34, 0.04), (-0.03, 0.40, 0.08), (0.02, 0.26, -0.08), (0.10, 0.38, -0.02)]
    cols = []
    for k, ch in enumerate(pattern):
        if ch == "b":
            cols.append((f"ball{k}", ("ball", 0.12), _ball(spots[k], (0.2 * (k - 2), 0.3, -0.1 * k))))
        else:
            body = RigidBody(translation=F(spots[k]), rotation=scenes.quat_from_scaled_axis((0.3, -0.2, 0.5)), linvel=F([-0.3, 0.2, 0.1]), dynamic=False)
            cols.append((f"host{k}", HostShapeSampling(*cuboid_callbacks(body, HOST_HE)), body))
    return cols


@pytest.mark.parametrize("pattern,batched,passes", [("bhb", 0, 3), ("bbhbb", 4, 3)])
def test_a_host_shape_splits_the_run(monkeypatch, pattern, batched, passes):
    """ball, host, ball: two runs of one, no batch at all.  ball, ball, host, ball, ball: two batches of two around the host arm."""
    pos, vel = S.fluid()
    (sb, stats_b, _), (sp, stats_p, _) = _run_pair(monkeypatch, pos, vel, lambda: _host_cols(pattern), 2, static_after=-1)
    nb = len(pattern)
    assert all(sp[0][f"b{k}_n"] > 20 for k in range(nb)), [sp[0][f"b{k}_n"] for k in range(nb)]
    assert np.abs(sp[0]["pushed"] - pos).max() > 0
    for s in stats_b:
        assert s[2] == batched and s[0] == passes, s
    for s in stats_p:
        assert s[2] == 0 and s[0] == nb, s


def test_statistics(monkeypatch):
    """Six colliders: at most 2 passes over the fluid and 2 host waits in a batched step; 6 passes and at least 6 waits without."""
    pos, vel = S.fluid()
    for batch in (True, False):
        cols = S.colliders()
        w, h, bounds, static, c = _world(monkeypatch, batch, pos, vel, cols)
        w.step_with_coupling(DT, GRAVITY, c)  # (the first batched step may repeat its pass to size the record buffer)
        S.move(cols, 0)
        w.step_with_coupling(DT, GRAVITY, c)
        passes, waits, batched, records = S.dcs_stats(w)
        print("batch" if batch else "per collider", passes, waits, batched, records)
        assert records == sum(b.num_particles() for b in bounds) > 100
        if batch:
            assert passes <= 2 and waits <= 2 and batched == 6
        else:
            assert passes == 6 and waits >= 6 and batched == 0


def test_record_buffer_growth(monkeypatch):
    """The record buffer starts at ONE record: the first pass overflows, writes nothing, and is repeated with a buffer that fits."""
    pos, vel = S.fluid()
    (sb, stats_b, _), (sp, stats_p, _) = _run_pair(monkeypatch, pos, vel, S.colliders, 2, env={"SALVA_HIP_DCSB_CAP0": "1"})
    assert stats_b[0][0] == 2 and stats_b[0][2] == 6, stats_b  # two passes in the first step ...
    assert stats_b[1][0] == 1, stats_b                          # ... one afterwards
    assert min(sp[0][f"b{k}_n"] for k in range(6)) > 20


def test_empty_fluid_and_distant_fluid(monkeypatch):
    # ---- colliders and no fluid particle at all
    w, h, bounds, static, c = _world(monkeypatch, True, np.zeros((0, 3), F), np.zeros((0, 3), F), S.colliders())
    for _ in range(2):
        w.step_with_coupling(DT, GRAVITY, c)
    assert [b.num_particles() for b in bounds] == [0] * 6
    pos_s, _ = w._boundary_particles(static)
    assert np.array_equal(np.array(pos_s, F), S.static_points())
    # ---- a fluid nowhere near any collider: every count is zero, the static rows are intact; then the fluid is where the colliders
    # are, and gone again (rows appear in front of and behind the static boundary, and leave)
    pos, vel = S.fluid()
    far = (pos + F([30.0, 0.0, 0.0])).astype(F)
    for batch in (True, False):
        w, h, bounds, static, c = _world(monkeypatch, batch, far, vel, S.colliders())
        w.step_with_coupling(DT, GRAVITY, c)
        assert [b.num_particles() for b in bounds] == [0] * 6
        assert S.dcs_stats(w)[3] == 0 and S.dcs_stats(w)[2] == (6 if batch else 0)
        pos_s, vel_s = w._boundary_particles(static)
        assert np.array_equal(np.array(pos_s, F), S.static_points()) and not np.array(vel_s).any()
        h.positions = pos
        w.step_with_coupling(DT, GRAVITY, c)
        assert min(b.num_particles() for b in bounds) > 20
        pos_s, _ = w._boundary_particles(static)
        assert np.array_equal(np.array(pos_s, F), S.static_points())
        h.positions = far
        w.step_with_coupling(DT, GRAVITY, c)
        assert [b.num_particles() for b in bounds] == [0] * 6
        pos_s, _ = w._boundary_particles(static)
        assert np.array_equal(np.array(pos_s, F), S.static_points())


def test_batch_on_a_folded_grid(monkeypatch):
    """A torus of 8 cells per axis (the block is 7 cells wide) with the overlapping ball and cuboid, and two strays far away."""
    pos, vel = S.fluid()
    pos = np.concatenate([pos, F([[0.1, -40.0, 0.05], [30.0, 0.4, -0.2]])])
    vel = np.concatenate([vel, np.zeros((2, 3), F)])
    (sb, stats_b, _), (sp, _, _) = _run_pair(monkeypatch, pos, vel, lambda: S.colliders()[:2], 4, env={"SALVA_HIP_FOLD_CELLS": "8"}, static_after=-1)
    assert min(sp[0]["b0_n"], sp[0]["b1_n"]) > 50 and np.abs(sp[0]["pushed"] - pos).max() > 0
    assert all(s[2] == 2 for s in stats_b)
    # ... and both equal the unfolded batched world in what the pass produces
    cols, probe = S.colliders()[:2], S.Probe()
    w, h, bounds, static, c = _world(monkeypatch, True, pos, vel, cols, env={"SALVA_HIP_NO_FOLD": "1"}, static_after=-1, probe=probe)
    st = w.step_with_coupling(DT, GRAVITY, c)
    unfolded = _state(w, st, h, bounds, static, probe)
    for k in ("pushed", "b0_pos", "b1_pos", "b0_src", "b1_src", "ncontacts"):
        assert np.array_equal(unfolded[k], sb[0][k]), k


# ------------------------------------------------------------------------------------------------------------ wrenches and poses
def _wrench_world():
    """Static boundaries of 1, 63, 64, 65 and 256 * BLOCK + 1 rows (the last makes the grid-stride loop run) that receive forces from
    a small block of fluid resting against them, one that does not want forces, one that is empty."""
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    pos = scenes.jitter(scenes.cube_fluid_positions(8, 8, 8, R), 0.1 * R, seed=3)
    h = w.add_fluid(Fluid(pos, R, 1000.0))
    rng = np.random.default_rng(9)
    bounds = []
    for n in (1, 63, 64, 65):  # points inside the block: whatever their arrangement, they are in contact with the fluid
        b = Boundary(((rng.random((n, 3)).astype(F) - F(0.5)) * F(0.3)).astype(F), wants_forces=True)
        bounds.append(w.add_boundary(b))
    # 256 * BLOCK + 1 rows: a sheet at spacing R under the block (257 x 255 points and two more); the block wets its middle
    i, k = np.meshgrid(np.arange(257, dtype=F), np.arange(255, dtype=F), indexing="ij")
    sheet = np.stack([(i.ravel() - F(128)) * F(R), np.full(i.size, F(-8 * R - 0.03)), (k.ravel() - F(127)) * F(R)], axis=1).astype(F)
    sheet = np.concatenate([sheet, F([[0.0, -8 * R - 0.06, 0.0], [0.02, -8 * R - 0.06, 0.0]])])
    assert len(sheet) == 256 * BLOCK + 1
    bounds.append(w.add_boundary(Boundary(sheet, wants_forces=True)))
    bounds.append(w.add_boundary(Boundary(((rng.random((40, 3)).astype(F) - F(0.5)) * F(0.3)).astype(F), wants_forces=False)))
    bounds.append(w.add_boundary(Boundary(np.zeros((0, 3), F))))
    w.step(DT, GRAVITY)
    return w, bounds


def test_wrenches_equal_the_single_calls():
    w, bounds = _wrench_world()
    slots = [b._slot for b in bounds] + [bounds[3]._slot]  # (one slot twice, about another point)
    rng = np.random.default_rng(4)
    points = rng.random((len(slots), 3)).astype(F)
    single_f, single_t = np.zeros((len(slots), 3), F), np.zeros((len(slots), 3), F)
    for k, s in enumerate(slots):
        _lib.check(w._L.salva_hip_get_boundary_wrench(w._h, s, points[k].ctypes.data_as(FP), single_f[k].ctypes.data_as(FP), single_t[k].ctypes.data_as(FP)))
    f, t = np.full((len(slots), 3), 7.0, F), np.full((len(slots), 3), 7.0, F)
    arr = (C.c_uint32 * len(slots))(*slots)
    _lib.check(w._L.salva_hip_get_boundary_wrenches(w._h, len(slots), arr, points.ctypes.data_as(FP), f.ctypes.data_as(FP), t.ctypes.data_as(FP)))
    assert np.array_equal(f, single_f) and np.array_equal(t, single_t)
    assert all(np.abs(single_f[k]).max() > 0 for k in range(5)), single_f  # every wanting boundary felt the fluid
    assert not single_f[5].any() and not single_f[6].any() and not single_t[5].any() and not single_t[6].any()
    assert not np.array_equal(single_t[3], single_t[7]) and np.array_equal(single_f[3], single_f[7])
    # an out-of-range slot: E_INVALID, outputs untouched
    f[:], t[:] = 7.0, 7.0
    bad = (C.c_uint32 * len(slots))(*(slots[:-1] + [len(bounds)]))
    rc = w._L.salva_hip_get_boundary_wrenches(w._h, len(slots), bad, points.ctypes.data_as(FP), f.ctypes.data_as(FP), t.ctypes.data_as(FP))
    assert rc == _lib.E_INVALID
    assert (f == 7.0).all() and (t == 7.0).all()


def _pose_world(monkeypatch):
    """Two statically and two dynamically sampled boundaries around a block of fluid, registered by hand (no coupling set)."""
    pos, vel = S.fluid()
    cols = S.colliders()
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    fl = Fluid(pos, R, 1000.0)
    fl.velocities = vel
    h = w.add_fluid(fl)
    rng = np.random.default_rng(21)
    bounds, bodies = [], []
    c = ColliderCouplingSet()
    for k, n in enumerate((70, 300)):
        b = w.add_boundary(Boundary(np.zeros((0, 3), F)))
        body = RigidBody(translation=F([0.45, 0.3 + 0.2 * k, 0.0]), rotation=scenes.quat_from_scaled_axis((0.1, 0.3 * k, 0.2)),
                         linvel=F([0.1, 0.2, -0.3]), angvel=F([1.0, 0.5, -2.0]), local_com=F([0.01, 0.02, 0.0]), dynamic=(k == 1))
        c.register_coupling(b, f"static{k}", body, StaticSampling(((rng.random((n, 3)).astype(F) - F(0.5)) * F(0.2)).astype(F)))
        bounds.append(b); bodies.append(body)
    for name, shape, body in cols[:2]:
        b = w.add_boundary(Boundary(np.zeros((0, 3), F)))
        c.register_coupling(b, name, body, DynamicContactSampling(shape))
        bounds.append(b); bodies.append(body)
    w.sync_to_device()
    c.update_boundaries(w)  # registers every sampling method with the library (and poses once)
    return w, h, bounds, bodies


def _poses(bodies, t):
    out = (_lib.RigidPose * len(bodies))()
    for k, body in enumerate(bodies):
        moved = RigidBody(translation=(body.translation + F([0.01 * t, 0.02 * t, 0.0])).astype(F), rotation=body.rotation, linvel=body.linvel,
                          angvel=body.angvel, local_com=body.local_com, dynamic=body.dynamic)
        out[k] = moved.pose()
    return out


def test_poses_equal_the_single_calls(monkeypatch):
    res = []
    for batched in (True, False):
        w, h, bounds, bodies = _pose_world(monkeypatch)
        order = [2, 0, 3, 1, 0]  # dynamic, static, dynamic, static, and the first static one again with another pose
        poses = _poses([bodies[k] for k in order], 1)
        poses[4] = _poses([bodies[0]], 3)[0]
        slots = (C.c_uint32 * len(order))(*[bounds[k]._slot for k in order])
        if batched:
            _lib.check(w._L.salva_hip_update_boundary_poses(w._h, len(order), slots, poses))
        else:
            for k in range(len(order)):
                _lib.check(w._L.salva_hip_update_boundary_pose(w._h, slots[k], C.byref(poses[k])))
        snap = [tuple(np.array(x, F) for x in w._boundary_particles(bounds[k])) for k in range(2)]
        st = w.step(DT, GRAVITY)
        res.append((snap, int(st.ncontacts), np.array(h.positions, F), np.array(h.velocities, F),
                    [np.array(bounds[k].positions, F) for k in (2, 3)]))
        if batched:
            # a non-finite rotation in the LAST pose rejects the whole call and changes nothing
            before = [tuple(np.array(x, F) for x in w._boundary_particles(bounds[k])) for k in range(2)]
            bad = _poses([bodies[k] for k in order], 5)
            bad[4].rotation[2] = float("nan")
            assert w._L.salva_hip_update_boundary_poses(w._h, len(order), slots, bad) == _lib.E_INVALID
            after = [tuple(np.array(x, F) for x in w._boundary_particles(bounds[k])) for k in range(2)]
            for a, b in zip(before, after):
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            st2 = w.step(DT, GRAVITY)  # the dynamic slots kept their poses too: the step is the one the other world takes
            res.append((int(st2.ncontacts), np.array(h.positions, F), [np.array(bounds[k].positions, F) for k in (2, 3)]))
        else:
            st2 = w.step(DT, GRAVITY)
            res.append((int(st2.ncontacts), np.array(h.positions, F), [np.array(bounds[k].positions, F) for k in (2, 3)]))
    (snap_a, nc_a, pa, va, dyn_a), after_a, (snap_b, nc_b, pb, vb, dyn_b), after_b = res
    for k in range(2):
        assert len(snap_a[k][0]) == (70, 300)[k]
        assert np.array_equal(snap_a[k][0], snap_b[k][0]) and np.array_equal(snap_a[k][1], snap_b[k][1]), k
        assert np.abs(snap_a[k][1]).max() > 0
    assert nc_a == nc_b and np.array_equal(pa, pb) and np.array_equal(va, vb)
    assert all(np.array_equal(x, y) for x, y in zip(dyn_a, dyn_b)) and min(len(x) for x in dyn_a) > 20
    assert after_a[0] == after_b[0] and np.array_equal(after_a[1], after_b[1]) and all(np.array_equal(x, y) for x, y in zip(after_a[2], after_b[2]))


# ------------------------------------------------------------------------------------------------------------------------ mirrors
class _SingleCallSet(ColliderCouplingSet):
    """The coupling set as it was before the batched entry points: one pose call and one wrench call per collider."""

    def update_boundaries(self, world):
        if not all(e.uploaded for e in self.entries.values()):
            super().update_boundaries(world)  # registers the sampling methods with the library (the poses are handed over again below)
        for e in self.entries.values():
            if e.body is not None:
                pose = e.body.pose()
                e.boundary.wants_forces = e.body.is_dynamic()
            else:
                pose = _lib.RigidPose()
                pose.rotation[3] = 1.0
            _lib.check(world._L.salva_hip_update_boundary_pose(world._h, e.boundary._slot, C.byref(pose)))

    def transmit_forces(self, world, dt):
        fp = FP
        for e in self.entries.values():
            b = e.boundary
            if b._world is not world or e.body is None or not b.wants_forces or b.num_particles() == 0:
                continue
            com = e.body.center_of_mass()
            f, t = np.zeros(3, F), np.zeros(3, F)
            _lib.check(world._L.salva_hip_get_boundary_wrench(world._h, b._slot, com.ctypes.data_as(fp), f.ctypes.data_as(fp), t.ctypes.data_as(fp)))
            e.body.apply_impulse(f * F(dt))
            e.body.apply_torque_impulse(t * F(dt))


def test_fluids_pipeline_equals_the_single_entry_point_loop():
    """Four bodies — two dynamic ones (a ball, a sampled box), a kinematic capsule, a fixed slab — ten steps."""
    pos = scenes.jitter(scenes.cube_fluid_positions(10, 10, 10, R), 0.1 * R, seed=7)
    pos[:, 1] += F(10 * R + 0.075)

    def bodies():
        return [RigidBody(translation=F([0.0, -0.03, 0.0]), rotation=scenes.quat_from_scaled_axis((0.02, 0.0, 0.04)), dynamic=False),
                RigidBody(translation=F([-0.22, 0.30, 0.02]), linvel=F([1.0, 0.1, 0.0]), angvel=F([0.0, 0.0, -3.0]), local_com=F([0.0, 0.01, 0.0]),
                          mass=20.0, principal_inertia=F([0.1, 0.1, 0.1])),
                RigidBody(translation=F([0.12, 0.40, 0.05]), linvel=F([-0.5, 0.0, 0.1]), dynamic=False),
                RigidBody(translation=F([0.05, 0.62, -0.05]), linvel=F([0.0, -0.5, 0.0]), mass=2.0, principal_inertia=F([0.01, 0.01, 0.01]))]

    box = scenes.cube_fluid_positions(4, 2, 4, R)

    def build(world, coupling, bs):
        fl = Fluid(pos, R, 1000.0)
        h = world.add_fluid(fl)
        b = [world.add_boundary(Boundary(np.zeros((0, 3), F))) for _ in range(4)]
        coupling.register_coupling(b[0], "slab", bs[0], DynamicContactSampling(("cuboid", (0.30, 0.04, 0.22))))
        coupling.register_coupling(b[1], "ball", bs[1], DynamicContactSampling(("ball", 0.11)))
        coupling.register_coupling(b[2], "capsule", bs[2], DynamicContactSampling(("capsule", 0.06, 0.05)))
        coupling.register_coupling(b[3], "box", bs[3], StaticSampling(box))
        return h, b

    ba, bb = bodies(), bodies()
    pipe = FluidsPipeline(R, 2.0)
    ha, bounds_a = build(pipe.liquid_world, pipe.coupling, ba)
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    c = _SingleCallSet()
    hb, bounds_b = build(w, c, bb)
    for _ in range(10):
        pipe.step(GRAVITY, DT)
        w.step_with_coupling(DT, GRAVITY, c)
        for body in ba + bb:
            body.integrate(DT, (0.0, 0.0, 0.0))
    assert np.array_equal(ha.positions, hb.positions) and np.array_equal(ha.velocities, hb.velocities)
    for x, y in zip(ba, bb):
        assert np.array_equal(x.linvel, y.linvel) and np.array_equal(x.angvel, y.angvel)
    assert np.abs(ba[1].linvel - F([1.0, 0.1, 0.0])).max() > 1e-3 and np.abs(ba[3].linvel - F([0.0, -0.5, 0.0])).max() > 1e-4
    assert S.dcs_stats(pipe.liquid_world)[2] == 3


def test_cpp_mirror_many_bodies_example():
    """examples/many_bodies3.cpp: nine half-density balls dropped on a pool through include/salva_hip.hpp's ColliderCouplingSet, all
    sampled in one pass per step.  They fall, meet the water, are slowed down and stay above the pool floor."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "many_bodies3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples")])
    out = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().splitlines()
    rows = [re.match(r"step (\d+): mean ball y (-?[\d.]+) vy (-?[\d.]+), lowest ball y (-?[\d.]+), (\d+) samples, dcs passes (\d+) waits (\d+) batched (\d+)", ln)
            for ln in lines]
    assert all(rows), lines
    y = [float(m.group(2)) for m in rows]
    vy = [float(m.group(3)) for m in rows]
    assert all(np.isfinite(y)) and all(np.isfinite(vy)), lines
    assert y[0] > y[-1], lines                                              # they fell
    assert max(int(m.group(5)) for m in rows) > 9 * 20, lines               # the fluid was projected onto them
    assert abs(vy[-1]) < 1.0 and float(rows[-1].group(4)) > 0.1, lines      # slowed down by the water, above the floor
    assert all(int(m.group(8)) == 9 and int(m.group(6)) <= 2 and int(m.group(7)) <= 2 for m in rows), lines
