"""User-defined NonPressureForces as kernels (SALVA_HIP_FORCE_DEVICE, include/salva_hip.h): the plugin of
examples/device_forces3.hip against the oracle and against the built-in XSPH kernel, the contact tables against the exported lists,
the statistics, the order and the dt lag of the callback, and misuse."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from parity import DT, GRAVITY
from oracle import oracle as O
from salva_amd import Boundary, DFSPHSolver, DeviceForce, Fluid, LiquidWorld, PluginForce, XSPHViscosity, _lib, scenes
from test_custom_force_gpu import CustomForceField, _scene

pytestmark = pytest.mark.gpu

R = 0.025
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGIN = os.path.join(ROOT, "examples", "libdevice_forces3.so")
ORIGIN = np.float32([0.3, 0.4, -0.2])
ALL = _lib.DEVICE_NEEDS_FF | _lib.DEVICE_NEEDS_FB | _lib.DEVICE_NEEDS_KERNEL
NSTEPS = 8


class RecordingField(PluginForce):
    """df3_field, remembering the timestep every call was given"""

    def __init__(self):
        super().__init__(PLUGIN, "df3_field", 0, ORIGIN)
        self.seen_dt = []

    def solve_device(self, view):
        self.seen_dt.append((view.dt, view.inv_dt))
        return super().solve_device(view)


def _device_run(forces, nsteps=NSTEPS):
    pos, vel, floor = _scene()
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    fl = Fluid(pos, R, 1000.0)
    fl.velocities = vel
    fl.nonpressure_forces += forces
    h = w.add_fluid(fl)
    w.add_boundary(Boundary(floor))
    for _ in range(nsteps):
        w.step(DT, GRAVITY)
    return w, h


@functools.lru_cache(maxsize=None)
def _field_and_oracle(field_first):
    """The 7^3 block over the floor with XSPH and the field, in either order, on the device and in the oracle: computed once per order."""
    pos, vel, floor = _scene()
    o = O.OracleWorld(R, 2.0, O.DFSPH)
    fo = o.add_fluid(pos, 1000.0, vel)

    def ofield(world, f, positions, velocities, densities, accelerations):
        accelerations += CustomForceField.field(ORIGIN, positions.astype(np.float32)).astype(np.float64)

    if field_first:
        o.add_custom_force(fo, ofield)
        o.add_xsph(fo, 0.5, 0.0)
    else:
        o.add_xsph(fo, 0.5, 0.0)
        o.add_custom_force(fo, ofield)
    o.add_boundary(floor)
    for _ in range(NSTEPS):
        o.step(DT, GRAVITY)
    field = RecordingField()
    w, h = _device_run([field, XSPHViscosity(0.5, 0.0)] if field_first else [XSPHViscosity(0.5, 0.0), field])
    return h.positions.copy(), h.velocities.copy(), o.fluid_vec(fo, "positions"), o.fluid_vec(fo, "velocities"), tuple(field.seen_dt)


def _assert_matches_oracle(p, v, ref_p, ref_v):
    dp = np.abs(p - ref_p).max()
    vref = max(np.abs(ref_v).max(), 2 * R / DT * 1e-2)
    dv = np.abs(v - ref_v).max()
    print("max |dx| = %.3e (bound %.3e), max |dv| = %.3e (bound %.3e)" % (dp, 1e-4 * R * NSTEPS, dv, 1e-4 * NSTEPS * vref))
    assert dp < 1e-4 * R * NSTEPS
    assert dv < 1e-4 * NSTEPS * vref


def test_device_field_matches_the_oracle():
    """[XSPHViscosity(0.5, 0), PluginForce(df3_field)] against the oracle's add_xsph + add_custom_force with the numpy field, 8 steps,
    at the host arm's tolerances (tests/test_custom_force_gpu.py).  Kind 9 is unknown to the parent commit: this test fails there."""
    p, v, ref_p, ref_v, seen = _field_and_oracle(False)
    assert len(seen) == NSTEPS
    _assert_matches_oracle(p, v, ref_p, ref_v)
    _, h2 = _device_run([XSPHViscosity(0.5, 0.0)])
    assert np.abs(v - h2.velocities).max() > 0.05  # the field did pull the fluid


# boundary.forces of the built-in XSPHViscosity(0.5, 0.3) against the HostXSPH host arm of tests/test_custom_force_gpu.py on this
# scene (moving floor that wants forces, 3 steps), max |dF| over the floor's particles, measured once on an MI355X: 2.852916718e-01,
# beside max |F| = 5.019453e-01 — HostXSPH adds no reaction force, so this distance is the whole XSPH reaction.  The bound for the
# device force is twice that; df3_xsph itself was measured at max |dF| = 1.341e-07 from the built-in kernel in the same run.
BUILTIN_VS_HOST_ARM = 2.852916718e-01


def _moving_floor_run(forces, wants_forces):
    pos, vel, floor = _scene()
    bvel = np.zeros_like(floor)
    bvel[:, 0] = 0.5
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    fl = Fluid(pos, R, 1000.0)
    fl.velocities = vel
    fl.nonpressure_forces += forces
    h = w.add_fluid(fl)
    b = Boundary(floor, wants_forces=wants_forces)
    b.velocities = bvel
    w.add_boundary(b)
    for _ in range(3):
        w.step(DT, GRAVITY)
    return h.positions.copy(), h.velocities.copy(), (np.array(b.forces, np.float32) if wants_forces else None)


@pytest.mark.parametrize("wants_forces", [False, True])
def test_device_xsph_equals_the_builtin_kernel(wants_forces):
    """df3_xsph over the view's contact tables and kernel values against XSPHViscosity(0.5, 0.3), a floor moving at 0.5 along x, 3
    steps: the bounds of test_host_xsph_over_exported_contacts_equals_the_device_kernel; with a floor that wants forces the reaction
    forces too, within twice the distance between the built-in kernel and the host arm."""
    a = _moving_floor_run([XSPHViscosity(0.5, 0.3)], wants_forces)
    b = _moving_floor_run([PluginForce(PLUGIN, "df3_xsph", ALL, [0.5, 0.3])], wants_forces)
    dp, dv = np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()
    print("max |dx| = %.3e (bound %.3e), max |dv| = %.3e (bound %.3e)" % (dp, 1e-6 * R * 30, dv, 2e-5 * np.abs(a[1]).max()))
    assert dp < 1e-6 * R * 30
    assert dv < 2e-5 * np.abs(a[1]).max()
    if wants_forces:
        df = np.abs(a[2] - b[2]).max()
        print("max |dF| = %.3e (bound %.3e), max |F| = %.3e" % (df, 2 * BUILTIN_VS_HOST_ARM, np.abs(a[2]).max()))
        assert np.abs(a[2]).max() > 0
        assert df <= 2 * BUILTIN_VS_HOST_ARM
        # (that bound would let the reaction go missing altogether; a sum of f32 terms added in fixed point has to meet the
        # project's 1e-5 relative tolerance of neighbour sums as well)
        assert df <= 1e-5 * np.abs(a[2]).max()


# ------------------------------------------------------------------------------------------------ the tables are the lists
class ViewReader(DeviceForce):
    """reads the whole view back inside the callback, with the exported lists of the same moment beside it"""

    def __init__(self, world, needs):
        super().__init__(needs)
        self.world, self.snaps = world, []

    def solve_device(self, v):
        w, n, nb = self.world, int(v.n), int(v.nb)
        rd = w.device_view_read
        s = dict(n=n, nb=nb, needs=int(v.needs), slot=int(v.fluid_slot), index=int(v.force_index), dt=(v.dt, v.inv_dt), h=v.h,
                 nullptrs=[v.ff_off, v.ff_j, v.fb_off, v.fb_j, v.ff_kern, v.fb_kern])
        s["posm"] = rd(v.posm, np.float32, 4 * n).reshape(-1, 4)
        s["vel"] = rd(v.vel, np.float32, 4 * n).reshape(-1, 4)
        s["rho"], s["model"], s["id"] = rd(v.rho, np.float32, n), rd(v.model, np.uint32, n), rd(v.id, np.uint32, n)
        s["rho0"] = rd(v.rho0, np.float32, v.nfluids)
        s["bposv"] = rd(v.bposv, np.float32, 4 * nb).reshape(-1, 4)
        s["bvel"] = rd(v.bvel, np.float32, 4 * nb).reshape(-1, 4)
        s["bid"] = rd(v.bid, np.uint32, nb)
        for k in ("ff", "fb"):
            if getattr(v, k + "_off"):
                off = rd(getattr(v, k + "_off"), np.uint64, n + 1)
                s[k + "_off"], s[k + "_j"] = off, rd(getattr(v, k + "_j"), np.uint32, int(off[-1]))
                if getattr(v, k + "_kern"):
                    s[k + "_kern"] = rd(getattr(v, k + "_kern"), np.float32, 4 * int(off[-1])).reshape(-1, 4)
        s["local"] = w.local_view()
        s["lists"] = (w.local_contacts(False), w.local_contacts(True))
        self.snaps.append(s)
        return 0


def _two_fluid_scene():
    """two fluids of density0 1000 and 500, 12 x 6 x 12 particles each at spacing 2R, one beside (above) the other: 6 cells = more
    than one 4-cell tile along every axis; over a floor"""
    blk = scenes.jitter(scenes.cube_fluid_positions(12, 12, 12, R), 0.1 * R, seed=31)
    blk[:, 1] += np.float32(12 * R + 2 * R)
    mid = np.float32(12 * R + 2 * R)
    lo, hi = np.ascontiguousarray(blk[blk[:, 1] < mid]), np.ascontiguousarray(blk[blk[:, 1] >= mid])
    assert len(lo) == len(hi) == 12 * 6 * 12
    floor = scenes.plane_lattice(16, 16, 0.0, R, -8 * 2 * R + R, -8 * 2 * R + R, layers=1)
    return lo, hi, floor


def _switched(env, make):
    keys = ("SALVA_HIP_SPLIT_S", "SALVA_HIP_NO_SPLIT", "SALVA_HIP_REF_HALO", "SALVA_HIP_FULL_HALO")
    old = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env)
    try:
        return make()  # (a world reads its switches when it is created)
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _tables_run(env, nsteps=3):
    lo, hi, floor = _two_fluid_scene()
    w = _switched(env, lambda: LiquidWorld(DFSPHSolver(), R, 2.0))
    reader = ViewReader(w, ALL)
    fa, fb = Fluid(lo, R, 1000.0), Fluid(hi, R, 500.0)
    fa.velocities = scenes.random_velocities(len(lo), 0.3, seed=32)
    fa.nonpressure_forces += [XSPHViscosity(0.5, 0.0), reader]
    ha, hb = w.add_fluid(fa), w.add_fluid(fb)
    w.add_boundary(Boundary(floor))
    for _ in range(nsteps):
        w.step(DT, GRAVITY)
    return w, (ha, hb), reader


def _rows(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))


def _check_tables(w, handles, s):
    n, nb = s["n"], s["nb"]
    assert n == sum(h.num_particles() for h in handles) and s["needs"] == ALL
    loc = s["local"]
    # ids are a permutation; models, densities and velocities are what the local view shows at the same moment
    assert np.array_equal(np.sort(s["id"]), np.arange(n)) and np.array_equal(s["id"], loc["ids"])
    assert np.array_equal(s["model"], loc["fluid_slots"]) and np.array_equal(s["rho"], loc["densities"])
    assert np.array_equal(s["vel"][:, :3], loc["velocities"]) and np.array_equal(s["posm"][:, :3], loc["positions"])
    assert np.array_equal(s["rho0"], np.float32([1000.0, 500.0]))
    for k, (loff, ljm, lj) in zip(("ff", "fb"), s["lists"]):
        off, j = s[k + "_off"], s[k + "_j"]
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
        assert np.array_equal(off, loff), "row lengths are nff / nfb: the offsets of the exported lists"
        total = int(off[-1])
        assert total > 0 and len(j) == total
        rows = _rows(off)
        if k == "ff":
            assert j.max() < n
            mine = s["model"][j].astype(np.uint64) << np.uint64(32) | j.astype(np.uint64)
        else:
            assert j.max() < nb
            bm = s["bvel"][j, 3].copy().view(np.uint32)
            assert (bm == 0).all()  # one boundary: its particles' host index is bid itself
            mine = bm.astype(np.uint64) << np.uint64(32) | s["bid"][j].astype(np.uint64)
        theirs = ljm[:total].astype(np.uint64) << np.uint64(32) | lj[:total].astype(np.uint64)
        a, b = np.lexsort((mine, rows)), np.lexsort((theirs, rows))
        assert np.array_equal(mine[a], theirs[b]), k + ": every row's (model, j) set is the exported row's"
    # list lengths against the step's own counts (host order through id)
    counts = np.concatenate([w.contact_counts(h) for h in handles])
    # kernel values: antisymmetric gradients bit for bit, the self entry, and the density they add up to
    off, j, kern = s["ff_off"], s["ff_j"].astype(np.int64), s["ff_kern"]
    rows = _rows(off)
    kij, kji = rows * n + j, j * n + rows
    a, b = np.argsort(kij, kind="stable"), np.argsort(kji, kind="stable")
    assert np.array_equal(kij[a], kji[b]), "the lists are symmetric"
    assert np.array_equal(kern[a, :3], -kern[b, :3]) and np.array_equal(kern[a, 3], kern[b, 3])
    h = np.float32(s["h"])
    w0 = np.float32(8.0) / (np.float32(np.pi) * h * h * h)
    me = rows == j
    assert me.sum() == n and (kern[me, :3] == 0).all() and np.abs(kern[me, 3] - w0).max() <= 1e-6 * w0
    dens = np.bincount(rows, weights=s["posm"][j, 3].astype(np.float64) * kern[:, 3], minlength=n)
    brows, bj = _rows(s["fb_off"]), s["fb_j"].astype(np.int64)
    dens += np.bincount(brows, weights=s["bposv"][bj, 3].astype(np.float64) * s["rho0"][s["model"][brows]] * s["fb_kern"][:, 3], minlength=n)
    err = np.abs(dens - s["rho"]).max() / np.abs(s["rho"]).max()
    rel = (np.abs(dens - s["rho"]) / s["rho"]).max()
    print("density from the tables: max relative error %.2e" % rel, "(over the largest density: %.2e)" % err)
    assert rel < 1e-5
    return counts


def test_the_tables_are_the_lists():
    """Two fluids over a floor, read back inside the callback in steps 1 and 3: offsets, (model, j) sets against
    salva_hip_get_local_contacts called in the same callback, antisymmetric kernel gradients, W(0) in the self entry, the density
    sum, velocities and ids against salva_hip_get_local."""
    w, handles, reader = _tables_run({})
    assert len(reader.snaps) == 3
    for s in (reader.snaps[0], reader.snaps[-1]):
        assert all(p for p in s["nullptrs"])
        counts = _check_tables(w, handles, s)
    # the last callback's rows against the counts the finished step reports, in host order
    s = reader.snaps[-1]
    assert np.array_equal(np.diff(s["ff_off"]).astype(np.uint32), counts[s["id"]])


def test_the_tables_with_split_tiles_and_a_referenced_only_halo():
    """The same with over-full tiles cut into parts (SALVA_HIP_SPLIT_S) and with the list builder keeping the referenced halo slots
    only (SALVA_HIP_REF_HALO): the walk the table kernel shares with the contact export covers both."""
    w0, _, _ = _tables_run({"SALVA_HIP_NO_SPLIT": "1", "SALVA_HIP_FULL_HALO": "1"}, nsteps=1)
    w, handles, reader = _tables_run({"SALVA_HIP_SPLIT_S": "200", "SALVA_HIP_REF_HALO": "1"})
    i0, i1 = w0.tile_tables(0)[0], w.tile_tables(0)[0]
    print("slots: unsplit %d, split %d; referenced-only halo: %d" % (i0[0], i1[0], i1[9]))
    assert i1[0] > i0[0] and i1[9] == 1 and i0[9] == 0
    for s in (reader.snaps[0], reader.snaps[-1]):
        _check_tables(w, handles, s)


# ------------------------------------------------------------------------------------------------ statistics
def test_statistics():
    lo, hi, floor = _two_fluid_scene()

    def world(forces_a, forces_b):
        w = LiquidWorld(DFSPHSolver(), R, 2.0)
        fa, fb = Fluid(lo, R, 1000.0), Fluid(hi, R, 500.0)
        fa.nonpressure_forces += forces_a
        fb.nonpressure_forces += forces_b
        w.add_fluid(fa), w.add_fluid(fb)
        w.add_boundary(Boundary(floor))
        return w, (fa, fb)

    # two fluids with a device force each, both asking for contacts: one build serves both
    w, fluids = world([PluginForce(PLUGIN, "df3_xsph", ALL, [0.5, 0.0])], [PluginForce(PLUGIN, "df3_xsph", ALL, [0.5, 0.0])])
    st = w.step(DT, GRAVITY)
    calls, builds, nbytes, waits = w.device_force_stats()
    assert (calls, builds, waits) == (2, 1, 0)
    n = len(lo) + len(hi)
    nff = int(sum(w.contact_counts(f).sum() for f in fluids))
    nfb = int(sum(w.contact_counts(f, True).sum() for f in fluids))
    assert nbytes == 2 * (n + 1) * 8 + (nff + nfb) * (4 + 16)
    # needs = 0: no build, and the view's contact pointers are NULL
    w, fluids = world([], [])
    reader = ViewReader(w, 0)
    fluids[0].nonpressure_forces.append(reader)
    w.step(DT, GRAVITY)
    assert w.device_force_stats() == (1, 0, 0, 0)
    assert not any(reader.snaps[0]["nullptrs"])
    # built-in forces only: nothing
    w, fluids = world([XSPHViscosity(0.5, 0.0)], [])
    w.step(DT, GRAVITY)
    assert w.device_force_stats() == (0, 0, 0, 0)
    assert st.nparticles == n


# ------------------------------------------------------------------------------------------------ order and lag
@pytest.mark.parametrize("field_first", [True, False])
def test_order_in_the_list_and_the_dt_lag(field_first):
    """[df3_field, XSPH] and [XSPH, df3_field] both match the oracle with the same order; timestep.dt() lags by one substep inside
    predict_advection (dfsph_solver.rs:693-702): (0, 0) on the first step, the previous step's afterwards."""
    p, v, ref_p, ref_v, seen = _field_and_oracle(field_first)
    _assert_matches_oracle(p, v, ref_p, ref_v)
    assert seen[0] == (0.0, 0.0)
    assert all(abs(dt - DT) < 1e-9 and abs(inv - 1 / DT) < 1e-3 for dt, inv in seen[1:]) and len(seen) == NSTEPS


def test_one_callback_per_cfl_substep():
    from test_cfl_gpu import DT as FRAME, _dam_break

    w, (fl,), _ = _dam_break().make_hip()
    force = RecordingField()
    fl.nonpressure_forces.append(force)
    w.set_cfl_substepping(2)
    nsub = []
    for _ in range(16):
        before = len(force.seen_dt)
        w.step(FRAME, GRAVITY)
        nsub.append(int(w.counters.nsubsteps))
        assert len(force.seen_dt) - before == nsub[-1] == w.device_force_stats()[0]
    print("substeps per step:", nsub)
    assert max(nsub) > 1  # (the collapsing column passes 0.4 * 2r / dt = 1.2 m/s within a few frames)


# ------------------------------------------------------------------------------------------------ misuse
def test_misuse_is_reported():
    pos, vel, floor = _scene()
    # the read-back helper only exists inside the device callback
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    w.add_fluid(Fluid(pos, R, 1000.0))
    w.step(DT, GRAVITY)
    buf = np.zeros(4, np.float32)
    assert w._L.salva_hip_device_view_read(w._h, buf.ctypes.data, buf.ctypes.data, 16) == _lib.E_INVALID
    # an entry without a callback
    desc = (_lib.ForceDesc * 1)()
    desc[0].kind = _lib.FORCE_DEVICE
    _lib.check(w._L.salva_hip_set_fluid_forces(w._h, 0, desc, 1))
    g = (C.c_float * 3)(0, -9.81, 0)
    assert w._L.salva_hip_step(w._h, DT, g, None) == _lib.E_INVALID
    assert b"salva_hip_set_device_force_callback" in w._L.salva_hip_last_error()
    desc[0].p[0] = 8.0  # not a sum of the three bits
    assert w._L.salva_hip_set_fluid_forces(w._h, 0, desc, 1) == _lib.E_INVALID

    # a callback that returns 1 aborts the step; the world is usable afterwards
    class Failing(DeviceForce):
        fail = True

        def solve_device(self, view):
            return 1 if self.fail else 0

    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    fl = Fluid(pos, R, 1000.0)
    bad = Failing()
    fl.nonpressure_forces.append(bad)
    h = w.add_fluid(fl)
    w.add_boundary(Boundary(floor))
    with pytest.raises(_lib.SalvaHipError) as e:
        w.step(DT, GRAVITY)
    assert e.value.code == _lib.E_INVALID
    bad.fail = False
    for _ in range(2):
        w.step(DT, GRAVITY)
    assert np.isfinite(h.positions).all() and w.device_force_stats()[0] == 1

    # stepping from inside the callback is refused, like every entry point that is not a getter of the local view
    class Reentrant(DeviceForce):
        def __init__(self, world):
            super().__init__(0)
            self.world, self.rc, self.n = world, None, None

        def solve_device(self, view):
            self.rc = self.world._L.salva_hip_step(self.world._h, DT, g, None)
            self.n = int(self.world._L.salva_hip_local_len(self.world._h))
            return 0

    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    fl = Fluid(pos, R, 1000.0)
    r = Reentrant(w)
    fl.nonpressure_forces.append(r)
    w.add_fluid(fl)
    w.step(DT, GRAVITY)
    assert r.rc == _lib.E_INVALID and r.n == len(pos)


def test_a_decomposed_world_refuses_the_kind():
    from salva_amd.dist import Comm

    pos, vel, floor = _scene()
    comms = Comm.loopback(1)
    try:
        # the force first, then the domain
        w = LiquidWorld(DFSPHSolver(), R, 2.0)
        fl = Fluid(pos, R, 1000.0)
        fl.nonpressure_forces.append(PluginForce(PLUGIN, "df3_field", 0, ORIGIN))
        w.add_fluid(fl)
        with pytest.raises(_lib.SalvaHipError) as e:
            w.set_domain(comms[0], -100, 100)
        assert e.value.code == _lib.E_INVALID
        # the domain first, then the force
        w = LiquidWorld(DFSPHSolver(), R, 2.0)
        w.add_fluid(Fluid(pos, R, 1000.0))
        w.set_domain(comms[0], -100, 100)
        desc = (_lib.ForceDesc * 1)()
        desc[0].kind = _lib.FORCE_DEVICE
        assert w._L.salva_hip_set_fluid_forces(w._h, 0, desc, 1) == _lib.E_INVALID
    finally:
        for c in comms:
            c.destroy()


def test_a_host_force_and_a_device_force_in_one_list():
    """[host CustomForceField, df3_field] on one fluid: both run at their places — twice the field of the oracle's single one is
    what the oracle computes with two callbacks."""
    pos, vel, floor = _scene()
    o = O.OracleWorld(R, 2.0, O.DFSPH)
    fo = o.add_fluid(pos, 1000.0, vel)

    def ofield(world, f, positions, velocities, densities, accelerations):
        accelerations += CustomForceField.field(ORIGIN, positions.astype(np.float32)).astype(np.float64)

    o.add_custom_force(fo, ofield)
    o.add_custom_force(fo, ofield)
    o.add_boundary(floor)
    for _ in range(NSTEPS):
        o.step(DT, GRAVITY)
    host, dev = CustomForceField(ORIGIN), RecordingField()
    w, h = _device_run([host, dev])
    assert host.calls == NSTEPS == len(dev.seen_dt)
    _assert_matches_oracle(h.positions, h.velocities, o.fluid_vec(fo, "positions"), o.fluid_vec(fo, "velocities"))
