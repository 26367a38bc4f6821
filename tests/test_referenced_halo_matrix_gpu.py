"""The referenced-only halo (test_referenced_halo_gpu.py) in every path that reads the tile tables: each case runs twice, with
SALVA_HIP_FULL_HALO=1 and with SALVA_HIP_REF_HALO=1, and the two runs must agree bit for bit (ref_halo_ab.ab: positions, velocities,
densities, contact counts, boundary forces, the per-step iteration / contact trace, the fullest box, the exported lists of the
first, second and last step, entry by entry).  Every case asserts that the second arm kept the referenced slots in EVERY step and
dropped a slot in some step; the cases where World::size_pass declines by design are in DECLINES and assert the opposite.

Which builder runs: k_nbr_tile_ref<M> (grid.hip) is the V = 1 builder with the compaction behind it; launch_nbr_build takes it for
every slot of a step that keeps the referenced halo — the slots of a cut tile (SALVA_HIP_SPLIT_S) included: a cut tile is a slot
with fewer cell planes, staged, compacted and ranked like any other.  The V = 0 builder serves worlds with more than 32 models
only, and those decline."""
import hashlib
import threading

import numpy as np
import pytest

from parity import DT, GRAVITY, Scene
from ref_halo_ab import OFF, ON, R, _bench_block, _info, _same, _same_exports, ab, check_switch, report, same_tree, switches
from salva_amd import (Becker2009Elasticity, Boundary, DFSPHSolver, Fluid, IISPHSolver, LiquidWorld, NonPressureForce, XSPHViscosity, dist,
                       scenes)

pytestmark = pytest.mark.gpu

# Cases in which `ref_step` (World::size_pass) is false by design, with the term of its condition they rest on.  No other case may
# assert info[9] == 0 in the kept arm.
DECLINES = {
    "speculative_first_pass": "!spec  (a speculative pass clamps its tables to the previous step's totals; the repeated pass of a miss keeps)",
    "more_than_32_models": "c.nmodels <= 32u && c.nbmodels <= 32u  (the bit-mask group tests of the V = 1 builder hold 32 models)",
}


def _tank_scene(nx, ny, nz, solver="dfsph", parts=1, densities=(1000.0,), forces=(("xsph", 0.5, 0.0),), wants_forces=False, seed=11, stir=0.2):
    """A jittered block in a tank, cut into `parts` fluids along x (one density0 and one force list each, cycled)."""
    s = Scene(R, 2.0, solver)
    fluid, shell = scenes.tank(nx, ny, nz, R)
    fluid = scenes.jitter(fluid, 0.1 * R, seed=seed)
    vel = scenes.random_velocities(len(fluid), stir, seed=4)
    groups = np.array_split(np.argsort(fluid[:, 0], kind="stable"), parts)  # (equal counts: no part is empty)
    per_part = isinstance(forces[0][0], tuple)
    for k in range(parts):
        sel = np.sort(groups[k])
        s.add_fluid(np.ascontiguousarray(fluid[sel]), np.ascontiguousarray(vel[sel]), densities[k % len(densities)],
                    forces=list(forces[k % len(forces)] if per_part else forces))
    s.add_boundary(shell, wants_forces=wants_forces)
    return s


def _viscous_block():
    """golden_scenes.scene_dfsph_viscous, 12 x 10 x 10: barely perturbed (the force diverges on rougher lattices in the reference itself)."""
    s = Scene(R, 2.0, "dfsph")
    pos = scenes.jitter(scenes.cube_fluid_positions(12, 10, 10, R), 0.02 * R, seed=42)
    vel = scenes.random_velocities(len(pos), 0.01, seed=12345)
    vel[:, 0] += np.float32(2.0) * pos[:, 1]
    s.add_fluid(pos, vel, 1000.0, forces=[("dfsph_viscosity", 0.6)])
    return s


# ---- 1. forces and reactions: the force lists of golden_scenes.SCENES on blocks large enough to drop a slot
FORCES = {
    "artificial_wants_forces": (lambda: _tank_scene(14, 14, 14, forces=(("artificial", 1.0, 0.5),), wants_forces=True), 12),
    "dfsph_viscosity": (_viscous_block, 4),
    "he2014_wcsph_iisph": (lambda: _tank_scene(16, 12, 14, solver="iisph", parts=2, densities=(1000.0, 800.0),
                                               forces=((("he2014", 1.0, 0.5),), (("wcsph_tension", 0.3, 0.0),)), wants_forces=True), 10),
    "akinci_xsph_dfsph": (lambda: _tank_scene(14, 14, 14, forces=(("xsph", 0.5, 0.2), ("akinci", 1.0, 10.0))), 12),
    "akinci_xsph_iisph_wants_forces": (lambda: _tank_scene(14, 14, 14, solver="iisph", forces=(("xsph", 0.5, 0.2), ("akinci", 1.0, 10.0)),
                                                           wants_forces=True), 10),
    "two_phase_wants_forces": (lambda: _tank_scene(16, 14, 14, parts=2, densities=(1000.0, 500.0), wants_forces=True), 10),
    "four_phase": (lambda: _tank_scene(16, 12, 16, parts=4, densities=(1000.0, 800.0, 600.0, 400.0), wants_forces=True), 10),
}


@pytest.mark.parametrize("case", sorted(FORCES))
def test_forces_and_reactions(case):
    """boundary.forces included, bit for bit: the step sums the reaction forces in fixed point (StepCtx::bforce_fx), so the sum does
    not depend on the order in which the atomics land.  (With float atomics the two arms differed by 8e-8 ... 2.3e-7 of the largest
    force in the five cases whose boundary wants its forces, and so did two runs of one build.)"""
    make, nsteps = FORCES[case]
    ab("forces/" + case, make(), nsteps)


# ---- 2. kernel pairings
@pytest.mark.parametrize("solver", ["dfsph", "iisph"])
@pytest.mark.parametrize("kernels", [("poly6", "spiky"), ("spiky", "viscosity")])
def test_kernel_pairings(solver, kernels):
    s = _bench_block(14, solver=solver)
    s.kernels = kernels
    ab(f"kernels/{solver}/{kernels[0]}+{kernels[1]}", s, 10)


# ---- 3. masses: three and four densities, general kernels (the default holds two masses) and the *_multi layouts
@pytest.mark.parametrize("max_masses", [None, "4"])
@pytest.mark.parametrize("nmass", [3, 4])
def test_three_and_four_masses(nmass, max_masses):
    s = _tank_scene(16, 12, 14, parts=nmass, densities=(1000.0, 800.0, 600.0, 400.0)[:nmass])
    ab(f"masses/{nmass}/max_masses={max_masses}", s, 10, env={"SALVA_HIP_MAX_MASSES": max_masses} if max_masses else {})


# ---- 4. launch shapes
SHAPES = {
    "split_700": (lambda: _bench_block(16), {"SALVA_HIP_SPLIT_S": "700"}),
    "split_260": (lambda: _bench_block(16), {"SALVA_HIP_SPLIT_S": "260"}),
    "light_class_with_strays": (lambda: _bench_block(14, strays=40), {"SALVA_HIP_LIGHT": "1", "SALVA_HIP_CLASSES": "1"}),
    # pairs.h pick_ds / pick_ds_p3 / pick_ds_p2: level k takes the k-th larger layout; 3 and beyond is the unbounded one
    "ds_level_1": (lambda: _bench_block(14), {"SALVA_HIP_DS_LEVEL": "1"}),
    "ds_level_2": (lambda: _bench_block(14), {"SALVA_HIP_DS_LEVEL": "2"}),
    "ds_level_3": (lambda: _bench_block(14), {"SALVA_HIP_DS_LEVEL": "3"}),
}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_launch_shapes(case):
    make, env = SHAPES[case]
    out = ab("shapes/" + case, make(), 10, env=env)
    if case == "light_class_with_strays":
        assert int(out[1][0].counters.sparse_class_passes) > 0  # (the classes did run beside the kept halo)


# ---- 5. host protocol
PROTOCOL = {"default": {}, "no_chain": {"SALVA_HIP_NO_CHAIN": "1"}, "no_pregrid": {"SALVA_HIP_NO_PREGRID": "1"},
            "no_defer_lists": {"SALVA_HIP_NO_DEFER_LISTS": "1"}}


@pytest.mark.parametrize("case", sorted(PROTOCOL))
def test_host_protocol(case):
    """NO_DEFER_LISTS sizes the kept halo exactly in every step (no bound, nothing to miss); the others predict it from the previous
    step's maxima plus a margin, which a settled block never outgrows: no pass is repeated either way."""
    out = ab("protocol/" + case, _bench_block(14), 20, env=PROTOCOL[case])
    assert int(out[1][5][-1][11]) == 0, out[1][5][-1]
    c = out[1][0].counters
    print("chained passes", int(c.chained_passes), "pre-enqueued grids adopted", int(c.pregrid_adopted))


def test_a_speculative_pass_declines_and_its_repeated_pass_keeps():
    """DECLINES["speculative_first_pass"].  SALVA_HIP_SPECULATE=1: a step whose speculative pass held staged the full box; a step
    whose speculative pass missed (or that could not speculate: the first) ran an exact pass, which keeps.  Per step, from the counters."""
    sc = _bench_block(14)
    runs = []
    for arm in (OFF, ON):
        with switches(dict(arm, SALVA_HIP_SPECULATE="1")):
            w, fls, _ = sc.make_hip()
        trace, infos, held = [], [], []
        for k in range(20):
            s0, d0 = int(w.counters.speculative_passes) if k else 0, int(w.counters.discarded_passes) if k else 0
            st = w.step(DT, GRAVITY)
            trace.append((st.n_divergence_iters, st.n_pressure_iters, int(st.ncontacts), int(st.reserved[0])))
            infos.append(_info(w))
            held.append(int(w.counters.speculative_passes) > s0 and int(w.counters.discarded_passes) == d0)
        runs.append((w, fls, trace, infos, held))
    (w0, f0, t0, i0, h0), (w1, f1, t1, i1, h1) = runs
    print("speculative passes that held:", sum(h1), "of", len(h1), "kept passes:", int(i1[-1][10]))
    assert all(int(i[9]) == 0 for i in i0)
    assert sum(h1) >= 1, h1  # the scene does speculate
    assert [int(i[9]) for i in i1] == [0 if h else 1 for h in h1], ([int(i[9]) for i in i1], h1)
    assert t1 == t0 and h1 == h0
    _same(w1, f1, w0, f0)
    assert int(w1.counters.discarded_passes) == int(w0.counters.discarded_passes)


def test_more_than_32_models_decline():
    """DECLINES["more_than_32_models"]: a world takes at most 32 fluids, so the term that can be true is the boundaries': a tank
    whose shell is 33 boundaries."""
    s = Scene(R, 2.0, "dfsph")
    fluid, shell = scenes.tank(14, 14, 14, R)
    fluid = scenes.jitter(fluid, 0.1 * R, seed=11)
    s.add_fluid(fluid, scenes.random_velocities(len(fluid), 0.2, seed=4), 1000.0, forces=[("xsph", 0.5, 0.0)])
    for part in np.array_split(np.arange(len(shell)), 33):
        s.add_boundary(np.ascontiguousarray(shell[part]))
    ab("declines/33_boundaries", s, 4, declined=True)


@pytest.mark.parametrize("solver,mode", [("dfsph", 1), ("dfsph", 2), ("iisph", 1)])
def test_cfl_substeps_build_their_lists_several_times_per_step(solver, mode):
    """The dam break of test_cfl_gpu.py (frame-sized steps), wider: every substep builds (and compacts) its own tables."""
    s = Scene(R, 2.0, solver)
    fluid, shell = scenes.tank(14, 18, 14, R, wall_cells=10)
    s.add_fluid(scenes.jitter(fluid, 0.05 * R, seed=42), None, 1000.0, forces=[("xsph", 0.5, 0.0)])
    s.add_boundary(shell)
    nsub = []
    # (a collapsing column under frame-sized steps: a kept halo may outgrow the previous substep's maximum plus an eighth — such a
    # pass is repeated, and counted)
    out = ab(f"protocol/cfl/{solver}/{mode}", s, 14, dt=1.0 / 60.0, may_miss=True, prepare=lambda w, f, b: w.set_cfl_substepping(mode),
             extra=lambda w, f, b: (nsub.append(len(w.substeps())), w.substeps())[1])
    assert max(nsub) > 1, nsub  # the scene really sub-steps
    assert int(out[1][5][-1][10]) > 14  # more kept builds than steps


# ---- 6. edits between steps
def _edit_sequence(state):
    """One seeded, fixed sequence of host edits, applied after the named steps to both arms."""
    rng_seed = 1234

    def between(k, w, fls, bds):
        rng = np.random.default_rng(rng_seed + k)
        f = w.fluids()._items[0]
        if k == 1:  # add_particles: a small block above the fluid
            p = np.array(f.positions)
            blk = scenes.cube_fluid_positions(5, 4, 5, R) + np.float32([p[:, 0].mean(), p[:, 1].max() + 4 * R, p[:, 2].mean()])
            f.add_particles(blk.astype(np.float32))
        elif k == 3:  # delete_particle_at_next_timestep
            for i in rng.choice(f.num_particles(), 60, replace=False):
                f.delete_particle_at_next_timestep(int(i))
        elif k == 5:  # delete k and add k in one gap: n unchanged
            p = np.array(f.positions)
            doomed = rng.choice(f.num_particles(), 64, replace=False)
            for i in doomed:
                f.delete_particle_at_next_timestep(int(i))
            blk = scenes.cube_fluid_positions(4, 4, 4, R) + np.float32([p[:, 0].min() + 6 * R, p[:, 1].max() + 4 * R, p[:, 2].min() + 6 * R])
            f.add_particles(blk.astype(np.float32))
        elif k == 7:  # a fluid swapped for one of equal size: the same particles, squeezed by 3 % about their centre (denser halos)
            p, v = np.array(f.positions), np.array(f.velocities)
            c = p.mean(axis=0)
            g = Fluid(((p - c) * np.float32(0.97) + c).astype(np.float32), R, 1000.0)
            g.velocities = v
            g.nonpressure_forces.append(XSPHViscosity(0.5, 0.0))
            w.remove_fluid(f)
            w.add_fluid(g)
        elif k == 9:  # a host edit of positions: a clump moves several tiles away, n unchanged
            p = np.array(f.positions)
            clump = np.argsort(p[:, 0] + p[:, 1] + p[:, 2])[-300:]
            p[clump] += np.float32([0.0, 1.2, 0.0])
            f.positions = p
        elif k == 11:  # boundary add
            p = np.array(f.positions)
            lid = scenes.plane_lattice(10, 10, float(np.percentile(p[:, 1], 90)) + 3 * R, R, float(p[:, 0].min()), float(p[:, 2].min()))
            state["lid"] = w.add_boundary(Boundary(lid.astype(np.float32)))
        elif k == 12:  # boundary move
            b = state["lid"]
            b.positions = (np.array(b.positions) + np.float32([2 * R, 0.0, 2 * R])).astype(np.float32)
        elif k == 13:  # boundary remove
            w.remove_boundary(state.pop("lid"))
        elif k == 14:
            state["old"] = w.checkpoint()
        elif k == 16:  # checkpoint -> restore into the same world two steps later is the OLDER state of equal n
            w.restore(state["old"])
    return between


def test_edits_between_steps():
    """add / delete / delete-and-add / swap / teleport / boundary add, move, remove / restore of an older checkpoint of equal n.
    Every one of them goes through World::upload_tables, which clears `lists_checked`: the step after an edit waits for its list
    statistics in the middle of the step and sizes the kept halo EXACTLY (defer_lists is false), so the stale prediction
    (ref_pred_valid && ref_pred_n == n) is never consulted and no pass is repeated — pinned: info[11] == 0 to the end."""
    state = {}
    out = ab("edits", _bench_block(14), 20, prepare=lambda w, f, b: state.clear(), between=_edit_sequence(state))
    i1 = out[1][5]
    print("edits: repeated passes per step:", [int(i[11]) for i in i1])
    assert int(i1[-1][11]) == 0, [int(i[11]) for i in i1]


def test_restore_into_a_fresh_world_in_both_arms():
    """checkpoint() of a full-box world after 6 steps -> a fresh world per arm -> restore() -> 8 more steps."""
    sc = _bench_block(14)
    with switches(OFF):
        w, fls, _ = sc.make_hip()
    for _ in range(6):
        w.step(DT, GRAVITY)
    ck = w.checkpoint()
    ab("edits/restore_fresh", sc, 8, prepare=lambda w2, f, b: w2.restore(ck))


# ---- 7. mid-step and after-step readers
class _Reader(NonPressureForce):
    """Adds nothing; hashes what a callback can pull in the middle of the step."""

    def __init__(self, world):
        self.world, self.h, self.calls = world, hashlib.sha1(), 0

    def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
        w = self.world[0]
        lv = w.local_view()
        for key in ("ids", "fluid_slots", "positions", "velocities", "densities", "volumes"):
            self.h.update(np.ascontiguousarray(lv[key]).tobytes())
        for boundary in (False, True):
            off, jm, j = w.local_contacts(boundary)
            assert int(off[-1]) == len(j) > 0
            for a in (off, jm, j):
                self.h.update(np.ascontiguousarray(a).tobytes())
        for a in (ff.offsets, ff.j_model, ff.j, fb.offsets, fb.j_model, fb.j):
            self.h.update(np.ascontiguousarray(a).tobytes())
        self.calls += 1


def test_a_force_callback_sees_the_same_lists_in_the_middle_of_the_step():
    sc = _bench_block(14)
    digests = []

    def prepare(w, fls, bds):
        rd = _Reader([w])
        fls[0].nonpressure_forces.append(rd)
        digests.append(rd)

    ab("readers/callback", sc, 8, prepare=prepare)
    assert digests[0].calls == digests[1].calls == 8
    assert digests[0].h.hexdigest() == digests[1].h.hexdigest()


def test_host_xsph_over_the_exported_contacts_of_a_kept_halo_equals_the_device_kernel():
    """test_custom_force_gpu.py's check under SALVA_HIP_REF_HALO=1, on a block large enough to drop slots, with that test's bounds."""
    from test_dist_gpu import _HostXsph

    class HXsph(_HostXsph, NonPressureForce):
        pass

    out = []
    for arm, forces in ((ON, [XSPHViscosity(0.4, 0.0)]), (ON, [HXsph(0.4)]), (OFF, [HXsph(0.4)])):
        sc = _bench_block(14, forces=())
        with switches(arm):
            w, (fl,), _ = sc.make_hip()
        fl.nonpressure_forces += forces
        infos = []
        for _ in range(3):
            w.step(DT, GRAVITY)
            infos.append(_info(w))
        if arm is ON:
            assert all(int(i[9]) == 1 for i in infos) and any(int(i[5]) < int(i[8]) for i in infos), infos
        else:
            assert all(int(i[9]) == 0 for i in infos), infos
        out.append((fl.positions.copy(), fl.velocities.copy()))
    # the host force over the lists exported from compacted tables: the same bits as over the full box's
    assert np.array_equal(out[1][0], out[2][0]) and np.array_equal(out[1][1], out[2][1])
    dp, dv = np.abs(out[0][0] - out[1][0]).max(), np.abs(out[0][1] - out[1][1]).max()
    print("host XSPH vs device under the kept halo: dp", dp, "dv", dv)
    assert dp < 1e-6 * R * 30
    assert dv < 2e-5 * np.abs(out[0][1]).max()


def test_queries_after_a_kept_halo_step():
    def queries(w, fls, bds):
        p = np.array(fls[0].positions)
        mid = p.mean(axis=0)
        box = w.particles_intersecting_aabb(mid - 0.15, mid + np.float32([0.1, 0.2, 0.15]))
        ball = w.particles_intersecting_shape(tuple(mid), (0.0, 0.0, 0.0, 1.0), ("ball", 0.18))
        return [sorted((k, i) for k, _, i in box), sorted((k, i) for k, _, i in ball)]

    out = ab("readers/queries", _bench_block(14), 6, extra=queries)
    assert len(out[1][6][-1][-1][0]) > 50 and len(out[1][6][-1][-1][1]) > 50


def test_an_elastic_block_beside_a_fluid():
    """Becker2009 elasticity keeps lists of its own (the rest neighbours); the fluid beside it goes through the tile tables."""
    def scene():
        s = Scene(R, 2.0, "dfsph")
        fluid, shell = scenes.tank(22, 12, 12, R)
        fluid = scenes.jitter(fluid, 0.05 * R, seed=9)
        left = fluid[:, 0] < np.median(fluid[:, 0])
        s.add_fluid(np.ascontiguousarray(fluid[left]), None, 1000.0, forces=[("xsph", 0.5, 0.0)])
        s.add_fluid(np.ascontiguousarray(fluid[~left]), None, 1000.0)
        s.add_boundary(shell)
        return s

    def prepare(w, fls, bds):
        fls[1].nonpressure_forces.append(Becker2009Elasticity(5e5, 0.3, True))

    def state(w, fls, bds):
        es = w.elasticity_state(fls[1], 0)
        return [es["rotations"], es["stress"]]

    ab("readers/elastic", scene(), 10, prepare=prepare, extra=state)


# ---- 8. coupling
def _coupled(name, build, nsteps, step):
    """build() -> (w, fluid, bounds, coupling, bodies); step(k, w, bounds, coupling, bodies) runs one coupled step.  The full-box
    arm runs twice: the first thing checked is that the reference build reproduces ITSELF on this scene.
    With float atomics a scene with a dynamic body did not: the wrench's last bits move the body, the body moves the boundary
    particles, the fluid follows.  With the fixed-point sums (StepCtx::bforce_fx) it does, and that is asserted."""
    runs = []
    for arm in (OFF, OFF, ON):
        with switches(arm):
            w, fl, bounds, coupling, bodies = build()
        trace, infos, forces = [], [], []
        for k in range(nsteps):
            st = step(k, w, bounds, coupling, bodies)
            trace.append((st.n_divergence_iters, st.n_pressure_iters, int(st.ncontacts), int(st.reserved[0])))
            infos.append(_info(w))
            forces.append([np.array(b.forces) if b.wants_forces and b.forces is not None else None for b in bounds] +
                          [np.array(b.positions) for b in bounds] + [(np.array(x.linvel), np.array(x.angvel)) for x in bodies])
        runs.append((w, fl, trace, infos, forces, [w.fluid_contacts(fl), w.fluid_contacts(fl, True)]))
    a, a2, b = runs
    itself = a[2] == a2[2] and np.array_equal(a[1].positions, a2[1].positions) and same_tree(a[4], a2[4])
    print(name, "the full-box arm reproduces itself:", itself)
    assert itself, "two runs of the full-box arm differ: boundary forces are no longer summed order-independently"
    report(name, fl.num_particles(), b[3])
    check_switch(a[3], b[3])
    assert b[2] == a[2]
    _same(b[0], [b[1]], a[0], [a[1]])
    _same_exports([b[5]], [a[5]])
    assert same_tree(b[4], a[4]), "boundary forces / sampled points / body velocities differ"


def test_static_sampled_bodies_under_the_kept_halo():
    """The raft / paddle / wall scene of test_coupling_gpu.py under a block of side 14."""
    import test_coupling_gpu as T
    from salva_amd import _lib
    from salva_amd.coupling import ColliderCouplingSet, RigidBody, StaticSampling

    def build():
        _, _, raft_pts, paddle_pts, wall_pts, raft, paddle = T._scene()
        pos = scenes.jitter(scenes.cube_fluid_positions(14, 14, 14, R), 0.05 * R, seed=11)
        pos[:, 1] += np.float32(14 * R + 3 * R)
        w = LiquidWorld(DFSPHSolver(), R, 2.0)
        fl = Fluid(pos, R, 1000.0)
        fl.velocities = scenes.random_velocities(len(pos), 0.05, seed=12)
        fl.nonpressure_forces.append(XSPHViscosity(0.5, 0.5))
        h = w.add_fluid(fl)
        coupling = ColliderCouplingSet()
        bounds = [w.add_boundary(Boundary(np.zeros((0, 3), np.float32))) for _ in range(3)]
        paddle.translation = np.float32([0.0, 14 * R, 0.0])
        coupling.register_coupling(bounds[0], "raft", raft, StaticSampling(raft_pts))
        coupling.register_coupling(bounds[1], "paddle", paddle, StaticSampling(paddle_pts))
        coupling.register_coupling(bounds[2], "wall", None, StaticSampling(wall_pts))
        return w, h, bounds, coupling, [raft, paddle]

    static = RigidBody(translation=np.float32([0.35, 0.0, 0.0]))

    def step(k, w, bounds, coupling, bodies):
        w.sync_to_device()
        coupling.update_boundaries(w)
        pose = static.pose()
        pose.has_body = 0
        _lib.check(w._L.salva_hip_update_boundary_pose(w._h, bounds[2]._slot, pose))
        st = w.step(DT, GRAVITY)
        coupling.transmit_forces(w, DT)
        for body in bodies:
            body.integrate(DT, (0.0, 0.0, 0.0))
        return st

    _coupled("coupling/static", build, 10, step)


@pytest.mark.parametrize("case", ["moving_ball_dfsph", "moving_ball_iisph", "cylinder+capsule", "host_shape"])
def test_dynamic_contact_sampling_under_the_kept_halo(case):
    """The boundary set changes every step: the moving-ball scene and the cylinder + capsule scene of test_dynamic_sampling_gpu.py,
    and the arm whose geometry calls come back to the host (test_host_shape_gpu.py)."""
    import test_dynamic_sampling_gpu as T
    import test_host_shape_gpu as HS

    def build():
        if case == "host_shape":
            pos, vel, slab, ball = HS._scene()
            w, h, bounds, c = HS._world(pos, vel, slab, ball, host=True)
            return w, h, bounds, c, [ball]
        pos, vel, slab, ball = T._calm_scene() if case.startswith("moving_ball") else T._scene()
        w, h, bounds, c = T._hip_world("iisph" if case.endswith("iisph") else "dfsph", pos, vel, slab, ball,
                                       shapes="cylinder+capsule" if case == "cylinder+capsule" else "cuboid+ball")
        return w, h, bounds, c, [ball, slab]

    def step(k, w, bounds, coupling, bodies):
        if case == "host_shape":
            st = w.step_with_coupling(DT, GRAVITY, coupling)
        else:
            T._hip_pose(w, coupling, bounds, bodies[1])
            st = w.step(DT, GRAVITY)
            coupling.transmit_forces(w, DT)
        bodies[0].integrate(DT, (0.0, 0.0, 0.0))
        return st

    _coupled("coupling/" + case, build, 10, step)


# ---- 9. decomposed worlds over the loopback transport
H = R * 2.0 * 2


def _dist_scene(nx=40, ny=12, nz=12, seed=5):
    pos, bpos = scenes.tank(nx, ny, nz, R, wall_cells=4)
    pos = scenes.jitter(pos, 0.1 * R, seed)
    vel = scenes.random_velocities(len(pos), 0.5, seed + 1)
    vel[:, 0] += 2.0  # the block drifts towards +x: particles change owner during the test
    return pos.astype(np.float32), vel.astype(np.float32), bpos.astype(np.float32)


def _run_ranks(env, nranks, nsteps, pos, vel, bpos, solver="dfsph", two_fluids=False, setup=None, between=None, slabs=None):
    """`nranks` in-process ranks (a daemon thread and a world each) as in test_dist_gpu.run_slabs; per rank: owned(), the per-step
    (divergence, pressure) iterations, the tile-table info of every step, and whatever `setup` / `between` leave in the rank's dict.
    The switches are set before the threads start and restored after the last one has joined."""
    cx = dist.cell_x(pos, H)
    slabs = slabs or dist.split_slabs(cx, nranks)
    owner = dist.owner_of(cx, slabs)
    comms = dist.Comm.loopback(nranks)
    parts = [np.arange(len(pos))]
    if two_fluids:
        upper = pos[:, 1] > np.median(pos[:, 1])
        parts = [parts[0][~upper], parts[0][upper]]
    counts = [sum(int((owner[p] == r).sum()) for p in parts) for r in range(nranks)]
    offsets = np.concatenate([[0], np.cumsum(counts)])
    res, errors = [dict() for _ in range(nranks)], [None] * nranks

    def rank_main(r):
        try:
            w = LiquidWorld(IISPHSolver() if solver == "iisph" else DFSPHSolver(), R, 2.0)
            fls = []
            for k, part in enumerate(parts):
                mine = part[owner[part] == r]
                f = Fluid(pos[mine], R, 1000.0 if k == 0 else 800.0)
                f.velocities = vel[mine]
                f.nonpressure_forces.append(XSPHViscosity(0.5, 0.3))
                fls.append(w.add_fluid(f))
            b = w.add_boundary(Boundary(bpos[dist.boundary_subset(bpos, H, slabs[r], r, nranks)]))
            st = res[r]
            st.update(w=w, fluids=fls, tank=b, slab=slabs[r], iters=[], infos=[], rank=r, nranks=nranks)
            if setup:
                setup(st)
            w.set_domain(comms[r], slabs[r][0], slabs[r][1], int(offsets[r]))
            for k in range(nsteps):
                if "pre" in st:
                    st["pre"](st)
                s = w.step(DT, GRAVITY)
                st["iters"].append((s.n_divergence_iters, s.n_pressure_iters, int(s.nparticles)))
                st["infos"].append(_info(w))
                if between and k + 1 < nsteps:
                    between(k, st)
            st["owned"] = w.owned()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors[r] = e

    with switches(env):
        threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(nranks)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
    for e in errors:  # a rank that raised leaves its peers waiting in the next exchange: report the cause first
        if e is not None:
            raise e
    assert not any(t.is_alive() for t in threads), "a rank hung"
    out = [dict(owned=st["owned"], iters=st["iters"], infos=st["infos"], extra=st.get("extra")) for st in res]
    for st in res:
        st.clear()  # (the worlds go before their communicators)
    for c in comms:
        c.destroy()
    return out


def _dist_ab(name, nranks, nsteps, scene=None, **kw):
    pos, vel, bpos = scene or _dist_scene()
    a = _run_ranks(OFF, nranks, nsteps, pos, vel, bpos, **kw)
    b = _run_ranks(ON, nranks, nsteps, pos, vel, bpos, **kw)
    for r in range(nranks):
        report(f"{name} rank {r}", len(b[r]["owned"][0]), b[r]["infos"])
        check_switch(a[r]["infos"], b[r]["infos"])
        assert a[r]["iters"] == b[r]["iters"], (r, a[r]["iters"], b[r]["iters"])
        for x, y in zip(a[r]["owned"], b[r]["owned"]):  # gids, positions, velocities, fluid slots: the rank's tile layout does not depend on the switch
            assert np.array_equal(x, y), f"rank {r}: owned() differs"
        assert same_tree(a[r]["extra"], b[r]["extra"]), f"rank {r}"
    for k in range(nsteps):
        assert len({x["iters"][k][:2] for x in b}) == 1, f"step {k}: the ranks disagree on iteration counts"
    return a, b


@pytest.mark.parametrize("nranks", [2, 3])
def test_slabs_dfsph_with_migration(nranks):
    pos, vel, bpos = _dist_scene()
    a, b = _dist_ab(f"dist/dfsph/{nranks}", nranks, 12, scene=(pos, vel, bpos))
    first = np.bincount(dist.owner_of(dist.cell_x(pos, H), dist.split_slabs(dist.cell_x(pos, H), nranks)), minlength=nranks)
    assert [len(x["owned"][0]) for x in b] != first.tolist(), "the scene was meant to exercise migration"


def test_slabs_two_fluids():
    _dist_ab("dist/two_fluids", 2, 10, two_fluids=True)


def test_slabs_iisph():
    _dist_ab("dist/iisph", 2, 10, solver="iisph")


def test_slabs_dynamic_sampling():
    from salva_amd.coupling import ColliderCouplingSet, DynamicContactSampling, RigidBody

    def setup(st):
        w = st["w"]
        empty = w.add_boundary(Boundary(np.zeros((0, 3), np.float32)))
        coupling = ColliderCouplingSet()
        body = RigidBody(translation=np.float32([0.02, 0.17, 0.01]), linvel=np.float32([-0.4, 0.1, 0.0]), angvel=np.float32([0.0, 0.5, 3.0]),
                         mass=5.0, principal_inertia=np.float32([0.03, 0.03, 0.03]))
        coupling.register_coupling(empty, "ball", body, DynamicContactSampling(("ball", 0.12)))
        st.update(ball=empty, coupling=coupling, extra=[])

        def pre(s):
            s["w"].sync_to_device()
            s["coupling"].update_boundaries(s["w"])  # (the body is not integrated: the same pose every step, on every rank)
        st["pre"] = pre

    def between(k, st):
        st["extra"].append([np.array(st["ball"].positions), np.array(st["ball"].velocities), [np.asarray(x) for x in st["ball"].sources()]])

    a, b = _dist_ab("dist/dynamic_sampling", 2, 10, setup=setup, between=between)
    assert len(b[0]["extra"][-1][0]) > 40, "the ball was meant to sit in the fluid"


def test_slabs_rebalance_recut():
    pos, vel, bpos = _dist_scene(nx=60)
    cx = dist.cell_x(pos, H)
    lo, hi = int(cx.min()), int(cx.max())
    span = hi - lo + 1
    slabs = [(lo, lo + span * 6 // 10 - 1), (lo + span * 6 // 10, lo + span * 8 // 10 - 1), (lo + span * 8 // 10, hi)]

    def between(k, st):
        if k % 2 == 1:
            w = st["w"]
            my = w.rebalance()
            w.remove_boundary(st["tank"])
            st["tank"] = w.add_boundary(Boundary(bpos[dist.boundary_subset(bpos, H, my, st["rank"], st["nranks"])]))
            st.setdefault("extra", []).append(my)

    a, b = _dist_ab("dist/rebalance", 3, 10, scene=(pos, vel, bpos), slabs=slabs, between=between)
    assert b[0]["extra"][0] != slabs[0], "the slabs were meant to be re-cut"


def test_slabs_collective_create_and_delete():
    pos, vel, bpos = _dist_scene()
    vel[:, 0] -= 2.0  # (no drift: the emitters stay above their ranks)
    cx = dist.cell_x(pos, H)
    slabs = dist.split_slabs(cx, 2)
    owner = dist.owner_of(cx, slabs)
    order = np.concatenate([np.nonzero(owner == r)[0] for r in range(2)])
    inv = np.empty(len(pos), np.int64)
    inv[order] = np.arange(len(pos))
    top, cut_x = pos[:, 1].max(), slabs[1][0] * H
    doomed = inv[np.nonzero((np.abs(pos[:, 0] - cut_x) < 1.1 * H) & (pos[:, 1] > np.median(pos[:, 1])))[0]].astype(np.uint32)
    assert len(doomed) >= 100

    def between(k, st):
        if k == 3:
            r = st["rank"]
            xm = 0.5 * (slabs[r][0] + slabs[r][1] + 1) * H
            blk = scenes.cube_fluid_positions(4, 3, 4, R) + np.float32([xm, top + 2 * H, pos[:, 2].mean()])
            st["w"].add_owned(st["fluids"][0], blk.astype(np.float32))
            st["extra"] = st["w"].delete_owned(doomed)

    a, b = _dist_ab("dist/create_delete", 2, 10, scene=(pos, vel, bpos), between=between)
    assert sum(len(x["owned"][0]) for x in b) == len(pos) + 2 * 48 - len(doomed)
