"""Becker2009Elasticity on the device (salva_amd/csrc/elastic.hip) against the numpy reading of becker2009_elasticity.rs
(tests/elasticity_reading.py): the rest state, one rotation / stress pass from the device's own inputs, one whole step against the
reading running as a host force, count changes, the state's lifetime through the API, chained steps, checkpoints, and the
behaviour of a block dropped on a floor."""
import numpy as np
import pytest

import salva_amd
from elasticity_reading import ElasticityReading, rest_contacts
from salva_amd import Boundary, DFSPHSolver, Fluid, IISPHSolver, LiquidWorld, XSPHViscosity, _lib, scenes

pytestmark = pytest.mark.gpu

R = 0.025
H = 4 * R
DT = 1.0 / 200.0
G = (0.0, -9.81, 0.0)
KIND = {"cubic": salva_amd.CubicSplineKernel, "poly6": salva_amd.Poly6Kernel, "spiky": salva_amd.SpikyKernel}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def elastic_block(ni=12, nj=6, nk=12, lift=0.0, jitter=0.05, seed=42):
    p = scenes.cube_fluid_positions(ni, nj, nk, R)
    if jitter:
        p = scenes.jitter(p, jitter * R, seed=seed)
    p = p.astype(np.float32)
    p[:, 1] += np.float32(lift)
    return p


def world_with(blocks, solver=None, floor=True, forces=None):
    w = LiquidWorld(solver or DFSPHSolver(), R, 2.0)
    fl = []
    for k, p in enumerate(blocks):
        f = Fluid(p, R, 1000.0)
        for force in (forces[k] if forces else [salva_amd.Becker2009Elasticity(5e5, 0.3, True)]):
            f.nonpressure_forces.append(force)
        fl.append(w.add_fluid(f))
    if floor:
        w.add_boundary(Boundary(scenes.plane_lattice(60, 60, -0.4, R, -1.5, -1.5)))
    return w, fl


def reading_rest(p, vol, h=H, kd=0):
    e = ElasticityReading(5e5, 0.3, True, kernel_density=kd)
    e.init(h, p.astype(np.float64), np.asarray(vol, np.float64) * 1000.0)
    return e


# ------------------------------------------------------------------------------------------------ 1. rest state
@pytest.mark.parametrize("uniform", [True, False])
def test_rest_state_matches_the_reading(uniform):
    p = elastic_block()
    w, (f,) = world_with([p])
    if not uniform:
        vol = (0.8 * (2 * R) ** 3 * (1.0 + 0.2 * scenes.lcg_uniform(len(p), 7))).astype(np.float32)
        f.volumes = vol
    vol = np.asarray(f.volumes, np.float64)
    p_before = f.positions.copy()
    w.step(DT, G)
    st = w.elasticity_state(f)
    assert np.array_equal(st["positions0"], p_before)
    off, j = rest_contacts(p_before, H)
    doff, dj = w.elasticity_contacts(f)
    assert st["ncontacts0"] == len(j)
    assert np.array_equal(np.diff(doff), np.diff(off)) and np.array_equal(dj, j)  # every row, pair by pair
    e = reading_rest(p_before, vol)
    assert rel(st["volumes0"], e.volumes0) < 1e-6


def test_rest_state_of_the_two_block_scene():
    blocks = [elastic_block(jitter=0.0, lift=0.55), elastic_block(jitter=0.0, lift=0.85)]
    w, fl = world_with(blocks, forces=[[salva_amd.Becker2009Elasticity(5e5, 0.3, True), XSPHViscosity(0.5, 1.0)],
                                       [salva_amd.Becker2009Elasticity(1e5, 0.3, True), XSPHViscosity(0.5, 1.0)]])
    before = [f.positions.copy() for f in fl]
    w.step(DT, G)
    for f, p in zip(fl, before):
        st = w.elasticity_state(f)
        off, j = rest_contacts(p, H)
        doff, dj = w.elasticity_contacts(f)
        assert st["ncontacts0"] == len(j) and np.array_equal(np.diff(doff), np.diff(off)) and np.array_equal(dj, j)
        assert rel(st["volumes0"], reading_rest(p, f.volumes).volumes0) < 1e-6


# ------------------------------------------------------------------------------------------------ 2. one pass from the same input
@pytest.mark.parametrize("nonlinear,kd,kg", [(False, "cubic", "cubic"), (True, "cubic", "cubic"), (True, "poly6", "spiky")])
def test_rotations_stresses_and_gradients_from_the_device_inputs(nonlinear, kd, kg):
    p = elastic_block(10, 6, 8)
    force = salva_amd.Becker2009Elasticity(5e5, 0.3, nonlinear, kernel_density=KIND[kd], kernel_gradient=KIND[kg])
    w, (f,) = world_with([p], forces=[[force]], floor=False)
    f.velocities = scenes.random_velocities(len(p), 0.5, seed=3)
    for _ in range(20):
        w.step(DT, (0.0, 0.0, 0.0))
    st0 = w.elasticity_state(f)
    pos = f.positions.copy()
    vol = np.asarray(f.volumes, np.float64)
    w.step(DT, (0.0, 0.0, 0.0))
    st1 = w.elasticity_state(f)
    e = ElasticityReading(5e5, 0.3, nonlinear, kernel_density=KIND[kd].kind, kernel_gradient=KIND[kg].kind)
    e.positions0 = st0["positions0"].astype(np.float64)
    e.volumes0 = st0["volumes0"].astype(np.float64)
    e.rotations = st0["rotations"].astype(np.float64)
    e.set_lists(H)
    e.rotations_and_stresses(H, pos.astype(np.float64), vol * 1000.0)
    assert np.abs(st1["rotations"] - e.rotations).max() < 1e-4
    assert rel(st1["grad_tr"], e.grad_tr) < 1e-4
    assert rel(st1["stress"], e.stress) < 1e-4


# ------------------------------------------------------------------------------------------------ 3. device against host
@pytest.mark.parametrize("solver", [DFSPHSolver, IISPHSolver])
@pytest.mark.parametrize("nonlinear", [False, True])
def test_one_step_device_force_against_the_reading_as_a_host_force(solver, nonlinear):
    """One step of the same world with the force native and with the reading as a host force, from a DEFORMED state: both worlds
    take the rest state at step 1 (where the force is zero), the random velocities deform the block, and step 3 is compared —
    there the reading's accelerations are tens of m/s^2, and a world without the force differs."""
    p = elastic_block(10, 6, 8)
    v0 = scenes.random_velocities(len(p), 0.5, seed=5)
    host = _HostElastic(5e5, 0.3, nonlinear)
    out = []
    for force in (salva_amd.Becker2009Elasticity(5e5, 0.3, nonlinear), host, None):
        w, (f,) = world_with([p], solver=solver(), forces=[[force] if force else []])
        f.velocities = v0
        w.step(DT, G)
        w.step(DT, G)
        out.append([f.positions.copy()])
        v = f.velocities.copy()
        w.step(DT, G)
        out[-1] += [f.velocities - v, f.positions.copy()]
    assert np.abs(out[0][0] - out[1][0]).max() < 1e-5 * R  # the same state before the compared step (up to f32 rounding)
    assert np.abs(host.e.accelerations(np.full(len(p), 0.8 * (2 * R) ** 3), 1000.0)).max() > 1.0  # m/s^2 on step 3's state
    assert rel(out[0][1], out[1][1]) < 1e-5
    assert np.abs(out[0][2] - out[1][2]).max() < 1e-5 * R
    assert np.abs(out[2][1] - out[0][1]).max() > 1e3 * np.abs(out[0][1] - out[1][1]).max()  # the force is what is compared


class _HostElastic(salva_amd.NonPressureForce):
    def __init__(self, E, nu, nl):
        self.e = ElasticityReading(E, nu, nl)

    def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
        self.e.solve(timestep, kernel_radius, ff, fb, fluid, boundaries, densities)


# ------------------------------------------------------------------------------------------------ 5. count changes
def test_count_changes_reinitialise_with_the_reference_quirks():
    p = elastic_block(8, 6, 8)
    w, (f,) = world_with([p], floor=False)
    c = p.mean(0)
    f.velocities = np.cross(np.float32([0.0, 20.0, 0.0]), p - c).astype(np.float32)  # a spin: rotations far from I
    e = ElasticityReading(5e5, 0.3, True)
    for _ in range(5):
        pos, vol = f.positions.copy(), np.asarray(f.volumes, np.float64)
        w.step(DT, (0.0, 0.0, 0.0))
        e.step(H, pos.astype(np.float64), vol, 1000.0)
    before = w.elasticity_state(f)
    assert np.abs(before["rotations"] - np.eye(3)).max() > 0.3
    for k in (3, 50, 200):
        f.delete_particle_at_next_timestep(k)
    w.sync_to_device()
    # between the count change and the next step the state keeps its old length and contents (the reference resizes in init)
    pend = w.elasticity_state(f)
    assert len(pend["volumes0"]) == len(p)
    for k in ("positions0", "volumes0", "rotations"):
        assert np.array_equal(pend[k], before[k])
    ck = w.checkpoint()  # a checkpoint across the pending change carries the old-length state
    assert len(ck["fluid0_force0_volumes0"]) == len(p)
    pos, vol = f.positions.copy(), np.asarray(f.volumes, np.float64)
    w.step(DT, (0.0, 0.0, 0.0))
    e.step(H, pos.astype(np.float64), vol, 1000.0)
    st = w.elasticity_state(f)
    assert len(st["volumes0"]) == len(p) - 3
    assert rel(st["volumes0"], e.volumes0) < 1e-6
    assert np.array_equal(st["positions0"], pos)
    e_after_delete_volumes0 = e.volumes0.copy()
    # the rotations of the re-initialised state against the reading's (warm-started by index from the old ones, new = I)
    assert np.abs(st["rotations"] - e.rotations).max() < 1e-4
    f.add_particles(np.array([[1.0, 1.0, 1.0], [1.02, 1.0, 1.0]], np.float32))
    w.sync_to_device()
    pos, vol = f.positions.copy(), np.asarray(f.volumes, np.float64)
    w.step(DT, (0.0, 0.0, 0.0))
    e.step(H, pos.astype(np.float64), vol, 1000.0)
    st = w.elasticity_state(f)
    assert rel(st["volumes0"], e.volumes0) < 1e-6
    assert np.abs(st["rotations"] - e.rotations).max() < 1e-4
    # the checkpoint taken across the pending change: restored, the next step re-initialises from the old length as above
    w2, (f2,) = world_with([p], floor=False)
    w2.restore(ck)
    w2.step(DT, (0.0, 0.0, 0.0))
    st2 = w2.elasticity_state(f2)
    assert len(st2["volumes0"]) == len(p) - 3 and rel(st2["volumes0"], e_after_delete_volumes0) < 1e-6


# ------------------------------------------------------------------------------------------------ 6. plumbing
def _drop(monkeypatch, env, nsteps=30):
    for k in ("SALVA_HIP_NO_CHAIN",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    w, (f,) = world_with([elastic_block(8, 6, 8, lift=-0.2)],
                         forces=[[salva_amd.Becker2009Elasticity(5e5, 0.3, True), XSPHViscosity(0.5, 1.0)]])
    chained = []
    for _ in range(nsteps):
        w.step(DT, G)
        chained.append(w.counters.chained_passes)
    return w, f, chained


def test_chained_steps_are_bit_identical_and_chain(monkeypatch):
    w0, f0, c0 = _drop(monkeypatch, {"SALVA_HIP_NO_CHAIN": "1"})
    w1, f1, c1 = _drop(monkeypatch, {})
    assert np.array_equal(f0.positions, f1.positions) and np.array_equal(f0.velocities, f1.velocities)
    assert np.array_equal(w0.elasticity_state(f0)["rotations"], w1.elasticity_state(f1)["rotations"])
    assert c0[-1] == 0
    assert c1[0] == 0 and c1[-1] > 0


def test_every_step_after_the_first_chains(monkeypatch):
    """Only the step that builds the rest state takes the plain path: a free block (no impact to break a chain) chains exactly
    when the same world without the force does, which is every step from the third on."""
    monkeypatch.delenv("SALVA_HIP_NO_CHAIN", raising=False)
    p = elastic_block(8, 6, 8)
    w, (f,) = world_with([p], floor=False, forces=[[salva_amd.Becker2009Elasticity(5e5, 0.3, True), XSPHViscosity(0.5, 1.0)]])
    f.velocities = scenes.random_velocities(len(p), 0.2, seed=9)
    wx, (fx,) = world_with([p], floor=False, forces=[[XSPHViscosity(0.5, 1.0)]])
    fx.velocities = f.velocities
    counts, plain = [], []
    for _ in range(20):
        w.step(DT, (0.0, 0.0, 0.0))
        wx.step(DT, (0.0, 0.0, 0.0))
        counts.append(w.counters.chained_passes)
        plain.append(wx.counters.chained_passes)
    # the world without the force does not chain its second step either (the first step's solves set what the chain decides on)
    assert counts == plain, (counts, plain)
    assert all(b == a + 1 for a, b in zip(counts[1:], counts[2:])), counts


def test_checkpoint_restore_carries_the_elastic_state():
    """The rest state and the rotations travel with the checkpoint.  NOT bit for bit, unlike what was first asked: the fluid's own
    restart is not (a restored world sorts its cells from host order, the running one from the last step's order, so the neighbour
    sums of the solver add in another sequence: tests/test_parity_gpu.py::test_checkpoint_restart_continues_the_run).  The elastic
    state itself comes back exactly; the run then follows the original to the same restart bounds."""
    mk = lambda: world_with([elastic_block(8, 6, 8, lift=-0.1)])
    wa, (fa,) = mk()
    for _ in range(10):
        wa.step(DT, G)
    ck = wa.checkpoint()
    wb, (fb,) = mk()
    wb.restore(ck)
    for _ in range(5):
        wa.step(DT, G)
        wb.step(DT, G)
    sa, sb = wa.elasticity_state(fa), wb.elasticity_state(fb)
    assert np.array_equal(sa["positions0"], sb["positions0"]) and np.array_equal(sa["volumes0"], sb["volumes0"])
    assert sa["ncontacts0"] == sb["ncontacts0"]
    assert np.abs(sa["rotations"] - sb["rotations"]).max() < 1e-4
    assert np.abs(fa.positions - fb.positions).max() < 1e-6 * R * 5
    # without the elastic state the restarted block takes its CURRENT shape as its rest shape: visibly different
    wc, (fc,) = mk()
    wc.restore({k: v for k, v in ck.items() if "_force" not in k})
    for _ in range(5):
        wc.step(DT, G)
    assert not np.array_equal(wc.elasticity_state(fc)["positions0"], sa["positions0"])


def test_state_lifetime_through_the_api():
    a, b = elastic_block(8, 6, 8), elastic_block(6, 6, 6, lift=0.6)
    w, (fa, fb) = world_with([a, b], forces=[[XSPHViscosity(0.5, 0.0)], [salva_amd.Becker2009Elasticity(5e5, 0.3, True)]])
    w.step(DT, G)
    p0 = w.elasticity_state(fb)["positions0"].copy()
    w.step(DT, G)
    w.remove_fluid(fa)  # swap-remove: the block moves into slot 0 and takes its state along
    w.step(DT, G)
    assert np.array_equal(w.elasticity_state(fb)["positions0"], p0)
    fb.nonpressure_forces.append(XSPHViscosity(0.5, 1.0))  # appending keeps entry 0 as it was
    w.step(DT, G)
    assert np.array_equal(w.elasticity_state(fb)["positions0"], p0)
    fb.nonpressure_forces[0] = salva_amd.Becker2009Elasticity(4e5, 0.3, True)  # another E: a fresh state
    cur = fb.positions.copy()
    w.step(DT, G)
    assert np.array_equal(w.elasticity_state(fb)["positions0"], cur)


def test_a_decomposed_world_rejects_the_force():
    from salva_amd import dist

    p = elastic_block(8, 6, 8)
    w, (f,) = world_with([p], floor=False)
    comm = dist.Comm.loopback(1)[0]
    cx = dist.cell_x(p, H)
    with pytest.raises(_lib.SalvaHipError):
        w.set_domain(comm, int(cx.min()), int(cx.max()), 0)
        w.step(DT, G)


# ------------------------------------------------------------------------------------------------ 7. behaviour
def _extent(p):
    return p.max(0) - p.min(0)


@pytest.mark.parametrize("elastic", [True, False])
def test_a_dropped_block_keeps_its_shape_only_with_the_force(elastic):
    p = elastic_block(10, 10, 10, jitter=0.0, lift=0.0)
    forces = [[salva_amd.Becker2009Elasticity(5e5, 0.3, True), XSPHViscosity(0.5, 1.0)] if elastic else [XSPHViscosity(0.5, 1.0)]]
    w, (f,) = world_with([p], forces=forces)
    rest = _extent(p)
    for _ in range(300):
        w.step(DT, G)
    ext = _extent(f.positions)
    assert np.isfinite(f.positions).all()
    if elastic:
        assert (np.abs(ext - rest) <= 0.15 * rest).all(), (ext, rest)
    else:
        assert ext[0] > 1.5 * rest[0], (ext, rest)
