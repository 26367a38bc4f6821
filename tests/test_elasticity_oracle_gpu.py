"""Becker2009Elasticity: trajectories of the device force against the CPU checker stepping the same scenes with the numpy reading
(tests/elasticity_reading.py) as its host force (OracleWorld.add_custom_force), and one step of a 10^6-particle block from the
device's own state, transplant-style (tests/transplant.py): the checker's step from a checkpoint of the device world."""
import numpy as np
import pytest

import salva_amd
from elasticity_reading import ElasticityReading, rest_contacts
from oracle import oracle as O
from parity import max_norm_diff
from salva_amd import Boundary, DFSPHSolver, Fluid, IISPHSolver, LiquidWorld, XSPHViscosity, scenes
from transplant import oracle_threads

pytestmark = pytest.mark.gpu

R = 0.025
H = 4 * R
DT = 1.0 / 200.0
G = (0.0, -9.81, 0.0)
VOL = np.float32(R) * np.float32(R) * np.float32(R) * np.float32(6.4)  # Fluid::new's volume, as the device computes it


def _reading_force(e, nparticles):
    vol = np.full(nparticles, VOL, np.float64)

    def fn(world, f, positions, velocities, densities, accelerations):
        accelerations += e.step(H, np.array(positions, np.float64), vol, 1000.0)
    return fn


def _run_pair(blocks, young, solver, nsteps, xsph):
    """The device world and the checker, fluids in the same order with [elasticity, (XSPH)] each, a floor lattice at y = 0.2."""
    floor = scenes.plane_lattice(60, 60, 0.2, R, -1.5, -1.5)
    w = LiquidWorld(DFSPHSolver() if solver == O.DFSPH else IISPHSolver(), R, 2.0)
    o = O.OracleWorld(R, 2.0, solver, threads=oracle_threads())
    fl, fo = [], []
    for p, E in zip(blocks, young):
        f = Fluid(p, R, 1000.0)
        f.nonpressure_forces.append(salva_amd.Becker2009Elasticity(E, 0.3, True))
        if xsph:
            f.nonpressure_forces.append(XSPHViscosity(0.5, 1.0))
        fl.append(w.add_fluid(f))
        k = o.add_fluid(p, 1000.0)
        o.add_custom_force(k, _reading_force(ElasticityReading(E, 0.3, True), len(p)))
        if xsph:
            o.add_xsph(k, 0.5, 1.0)
        fo.append(k)
    w.add_boundary(Boundary(floor))
    o.add_boundary(floor)
    for _ in range(nsteps):
        w.step(DT, G)
        o.step(DT, G)
    return fl, fo, o


def _block(lift, jitter=0.0):
    p = scenes.cube_fluid_positions(12, 6, 12, R)
    if jitter:
        p = scenes.jitter(p, jitter * R, seed=11)
    p = p.astype(np.float32)
    p[:, 1] += np.float32(lift)
    return p


def _compare(fl, fo, o, nsteps):
    for f, k in zip(fl, fo):
        ref_p, ref_v = o.fluid_vec(k, "positions"), o.fluid_vec(k, "velocities")
        vref = max(float(np.abs(ref_v).max()), 2 * R / DT * 1e-2)
        assert max_norm_diff(f.positions, ref_p) < 1e-4 * R * nsteps
        assert max_norm_diff(f.velocities, ref_v) < 1e-4 * vref * nsteps


def test_elasticity3_dfsph_trajectory_against_the_checker():
    """examples3d/elasticity3.rs: two 12 x 6 x 12 blocks, E = 5e5 and 1e5, nu = 0.3, nonlinear, with XSPH(0.5, 1.0); 30 steps.
    The ground is a lattice at the top of elasticity3's cuboid (y = 0.2) instead of its contact sampling: the blocks start 0.4
    above it and do not reach it within the 30 steps, so the elastic force is what acts."""
    ground, r6 = 0.2, R * 6
    blocks = [_block(ground + r6 + 0.4), _block(ground + 4 * r6 + 0.4)]
    fl, fo, o = _run_pair(blocks, [5e5, 1e5], O.DFSPH, 30, True)
    _compare(fl, fo, o, 30)


def test_one_block_iisph_trajectory_against_the_checker():
    fl, fo, o = _run_pair([_block(0.2 + R * 6 + 0.05, jitter=0.1)], [5e5], O.IISPH, 20, False)
    _compare(fl, fo, o, 20)


def test_full_size_block_one_step_from_the_device_state():
    """10^6 particles: rest lists row by row against the reading, then one step of the checker + reading from a checkpoint of the
    device world (rest state, rotations and the fluid's state), held to the step-0 bounds."""
    side = 100
    p = scenes.jitter(scenes.cube_fluid_positions(side, side, side, R), 0.05 * R, seed=42).astype(np.float32)
    p[:, 1] -= p[:, 1].min() - np.float32(2 * R)
    vel = scenes.random_velocities(len(p), 0.05, seed=7)
    half = side * R + 4 * R
    nfl = int(2 * half / (2 * R)) + 1
    floor = scenes.plane_lattice(nfl, nfl, 0.0, R, -half, -half)
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    f = Fluid(p, R, 1000.0)
    f.velocities = vel
    f.nonpressure_forces.append(salva_amd.Becker2009Elasticity(5e5, 0.3, True))
    w.add_fluid(f)
    w.add_boundary(Boundary(floor))
    w.step(DT, G)  # takes the rest state (its force is zero)
    off, j = rest_contacts(p, H)
    doff, dj = w.elasticity_contacts(f)
    assert np.array_equal(np.diff(doff.astype(np.int64)), np.diff(off)), "rest-list lengths differ"
    assert np.array_equal(dj, j)
    ck = w.checkpoint()
    e = ElasticityReading(5e5, 0.3, True)
    e.positions0 = ck["fluid0_force0_positions0"].astype(np.float64)
    e.volumes0 = ck["fluid0_force0_volumes0"].astype(np.float64)
    e.rotations = ck["fluid0_force0_rotations"].astype(np.float64)
    e.off, e.j = off, j
    o = O.OracleWorld(R, 2.0, O.DFSPH, threads=oracle_threads())
    k = o.add_fluid(p, 1000.0, vel)
    o.add_custom_force(k, _reading_force(e, len(p)))
    o.add_boundary(floor)
    o.restore(ck)
    w.step(DT, G)
    o.step(DT, G)
    ref_p, ref_v = o.fluid_vec(k, "positions"), o.fluid_vec(k, "velocities")
    vref = max(float(np.abs(ref_v).max()), 2 * R / DT * 1e-2)
    assert max_norm_diff(f.positions, ref_p) < 1e-4 * R
    assert max_norm_diff(f.velocities, ref_v) < 1e-4 * vref
