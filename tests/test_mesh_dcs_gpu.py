"""ColliderSampling::DynamicContactSampling on a triangle mesh (salva_hip_set_boundary_dynamic_sampling_mesh; dcs.hip
k_dcs_project_mesh) against the host arm whose callbacks are the numpy reading (tests/mesh_reading.py) posed by the
same body: the scene of tests/test_host_shape_gpu.py, bit for bit after every step.  And the reduced heightfield3 scene: a boundary
sampled from the mesh on the device against the reading's points uploaded by hand."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_fixtures as X
import mesh_reading as M
import sampling_reading as R
from parity import DT, GRAVITY
from salva_amd import ArtificialViscosity, Boundary, DFSPHSolver, Fluid, LiquidWorld, XSPHViscosity, _lib, sampling, scenes
from salva_amd.coupling import ColliderCouplingSet, DynamicContactSampling, HostShapeSampling, RigidBody, StaticSampling
from test_host_shape_gpu import BALL_R, CUBOID_HE, R as RAD, _scene, to_local, to_world

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mesh_callbacks(body, v, t, normals, log=None):
    """`compute_aabb` (parry's Aabb::transform_by: the local box's centre posed, -+ |R| half_extents) and
    `project_point_and_get_feature` of the posed mesh, f32 as dcs.hip computes them."""
    lo, hi = M.mesh_aabb(v)
    centre, he = ((lo + hi) * F(0.5)).astype(F), ((hi - lo) * F(0.5)).astype(F)

    def aabb():
        i, j, k, w = (F(x) for x in body.rotation)
        ww, ii, jj, kk = w * w, i * i, j * j, k * k
        ij, wk, wj, ik, jk, wi = i * j * F(2), w * k * F(2), w * j * F(2), i * k * F(2), j * k * F(2), w * i * F(2)
        m = np.abs(np.array([[ww + ii - jj - kk, ij - wk, wj + ik], [wk + ij, ww - ii + jj - kk, jk - wi], [ik - wj, wi + jk, ww - ii - jj + kk]], F))
        ext = ((m[:, 0] * he[0] + m[:, 1] * he[1]) + m[:, 2] * he[2]).astype(F)
        c = to_world(body, centre[None])[0]
        return c - ext, c + ext

    def project(pts):
        proj, inside = M.mesh_project(v, t, normals, to_local(body, pts))
        if log is not None:
            log.append(int(inside.sum()))
        return to_world(body, proj), inside

    return aabb, project


def _world(pos, vel, colliders, host):
    """colliders: [(body, (v, t, oriented), log)]"""
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    fl = Fluid(pos, RAD, 1000.0)
    fl.velocities = vel
    fl.nonpressure_forces.append(XSPHViscosity(0.5, 0.5))
    h = w.add_fluid(fl)
    bounds = [w.add_boundary(Boundary(np.zeros((0, 3), F))) for _ in colliders]
    c = ColliderCouplingSet()
    for k, (body, (v, t, oriented), log) in enumerate(colliders):
        if host:
            c.register_coupling(bounds[k], k, body, HostShapeSampling(*mesh_callbacks(body, v, t, M.pseudo_normals(v, t) if oriented else None, log)))
        else:
            c.register_coupling(bounds[k], k, body, DynamicContactSampling(sampling.Mesh(v, t, oriented=oriented)))
    w.sync_to_device()
    _lib.check(w._L.salva_hip_set_timestep(w._h, DT, 1.0 / DT))  # (so that the prediction x + v dt is exercised from the first step)
    return w, h, bounds, c


def _compare(step, ha, hb, ba, bb):
    counts = []
    for k in range(len(ba)):
        na, nb = ba[k].num_particles(), bb[k].num_particles()
        assert na == nb, f"step {step} boundary {k}: {nb} points from the host arm vs {na}"
        _, pa = ba[k].sources()
        _, pb = bb[k].sources()
        assert np.array_equal(pa, pb), f"step {step} boundary {k}: different fluid particles were sampled"
        assert np.array_equal(ba[k].positions, bb[k].positions), f"step {step} boundary {k}: projections differ"
        assert np.array_equal(ba[k].velocities, bb[k].velocities), f"step {step} boundary {k}: velocities differ"
        counts.append(na)
    assert np.array_equal(ha.positions, hb.positions), f"step {step}: fluid positions differ"
    assert np.array_equal(ha.velocities, hb.velocities), f"step {step}: fluid velocities differ"
    return counts


def _slab_mesh():
    v, t, _ = X.cube()
    return (v * (F(2) * F(CUBOID_HE))).astype(F), t, True


def _tetra_mesh():
    v, t, _ = X.tetrahedron()
    return (v * F(BALL_R / 0.17)).astype(F), t, True


def test_oriented_meshes_match_the_host_arm_bit_for_bit():
    """(a) as the rotated slab, (e) moving and spinning where the ball was."""
    pos, vel, slab_a, body_a = _scene()
    _, _, slab_b, body_b = _scene()
    pushed = []
    wa, ha, ba, ca = _world(pos, vel, [(slab_a, _slab_mesh(), None), (body_a, _tetra_mesh(), None)], host=False)
    wb, hb, bb, cb = _world(pos, vel, [(slab_b, _slab_mesh(), pushed), (body_b, _tetra_mesh(), None)], host=True)
    most = [0, 0]
    for step in range(6):
        wa.step_with_coupling(DT, GRAVITY, ca)
        wb.step_with_coupling(DT, GRAVITY, cb)
        for body in (body_a, body_b):
            body.integrate(DT, (0.0, 0.0, 0.0))
        counts = _compare(step, ha, hb, ba, bb)
        most = [max(m, c) for m, c in zip(most, counts)]
    print("emitted (max per boundary)", most, "particles inside the slab per step", pushed)
    assert most[0] > 50 and most[1] > 50
    assert max(pushed) >= 1, "no particle was ever inside the slab: the push-out branch was not covered"


def test_a_height_field_samples_contacts_and_pushes_nothing():
    """(d) rising towards the block from below, not oriented: is_inside is false everywhere, so until the first emitted point the
    fluid is the fluid of a world without the collider, and afterwards the two arms still agree bit for bit."""
    pos, vel, _, _ = _scene()
    v, t, _ = X.heightfield9()
    v = (v * F([0.8, 0.04, 0.8])).astype(F)
    top = float(v[:, 1].max())
    gap = 1.5 * 0.1 + 0.025  # reach = 1.5 h, h = 4 r = 0.1: out of reach at first, in reach after three steps of 2 m/s
    start = F([0.0, float(pos[:, 1].min()) - gap - top, 0.0])
    mk = lambda: RigidBody(translation=start.copy(), linvel=F([0.0, 2.0, 0.0]), dynamic=False)  # noqa: E731
    body_a, body_b = mk(), mk()
    inside = []
    wa, ha, ba, ca = _world(pos, vel, [(body_a, (v, t, False), None)], host=False)
    wb, hb, bb, cb = _world(pos, vel, [(body_b, (v, t, False), inside)], host=True)
    wc, hc, _, cc = _world(pos, vel, [], host=False)
    counts = []
    for step in range(6):
        wa.step_with_coupling(DT, GRAVITY, ca)
        wb.step_with_coupling(DT, GRAVITY, cb)
        wc.step_with_coupling(DT, GRAVITY, cc)
        for body in (body_a, body_b):
            body.integrate(DT, (0.0, 0.0, 0.0))
        counts += _compare(step, ha, hb, ba, bb)
        if max(counts) == 0:
            assert np.array_equal(ha.positions, hc.positions) and np.array_equal(ha.velocities, hc.velocities), f"step {step}"
    print("emitted per step", counts, "inside per step (host arm)", inside)
    assert counts[0] == 0 and max(counts) > 50
    assert sum(inside) == 0


# ---------------------------------------------------------------------------------------------- the reduced heightfield3 scene
def test_heightfield_scene_from_mesh_equals_uploaded_samples():
    r = 0.15
    heights = X._heights(9, 12)
    scale = (6.0, 1.0, 6.0)
    v, t = M.heightfield_mesh(heights, scale)
    _, pts, _ = M.sample_mesh(v, t, r, R.SURFACE)
    pos = scenes.cube_fluid_positions(8, 8, 8, r)
    pos[:, 1] += F(1.0 + 8 * r + 0.5)
    res = []
    for from_mesh in (True, False):
        w = LiquidWorld(DFSPHSolver(), r, 2.0)
        fl = Fluid(pos, r, 1000.0)
        fl.velocities = np.tile(F([0.0, -10.0, 0.0]), (len(pos), 1))
        fl.nonpressure_forces.append(ArtificialViscosity(1.0, 0.0))
        h = w.add_fluid(fl)
        b = w.add_boundary(Boundary([]))
        c = ColliderCouplingSet()
        c.register_coupling(b, "ground", None, StaticSampling.from_shape(sampling.Mesh.heightfield(heights, scale)) if from_mesh else StaticSampling(pts))
        for _ in range(60):
            w.step_with_coupling(DT, GRAVITY, c)
        assert b.num_particles() == len(pts) > 0
        res.append((np.array(h.positions), np.array(h.velocities)))
    assert np.isfinite(res[0][0]).all() and np.isfinite(res[0][1]).all()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[0][0][:, 1].min() > -1.0, "the fluid fell through the height field"


def test_cpp_mirror_heightfield_example():
    """examples/heightfield3.cpp: the reference scene's parameters through include/salva_hip.hpp's `salva::Mesh`."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "heightfield3"], check=True, capture_output=True)
    out = subprocess.run([os.path.join(ROOT, "examples", "heightfield3"), "200"], check=True, capture_output=True, text=True, timeout=300).stdout
    m = re.search(r"(\d+) boundary samples", out)
    assert m and int(m.group(1)) > 1000, out
    box = re.search(r"fluid bounding box after 200 steps: \[([0-9.e+-]+), ([0-9.e+-]+), ([0-9.e+-]+)\] - \[([0-9.e+-]+), ([0-9.e+-]+), ([0-9.e+-]+)\]", out)
    assert box, out
    vals = [float(x) for x in box.groups()]
    assert np.isfinite(vals).all(), out
    assert vals[1] > -1.0, out  # nothing fell through the ground
