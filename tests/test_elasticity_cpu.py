"""Becker2009Elasticity without a GPU: the numpy reading of becker2009_elasticity.rs (tests/elasticity_reading.py) checked against
what the force must do on simple bodies, and the new surface of the C header, the Python mirror and the C++ mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from elasticity_reading import ElasticityReading, coefficients, kernel_w, rest_contacts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_P = 0.025
H = R_P * 2.0 * 2.0


def block(ni, nj, nk, r=R_P):
    from salva_amd import scenes

    return scenes.cube_fluid_positions(ni, nj, nk, r).astype(np.float64)


def rot_matrix(axis, angle):
    u = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


@pytest.mark.parametrize("nonlinear", [False, True])
def test_body_at_rest_has_identity_rotations_no_stress_no_force(nonlinear):
    p = block(6, 5, 4)
    vol = np.full(len(p), 0.8 * (2 * R_P) ** 3)
    e = ElasticityReading(5e5, 0.3, nonlinear)
    a = e.step(H, p, vol, 1000.0)
    assert np.abs(e.rotations - np.eye(3)).max() == 0.0
    assert np.abs(e.stress).max() < 1e-9 * 5e5
    assert np.abs(a).max() < 1e-9


@pytest.mark.parametrize("nonlinear", [False, True])
def test_rigid_motion_gives_the_rotation_back_and_no_force(nonlinear):
    from salva_amd import scenes

    p0 = scenes.jitter(scenes.cube_fluid_positions(8, 6, 5, R_P), 0.1 * R_P).astype(np.float64)
    vol = np.full(len(p0), 0.8 * (2 * R_P) ** 3)
    e = ElasticityReading(5e5, 0.3, nonlinear)
    e.step(H, p0, vol, 1000.0)  # rest state
    Q = rot_matrix([0.3, -1.0, 0.5], 0.7)
    p = p0 @ Q.T + np.array([0.4, -0.2, 1.1])
    a = e.step(H, p, vol, 1000.0)
    assert np.abs(e.rotations - Q).max() < 1e-6
    assert np.abs(e.stress).max() < 1e-6 * 5e5
    assert np.abs(a).max() < 1e-4  # vs ~10 m/s^2 under a 1 % stretch


def test_three_particle_quirks():
    """Quirk 2: volumes0 = m / (2 sum_j m_j W_ij), self pair included; quirk 1: after a count change the kept entries add to
    their old value; quirk 3: the shear stress carries 0.564, not 0.5."""
    h = 1.0
    p = np.array([[0.0, 0.0, 0.0], [0.4, 0.0, 0.0], [0.0, 0.7, 0.0]])
    m = np.array([1.0, 2.0, 3.0])
    e = ElasticityReading(1000.0, 0.25, False)
    e.init(h, p, m)
    w = lambda a, b: float(kernel_w(np.linalg.norm(p[a] - p[b]), h))
    pairs = {0: [0, 1, 2], 1: [0, 1, 2], 2: [0, 1, 2]}
    assert np.linalg.norm(p[1] - p[2]) < h
    for i in range(3):
        s = sum(m[j] * w(i, j) for j in pairs[i])
        assert e.volumes0[i] == pytest.approx(m[i] / (2.0 * s), rel=1e-12)
    v_old = e.volumes0.copy()
    # one particle more: entries 0..2 keep their (inverted) values and the new sums are added to them
    p4 = np.vstack([p, [[5.0, 5.0, 5.0]]])
    m4 = np.append(m, 4.0)
    e.init(h, p4, m4)
    for i in range(3):
        s = sum(m[j] * w(i, j) for j in pairs[i])
        assert e.volumes0[i] == pytest.approx(m4[i] / (v_old[i] + 2.0 * s), rel=1e-12)
    assert e.volumes0[3] == pytest.approx(4.0 / (2.0 * 4.0 * float(kernel_w(0.0, h))), rel=1e-12)
    # quirk 3: a pure shear F = [[0, g], [0, 0]] gives sigma_xy = g * 0.564 * d2 in the linear strain
    d0, d1, d2 = coefficients(1000.0, 0.25)
    e2 = ElasticityReading(1000.0, 0.25, False)
    e2.init(h, p, m)
    q = p.copy()
    q[:, 0] += 0.05 * q[:, 1]  # x += 0.05 y
    e2.rotations_and_stresses(h, q, m)
    F = e2.grad_tr
    assert e2.stress[:, 3] == pytest.approx((F[:, 1, 0] + F[:, 0, 1]) * 0.564 * d2, rel=1e-12)
    assert e2.stress[:, 0] == pytest.approx(d0 * F[:, 0, 0] + d1 * F[:, 1, 1] + d1 * F[:, 2, 2], rel=1e-12, abs=1e-12)


def test_rest_contacts_are_symmetric_and_include_self():
    p = block(5, 4, 3)
    off, j = rest_contacts(p.astype(np.float32), H)
    n = len(p)
    i = np.repeat(np.arange(n), np.diff(off))
    assert set(zip(i.tolist(), j.tolist())) == set(zip(j.tolist(), i.tolist()))
    assert all(k in j[off[k]:off[k + 1]] for k in range(n))
    assert all((np.diff(j[off[k]:off[k + 1]]) > 0).all() for k in range(n))


def test_header_declares_the_force_and_its_state():
    src = open(os.path.join(ROOT, "include", "salva_hip.h")).read()
    assert "SALVA_HIP_FORCE_BECKER2009 = 8" in src
    assert "salva_hip_get_elasticity_state(" in src and "salva_hip_set_elasticity_state(" in src
    from salva_amd import _lib

    assert _lib.FORCE_BECKER2009 == 8
    assert {"salva_hip_get_elasticity_state", "salva_hip_set_elasticity_state"} <= set(_lib.EXPORTED_SYMBOLS)


def test_python_mirror_fills_the_descriptor():
    import salva_amd

    d = salva_amd.Becker2009Elasticity(5e5, 0.3, True)._desc()
    assert d.kind == 8
    assert list(d.p)[:5] == [5e5, pytest.approx(0.3), 1.0, 0.0, 0.0]
    d = salva_amd.Becker2009Elasticity(1e5, 0.25, False, kernel_density=salva_amd.Poly6Kernel,
                                       kernel_gradient=salva_amd.SpikyKernel)._desc()
    assert list(d.p)[:5] == [1e5, 0.25, 0.0, 1.0, 2.0]


def test_cpp_mirror_compiles_with_the_force():
    with tempfile.NamedTemporaryFile("w", suffix=".cpp", delete=False) as f:
        f.write('#include "%s"\nint main() { salva::Becker2009Elasticity e(5e5f, 0.3f, true); '
                'salva::Becker2009ElasticityT<salva::Poly6Kernel, salva::SpikyKernel> t(1e5f, 0.3f, false); '
                'SalvaHipForceDesc d = e.desc(), q = t.desc(); return (d.kind == SALVA_HIP_FORCE_BECKER2009 && q.p[4] == 2.0f) ? 0 : 1; }\n'
                % os.path.join(ROOT, "include", "salva_hip.hpp"))
        path = f.name
    try:
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", path])
    finally:
        os.unlink(path)
