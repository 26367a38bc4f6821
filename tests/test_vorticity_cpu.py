"""Vorticity confinement without a GPU: closed cases of tests/vorticity_reading.py, its f32 mode inside the derived
bounds against its f64 mode on the scenes of tests/force_cases.py, three wrong readings that the same bounds reject, and the numbers
the header, salva_amd._lib and the three mirrors agree on."""
import functools
import os
import re

import numpy as np
import pytest

import force_cases as FC
import vorticity_reading as VR
from force_reading import Snapshot
from numpy_reading import pair_tables, spline_dw
from salva_amd import VorticityConfinement, _lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, H = 0.025, 0.1
EPS, KAPPA = 0.1, 0.05


def _snapshot(x, v, m=None, rho=None, kernels=("cubic", "cubic")):
    """one fluid, no boundary; rho: the SPH density of the positions unless given"""
    x = np.asarray(x, np.float64)
    n = len(x)
    m = np.full(n, 1000.0 * 0.8 * (2 * R) ** 3) if m is None else m
    if rho is None:
        mask, w, _ = pair_tables(x, x, H, *kernels)
        rho = (w * m[None, :]).sum(axis=1)
    none = np.zeros((0, 3))
    return Snapshot(x, v, m, rho, np.zeros(n, np.int64), [1000.0], np.zeros((n, 3)), none, none, np.zeros(0), np.zeros(0, np.int64), H,
                    kernels, 0.005, 200.0)


def test_rigid_rotation_on_a_lattice():
    """(a) v = Omega x x on an unjittered 9^3 lattice: every particle whose full neighbourhood is present (two lattice steps from every
    face: the contacts reach exactly h along the axes) has omega_i = 2 Omega s_i with s_i = -(sum_j m_j r_ij W'(r_ij)) / (3 rho_i) — the
    cubic symmetry turns sum_j f(r_ij) r_ij r_ij^T into a multiple of the identity — to f64 rounding; eta_i = 0 to rounding there (the
    neighbours that carry a gradient are one step away and have the same n), so no force."""
    idx = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    x = (idx - 4) * (2.0 * R)  # (in f64: the f32 lattice of scenes.cube_fluid_positions is symmetric to 1e-8 only)
    Om = np.array([0.3, -1.1, 0.7])
    s = _snapshot(x, np.cross(Om, x))
    r = VR.read(s, 0, EPS, KAPPA, f32_contacts=False)
    full = ((idx >= 2) & (idx <= 6)).all(axis=1)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    # (the six pairs at h along the axes are in or out of the lists as the coordinates round; they carry no gradient)
    assert full.sum() == 125 and ((d < 0.99 * H).sum(axis=1)[full] == 27).all() and (r.contacts[full] >= 27).all()
    s_i = -(np.where(d <= H, s.m[None, :] * d * spline_dw(d, H), 0.0)).sum(axis=1) / (3.0 * s.rho)
    want = 2.0 * Om[None, :] * s_i[:, None]
    err = np.abs(r.omega[full] - want[full]).max() / np.abs(want[full]).max()
    print("rigid rotation: s = %.6f (1 in the continuum), omega - 2 Omega s = %.1e of it" % (s_i[full][0], err))
    assert 0.5 < s_i[full][0] < 1.5 and err < 1e-12
    top = r.n[full].max()
    assert np.abs(r.eta[full]).max() * H <= 1e-12 * top                      # (eta is a gradient: n / h is its scale)
    assert np.abs(r.acc[full]).max() <= 1e-10 * EPS * top                    # kappa n / h in the denominator: 1e-12 / kappa
    assert np.abs(r.acc[~full]).max() > 1e-3 * EPS * top                     # the block's skin does feel a gradient of n
    # the hard normalisation would turn that rounding noise into a unit vector: what kappa is for
    assert VR.read(s, 0, EPS, 0.0, f32_contacts=False).D[full].max() * H <= 1e-12 * top


def test_uniform_translation_adds_nothing_exactly():
    """(b) v_i - v_j = 0 exactly: omega = 0, D = 0 and nothing is added anywhere, surface included, in f64 and in f32, kappa or none"""
    x = scenes.jitter(scenes.cube_fluid_positions(7, 7, 7, R), 0.1 * R, seed=5).astype(np.float64)
    v = np.tile(np.float32([0.3, -0.2, 0.9]).astype(np.float64), (len(x), 1))
    for f32 in (False, True):
        for kappa in (KAPPA, 0.0):
            r = VR.read(_snapshot(x, v), 0, EPS, kappa, f32=f32)
            assert not r.omega.any() and not r.n.any() and not r.eta.any() and not r.D.any() and not r.acc.any()
            assert np.isfinite(r.acc).all()


def lamb_oseen_block(nx, ny, nz, seed=7):
    x = scenes.jitter(scenes.cube_fluid_positions(nx, ny, nz, R), 0.1 * R, seed=seed).astype(np.float64)
    centre = 0.5 * (x.min(axis=0) + x.max(axis=0))
    return x, (centre[0], centre[2])


def test_lamb_oseen_column_is_spun_up():
    """(c) a Lamb-Oseen column along y on a jittered block: |omega| falls away from the axis, eta points at it, N x omega is along
    the swirl.  The force's power sum_i m_i a_i . v_i is positive, and its tangential component is positive for the particles between
    one and two core radii (every one of them).  This fixes every sign: of the curl, of eta, of the force's cross product."""
    core = 0.1
    x, c = lamb_oseen_block(11, 5, 11)
    v = VR.lamb_oseen(x, c, 0.5, core)
    s = _snapshot(x, v)
    r = VR.read(s, 0, EPS, KAPPA)
    power = float((s.m[:, None] * r.acc * v).sum())
    rad = np.stack([x[:, 0] - c[0], np.zeros(len(x)), x[:, 2] - c[1]], axis=1)
    dist = np.sqrt((rad ** 2).sum(axis=1))
    tangent = np.cross([0.0, 1.0, 0.0], rad / dist[:, None])
    ring = (dist >= core) & (dist <= 2 * core)
    a_t = (r.acc * tangent).sum(axis=1)
    print("Lamb-Oseen: power %.3e W, omega_y on the axis %.2f (continuum %.2f), tangential a in the ring: min %.3e mean %.3e of eps |omega| = %.3e"
          % (power, r.omega[np.argmin(dist), 1], 0.5 / (np.pi * core ** 2), a_t[ring].min(), a_t[ring].mean(), EPS * r.n[ring].mean()))
    assert ring.sum() >= 100 and power > 0 and (a_t[ring] > 0).all()
    assert (r.omega[ring, 1] > 0).all()                        # the curl of a rotation about +y points along +y
    assert ((r.eta * rad).sum(axis=1)[ring] < 0).all()         # |omega| grows towards the axis


def test_isolated_particle_and_coincident_pair():
    """(d) finite, zero: a particle with no neighbour, and two at one point (zero gradient) whatever their velocities"""
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    v = np.array([[1.0, 2.0, 3.0], [0.5, 0.0, 0.0], [-0.5, 0.3, 0.0]])
    for f32 in (False, True):
        for kappa in (KAPPA, 0.0):
            r = VR.read(_snapshot(x, v), 0, EPS, kappa, f32=f32)
            for a in (r.omega, r.n, r.eta, r.D, r.acc):
                assert np.isfinite(a).all() and not a.any()
            assert np.isfinite(r.b_acc).all()  # (not zero: the bound is in units of G_max, whatever the pair's own gradient)
    assert list(r.contacts) == [1, 2, 2]


# ---------------------------------------------------------------------------------------------------- the scenes of force_cases.py
SCENES = {"A": ("A", 0), "A2": ("A2", 0), "B0": ("B", 0), "B1": ("B", 1)}


@functools.lru_cache(maxsize=None)
def _snapshots(name):
    """the state a recording custom force saw in the f32 build of the CPU oracle at the compared steps: values an f32 implementation
    can hold, so that both modes of the reading start from the same numbers"""
    scene, target = SCENES[name]
    case = FC.Case("%s-vorticity" % name, scene, ("cubic", "cubic"), target, ())
    sc, steps, _ = FC.run_oracle(case, False)
    return [FC.oracle_snapshot(case, sc, steps[step][0]) for step in FC.COMPARED], target


@functools.lru_cache(maxsize=None)
def _f64(name, k):
    snaps, target = _snapshots(name)
    return VR.read(snaps[k], target, EPS, KAPPA)


def _fractions(got, ref):
    """worst |got - ref| / bound over the rows, for omega, eta and the acceleration (rows whose bound is zero must agree exactly)"""
    out = {}
    for key, b in (("omega", ref.b_omega), ("eta", ref.b_eta), ("acc", ref.b_acc)):
        dev = np.abs(getattr(got, key).astype(np.float64) - getattr(ref, key)).max(axis=1)
        assert (dev[b == 0] == 0).all(), key
        out[key] = float((dev[b > 0] / b[b > 0]).max())
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_f32_mode_stays_inside_the_bounds(name):
    """every row, omega, eta and the acceleration; the worst fraction of each bound is printed"""
    snaps, target = _snapshots(name)
    for k, s in enumerate(snaps):
        ref = _f64(name, k)
        assert ref.rows.sum() == len(FC.SCENES[SCENES[name][0]]()["fluids"][target]["pos"])
        worst = {}
        for seed in (1, 2):
            for key, f in _fractions(VR.read(s, target, EPS, KAPPA, f32=True, seed=seed), ref).items():
                worst[key] = max(worst.get(key, 0.0), f)
        top = np.abs(ref.acc).max()
        print("%s step %d: max |omega| %.3g, max |a| %.3g, median bound on a %.2e of it; f32 - f64 as a fraction of the bound: omega %.3f, "
              "eta %.3f, a %.3f" % (name, FC.COMPARED[k] + 1, ref.n.max(), top, np.median(ref.b_acc[ref.rows]) / top, worst["omega"],
                                     worst["eta"], worst["acc"]))
        assert top > 0 and max(worst.values()) <= 1.0
        # the bounds mean something: nine rows in ten are held to a hundredth of the largest acceleration or better
        assert np.quantile(ref.b_acc[ref.rows], 0.9) <= 1e-2 * top


@pytest.mark.parametrize("mutation", VR.MUTATIONS)
@pytest.mark.parametrize("name", list(SCENES))
def test_a_wrong_reading_leaves_the_bound(name, mutation):
    """the opposite sign of the cross product; eta without the - n_i term; m_j / rho_i for m_j / rho_j in pass 2"""
    snaps, target = _snapshots(name)
    for k, s in enumerate(snaps):
        ref = _f64(name, k)
        wrong = VR.read(s, target, EPS, KAPPA, mutation=mutation)
        dev = np.abs(wrong.acc - ref.acc).max(axis=1)
        out = int((dev > ref.b_acc).sum())
        print("%s step %d %s: %d of %d rows leave the bound, the worst by a factor %.3g" % (
            name, FC.COMPARED[k] + 1, mutation, out, ref.rows.sum(), (dev[ref.b_acc > 0] / ref.b_acc[ref.b_acc > 0]).max()))
        assert out > 0


# ---------------------------------------------------------------------------------------------------- numbers and mirrors
def _text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_lib_and_mirrors_agree():
    header = _text("include", "salva_hip.h")
    assert re.search(r"SALVA_HIP_FORCE_VORTICITY_CONFINEMENT = 10\b", header) and re.search(r"SALVA_HIP_FIELD_VORTICITY = 8\b", header)
    assert _lib.FORCE_VORTICITY_CONFINEMENT == 10 and _lib.FIELD_VORTICITY == 8
    d = VorticityConfinement(0.25)._desc()
    assert d.kind == 10 and list(d.p) == [0.25, np.float32(0.05), 0.0, 0.0, 0.0, 0.0, 0.0]
    d = VorticityConfinement(0.5, 0.0)._desc()
    assert d.kind == 10 and list(d.p) == [0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    hpp = _text("include", "salva_hip.hpp")
    assert re.search(r"struct VorticityConfinement : NonPressureForce", hpp)
    assert re.search(r"VorticityConfinement\(Real strength_, Real kappa_ = \(Real\)0\.05\)", hpp)
    assert re.search(r"SalvaHipForceDesc d\{SALVA_HIP_FORCE_VORTICITY_CONFINEMENT, \{strength, kappa\}\};", hpp)
    assert "SALVA_HIP_FIELD_VORTICITY" in hpp
    ffi = _text("bindings", "rust", "salva3d-hip", "src", "ffi.rs")
    assert "pub const SALVA_HIP_FORCE_VORTICITY_CONFINEMENT: i32 = 10;" in ffi and "pub const SALVA_HIP_FIELD_VORTICITY: i32 = 8;" in ffi
    rs = _text("bindings", "rust", "salva3d-hip", "src", "liquid_world.rs")
    assert re.search(r"pub struct VorticityConfinement", rs) and "kappa: 0.05" in rs
    assert re.search(r"ffi::SALVA_HIP_FORCE_VORTICITY_CONFINEMENT, \[self\.strength, self\.kappa, 0\.0, 0\.0, 0\.0, 0\.0, 0\.0\]", rs)
    assert "ffi::SALVA_HIP_FIELD_VORTICITY" in rs
