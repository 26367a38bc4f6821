"""A dense numpy reading of vorticity confinement (include/salva_hip.h, SALVA_HIP_FORCE_VORTICITY_CONFINEMENT): all
pairs, no grid, written from the header's contract and not from the kernels.  It takes a force_reading.Snapshot (the state a probe
in front of or behind the force recorded) and returns omega, n = |omega|, eta and the force's own accelerations, with the bound each
may be held to, per row.  The pair tables (contact mask, gradient) are tests/numpy_reading.py's.

  pass 1   omega_i = (sum_j m_j (v_i - v_j) x grad W_ij) / rho_i,   n_i = |omega_i|
  pass 2   eta_i = sum_j (m_j / rho_j) (n_j - n_i) grad W_ij
  force    D_i = |eta_i| + kappa n_i / h;   a_i = eps (eta_i / D_i) x omega_i, and nothing where D_i == 0

j runs over the fluid-fluid contacts of i inside the same fluid.  `f32=True` computes everything in float32 and sums every row in a
shuffled order: the distance between the two modes is the floor no f32 implementation can be asked to beat, and
tests/test_vorticity_cpu.py holds it to the bounds below.

The bounds are derived, not chosen.  u = 2^-24 is one rounding of an f32 operation relative to its result.  A sum of k terms computed
in f32 in any order may differ from the exact sum of the same inputs by at most (k + c) u A: k - 1 roundings of a partial sum below A,
and c for one term.  As in tests/field_reading.py, A is in units of the largest magnitude a term can take and not of the term itself,
because the cancellations inside a term (the kernel's (1 - q)^2, the two products of a cross product's component) are absolute: G_max is
the largest |dW/dr| of the world's gradient kernel on (0, h].  k is the row's number of same-fluid contacts (the self contact counted).

  omega   term = m_j (v_ij x grad W_ij), per component at most m_j |v_ij| G_max: A_i = sum_j m_j |v_ij| G_max / rho_i.  One term:
          grad W_ij as a vector costs 16 u G_max (three differences, r^2, the reciprocal root at 1 ulp, q, the polynomial:
          tests/field_reading.py); v_ij 1 u; a component of the cross product two products and a difference, 3 u of |v_ij| |grad W|;
          the product with m_j 1 u; the quotient by rho_i 1 u: 22, and C_OMEGA = 24 leaves two for second-order terms.
          n: |n' - n| <= |omega' - omega| <= sqrt(3) x the bound on a component, + 3 u n (three squares, two sums, halved by the root,
          the root).
  eta     term = V_j (n_j - n_i) grad W_ij with V_j = m_j / rho_j: A_i = sum_j V_j |n_j - n_i| G_max.  One term: 16 u for the gradient,
          1 u each for V_j, the difference and the two products: 20, C_ETA = 22.  The n that enter are themselves only known within
          their bound b_n: first-order propagation adds sum_j V_j (b_n,j + b_n,i) |grad W_ij|, with the gradient's actual magnitude.
          Fed the omega of the implementation under test (`omega=`), b_n is 3 u n alone: the two sources of error are seen apart.
  a       with E = sqrt(3) x the bound on a component of eta, as a vector, and k' = kappa / h (one more rounding):
            |dD| <= E + k' b_n + 4 u D                    (squares, sums, root, the product, the sum)
            |dN| <= (E + |dD|) / (D - |dD|) + 4 u         (N = eta / D, |N| <= 1: d(eta / D) = d eta / D' - eta dD / (D D'))
            |da| <= eps (|dN| n + |d omega|) + 6 u eps n  (as a vector; the cross product, the product with eps)
          and never more than 2 eps (n + b_n) (1 + 8 u): |N| <= 1 bounds both values themselves.  That cap is what holds where D - |dD|
          <= 0 — where the reading cannot tell D from zero the numerator is within rounding of zero too.  D in the denominator is the
          point of kappa: the bound is small where the force is not rounding noise.

Test infrastructure only."""
from dataclasses import dataclass

import numpy as np

from numpy_reading import KERNELS, pair_tables

U = 2.0 ** -24
C_OMEGA, C_ETA = 24.0, 22.0
MUTATIONS = ("cross_sign", "no_minus_ni", "rho_i")  # named wrong readings: tests/test_vorticity_cpu.py shows the bounds reject each


def g_max(kernel_gradient, h):
    """the largest |dW/dr| on (0, h], numerically (cubic: 2 x 8 / (pi h^4) at q = 1/3; spiky: 45 / (pi h^4) towards q = 0)"""
    q = np.linspace(0.0, 1.0, 1 << 14)[1:]
    return float(np.abs(KERNELS[kernel_gradient][1](q * h, h)).max()) * (1.0 + 1e-6)


@dataclass
class Vorticity:
    rows: np.ndarray       # (n) bool: the fluid's particles; everything below is zero on the other rows
    contacts: np.ndarray   # (n) same-fluid contacts per row, the self contact included
    omega: np.ndarray      # (n, 3)
    n: np.ndarray          # (n)
    eta: np.ndarray        # (n, 3)
    D: np.ndarray          # (n)
    acc: np.ndarray        # (n, 3) the force's own accelerations
    b_omega: np.ndarray    # (n) per component
    b_n: np.ndarray        # (n)
    b_eta: np.ndarray      # (n) per component
    b_acc: np.ndarray      # (n) as a vector (so per component as well)


def _row_sums(terms, f32, rng):
    """sum over axis 1: float64 pairwise, or float32 one term after the other in a shuffled order"""
    if not f32:
        return terms.sum(axis=1)
    order = rng.permutation(terms.shape[1])
    return np.cumsum(terms[:, order], axis=1, dtype=np.float32)[:, -1]


def read(s, fluid, strength, kappa=0.05, f32=False, seed=1, omega=None, f32_contacts=True, mutation=None):
    """The reading of a Snapshot `s` for the entry (strength, kappa) on `fluid`.  `omega` (n, 3): pass 2 and the force take this
    vorticity (rows of the fluid) instead of pass 1's.  `mutation`: one of MUTATIONS.  The parameters are rounded to f32 first: that
    is how they cross the C ABI."""
    assert mutation in (None,) + MUTATIONS
    dt = np.float32 if f32 else np.float64
    rng = np.random.default_rng(seed)
    eps, kap, h = float(np.float32(strength)), float(np.float32(kappa)), s.h
    x, v, m, rho = s.x.astype(dt), s.v.astype(dt), s.m.astype(dt), s.rho.astype(dt)
    rows = s.model == fluid
    mask, _, g = pair_tables(x, x, h, *s.kernels, f32_contacts=f32_contacts)
    inside = mask & rows[:, None] & rows[None, :]
    g = np.where(inside[:, :, None], g, 0).astype(dt)
    contacts = inside.sum(axis=1)
    # ---- pass 1
    u = v[:, None, :] - v[None, :, :]
    cross = np.cross(g, u) if mutation == "cross_sign" else np.cross(u, g)
    rho_safe = np.where(rows, rho, 1).astype(dt)
    om = (_row_sums(cross * m[None, :, None], f32, rng) / rho_safe[:, None]).astype(dt)
    om = np.where(rows[:, None], om, 0).astype(dt)
    # bounds, from the f64 values of the same inputs
    G = g_max(s.kernels[1], h)
    gabs = np.sqrt((g.astype(np.float64) ** 2).sum(axis=2))
    uabs = np.sqrt(((s.v[:, None, :] - s.v[None, :, :]) ** 2).sum(axis=2))
    rho64 = np.where(rows, s.rho, 1.0)
    A_om = np.where(inside, s.m[None, :] * uabs, 0.0).sum(axis=1) * G / rho64
    b_om = (contacts + C_OMEGA) * U * A_om
    if omega is not None:
        om = np.where(rows[:, None], np.asarray(omega, np.float64), 0.0).astype(dt)
        b_om = np.zeros(len(x))
    n = np.sqrt((om * om).sum(axis=1)).astype(dt)
    n64 = n.astype(np.float64)
    b_n = np.sqrt(3.0) * b_om + 3.0 * U * n64
    # ---- pass 2
    vol = (m / rho_safe).astype(dt)
    weight = np.broadcast_to(vol[None, :], inside.shape)
    if mutation == "rho_i":
        weight = m[None, :] / rho_safe[:, None]
    dn = n[None, :] - (0 if mutation == "no_minus_ni" else n[:, None])
    eta = _row_sums((weight * dn)[:, :, None] * g, f32, rng).astype(dt)
    eta = np.where(rows[:, None], eta, 0).astype(dt)
    vol64 = s.m / rho64
    A_eta = np.where(inside, vol64[None, :] * np.abs(n64[None, :] - n64[:, None]), 0.0).sum(axis=1) * G
    prop = np.where(inside, vol64[None, :] * (b_n[None, :] + b_n[:, None]) * gabs, 0.0).sum(axis=1)
    b_eta = (contacts + C_ETA) * U * A_eta + prop
    # ---- force
    kh = dt(dt(kap) / dt(h))
    E = np.sqrt((eta * eta).sum(axis=1)).astype(dt)
    D = (E + kh * n).astype(dt)
    on = rows & (D > 0)
    N = eta / np.where(on, D, 1).astype(dt)[:, None]
    acc = np.where(on[:, None], dt(eps) * np.cross(N, om), 0).astype(dt)
    D64 = D.astype(np.float64)
    dE = np.sqrt(3.0) * b_eta
    dD = dE + (kap / h) * b_n + 4.0 * U * D64
    room = D64 - dD
    dN = (dE + dD) / np.where(room > 0, room, 1.0) + 4.0 * U
    first = eps * (dN * n64 + np.sqrt(3.0) * b_om) + 6.0 * U * eps * n64
    cap = 2.0 * eps * (n64 + b_n) * (1.0 + 8.0 * U)
    b_acc = np.where(room > 0, np.minimum(first, cap), cap)
    if f32:
        assert om.dtype == eta.dtype == acc.dtype == np.float32 and g.dtype == np.float32
    zero = lambda a: np.where(rows, a, 0.0)
    return Vorticity(rows, contacts, om, n, eta, D, acc, zero(b_om), zero(b_n), zero(b_eta), zero(b_acc))


def enstrophy(m, omega):
    """sum_i m_i |omega_i|^2 in float64"""
    return float((np.asarray(m, np.float64) * (np.asarray(omega, np.float64) ** 2).sum(axis=1)).sum())


def lamb_oseen(pos, centre, gamma, core):
    """velocities of a Lamb-Oseen vortex column along y through `centre`: v_theta = gamma / (2 pi r) (1 - exp(-r^2 / core^2))"""
    p = np.asarray(pos, np.float64)
    dx, dz = p[:, 0] - centre[0], p[:, 2] - centre[1]
    r2 = dx * dx + dz * dz
    swirl = np.where(r2 > 0, gamma / (2.0 * np.pi * np.where(r2 > 0, r2, 1.0)) * -np.expm1(-r2 / core ** 2), 0.0)  # v_theta / r
    vel = np.zeros_like(p)
    vel[:, 0], vel[:, 2] = swirl * dz, -swirl * dx  # y^ x r^: the rotation about +y
    return vel
