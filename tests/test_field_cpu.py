"""The field evaluator's reading (tests/field_reading.py) and its standard case, checked without a GPU: the case meets the conditions
the GPU tests rely on, the reading agrees with the existing independent reading (tests/numpy_reading.py) where the two overlap and
with itself (fraction against density, gradient against a difference quotient), and the library exports the two entry points."""
import numpy as np
import pytest

import field_reading as fr
import numpy_reading as nr


@pytest.fixture(scope="module")
def case():
    return fr.standard_case()


@pytest.fixture(scope="module")
def readings(case):
    c = case
    border = 1.0e-4 * c["r"]
    return (fr.evaluate(c["points"], c["x"], c["v"], c["vol"], c["rho0"], c["h"], border=border),
            fr.evaluate(c["nodes"], c["x"], c["v"], c["vol"], c["rho0"], c["h"], border=border))


def test_standard_case_shapes(case):
    assert len(case["x"]) == 1386 and len(case["points"]) == 3001
    assert case["dims"] == (39, 33, 29) and all(d % 8 for d in case["dims"])
    assert 0 < case["n0"] < len(case["x"])
    assert len(np.unique(case["v"], axis=0)) == len(case["v"])
    for a in range(3):
        assert len(np.unique(case["v"][:, a])) == len(case["v"])


def test_standard_case_conditions(readings):
    for name, ref in zip(("points", "nodes"), readings):
        share_border, n_max, share_empty = ref["border"].mean(), int(ref["n"].max()), (ref["n"] == 0).mean()
        print(f"{name}: borderline {100 * share_border:.2f} %, n_max {n_max}, empty support {100 * share_empty:.1f} %")
        assert share_border <= 0.01
        assert n_max <= 150
        assert share_empty >= 0.20


def test_density_at_the_particles_matches_the_second_reading(case):
    c = case
    one = slice(0, c["n0"])  # one fluid, no boundary
    x, vol = c["x"][one], c["vol"][one]
    for name, kind in (("cubic", fr.CUBIC), ("poly6", fr.POLY6), ("spiky", fr.SPIKY), ("viscosity", fr.VISCOSITY)):
        ref = fr.evaluate(x, x, c["v"][one], vol, c["rho0"][one], c["h"], kd=kind)
        _, w, _ = nr.pair_tables(x.astype(np.float64), x.astype(np.float64), c["h"], name, name)
        rho = w @ (vol.astype(np.float64) * fr.DENSITY0[0])  # compute_densities of the second reading (DenseWorld.step)
        assert np.abs(ref["density"] - rho).max() <= 1.0e-12 * np.abs(rho).max(), name
        assert (ref["n"] >= 1).all()


def test_fraction_is_density_over_density0(case):
    c = case
    one = slice(0, c["n0"])
    ref = fr.evaluate(c["points"], c["x"][one], c["v"][one], c["vol"][one], c["rho0"][one], c["h"])
    assert np.abs(ref["fraction"] * fr.DENSITY0[0] - ref["density"]).max() <= 1.0e-12 * ref["density"].max()


@pytest.mark.parametrize("kind", [fr.CUBIC, fr.POLY6, fr.SPIKY])
def test_gradient_is_the_derivative_of_density(case, kind):
    """Central differences of the reading's own density at step e: the truncation error is e^2 / 6 times the third derivative, bounded
    here by the difference between the quotients at e and 2 e (Richardson: that difference is three times the error at e), plus the
    rounding of the quotient."""
    c = case
    pts = c["points"][:400].astype(np.float64)
    e = 1.0e-3 * c["h"]

    def quotient(step):
        q = np.zeros((len(pts), 3))
        for a in range(3):
            d = np.zeros(3)
            d[a] = step
            hi = fr.evaluate(pts + d, c["x"], c["v"], c["vol"], c["rho0"], c["h"], kd=kind, q_min=0.0)["density"]
            lo = fr.evaluate(pts - d, c["x"], c["v"], c["vol"], c["rho0"], c["h"], kd=kind, q_min=0.0)["density"]
            q[:, a] = (hi - lo) / (2.0 * step)
        return q

    ref = fr.evaluate(pts, c["x"], c["v"], c["vol"], c["rho0"], c["h"], kd=kind, kg=kind, q_min=0.0, border=2.5 * e)
    q1, q2 = quotient(e), quotient(2.0 * e)
    # (a point with a pair within 2 e of the support's edge or of the spline's knot sees a kink of a higher derivative: left out)
    smooth = ~ref["border"]
    truncation = np.abs(q2 - q1) / 3.0 + 1.0e-9 * np.abs(ref["gradient"]).max()
    err = np.abs(ref["gradient"] - q1)
    print("worst error / truncation:", float((err[smooth] / (2.0 * truncation[smooth] + 1e-300)).max()))
    assert smooth.mean() > 0.5
    assert (err[smooth] <= 2.0 * truncation[smooth] + 1.0e-6 * np.abs(ref["gradient"]).max()).all()


def test_exported_symbols():
    from salva_amd import _lib

    assert "salva_hip_evaluate_fields" in _lib.EXPORTED_SYMBOLS and "salva_hip_evaluate_fields_lattice" in _lib.EXPORTED_SYMBOLS
    out = _lib.FieldOut()
    assert [f[0] for f in out._fields_] == ["density", "fraction", "velocity", "gradient", "count"]
