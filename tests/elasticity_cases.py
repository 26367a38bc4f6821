"""The case matrix of tests/test_elasticity_isolated_gpu.py and the CPU side of it (tests/test_elasticity_reading_cpu.py).

A case is one world: elastic fluids (a body and the Young's moduli of its Becker2009Elasticity entries), optionally a plain fluid in
front of them, and a list of steps.  The world steps once from the rest positions; then, per step, the rotations are written as
the warm start, the positions become  (p0 D^T) Q^T + t  with zero velocities, the world steps and the state is read.  `cpu_units`
plays the same steps through tests/elasticity_reading.py in float64 and in its f32 replay, from the inputs the device will see
(f32 positions, f32 masses, f32 volumes0), and returns per step and per force entry what the CPU test asserts and what the GPU test
takes its scales from.  No GPU is needed to import this."""
import functools
from collections import namedtuple

import numpy as np

import elasticity_reading as er
from salva_amd import scenes

R = 0.025
H = 4 * R
DT = 1.0 / 200.0
RHO0 = 1000.0
NU = 0.3
T = (0.3, -0.2, 0.1)
AXIS = (0.3, 1.0, -0.5)
AXIS_FLAT = (1.0, 0.2, 0.3)  # of the sheet and the rod
KINDS = {"cubic": er.CUBIC, "poly6": er.POLY6, "spiky": er.SPIKY}
DEFORMATIONS = {
    "I": np.eye(3),
    "shear": np.array([[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),  # x += 0.2 y
    "stretch": np.diag([1.15, 0.9, 1.05]),
    "invert": -np.eye(3),  # the body through its centre: A_pq is symmetric and negative definite
}

# warm: "identity" (a cold start), "carry" (the R the previous step left: the device's own on the device, the reading's on the CPU)
# or "tilted" (a 50 degree rotation: something an extraction that does nothing must hand back bit for bit)
Step = namedtuple("Step", "angle D warm compare")
Step.__new__.__defaults__ = ("identity", True)
# fluids: ((body, (young moduli, one per Becker2009Elasticity entry)), ...) in world order, behind the plain fluid if there is one
Case = namedtuple("Case", "id family fluids steps nonlinear kernels axis spread plain")


def rotation(axis, degrees):
    u = np.asarray(axis, np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    th = np.radians(degrees)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _lattice(ni, nj, nk, jitter, seed):
    p = scenes.cube_fluid_positions(ni, nj, nk, R)
    return (scenes.jitter(p, jitter * R, seed=seed) if jitter else p).astype(np.float32)


@functools.lru_cache(maxsize=None)
def body(name):
    """rest positions (n, 3) f32, centred on the origin"""
    if name == "block":
        p = _lattice(8, 6, 8, 0.05, 42)
    elif name in ("block255", "block256", "block257"):  # one particle dropped from / added at the last corner of an 8 x 4 x 8 block
        p = _lattice(8, 4, 8, 0.05, 43)
        if name == "block255":
            p = p[:-1]
        if name == "block257":
            p = np.concatenate([p, p[-1:] + np.float32([2 * R, 0.0, 0.0])])
    elif name == "second":  # the second elastic fluid of the "behind" case: 257 particles, a metre to the side
        p = np.concatenate([_lattice(8, 4, 8, 0.05, 44), np.float32([[9 * R, 3 * R, 7 * R]])]) + np.float32([1.0, 0.0, 0.0])
    elif name == "sheet":
        p = _lattice(9, 1, 9, 0.05, 45)
    elif name == "sheet_flat":
        p = _lattice(9, 1, 9, 0.0, 0)
    elif name == "rod":
        p = _lattice(1, 12, 1, 0.05, 46)
    elif name == "block+twin":  # two coincident particles: an interior particle of the block twice
        p = _lattice(8, 6, 8, 0.05, 42)
        p = np.concatenate([p, p[(3 * 6 + 3) * 8 + 4][None]])
    else:
        assert name == "single"
        p = np.float32([[0.0, 0.0, 0.0]])
    return np.ascontiguousarray(p, np.float32)


@functools.lru_cache(maxsize=None)
def plain_body():
    """the plain fluid of the "behind" case: 300 particles around t, half a spacing off the lattice, so that it shares its cells
    with the moved elastic body"""
    return (_lattice(10, 6, 5, 0.05, 47) + np.float32(T) + np.float32(R)).astype(np.float32)


def volumes(case, name):
    n = len(body(name))
    v = np.full(n, (2 * R) ** 3 * 0.8, np.float32)
    if case.spread:  # masses spread by 20 % inside the fluid
        v = (0.8 * (2 * R) ** 3 * (1.0 + 0.2 * scenes.lcg_uniform(n, 7))).astype(np.float32)
    return v


def positions(case, step, name):
    """(p0 D^T) Q^T + t, rounded to f32: what is written into the fluid"""
    if step.D == "invert":  # p = -p0 exactly, no translation: rounding p_j - p_i would leave A_pq symmetric only to 1e-7
        return -body(name)
    Q = rotation(case.axis, step.angle)
    return (((body(name).astype(np.float64) @ DEFORMATIONS[step.D].T) @ Q.T) + np.asarray(T)).astype(np.float32)


def warm_start(step, n, carried):
    if step.warm == "carry":
        return np.asarray(carried, np.float32)
    W = rotation((0.2, -0.4, 1.0), 50.0) if step.warm == "tilted" else np.eye(3)
    return np.tile(W.astype(np.float32), (n, 1, 1))


def is_rigid(step):
    return step.D == "I"


def _case(id, family, steps, body_="block", moduli=(5e5,), nonlinear=True, kernels=("cubic", "cubic"), axis=AXIS, spread=False,
          plain=False, fluids=None):
    return Case(id, family, fluids or ((body_, tuple(moduli)),), tuple(steps), nonlinear, kernels, axis, spread, plain)


def _cold(angles, D):
    return [Step(a, D) for a in angles]


FOLLOW_UP = Step(30, "I")  # the step every invariant case ends with, compared like a rigid case
CASES = []
for _nl in (False, True):
    _s = "-nl" if _nl else "-lin"
    CASES += [_case("rigid" + _s, "compare", _cold((10, 30, 60, 90), "I"), nonlinear=_nl),
              _case("sheared" + _s, "compare", _cold((30, 60), "shear"), nonlinear=_nl),
              _case("stretched" + _s, "compare", _cold((30, 60), "stretch"), nonlinear=_nl)]
CASES += [
    _case("stretched-poly6-spiky", "compare", _cold((30, 60), "stretch"), kernels=("poly6", "spiky")),
    _case("accumulated", "compare", [Step(40 * k, "stretch", "identity" if k == 1 else "carry") for k in range(1, 10)]),
    _case("sheet", "compare", _cold((40, 90), "I"), body_="sheet", axis=AXIS_FLAT),
    _case("sheet-flat", "compare", _cold((40, 90), "I"), body_="sheet_flat", axis=AXIS_FLAT),
    _case("rod", "compare", _cold((20, 60), "I"), body_="rod", axis=AXIS_FLAT),
    # beyond 120 degrees sum_c R_c . A_c is negative at a cold start, and |.| in the update's divisor is what matters.  Most bodies
    # are ill-conditioned there (part 3); the flat sheet about this axis meets both admission conditions (R floor 6e-7, den ratio
    # 0.35 to 0.45), so it is compared
    _case("sheet-flat-negative-den", "compare", _cold((126, 134), "I"), body_="sheet_flat"),
    _case("n255", "compare", _cold((60,), "I"), body_="block255"),
    _case("n256", "compare", _cold((60,), "I"), body_="block256"),
    _case("n257", "compare", _cold((60,), "I"), body_="block257"),
    _case("volumes", "compare", _cold((60,), "stretch"), spread=True),
    _case("behind", "compare", _cold((60,), "stretch"), plain=True, fluids=(("block", (5e5,)), ("second", (2e5,)))),
    _case("two-entries", "compare", _cold((60,), "stretch"), moduli=(5e5, 1e5)),
    # part 3: where the extraction does not converge, or has nothing to work on — invariants only, then a compared step.
    # The sheared body at 90 degrees was asked for as a comparison case and is here because it fails both admission conditions of
    # tests/test_elasticity_reading_cpu.py (measured: R floor 3.7e-4, |den| down to 0.003 of its converged value).
    _case("cold-rigid", "invariant", [Step(a, "I", "identity", False) for a in (120, 150, 179)] + [FOLLOW_UP]),
    _case("cold-sheared", "invariant", [Step(a, "shear", "identity", False) for a in (90, 120, 150, 179)] + [FOLLOW_UP]),
    _case("rod-90", "invariant", [Step(90, "I", "identity", False), FOLLOW_UP], body_="rod", axis=AXIS_FLAT),
    _case("inverted", "invariant", [Step(0, "invert", "identity", False), FOLLOW_UP]),
    _case("single", "invariant", [Step(30, "I", "tilted", False), FOLLOW_UP], fluids=(("single", (5e5,)), ("block", (5e5,)))),
    _case("coincident", "invariant", [Step(60, "stretch", "identity", False), FOLLOW_UP], body_="block+twin"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
UNCHANGED = ("inverted", "single")  # cases whose first step must hand the warm start back bit for bit ("single": its one-particle fluid)


def reading(case, name, modulus):
    """an ElasticityReading of that entry with the rest state a device would hold: f32 positions0, f32 volumes0"""
    e = er.ElasticityReading(modulus, NU, case.nonlinear, KINDS[case.kernels[0]], KINDS[case.kernels[1]])
    p0 = body(name)
    m = volumes(case, name) * np.float32(RHO0)
    e.init(H, p0.astype(np.float64), m.astype(np.float64))
    e.volumes0 = e.volumes0.astype(np.float32).astype(np.float64)
    return e, m


def evaluate(e, p, m, warm, dtype):
    """the pass from those inputs in `dtype`, on a copy of the reading: (copy, accelerations)"""
    c = er.ElasticityReading.__new__(er.ElasticityReading)
    c.__dict__.update(e.__dict__)
    c.rotations = np.asarray(warm, np.float64)
    c.rotations_and_stresses(H, p, m, dtype=dtype)
    return c, c.accelerations(m, 1.0, dtype=dtype)


def magnitudes(c, acc):
    return {"F": float(np.abs(c.grad_tr).max()), "stress": float(np.abs(c.stress).max()), "acc": float(np.abs(acc).max())}


def twin(step):
    """the stretched twin of a rigid step: the same angle and warm start, the body stretched"""
    return step._replace(D="stretch")


def den_ratio(A, warm):
    """min over the 20 iterations and the particles of |sum_c R_c . A_c| / its value at the converged rotation (float64)"""
    A = np.asarray(A, np.float64)
    conv = np.abs(np.einsum("nrc,nrc->n", er.rotation_from_matrix_eps(A, warm, max_iter=400), A))
    worst = np.inf
    for k in range(20):
        Rk = er.rotation_from_matrix_eps(A, warm, max_iter=k)
        worst = min(worst, float((np.abs(np.einsum("nrc,nrc->n", Rk, A)) / conv).min()))
    return worst


@functools.lru_cache(maxsize=None)
def cpu_units(case_id):
    """Per step, per elastic fluid and per entry: a dict with the f32 floors of R (absolute), F, stress and the accelerations (of
    the scale: the field's largest float64 magnitude, the stretched twin's where the step is rigid), the scales, |R20 - Q|, how far
    R20 is from the rotation 400 more iterations reach (`R_short`), the den ratio, and the share of the nonlinear term F sigma d in the force.

    The acceleration floor is that of the force pass alone, as the device is compared: the f32 replay of `accelerations` against
    the float64 one, both on the f32 replay's rotations, stresses and gradients."""
    case = BY_ID[case_id]
    out = []
    for g, (name, moduli) in enumerate(case.fluids):
        for q, E in enumerate(moduli):
            e, m = reading(case, name, E)
            n = len(m)
            carried = None
            for k, step in enumerate(case.steps):
                p, Q = positions(case, step, name), rotation(case.axis, step.angle)
                warm = warm_start(step, n, carried)
                c64, a64 = evaluate(e, p, m, warm, np.float64)
                c32, a32 = evaluate(e, p, m, warm, np.float32)
                carried = c64.rotations.astype(np.float32)
                # the force pass by itself: float64 on the f32 replay's state
                s = er.ElasticityReading.__new__(er.ElasticityReading)
                s.__dict__.update(c64.__dict__)
                s.rotations, s.stress, s.grad_tr = (np.asarray(x, np.float64) for x in (c32.rotations, c32.stress, c32.grad_tr))
                a64_on_32 = s.accelerations(m, 1.0)
                scale = magnitudes(c64, a64)
                if is_rigid(step) and n > 1:
                    t64, ta64 = evaluate(e, positions(case, twin(step), name), m, warm, np.float64)
                    scale = magnitudes(t64, ta64)
                u = dict(fluid=g, entry=q, step=k, n=n, scale=scale, own=magnitudes(c64, a64))
                u["floor"] = {"R": float(np.abs(c32.rotations - c64.rotations).max()) if n > 1 else 0.0}
                for key, x32, x64 in (("F", c32.grad_tr, c64.grad_tr), ("stress", c32.stress, c64.stress), ("acc", a32, a64_on_32)):
                    u["floor"][key] = float(np.abs(x32 - x64).max() / scale[key]) if scale[key] > 0 else 0.0
                u["R_minus_Q"] = float(np.abs(c64.rotations - Q).max())
                u["R_short"] = float(np.abs(c64.rotations - er.rotation_from_matrix_eps(c64.A_pq, c64.rotations, max_iter=400)).max())
                u["unchanged32"] = bool(np.array_equal(c32.rotations, warm))
                u["den_ratio"] = den_ratio(c64.A_pq, warm) if n > 1 else 1.0
                u["den_first"] = float(np.einsum("nrc,nrc->n", warm.astype(np.float64), c64.A_pq).max())  # (of the first iteration)
                u["orth32"] = float(np.abs(np.einsum("nij,nkj->nik", c32.rotations.astype(np.float64), c32.rotations.astype(np.float64))
                                           - np.eye(3)).max())
                if case.nonlinear and n > 1:
                    lin = er.ElasticityReading.__new__(er.ElasticityReading)
                    lin.__dict__.update(c64.__dict__)
                    lin.nonlinear = False
                    u["nonlinear_share"] = float(np.abs(a64 - lin.accelerations(m, 1.0)).max() / max(scale["acc"], 1e-300))
                out.append(u)
    return out


def compared(case_id):
    case = BY_ID[case_id]
    return [u for u in cpu_units(case_id) if case.steps[u["step"]].compare and u["n"] > 1]


def scale_of(case_id, fluid, entry, step):
    return next(u["scale"] for u in cpu_units(case_id) if (u["fluid"], u["entry"], u["step"]) == (fluid, entry, step))
