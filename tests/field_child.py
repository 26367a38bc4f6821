"""Worlds and jobs of tests/test_field_gpu.py.  A job that needs an environment switch of its own (SALVA_HIP_FIELD_ARM,
SALVA_HIP_FOLD_CELLS: read when a world is created) runs in a fresh child process: `python field_child.py JOB OUT.npz`.

Test infrastructure only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import field_reading as fr  # noqa: E402

DT = 1.0 / 200.0
GRAVITY = (0.0, -9.81, 0.0)
COMBOS = (("cubic", "cubic"), ("poly6", "spiky"), ("viscosity", "viscosity"))
KINDS = {"cubic": fr.CUBIC, "poly6": fr.POLY6, "spiky": fr.SPIKY, "viscosity": fr.VISCOSITY}
ALL = dict(density=True, fraction=True, velocity=True, gradient=True, count=True)


def kernel_class(name):
    import salva_amd

    return {"cubic": salva_amd.CubicSplineKernel, "poly6": salva_amd.Poly6Kernel, "spiky": salva_amd.SpikyKernel,
            "viscosity": salva_amd.ViscosityKernel}[name]


def standard_world(case, kd="cubic", kg="cubic", extra=None):
    """The standard case's two fluids (`extra`: positions appended to fluid 1, default volume, zero velocity)."""
    from salva_amd import DFSPHSolver, Fluid, LiquidWorld

    w = LiquidWorld(DFSPHSolver(kernel_class(kd), kernel_class(kg)), case["r"], fr.SMOOTHING)
    n0 = case["n0"]
    fluids = []
    for s, rows in enumerate((slice(0, n0), slice(n0, None))):
        x, v, vol = case["x"][rows], case["v"][rows], case["vol"][rows]
        if extra is not None and s == 1:
            x = np.concatenate([x, np.asarray(extra, np.float32)])
            v = np.concatenate([v, np.zeros((len(extra), 3), np.float32)])
        f = Fluid(x, case["r"], fr.DENSITY0[s])
        f.velocities = v
        if extra is None or s == 0:
            f.volumes = vol
        else:
            f.volumes = np.concatenate([vol, np.full(len(extra), f.default_particle_volume(), np.float32)])
        fluids.append(w.add_fluid(f))
    return w, fluids


def flat(result):
    return {k: np.ascontiguousarray(a).reshape(-1, 3) if k in ("velocity", "gradient") else np.ascontiguousarray(a).reshape(-1) for k, a in result.items()}


def crowd(case):
    """600 particles inside one cell of the grid (a cube of 0.8 h well inside the cloud), seeded."""
    h = case["h"]
    corner = np.floor(np.array([0.3, 0.2, 0.15]) / h) * h + 0.1 * h
    return (corner + np.random.default_rng(11).uniform(0.0, 0.8 * h, (600, 3))).astype(np.float32)


def coarse_lattices(case):
    """(origin, spacing, dims) at spacing h and 3 h over the standard box"""
    h, lo = np.float32(case["h"]), case["origin"]
    extent = (np.array(case["dims"]) - 1) * case["r"]
    return [(lo, np.float32(k) * h, tuple(int(e // (k * float(h))) + 2 for e in extent)) for k in (1.0, 3.0)]


def basic3_world(nparticles=15, r=0.05):
    """The scene of examples/basic3.cpp and examples/field_grid3.cpp: the basic3 block over lattice plates (ground and four walls),
    DFSPH + XSPH."""
    from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, XSPHViscosity

    F = np.float32
    r = F(r)
    i = np.arange(nparticles).astype(F)
    c = i * r * F(2.0) + r - F(nparticles) * r  # examples3d/helper.rs:4-20
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    thickness, width, height = F(0.2), F(2.5), F(0.7)
    block = np.stack([x.ravel(), y.ravel() + (thickness + F(nparticles) * r), z.ravel()], axis=1).astype(F)
    w = LiquidWorld(DFSPHSolver(), float(r), 2.0)
    f = Fluid(block, float(r), 1000.0)
    f.nonpressure_forces.append(XSPHViscosity(0.5, 0.0))
    w.add_fluid(f)

    def axis(a, b):  # for (x = a; x <= b + 1e-4f; x += 2r), in f32
        out, v = [], F(a)
        while v <= F(b) + F(1e-4):
            out.append(v)
            v = F(v + F(2.0) * r)
        return np.array(out, F)

    def plate(x0, x1, y0, y1, z0, z1):
        gx, gy, gz = np.meshgrid(axis(x0, x1), axis(y0, y1), axis(z0, z1), indexing="ij")
        return np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(F)

    top = F(2.0) * height
    for box in ((-width, width, thickness, thickness, -width, width), (-width, width, thickness, top, width, width),
                (-width, width, thickness, top, -width, -width), (width, width, thickness, top, -width, width),
                (-width, -width, thickness, top, -width, width)):
        w.add_boundary(Boundary(plate(*box)))
    return w, f


def field_grid3(nsteps=50):
    """What examples/field_grid3.cpp prints, through the Python mirror: (nodes above 0.5, nodes, fill height)."""
    w, f = basic3_world()
    for _ in range(nsteps):
        w.step(DT, GRAVITY)
    r = np.float32(0.05)
    x = np.array(f.positions, np.float32)
    lo = (x.min(axis=0) - np.float32(4.0) * r).astype(np.float32)
    dims = tuple(int(np.floor((x.max(axis=0)[a] + np.float32(4.0) * r - lo[a]) / r)) + 1 for a in range(3))
    frac = w.evaluate_lattice(lo, r, dims, density=False, fraction=True)["fraction"]
    above = frac > 0.5
    rows = np.nonzero(above.any(axis=(0, 2)))[0]
    height = float(lo[1] + np.float32(rows.max()) * r) if len(rows) else float("nan")
    return int(above.sum()), int(above.size), height


def dam_break():
    """basic3_world; when the step's grid is to be folded (SALVA_HIP_FOLD_CELLS), one stray particle 100 cells below the ground makes
    the fluid's box long enough for it."""
    w, f = basic3_world()
    if os.environ.get("SALVA_HIP_FOLD_CELLS"):
        f.add_particles(np.float32([[0.3, -20.0, 0.1]]))
    return w, f


def state_job():
    """Test 8: evaluate after 10 steps, edit positions, evaluate again, step on to 20; and a twin world that never evaluates."""
    out = {}
    w, f = dam_break()
    twin, ft = dam_break()
    for _ in range(10):
        w.step(DT, GRAVITY)
        twin.step(DT, GRAVITY)
    x = np.array(f.positions, np.float32).copy()
    lo, hi = x.min(axis=0) - 0.15, x.max(axis=0) + 0.15
    pts = np.random.default_rng(5).uniform(lo, hi, (2000, 3)).astype(np.float32)
    out["pts"] = pts
    for k, v in flat(w.evaluate_fields(pts, **ALL)).items():
        out["a_" + k] = v
    out["a_x"], out["a_v"] = np.array(f.positions, np.float32), np.array(f.velocities, np.float32)
    out["a_vol"] = np.array(f.volumes, np.float32)
    for _ in range(10):
        w.step(DT, GRAVITY)
        twin.step(DT, GRAVITY)
    out["end_x"], out["end_v"] = np.array(f.positions, np.float32), np.array(f.velocities, np.float32)
    out["twin_x"], out["twin_v"] = np.array(ft.positions, np.float32), np.array(ft.velocities, np.float32)
    # an edit on the host, then the evaluation sees it
    moved = np.array(f.positions, np.float32).copy()
    moved[::3] += np.float32([0.01, 0.02, -0.01])
    f.positions = moved
    for k, v in flat(w.evaluate_fields(pts, **ALL)).items():
        out["b_" + k] = v
    out["b_x"], out["b_v"] = np.array(f.positions, np.float32), np.array(f.velocities, np.float32)
    return out


def arms_job():
    """Tests 1 and 6 under whatever SALVA_HIP_FIELD_ARM says: the standard lattice for the three kernel pairs, and the crowded cloud
    on the two coarse lattices."""
    case = fr.standard_case()
    out = {}
    for kd, kg in COMBOS:
        w, _ = standard_world(case, kd, kg)
        for k, v in flat(w.evaluate_lattice(case["origin"], case["spacing"], case["dims"], **ALL)).items():
            out[f"{kd}_{kg}_{k}"] = v
    w, _ = standard_world(case, extra=crowd(case))
    for n, (origin, spacing, dims) in enumerate(coarse_lattices(case)):
        for k, v in flat(w.evaluate_lattice(origin, spacing, dims, **ALL)).items():
            out[f"coarse{n}_{k}"] = v
    for k, v in flat(w.evaluate_lattice(case["origin"], case["spacing"], case["dims"], **ALL)).items():
        out[f"crowd_{k}"] = v
    return out


def device_job():
    """Test 9: points and outputs in torch tensors on the device, both entry points; the host-pointer calls' results beside them.
    (torch is imported before the library is loaded, as in bench.py: one HIP runtime per process.)"""
    import torch

    case = fr.standard_case()
    w, _ = standard_world(case)
    dev = torch.device("cuda:0")
    out = {}

    def buffers(m):
        return {k: torch.full((m * (3 if k in ("velocity", "gradient") else 1),), -1, dtype=torch.int32 if k == "count" else torch.float32, device=dev)
                for k in ALL}

    m = len(case["points"])
    pts = torch.from_numpy(case["points"]).to(dev).contiguous()
    bufs = buffers(m)
    torch.cuda.synchronize()
    w.evaluate_fields_device(pts.data_ptr(), m, **{k: b.data_ptr() for k, b in bufs.items()})
    for k, b in bufs.items():
        out["dev_points_" + k] = b.cpu().numpy()
    for k, v in flat(w.evaluate_fields(case["points"], **ALL)).items():
        out["host_points_" + k] = v
    bufs = buffers(len(case["nodes"]))
    torch.cuda.synchronize()
    w.evaluate_lattice_device(case["origin"], case["spacing"], case["dims"], **{k: b.data_ptr() for k, b in bufs.items()})
    for k, b in bufs.items():
        out["dev_nodes_" + k] = b.cpu().numpy()
    for k, v in flat(w.evaluate_lattice(case["origin"], case["spacing"], case["dims"], **ALL)).items():
        out["host_nodes_" + k] = v
    return out


if __name__ == "__main__":
    result = {"state": state_job, "arms": arms_job, "device": device_job}[sys.argv[1]]()
    np.savez(sys.argv[2], **result)
