"""Jobs of tests/test_surface_gpu.py that need a process of their own: `python surface_child.py JOB OUT.npz`.  A job under an
environment switch (SALVA_HIP_FIELD_ARM: read when a world is created), the job that loads torch before the library (one HIP runtime per
process), and the twin worlds of the state test.

Test infrastructure only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import field_child as fc  # noqa: E402
import field_reading as fr  # noqa: E402
import surface_reading as sr  # noqa: E402

SURFACES = (("fraction", 0.5), ("density", 400.0))


def arms_job():
    """Test 3 under whatever SALVA_HIP_FIELD_ARM says: the standard world's two surfaces beside the device's own lattices."""
    case = fr.standard_case()
    w, _ = fc.standard_world(case)
    out = {}
    for field, iso in SURFACES:
        lattice = w.evaluate_lattice(case["origin"], case["spacing"], case["dims"], density=field == "density", fraction=field == "fraction")[field]
        mesh = w.extract_surface(case["origin"], case["spacing"], case["dims"], iso=iso, field=field)
        out[field + "_lattice"], out[field + "_vertices"], out[field + "_triangles"] = lattice, mesh["vertices"], mesh["triangles"]
    return out


def device_job():
    """Tests 1 and 2 from device memory: the two small lattices in torch tensors, the mesh into torch tensors (count call, fill call)."""
    import torch

    from salva_amd import DFSPHSolver, LiquidWorld

    dev = torch.device("cuda:0")
    w = LiquidWorld(DFSPHSolver(), 0.025, 2.0)
    out = {}
    for name, values, iso in (("random", sr.random_lattice(), 0.5), ("linear", sr.linear_lattice(), sr.LINEAR_ISO)):
        v = torch.from_numpy(values).to(dev).contiguous()
        torch.cuda.synchronize()
        nv, nt = w.extract_surface_device(sr.LATTICE_ORIGIN, sr.LATTICE_SPACING, values.shape, iso=iso, values=v.data_ptr())
        vertices = torch.full((nv * 3,), -1.0, dtype=torch.float32, device=dev)
        triangles = torch.full((nt * 3,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        got = w.extract_surface_device(sr.LATTICE_ORIGIN, sr.LATTICE_SPACING, values.shape, iso=iso, values=v.data_ptr(), vertices=vertices.data_ptr(),
                                       triangles=triangles.data_ptr(), vertex_capacity=nv, triangle_capacity=nt)
        assert got == (nv, nt)
        out[name + "_vertices"] = vertices.cpu().numpy().reshape(nv, 3)
        out[name + "_triangles"] = triangles.cpu().numpy().view(np.uint32).reshape(nt, 3)
    return out


def surface_of(w):
    origin, dims = w.surface_lattice(0.05)
    return w.extract_surface(origin, 0.05, dims, normals=True, velocities=True)


def state_job():
    """Test 8: extract after 10 steps, step on to 20; and a twin world that never extracts."""
    out = {}
    w, f = fc.dam_break()
    twin, ft = fc.dam_break()
    for _ in range(10):
        w.step(fc.DT, fc.GRAVITY)
        twin.step(fc.DT, fc.GRAVITY)
    mesh = surface_of(w)
    out["nv"], out["nt"] = np.int64(len(mesh["vertices"])), np.int64(len(mesh["triangles"]))
    for _ in range(10):
        w.step(fc.DT, fc.GRAVITY)
        twin.step(fc.DT, fc.GRAVITY)
    out["end_x"], out["end_v"] = np.array(f.positions, np.float32), np.array(f.velocities, np.float32)
    out["twin_x"], out["twin_v"] = np.array(ft.positions, np.float32), np.array(ft.velocities, np.float32)
    return out


def surface3(nsteps=50):
    """What examples/surface3.cpp computes, through the Python mirror: the basic3 block after `nsteps` steps, the lattice from
    fluid_bounds at spacing r, the surface fraction = 0.5 with normals."""
    w, _ = fc.basic3_world()
    for _ in range(nsteps):
        w.step(fc.DT, fc.GRAVITY)
    origin, dims = w.surface_lattice(0.05)
    return w.extract_surface(origin, 0.05, dims, iso=0.5, field="fraction", normals=True)


if __name__ == "__main__":
    result = {"arms": arms_job, "device": device_job, "state": state_job}[sys.argv[1]]()
    np.savez(sys.argv[2], **result)
