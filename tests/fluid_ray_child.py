"""Jobs of tests/test_fluid_ray_gpu.py that want a process of their own: `python fluid_ray_child.py JOB OUT.npz`.

Test infrastructure only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fluid_ray_reading as rr  # noqa: E402

DT = 1.0 / 200.0
GRAVITY = (0.0, -9.81, 0.0)
OUTPUTS = ("t", "fluid", "index", "normal", "thickness")


def depth_image3(nsteps=5):
    """What examples/depth_image3.cpp prints, through the Python mirror: a block of 10^3 particles (r = 0.05, the basic3 lattice)
    dropped for a few steps without boundaries, then a 64 x 48 camera above it looking down -y."""
    from salva_amd import DFSPHSolver, Fluid, LiquidWorld

    F = np.float32
    r, n = F(0.05), 10
    c = np.arange(n).astype(F) * r * F(2.0) + r - F(n) * r
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    block = np.stack([x.ravel(), y.ravel() + F(1.0), z.ravel()], axis=1).astype(F)
    w = LiquidWorld(DFSPHSolver(), float(r), 2.0)
    w.add_fluid(Fluid(block, float(r), 1000.0))
    for _ in range(nsteps):
        w.step(DT, GRAVITY)
    cam = {"origin": [0.0, 3.0, 0.0], "forward": [0.0, -1.0, 0.0], "right": [0.8, 0.0, 0.0], "up": [0.0, 0.0, 0.6], "width": 64, "height": 48}
    got = w.cast_camera(cam, thickness=True)
    hit = np.isfinite(got["t"])
    return (int(hit.sum()), float(got["t"][hit].astype(np.float64).sum()), float(got["t"][hit].min()), float(got["thickness"].astype(np.float64).sum()),
            float(got["thickness"][hit].min()))


def device_job():
    """Rays and outputs in torch tensors on the device, both entry points; the host-pointer calls' results beside them.  (torch is
    imported before the library is loaded: one HIP runtime per process.)"""
    import torch

    case = rr.standard_case()
    w, _ = rr.make_world(case["x"], case["slots"])
    dev = torch.device("cuda:0")
    out = {}

    def buffers(m):
        return {k: torch.full((m * (3 if k == "normal" else 1),), -1, dtype=torch.int32 if k in ("fluid", "index") else torch.float32, device=dev)
                for k in OUTPUTS}

    m = len(case["origins"])
    o, d = (torch.from_numpy(case[k]).to(dev).contiguous() for k in ("origins", "directions"))
    bufs = buffers(m)
    torch.cuda.synchronize()
    w.cast_rays_device(o.data_ptr(), d.data_ptr(), m, **{k: b.data_ptr() for k, b in bufs.items()})
    for k, b in bufs.items():
        out["dev_rays_" + k] = b.cpu().numpy()
    for k, v in w.cast_rays(case["origins"], case["directions"], normals=True, thickness=True).items():
        out["host_rays_" + k] = v
    cam = case["camera"]
    bufs = buffers(cam["width"] * cam["height"])
    torch.cuda.synchronize()
    w.cast_camera_device(cam, **{k: b.data_ptr() for k, b in bufs.items()})
    for k, b in bufs.items():
        out["dev_camera_" + k] = b.cpu().numpy()
    for k, v in w.cast_camera(cam, normals=True, thickness=True).items():
        out["host_camera_" + k] = v
    return out


if __name__ == "__main__":
    result = {"device": device_job}[sys.argv[1]]()
    np.savez(sys.argv[2], **result)
