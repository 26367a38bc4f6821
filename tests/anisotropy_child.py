"""Worlds and jobs of tests/test_anisotropy_gpu.py.  A job that needs a process of its own (torch loaded before the library; a twin
world stepped beside the one that calls) runs as `python anisotropy_child.py JOB OUT.npz`.

Test infrastructure only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import anisotropy_reading as ar  # noqa: E402
import field_child as fc  # noqa: E402
import field_reading as fr  # noqa: E402


def mirror(p):
    """anisotropy_reading.Params -> salva_amd.Anisotropy"""
    from salva_amd import Anisotropy

    return Anisotropy(lam=p.lam, k_r=p.k_r, k_s=p.k_s, k_n=p.k_n, n_eps=p.n_eps)


def one_fluid_world(x, vol, r, kd="cubic", kg="cubic", density0=fr.DENSITY0[0]):
    from salva_amd import DFSPHSolver, Fluid, LiquidWorld

    w = LiquidWorld(DFSPHSolver(fc.kernel_class(kd), fc.kernel_class(kg)), r, fr.SMOOTHING)
    f = Fluid(np.asarray(x, np.float32), r, density0)
    f.volumes = np.asarray(vol, np.float32) if np.ndim(vol) else np.full(len(x), vol, np.float32)
    w.add_fluid(f)
    return w, f


def flat(result):
    return {k: np.ascontiguousarray(a).reshape(-1, 3) if k == "gradient" else np.ascontiguousarray(a).reshape(-1) for k, a in result.items()}


ALL = dict(density=True, fraction=True, gradient=True)


def device_job():
    """Points and outputs in torch tensors on the device, all four calls; the host-pointer calls' results beside them."""
    import ctypes as C

    import torch

    from salva_amd import _lib

    case = ar.standard_cloud()
    w, _ = fc.standard_world(case)
    w.sync_to_device(apply_removal=False)
    dev = torch.device("cuda:0")
    prm = mirror(ar.Params())
    p = prm._struct()
    out = {}

    def ptr(t, kind=C.c_float):
        return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(kind))

    for where, m in (("points", len(case["points"])), ("nodes", len(case["nodes"]))):
        bufs = {k: torch.full((m * (3 if k == "gradient" else 1),), -1.0, dtype=torch.float32, device=dev) for k in ALL}
        fo = _lib.AnisoFieldOut()
        for k, b in bufs.items():
            setattr(fo, k, ptr(b))
        torch.cuda.synchronize()
        if where == "points":
            pts = torch.from_numpy(case["points"]).to(dev).contiguous()
            _lib.check(w._L.salva_hip_evaluate_fields_anisotropic(w._h, 3, C.byref(p), m, ptr(pts), _lib.FIELD_POINTS_ON_DEVICE | _lib.FIELD_OUT_ON_DEVICE,
                                                                  C.byref(fo)))
            host = flat(w.evaluate_fields(case["points"], anisotropy=prm, **ALL))
        else:
            o, d = np.ascontiguousarray(case["origin"], np.float32), np.ascontiguousarray(case["dims"], np.uint32)
            _lib.check(w._L.salva_hip_evaluate_fields_anisotropic_lattice(w._h, 3, C.byref(p), o.ctypes.data_as(C.POINTER(C.c_float)), float(case["spacing"]),
                                                                          d.ctypes.data_as(C.POINTER(C.c_uint32)), _lib.FIELD_OUT_ON_DEVICE, C.byref(fo)))
            host = flat(w.evaluate_lattice(case["origin"], case["spacing"], case["dims"], anisotropy=prm, **ALL))
        for k, b in bufs.items():
            out[f"dev_{where}_{k}"] = b.cpu().numpy()
            out[f"host_{where}_{k}"] = host[k]
    n = len(case["x"])
    rows = {"centres": torch.full((3 * n,), -1.0, dtype=torch.float32, device=dev), "metric": torch.full((6 * n,), -1.0, dtype=torch.float32, device=dev),
            "count": torch.full((n,), -1, dtype=torch.int32, device=dev)}
    ao = _lib.AnisotropyOut()
    ao.centres, ao.metric, ao.count, ao.row_capacity = ptr(rows["centres"]), ptr(rows["metric"]), ptr(rows["count"], C.c_uint32), n
    nrows = C.c_uint64(0)
    torch.cuda.synchronize()
    _lib.check(w._L.salva_hip_compute_anisotropy(w._h, 3, C.byref(p), _lib.ANISOTROPY_OUT_ON_DEVICE, C.byref(ao), C.byref(nrows)))
    host = w.anisotropy(prm)
    for k, b in rows.items():
        out["dev_" + k] = b.cpu().numpy()
        out["host_" + k] = host[k].reshape(-1)
    out["nrows"] = np.array([nrows.value])
    return out


def state_job():
    """A small dam break: after 10 steps every anisotropic call, then 10 more steps; a twin world that never calls."""
    out = {}
    w, f = fc.basic3_world()
    twin, ft = fc.basic3_world()
    for _ in range(10):
        w.step(fc.DT, fc.GRAVITY)
        twin.step(fc.DT, fc.GRAVITY)
    prm = mirror(ar.Params())
    x = np.array(f.positions, np.float32).copy()
    r = np.float32(0.05)
    lo = (x.min(axis=0) - np.float32(4.0) * r).astype(np.float32)
    dims = tuple(int(np.floor((x.max(axis=0)[a] + np.float32(4.0) * r - lo[a]) / (2 * r))) + 1 for a in range(3))
    for tag in ("a", "b"):  # twice: the same bits
        rows = w.anisotropy(prm)
        for k, v in rows.items():
            out[f"{tag}_{k}"] = v
        mesh = w.extract_surface(lo, 2 * r, dims, anisotropy=prm, normals=True)
        for k, v in mesh.items():
            out[f"{tag}_{k}"] = v
        out[f"{tag}_lattice"] = w.evaluate_lattice(lo, 2 * r, dims, density=False, fraction=True, anisotropy=prm)["fraction"]
    out["x"], out["vol"] = x, np.array(f.volumes, np.float32)
    for _ in range(10):
        w.step(fc.DT, fc.GRAVITY)
        twin.step(fc.DT, fc.GRAVITY)
    out["end_x"], out["end_v"] = np.array(f.positions, np.float32), np.array(f.velocities, np.float32)
    out["twin_x"], out["twin_v"] = np.array(ft.positions, np.float32), np.array(ft.velocities, np.float32)
    return out


def anisotropic_surface3(nsteps=50):
    """What examples/anisotropic_surface3.cpp computes, through the Python mirror: the basic3 block after `nsteps` steps, a lattice at
    spacing r around the fluid's box grown by 2h, the surface fraction = 0.5 with normals, isotropic and anisotropic."""
    w, _ = fc.basic3_world()
    for _ in range(nsteps):
        w.step(fc.DT, fc.GRAVITY)
    origin, dims = w.surface_lattice(0.05, margin=float(np.float32(2.0) * np.float32(w.h())))
    return (w.extract_surface(origin, 0.05, dims, iso=0.5, field="fraction", normals=True),
            w.extract_surface(origin, 0.05, dims, iso=0.5, field="fraction", normals=True, anisotropy=mirror(ar.Params())))


if __name__ == "__main__":
    result = {"device": device_job, "state": state_job}[sys.argv[1]]()
    np.savez(sys.argv[2], **result)
