"""Worlds and jobs of tests/test_diffuse_gpu.py.  A job that needs a process of its own (torch loaded before the library; a twin world
stepped beside the one that calls; a folded step grid) runs as `python diffuse_child.py JOB OUT.npz`.

Test infrastructure only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import diffuse_reading as dr  # noqa: E402
import field_child as fc  # noqa: E402
import field_reading as fr  # noqa: E402

NAMES = ("trapped_air", "wave_crest", "energy", "normal", "count")
WIDTH = dict(trapped_air=1, wave_crest=1, energy=1, normal=3, count=1)


def mirror(p):
    """diffuse_reading.Params -> salva_amd.Diffuse (the same field names)"""
    import dataclasses

    from salva_amd import Diffuse

    return Diffuse(**dataclasses.asdict(p))


EMIT_DT = 1.0 / 200.0


def emit_params(seed=11):
    """on the standard cloud: some hundreds emitted, some rows at max_per_particle, most rows nothing (tests/test_diffuse_cpu.py)"""
    return dr.Params(trapped_air=(0.2, 1.2), wave_crest=(0.5, 3.0), energy=(0.02, 0.3), k_ta=300.0, k_wc=1200.0, max_per_particle=4, seed=seed)


def standard_rows(case):
    """slot and index of each packed row of the standard cloud's two fluids"""
    return dr.rows_of([(0, case["n0"]), (1, len(case["x"]) - case["n0"])])


def still_block():
    """A jittered 7 x 7 x 7 block in slow motion, and hand-placed diffuse particles: deep inside, on a face, just off a face, far outside,
    one off a face with a lifetime below dt (foam: it dissolves), one NaN, one outside the kill box, and a second one inside (order and ids after removal)."""
    rng = np.random.default_rng(43)
    r, h = fr.R, float(fr.H32)
    base = dr.lattice(7, 7, 7, 2.0 * r)
    x = dr.separate((base + rng.uniform(-0.2 * r, 0.2 * r, base.shape)).astype(np.float32), np.full(base.shape, 0.2 * r), h, rng)
    c = 6.0 * r
    pts = np.float32([[c, c, c], [c, 12.0 * r + 0.5 * r, c], [c, 12.0 * r + 3.2 * r, c], [5.0, 5.0, 5.0], [c + r, 12.0 * r + 2.0 * r, c], [np.nan, c, c],
                      [c, c, -0.2], [c - r, c + r, c]])
    vel = np.float32([[0.1, 0.2, 0.3], [0.0, 1.0, 0.0], [0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.1], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0],
                      [0.3, 0.0, 0.0]])
    life = np.float32([3.0, 3.0, 3.0, 3.0, 0.5 * EMIT_DT, 3.0, 3.0, 3.0])
    box = ((-1.0, -1.0, -0.1), (10.0, 10.0, 10.0))
    return {"r": r, "h": h, "x": x, "v": (0.2 * dr.flow(x)).astype(np.float32), "vol": np.full(len(x), 0.8 * (2.0 * r) ** 3, np.float32), "points": pts,
            "velocities": vel, "lifetime": life, "kill_box": box}



def one_fluid_world(x, v, vol, r, kd="cubic", kg="cubic", density0=fr.DENSITY0[0]):
    from salva_amd import DFSPHSolver, Fluid, LiquidWorld

    w = LiquidWorld(DFSPHSolver(fc.kernel_class(kd), fc.kernel_class(kg)), r, fr.SMOOTHING)
    f = Fluid(np.asarray(x, np.float32), r, density0)
    f.volumes = np.asarray(vol, np.float32)
    f.velocities = np.asarray(v, np.float32)
    w.add_fluid(f)
    return w, f


def device_job():
    """Every output in a torch tensor on the device; the host-pointer call's results beside them."""
    import ctypes as C

    import torch

    case = dr.standard_cloud()
    w, _ = fc.standard_world(case)
    dev = torch.device("cuda:0")
    n = len(case["x"])
    bufs = {k: torch.full((n * WIDTH[k],), -1, dtype=torch.int32 if k == "count" else torch.float32, device=dev) for k in NAMES}
    torch.cuda.synchronize()
    out = {"counted": np.array([w.diffuse_potentials_device()])}
    out["nrows"] = np.array([w.diffuse_potentials_device(row_capacity=n, **{k: b.data_ptr() for k, b in bufs.items()})])
    host = w.diffuse_potentials()
    for k, b in bufs.items():
        out["dev_" + k] = b.cpu().numpy()
        out["host_" + k] = host[k].reshape(-1)
    assert C.sizeof(C.c_float) == 4
    return out


def foam_params():
    """the parameters of examples/foam3.cpp: the basic3 dam break is small and slow, so the clamps are low"""
    return dr.Params(trapped_air=(1.0, 10.0), wave_crest=(0.5, 4.0), energy=(0.1, 2.0), k_ta=200.0, k_wc=2000.0, max_per_particle=4, seed=3)


def state_job():
    """A small dam break (with SALVA_HIP_FOLD_CELLS: on a folded step grid): the potentials and an update of a diffuse set before the
    first step and after every one of 20 steps; a twin world that never calls."""
    out = {}
    w, f = fc.dam_break()
    twin, ft = fc.dam_break()
    first = w.diffuse_potentials()
    out["first_count"], out["first_energy"] = first["count"], first["energy"]
    ds = w.create_diffuse(20000, mirror(foam_params()))
    ds.add(np.float32([[0.0, 0.6, 0.0], [0.1, 0.5, 0.1]]), np.zeros((2, 3), np.float32))
    ds.update(fc.DT)  # before the first step
    out["first_set"] = np.array([len(ds), ds.stats()["emitted"]])
    for step in range(20):
        w.step(fc.DT, fc.GRAVITY)
        twin.step(fc.DT, fc.GRAVITY)
        ds.update(fc.DT)
        got = w.diffuse_potentials()
        if step == 9:
            out["x"], out["v"], out["vol"] = np.array(f.positions, np.float32), np.array(f.velocities, np.float32), np.array(f.volumes, np.float32)
            again = w.diffuse_potentials()
            for k in NAMES:
                out["a_" + k], out["b_" + k] = got[k], again[k]
    out["end_x"], out["end_v"] = np.array(f.positions, np.float32), np.array(f.velocities, np.float32)
    out["twin_x"], out["twin_v"] = np.array(ft.positions, np.float32), np.array(ft.velocities, np.float32)
    st = ds.stats()
    out["set_stats"] = np.array([st["count"], st["total_emitted"], st["total_dissolved"], st["total_killed"], st["total_dropped"], len(ds)])
    return out


def set_device_job():
    """add and get with torch tensors on the device against the host-pointer arms, on two sets of one world"""
    import torch

    b = still_block()
    w, _ = one_fluid_world(b["x"], b["v"], b["vol"], b["r"])
    dev = torch.device("cuda:0")
    keep = np.isfinite(b["points"]).all(axis=1)
    x, v, life = b["points"][keep], b["velocities"][keep], b["lifetime"][keep]
    n = len(x)
    host, other = w.create_diffuse(64), w.create_diffuse(64)
    host.add(x, v, life)
    tx, tv, tl = (torch.from_numpy(np.ascontiguousarray(a)).to(dev).contiguous() for a in (x.reshape(-1), v.reshape(-1), life))
    torch.cuda.synchronize()
    other.add_device(n, tx.data_ptr(), tv.data_ptr(), tl.data_ptr())
    for s in (host, other):
        s.update(EMIT_DT, mirror(dr.Params(k_ta=0.0, k_wc=0.0)))
    out = {}
    bufs = {"positions": torch.full((3 * 64,), -1.0, device=dev), "velocities": torch.full((3 * 64,), -1.0, device=dev),
            "lifetime": torch.full((64,), -1.0, device=dev), "kind": torch.full((64,), -1, dtype=torch.int32, device=dev),
            "id": torch.full((64,), -1, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize()
    out["n_dev"] = np.array([other.get_device(64, **{k: t.data_ptr() for k, t in bufs.items()})])
    for name, got in (("host", host.get()), ("other", other.get())):
        for k, a in got.items():
            out[f"{name}_{k}"] = a.reshape(-1)
    for k, t in bufs.items():
        out["dev_" + k] = t.cpu().numpy()
    return out


def foam3(nsteps=60):
    """What examples/foam3.cpp prints, through the Python mirror: the basic3 dam break, an update after every step; the counts per kind
    and the totals of the set."""
    w, _ = fc.basic3_world()
    ds = w.create_diffuse(20000, mirror(foam_params()))
    for _ in range(nsteps):
        w.step(fc.DT, fc.GRAVITY)
        ds.update(fc.DT)
    st = ds.stats()
    return tuple(st[k] for k in ("count", "spray", "foam", "bubble", "new", "total_emitted", "total_dissolved", "total_killed", "total_dropped"))


def whitewater_potentials3(nsteps=50):
    """What examples/whitewater_potentials3.cpp prints, through the Python mirror: the basic3 block, the potentials after every step;
    of the last step (rows, most neighbours, with a normal, on a crest, trapped air above 5, energy above 5)."""
    from salva_amd import Diffuse

    w, _ = fc.basic3_world()
    prm = Diffuse()
    for _ in range(nsteps):
        w.step(fc.DT, fc.GRAVITY)
        p = w.diffuse_potentials(prm)
    return (len(p["count"]), int(p["count"].max()), int((p["normal"] != 0).any(axis=1).sum()), int((p["wave_crest"] > 0).sum()),
            int((p["trapped_air"] > np.float32(5.0)).sum()), int((p["energy"] > np.float32(5.0)).sum()))


if __name__ == "__main__":
    result = {"device": device_job, "state": state_job, "set_device": set_device_job}[sys.argv[1]]()
    np.savez(sys.argv[2], **result)
