"""The potentials of diffuse particles (include/salva_hip.h "Diffuse particles") on the device against the reading
tests/diffuse_reading.py: `count` exactly; trapped_air, energy and normal against the f64 reading at the tolerances derived in its
docstring; wave_crest against the reading fed the device's own normals, so that only the sum is under test.  A discontinuous decision
the device may take either way widens a row's bound by the terms at stake, and such rows are at most 1 % of a cloud.  Jobs that need
a process of their own run as children (tests/diffuse_child.py).
The diffuse set (salva_hip_create_diffuse ... salva_hip_update_diffuse) is compared bit for bit with the f32 restatement of the reading,
fed the device's own potentials and the device's own evaluate_fields outputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import diffuse_child as dc
import diffuse_reading as dr
import field_child as fc
from salva_amd import _lib

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
CANARY = 0x7FC0BEEF
DEFAULT = dr.Params()


@pytest.fixture(scope="module")
def case():
    return dr.standard_cloud()


@pytest.fixture(scope="module")
def shapes():
    return dr.shapes_cloud()


@pytest.fixture(scope="module")
def world(hip_lib, case):
    return fc.standard_world(case)


@pytest.fixture(scope="module")
def rows(world):
    """the device's potentials of the standard cloud at the default parameters, shared and left unchanged"""
    return world[0].diffuse_potentials()


def child(job, tmp_path, **env):
    out = str(tmp_path / (job + ".npz"))
    e = dict(os.environ)
    for k in ("SALVA_HIP_FIELD_ARM", "SALVA_HIP_FOLD_CELLS", "SALVA_HIP_NO_FOLD"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "diffuse_child.py"), job, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def last_error():
    return _lib.lib().salva_hip_last_error().decode()


def u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def params(p=DEFAULT, **edit):
    s = dc.mirror(p)._struct()
    for k, v in edit.items():
        setattr(s, k, v)
    return s


def raw(w, mask, p, out, nrows, flags=0):
    return w._L.salva_hip_diffuse_potentials(w._h, mask, C.byref(p) if p is not None else None, flags, C.byref(out) if out is not None else None,
                                             C.byref(nrows) if nrows is not None else None)


def canaries(n, names=dc.NAMES, spare=1):
    """buffers full of canaries with `spare` rows more than n, and a SalvaHipDiffusePotentialsOut over those of `names`"""
    bufs = {k: np.full((n + spare) * dc.WIDTH[k], CANARY, np.uint32) for k in dc.NAMES}
    out = _lib.DiffusePotentialsOut()
    for k in names:
        setattr(out, k, u32p(bufs[k]) if k == "count" else C.cast(u32p(bufs[k]), C.POINTER(C.c_float)))
    out.row_capacity = n
    return bufs, out


def check(got, x, v, vol, rho0, h, p=DEFAULT, kg="cubic"):
    """every output against the reading; returns the reading and the share of rows with a widened bound"""
    ref = dr.potentials(x, v, vol, rho0, h, p, kg=fc.KINDS[kg])
    wide = dr.compare(got, ref, p)
    k = dr.crest(x, v, h, got["normal"], p)
    wide = wide | dr.compare_crest(got["wave_crest"], k)
    print(f"{int(wide.sum())} of {len(wide)} rows with a widened bound")
    assert wide.sum() <= 0.01 * len(wide)
    bad = ~ref["finite"]
    assert all((np.asarray(got[name])[bad] == 0).all() for name in dc.NAMES)  # a non-finite row: zeros and count 0
    return ref, k


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kd,kg", fc.COMBOS)
def test_potentials_of_the_standard_cloud(hip_lib, case, kd, kg):
    """before the first step, two fluids, the three gradient kernels"""
    w, _ = fc.standard_world(case, kd, kg)
    got = w.diffuse_potentials()
    ref, k = check(got, case["x"], case["v"], case["vol"], case["rho0"], case["h"], kg=kg)
    assert (got["trapped_air"] > 0).mean() > 0.9 and (k["wave_crest"] > 0).mean() > 0.1 and 0.2 < ref["has_normal"].mean() < 0.8
    again = w.diffuse_potentials()
    for name in dc.NAMES:
        assert np.array_equal(got[name].view(np.uint32), again[name].view(np.uint32)), name  # the order of every sum is fixed


@pytest.mark.parametrize("surface_min,crest_cos", [(0.25, 0.6), (0.0, -1.0), (1.0, 0.95)])
def test_potentials_of_the_shapes(hip_lib, shapes, surface_min, crest_cos):
    p = dr.Params(surface_min, crest_cos)
    w, _ = dc.one_fluid_world(shapes["x"], shapes["v"], shapes["vol"], shapes["r"])
    got = w.diffuse_potentials(dc.mirror(p))
    ref, k = check(got, shapes["x"], shapes["v"], shapes["vol"], shapes["rho0"], shapes["h"], p)
    parts = shapes["parts"]
    for name in ("lone", "stray", "nan"):
        assert got["count"][parts[name]].tolist() == [0] and (got["trapped_air"][parts[name]] == 0).all() and (got["normal"][parts[name]] == 0).all()
    assert got["energy"][parts["lone"]][0] > 0 and got["energy"][parts["nan"]][0] == 0
    assert got["count"][parts["same"]].tolist() == [1, 1] and (got["trapped_air"][parts["same"]] == 0).all()
    # eps < r <= 1e-5 h: no gradient from the cubic spline, whatever the threshold
    assert got["count"][parts["close"]].tolist() == [1, 1] and (got["normal"][parts["close"]] == 0).all() and (got["trapped_air"][parts["close"]] > 0).all()
    rest = shapes["rest"]
    assert got["energy"][rest] == 0 and got["wave_crest"][rest] == 0 and got["trapped_air"][rest] > 0
    if surface_min == 0.0:  # every particle with a gradient has a normal, and a unit one
        has = ref["gnorm"] > 0
        assert np.array_equal((got["normal"] != 0).any(axis=1), has)
        assert np.abs(np.linalg.norm(got["normal"][has].astype(np.float64), axis=1) - 1.0).max() <= 4.0 * dr.U


def test_fluid_mask(world, rows, case):
    w, (f0, f1) = world
    n0 = case["n0"]
    for fluids, sl in (([f0], slice(0, n0)), ([1], slice(n0, None))):
        got = w.diffuse_potentials(fluids=fluids)
        assert len(got["count"]) == len(case["x"][sl])
        check(got, case["x"][sl], case["v"][sl], case["vol"][sl], case["rho0"][sl], case["h"])
        assert not np.array_equal(got["count"], rows["count"][sl])  # (the other fluid's particles are nobody's neighbours)
    nrows = C.c_uint64(0)
    assert raw(w, 0b100, params(), None, nrows) == _lib.E_INVALID and "selects no existing fluid" in last_error()
    assert raw(w, 0b110, params(), None, nrows) == _lib.OK and nrows.value == len(case["x"]) - n0  # (an absent fluid beside an existing one)


def test_output_subsets(world, rows, case):
    """an output that is not asked for is not written, and the others keep their bits - the sums only it needs are not made"""
    w, _ = world
    n = len(case["x"])
    nrows = C.c_uint64(0)
    for names in [(k,) for k in dc.NAMES] + [("trapped_air", "count"), ("wave_crest", "energy"), ("normal", "wave_crest")]:
        bufs, out = canaries(n, names)
        assert raw(w, 3, params(), out, nrows) == _lib.OK, last_error()
        for k in dc.NAMES:
            if k in names:
                assert np.array_equal(bufs[k][:n * dc.WIDTH[k]], rows[k].reshape(-1).view(np.uint32)), (names, k)
                assert (bufs[k][n * dc.WIDTH[k]:] == CANARY).all(), (names, k)
            else:
                assert (bufs[k] == CANARY).all(), (names, k)


def test_rows_counts_and_capacity(world, rows, case):
    w, _ = world
    n = len(case["x"])
    nrows = C.c_uint64(0)
    assert raw(w, 3, params(), None, nrows) == _lib.OK and nrows.value == n  # count only
    bufs, out = canaries(n)
    out.row_capacity = n - 1
    nrows = C.c_uint64(0)
    assert raw(w, 3, params(), out, nrows) == _lib.E_CAPACITY and nrows.value == n, last_error()
    assert "row_capacity" in last_error() and all((b == CANARY).all() for b in bufs.values())
    out.row_capacity = n + 1
    assert raw(w, 3, params(), out, nrows) == _lib.OK and nrows.value == n, last_error()
    for k in dc.NAMES:
        assert np.array_equal(bufs[k][:n * dc.WIDTH[k]], rows[k].reshape(-1).view(np.uint32)), k
        assert (bufs[k][n * dc.WIDTH[k]:] == CANARY).all(), k
    empty = _lib.DiffusePotentialsOut()  # no pointer at all: nothing to do
    empty.row_capacity = n
    assert raw(w, 3, params(), empty, nrows) == _lib.OK and nrows.value == n


def test_device_pointers(hip_lib, tmp_path):
    """every output in a torch tensor on the device: the bits of the host-pointer call"""
    s = child("device", tmp_path)
    assert int(s["counted"][0]) == int(s["nrows"][0]) == len(s["host_count"]) == 1386
    for k in dc.NAMES:
        assert np.array_equal(s["dev_" + k].view(np.uint32).reshape(-1), s["host_" + k].view(np.uint32).reshape(-1)), k
    assert s["host_trapped_air"].max() > 1.0 and s["host_count"].max() > 20


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [None, "64"])
def test_state(hip_lib, tmp_path, fold):
    """A twin world that never asks has the same fluid bits after 20 steps as one that asks after every step; the call works before
    the first step; a second call gives the same bits; the call sees the arrays get_fluid returns.  fold: the same with the step's
    grid folded (SALVA_HIP_FOLD_CELLS=64)."""
    s = child("state", tmp_path, **({"SALVA_HIP_FOLD_CELLS": fold} if fold else {}))
    assert np.array_equal(s["end_x"], s["twin_x"]) and np.array_equal(s["end_v"], s["twin_v"])
    assert s["first_count"].max() > 20 and (s["first_energy"] == 0).all()  # at rest before the first step
    for k in dc.NAMES:
        assert np.array_equal(s["a_" + k].view(np.uint32), s["b_" + k].view(np.uint32)), k
    h = float(np.float32(np.float32(0.05) * np.float32(2.0) * np.float32(2.0)))
    # (a simulated cloud is not separated: the rows with a pair on the border of h are left out of the exact comparison)
    ref = dr.potentials(s["x"], s["v"], s["vol"], 1000.0, h)
    keep = np.setdiff1d(np.arange(len(ref["count"])), np.unique(dr.near_the_border(s["x"], h)))
    assert len(keep) > 0.9 * len(ref["count"])
    assert np.array_equal(s["a_count"].astype(np.int64)[keep], ref["count"][keep])
    tol = dr.tol_sum(ref["n"], ref["A_trapped"], dr.C_TRAPPED)
    assert (np.abs(s["a_trapped_air"].astype(np.float64) - ref["trapped_air"])[keep] <= tol[keep]).all()
    assert s["a_energy"].max() > 0 and (s["a_normal"] != 0).any()


# 3 ------------------------------------------------------------------------------------------------
def test_refusals_and_edge_cases(hip_lib, case):
    from salva_amd import dist

    w, _ = fc.standard_world(case)
    w.sync_to_device(apply_removal=False)
    n = len(case["x"])
    nrows = C.c_uint64(0)
    bufs, out = canaries(n)

    def refused(code, want=_lib.E_INVALID, text=None):
        assert code == want, (code, last_error())
        if text:
            assert text in last_error(), last_error()
        assert all((b == CANARY).all() for b in bufs.values())
        w.step(fc.DT, (0.0, 0.0, 0.0))  # the world steps on after every refusal

    nan, inf = float("nan"), float("inf")
    for edit in (dict(surface_min=-0.1), dict(surface_min=nan), dict(surface_min=inf), dict(crest_cos=1.5), dict(crest_cos=-1.5), dict(crest_cos=nan),
                 dict(ta_lo=nan), dict(ta_lo=-1.0), dict(ta_lo=30.0), dict(ta_hi=inf), dict(wc_lo=8.0), dict(wc_hi=nan), dict(en_lo=60.0), dict(en_hi=nan),
                 dict(k_ta=-1.0), dict(k_ta=nan), dict(k_wc=inf), dict(max_per_particle=65), dict(n_spray=21), dict(k_b=nan), dict(k_b=inf),
                 dict(k_d=1.5), dict(k_d=nan), dict(life_lo=-1.0), dict(life_lo=6.0), dict(life_hi=inf), dict(life_lo=nan), dict(has_kill_box=2),
                 dict(struct_size=124), dict(version=2)):
        refused(raw(w, 3, params(**edit), out, nrows))
    box = params(has_kill_box=1)
    box.kill_lo[1], box.kill_hi[1] = 1.0, 0.0
    refused(raw(w, 3, box, out, nrows), text="kill_lo")
    box.kill_lo[1] = nan
    box.has_kill_box = 0
    refused(raw(w, 3, box, out, nrows), text="NaN")
    grav = params()
    grav.gravity[2] = inf
    refused(raw(w, 3, grav, out, nrows), text="gravity")
    refused(raw(w, 3, None, out, nrows), text="null")
    refused(raw(w, 3, params(), out, None))
    refused(raw(w, 3, params(), out, nrows, flags=2), text="unknown flag")
    refused(raw(w, 0, params(), out, nrows), text="selects no existing fluid")
    assert raw(w, 3, params(), out, nrows) == _lib.OK and nrows.value == n and (bufs["count"][:n] != CANARY).all()
    # two strays far away: the table over the fluids' own box has more than 2^27 cells
    ws, _ = fc.standard_world(case, extra=np.float32([[1.0e6 * case["h"], 0.0, 0.0], [0.1, -1.0e6 * case["h"], 0.2]]))
    ws.sync_to_device(apply_removal=False)
    bufs, out = canaries(n + 2)
    assert raw(ws, 3, params(), out, nrows) == _lib.E_CAPACITY and "2^27 cells" in last_error() and nrows.value == n + 2
    assert all((b == CANARY).all() for b in bufs.values())
    # a world without a finite particle: zeros
    wn, _ = dc.one_fluid_world(np.full((5, 3), np.nan, np.float32), np.ones((5, 3), np.float32), np.full(5, 1.0e-4, np.float32), case["r"])
    assert all((a == 0).all() and len(a) == 5 for a in wn.diffuse_potentials().values())
    with pytest.raises(ValueError):
        w.diffuse_potentials(density=True)
    # a loopback-decomposed world
    wd, _ = fc.standard_world(case)
    wd.sync_to_device(apply_removal=False)
    wd.set_domain(dist.Comm.loopback(1)[0], -1000, 1000)
    assert raw(wd, 3, params(), None, nrows) == _lib.E_INVALID and "host-order arrays are not maintained" in last_error()


def test_refused_inside_a_force_callback(hip_lib, case):
    from salva_amd import NonPressureForce

    class Calls(NonPressureForce):
        def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
            nrows = C.c_uint64(0)
            self.seen = (raw(self.world, 3, params(), None, nrows), last_error())

    w, (f0, _) = fc.standard_world(case)
    force = Calls()
    force.world = w
    f0.nonpressure_forces.append(force)
    st = w.step(fc.DT, (0.0, 0.0, 0.0))
    assert force.seen[0] == _lib.E_INVALID and "callback" in force.seen[1], force.seen
    assert st is not None and w._nsteps == 1  # the step completed


def test_mirrors(world, rows, case):
    from salva_amd import Diffuse

    w, _ = world
    n = len(case["x"])
    assert {k: (a.shape, a.dtype) for k, a in rows.items()} == {
        "trapped_air": ((n,), np.float32), "wave_crest": ((n,), np.float32), "energy": ((n,), np.float32), "normal": ((n, 3), np.float32),
        "count": ((n,), np.uint32)}
    some = w.diffuse_potentials(Diffuse(), wave_crest=False, normal=False)
    assert set(some) == {"trapped_air", "energy", "count"} and np.array_equal(some["trapped_air"], rows["trapped_air"])
    # the thresholds reach the device: a higher surface_min leaves fewer normals, a gate that is always open more crests
    strict = w.diffuse_potentials(Diffuse(surface_min=1.0))
    assert 0 < (strict["normal"] != 0).any(axis=1).sum() < (rows["normal"] != 0).any(axis=1).sum()
    opened = w.diffuse_potentials(Diffuse(crest_cos=-1.0))
    assert (opened["wave_crest"] > 0).sum() > (rows["wave_crest"] > 0).sum()


def test_whitewater_potentials3_example_agrees_with_the_python_mirror(hip_lib):
    """examples/whitewater_potentials3.cpp (the C++ mirror): the basic3 dam break, the potentials after every one of 50 steps; the counts
    it prints for the last step are the Python mirror's of the same scene."""
    import re

    root = os.path.dirname(TESTS)
    exe = os.path.join(root, "examples", "whitewater_potentials3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "whitewater_potentials3"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"(\d+) particles after 50 steps; at most (\d+) neighbours\nwith a normal: (\d+); on a crest: (\d+); trapped air above 5.0: (\d+); "
                  r"energy above 5.0: (\d+)", r.stdout)
    assert m, r.stdout
    got = tuple(int(g) for g in m.groups())
    want = dc.whitewater_potentials3()
    print(got)
    assert got == want and got[0] == 3375 and 0 < got[3] < got[2] < got[0]


# 4 ------------------------------------------------------------------------------------------------ the diffuse set
SET_KEYS = ("positions", "velocities", "lifetime", "kind", "id")


def same_bits(got, want, upto=None):
    for k in SET_KEYS:
        a, b = np.ascontiguousarray(got[k][:upto]), np.ascontiguousarray(want[k][:upto])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, a.shape, b.shape)


def emitted_by(case, p, capacity=100000, updates=1):
    """a fresh standard world, a set and `updates` updates with p; what the set holds, its stats after each, the device's potentials"""
    w, _ = fc.standard_world(case)
    prm = dc.mirror(p)
    pot = w.diffuse_potentials(prm)
    ds = w.create_diffuse(capacity, prm)
    stats = []
    for _ in range(updates):
        ds.update(dc.EMIT_DT)
        stats.append(ds.stats())
    return w, ds, ds.get(), stats, pot


def test_emission_is_the_f32_reading_bit_for_bit(hip_lib, case):
    """an update of an empty set before the first step: emission alone, from the device's own potentials"""
    p = dc.emit_params()
    slot, index = dc.standard_rows(case)
    w, ds, got, (st,), pot = emitted_by(case, p)
    new, (emitted, dropped), c = dr.emit(case["x"], case["v"], slot, index, pot, p, dc.EMIT_DT, 0, case["r"], 0, 100000)
    print(f"{emitted} emitted, {int((c == p.max_per_particle).sum())} rows at the limit, {int((c == 0).sum())} rows emit nothing")
    assert emitted >= 200 and (c == p.max_per_particle).any() and (c == 0).any()
    assert len(ds) == emitted and (st["count"], st["new"], st["emitted"], st["dropped"], st["total_emitted"]) == (emitted, emitted, emitted, 0, emitted)
    same_bits(got, new)
    # the same seed in another world: the same bits; another seed: other places, and the total the reading gives for it
    _, _, again, _, _ = emitted_by(case, p)
    same_bits(again, got)
    q = dc.emit_params(seed=12)
    _, _, other, (st2,), pot2 = emitted_by(case, q)
    new2, (emitted2, _), _ = dr.emit(case["x"], case["v"], slot, index, pot2, q, dc.EMIT_DT, 0, case["r"], 0, 100000)
    same_bits(other, new2)
    assert st2["emitted"] == emitted2 and not np.array_equal(other["positions"][:50], got["positions"][:50])
    assert abs(emitted2 - emitted) <= 6.0 * np.sqrt(emitted)  # (the counts differ by the rounding draw alone)
    # a capacity smaller than the need: the first particles in order, the rest dropped and counted
    room = emitted // 3
    _, small, few, (st3,), _ = emitted_by(case, p, capacity=room)
    assert len(small) == room and (st3["emitted"], st3["dropped"], st3["total_dropped"]) == (room, emitted - room, emitted - room)
    same_bits(few, got, upto=room)


def test_a_second_update_advects_the_first_and_counts_on(hip_lib, case):
    """two updates of one set: the particles of the first are advected by the evaluator's outputs at their places, survivors keep
    order and ids, and the second emission uses the next update counter and the next ids"""
    p = dc.emit_params()
    slot, index = dc.standard_rows(case)
    w, ds, first, (st1,), pot = emitted_by(case, p)
    at = w.evaluate_fields(first["positions"], density=False, velocity=True, count=True)
    ds.update(dc.EMIT_DT)
    got, st2 = ds.get(), ds.stats()
    moved, (dissolved, killed) = dr.advect(first["positions"], first["velocities"], first["lifetime"], first["id"], at["count"], at["velocity"], p, dc.EMIT_DT)
    new, (emitted, dropped), _ = dr.emit(case["x"], case["v"], slot, index, pot, p, dc.EMIT_DT, 1, case["r"], st1["emitted"], 100000 - len(moved["id"]))
    want = {k: np.concatenate([moved[k], new[k]]) for k in SET_KEYS}
    same_bits(got, want)
    assert len(set(moved["kind"].tolist())) >= 2 and emitted > 100 and not np.array_equal(new["positions"][:20], first["positions"][:20])
    kinds = np.bincount(got["kind"], minlength=4)
    assert [st2[k] for k in ("spray", "foam", "bubble", "new")] == kinds.tolist() and st2["count"] == len(got["id"])
    assert (st2["dissolved"], st2["killed"], st2["emitted"], st2["total_emitted"]) == (dissolved, killed, emitted, st1["emitted"] + emitted)
    ds.clear()
    assert len(ds) == 0 and ds.stats()["count"] == 0 and ds.stats()["total_emitted"] == st1["emitted"] + emitted
    ds.add(case["x"][:3], case["v"][:3])
    assert ds.get()["id"].tolist() == [st1["emitted"] + emitted + k for k in range(3)] and ds.get()["lifetime"].tolist() == [5.0] * 3  # ids run on


def test_advection_of_hand_placed_particles(hip_lib):
    """A block in slow motion; particles deep inside, on a face, off a face, far outside, short-lived, NaN, outside the kill box.  The
    class limits are set from the evaluator's own counts, so that N = n_spray and N = n_bubble occur by construction."""
    b = dc.still_block()
    w, _ = dc.one_fluid_world(b["x"], b["v"], b["vol"], b["r"])
    at = w.evaluate_fields(b["points"], density=False, velocity=True, count=True)
    n = at["count"].astype(np.int64)
    print("counts at the diffuse particles:", n.tolist())
    assert n[0] > n[1] >= n[4] >= n[2] > 0 and n[7] > n[1] and n[3] == 0 and n[5] == 0
    p = dr.Params(n_spray=int(n[2]), n_bubble=int(n[1]), k_ta=0.0, k_wc=0.0, kill_box=b["kill_box"], gravity=(0.0, -9.81, 0.0))
    ds = w.create_diffuse(16, dc.mirror(p))
    ds.add(b["points"], b["velocities"], b["lifetime"])
    seeded = ds.get()
    assert seeded["kind"].tolist() == [dr.NEW] * 8 and seeded["id"].tolist() == list(range(8)) and ds.stats()["new"] == 8
    assert np.array_equal(seeded["positions"].view(np.uint32), b["points"].view(np.uint32))
    ds.update(dc.EMIT_DT)
    got, st = ds.get(), ds.stats()
    want, (dissolved, killed) = dr.advect(b["points"], b["velocities"], b["lifetime"], np.arange(8), n, at["velocity"], p, dc.EMIT_DT)
    same_bits(got, want)
    # inside: bubble; on the face (N = n_bubble) and off it (N = n_spray): foam; far outside: spray; short-lived foam dissolves; two killed
    assert got["id"].tolist() == [0, 1, 2, 3, 7] and got["kind"].tolist() == [dr.BUBBLE, dr.FOAM, dr.FOAM, dr.SPRAY, dr.BUBBLE]
    assert (dissolved, killed) == (1, 2) and (st["dissolved"], st["killed"], st["emitted"], st["count"]) == (1, 2, 0, 5)
    assert (st["spray"], st["foam"], st["bubble"], st["new"]) == (1, 2, 2, 0)
    assert st["count"] + st["total_dissolved"] + st["total_killed"] == 8 + st["total_emitted"]  # the stats add up
    assert got["velocities"][3][1] < 0 and got["lifetime"][1] == np.float32(3.0) - np.float32(dc.EMIT_DT)  # the spray falls, the foam ages


def test_set_state(hip_lib, tmp_path):
    """(with test_state's twin above: the world that updates a set after every step keeps the twin's fluid bits)"""
    s = child("state", tmp_path)
    assert np.array_equal(s["end_x"], s["twin_x"]) and np.array_equal(s["end_v"], s["twin_v"])
    assert s["first_set"].tolist() == [2, 0]  # before the first step: the two seeds, nothing emitted by a fluid at rest
    count, emitted, dissolved, killed, dropped, length = s["set_stats"].tolist()
    assert emitted > 0 and count == length == 2 + emitted - dissolved - killed and dropped == 0


def test_set_device_pointers(hip_lib, tmp_path):
    s = child("set_device", tmp_path)
    n = int(s["n_dev"][0])
    assert n == len(s["host_id"]) == len(s["other_id"]) and n >= 4
    for k, width in (("positions", 3), ("velocities", 3), ("lifetime", 1), ("kind", 1), ("id", 1)):
        assert np.array_equal(s["host_" + k].view(np.uint32), s["other_" + k].view(np.uint32)), k        # add: device arm = host arm
        assert np.array_equal(s["dev_" + k][:width * n].view(np.uint32), s["other_" + k].view(np.uint32)), k  # get: device arm = host arm
        assert (s["dev_" + k][width * n:].view(np.int32) == (-1 if k in ("kind", "id") else np.float32(-1.0).view(np.int32))).all(), k


def test_set_refusals(hip_lib, case):
    from salva_amd import dist

    w, _ = fc.standard_world(case)
    w.sync_to_device(apply_removal=False)
    Lw, h = w._L, w._h
    sid = C.c_uint32(77)
    assert Lw.salva_hip_create_diffuse(h, 0, C.byref(sid)) == _lib.E_INVALID and Lw.salva_hip_create_diffuse(h, 1 << 31, C.byref(sid)) == _lib.E_INVALID
    assert Lw.salva_hip_create_diffuse(h, 8, None) == _lib.E_INVALID and sid.value == 77
    ds = w.create_diffuse(8)
    p = params()
    x = np.zeros((9, 3), np.float32)
    fp = C.POINTER(C.c_float)
    xp = x.ctypes.data_as(fp)
    assert Lw.salva_hip_add_diffuse(h, ds._set, 9, xp, xp, None, 0) == _lib.E_CAPACITY and "room left" in last_error() and len(ds) == 0
    assert Lw.salva_hip_add_diffuse(h, ds._set, 2, xp, None, None, 0) == _lib.E_INVALID and Lw.salva_hip_add_diffuse(h, ds._set, 2, xp, xp, None, 4) == _lib.E_INVALID
    assert Lw.salva_hip_add_diffuse(h, ds._set, 0, None, None, None, 0) == _lib.OK
    ds.add(x[:5], x[:5])
    n = C.c_uint64(0)
    out = _lib.DiffuseOut()
    ids = np.full(8, CANARY, np.uint32)
    out.id, out.row_capacity = u32p(ids), 4
    assert Lw.salva_hip_get_diffuse(h, ds._set, 0, C.byref(out), C.byref(n)) == _lib.E_CAPACITY and n.value == 5 and (ids == CANARY).all()
    out.row_capacity = 5
    assert Lw.salva_hip_get_diffuse(h, ds._set, 0, C.byref(out), C.byref(n)) == _lib.OK and ids.tolist() == [0, 1, 2, 3, 4] + [CANARY] * 3
    assert Lw.salva_hip_get_diffuse(h, ds._set, 2, C.byref(out), C.byref(n)) == _lib.E_INVALID and Lw.salva_hip_get_diffuse(h, ds._set, 0, None, None) == _lib.E_INVALID
    assert Lw.salva_hip_get_diffuse_stats(h, ds._set, None) == _lib.E_INVALID
    for dt in (float("nan"), float("inf"), -1.0e-3):
        assert Lw.salva_hip_update_diffuse(h, ds._set, 3, C.byref(p), dt) == _lib.E_INVALID and "dt" in last_error()
    assert Lw.salva_hip_update_diffuse(h, ds._set, 3, None, 0.005) == _lib.E_INVALID
    assert Lw.salva_hip_update_diffuse(h, ds._set, 0b100, C.byref(p), 0.005) == _lib.E_INVALID and "selects no existing fluid" in last_error()
    assert Lw.salva_hip_update_diffuse(h, ds._set, 3, C.byref(params(k_d=2.0)), 0.005) == _lib.E_INVALID
    assert Lw.salva_hip_update_diffuse(h, 5, 3, C.byref(p), 0.005) == _lib.E_INVALID and "no such diffuse set" in last_error()
    assert len(ds) == 5 and Lw.salva_hip_update_diffuse(h, ds._set, 3, C.byref(p), 0.0) == _lib.OK  # dt = 0 is allowed
    w.step(fc.DT, (0.0, 0.0, 0.0))
    ds.destroy()
    for code in (Lw.salva_hip_update_diffuse(h, ds._set, 3, C.byref(p), 0.005), Lw.salva_hip_destroy_diffuse(h, ds._set), Lw.salva_hip_clear_diffuse(h, ds._set),
                 Lw.salva_hip_get_diffuse(h, ds._set, 0, None, C.byref(n)), Lw.salva_hip_add_diffuse(h, ds._set, 1, xp, xp, None, 0)):
        assert code == _lib.E_INVALID and "destroyed" in last_error()
    w.step(fc.DT, (0.0, 0.0, 0.0))
    # a loopback-decomposed world
    wd, _ = fc.standard_world(case)
    wd.sync_to_device(apply_removal=False)
    dd = wd.create_diffuse(8)
    wd.set_domain(dist.Comm.loopback(1)[0], -1000, 1000)
    assert wd._L.salva_hip_update_diffuse(wd._h, dd._set, 3, C.byref(p), 0.005) == _lib.E_INVALID and "host-order arrays are not maintained" in last_error()


def test_update_refused_inside_a_force_callback(hip_lib, case):
    from salva_amd import NonPressureForce

    class Calls(NonPressureForce):
        def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
            p = params()
            self.seen = (self.world._L.salva_hip_update_diffuse(self.world._h, self.set._set, 3, C.byref(p), 0.005), last_error())

    w, (f0, _) = fc.standard_world(case)
    force = Calls()
    force.world, force.set = w, w.create_diffuse(8)
    f0.nonpressure_forces.append(force)
    st = w.step(fc.DT, (0.0, 0.0, 0.0))
    assert force.seen[0] == _lib.E_INVALID and "callback" in force.seen[1], force.seen
    assert st is not None and w._nsteps == 1


def test_foam3_example_agrees_with_the_python_mirror(hip_lib):
    """examples/foam3.cpp (the C++ mirror): the basic3 dam break, an update after every one of 60 steps; the counts per kind and the
    totals it prints are the Python mirror's of the same scene."""
    import re

    root = os.path.dirname(TESTS)
    exe = os.path.join(root, "examples", "foam3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "foam3"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"after 60 steps: (\d+) diffuse particles: spray (\d+), foam (\d+), bubbles (\d+), new (\d+)\n"
                  r"emitted (\d+), dissolved (\d+), killed (\d+), dropped (\d+)", r.stdout)
    assert m, r.stdout
    got = tuple(int(g) for g in m.groups())
    want = dc.foam3()
    print(got)
    assert got == want and got[0] > 0 and got[5] >= got[0] and got[0] == sum(got[1:5])
