"""One step from long-run device states against the CPU oracle (tests/transplant.py).

At the bench sizes the lockstep oracle runs (tests/test_full_size_gpu.py) see the first 30-32 steps only; the trajectories diverge
chaotically long before the settled tank, the stray particles, the folded grid and the two-tile plane layouts of the later steps.
Here each device world runs with every fast path at its default, and at fixed steps its checkpoint is loaded into fresh oracle
worlds and the next device step is compared with one oracle step: identical inputs, so contact sets exact and every field at
step-0 bounds.  Each checkpoint also asserts the regime it is there for (halo size, launch classes, fold, chain, pre-enqueued
grid), so that a drifting scene fails loudly instead of silently testing the easy regime.  The whole file: 136 s on an MI355X box
with 16 oracle threads (config 2 56 s, config 4 30 s, the 8 x 10^6 world 24 s)."""
import re
import time

import numpy as np
import pytest

from parity import DT, GRAVITY, Scene
from transplant import one_step_against_oracle

pytestmark = pytest.mark.gpu
R = 0.025
SWITCHES = ("SALVA_HIP_NO_CLASSES", "SALVA_HIP_CLASSES", "SALVA_HIP_NO_PLANES", "SALVA_HIP_NO_FOLD", "SALVA_HIP_NO_SPLIT", "SALVA_HIP_LIGHT",
            "SALVA_HIP_SPLIT_S", "SALVA_HIP_NO_TWO_MASS", "SALVA_HIP_NO_PREGRID", "SALVA_HIP_FOLD_CELLS", "SALVA_HIP_SPEC_TIGHT",
            "SALVA_HIP_MAX_MASSES", "SALVA_HIP_TILE_TRACE", "SALVA_HIP_SPECULATE", "SALVA_HIP_NO_SPECULATION")
TRACE = re.compile(r"salva_hip tiles: .* \| fold (\d+) (\d+) (\d+)")


@pytest.fixture
def defaults(monkeypatch):
    """Every fast path at its default: none of the product's A/B switches set."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def config_scene(config, side=100):
    """bench.build_config + bench.make_config_world as a parity.Scene."""
    import bench

    fluids, shell = bench.build_config(config, side)
    s = Scene(R, 2.0, "iisph" if config == 3 else "dfsph")
    for pos, rho0 in fluids:
        s.add_fluid(pos, None, rho0, forces=[("akinci", 1.0, 10.0)] if config == 3 else [("xsph", 0.5, 0.0)])
    s.add_boundary(shell)
    return s


def run_to(w, k, target):
    while k < target:
        w.step(DT, GRAVITY)
        k += 1
    return k


def run_to_stable_box(w, fls, k, first, last):
    """Step until the last two steps have left the particles' cell box as they found it, from step `first` on (at most to `last`):
    the step before the last ran on the box its predecessor used, so it enqueued the next step's grid part, and the last one kept
    the box, so the device opened the gate for it (world_step.hip, World::publish_end_of_step; world.h PreGrid) — the next step adopts it.  Returns
    the step count.  (Positions read between the steps do not change the path: the twin of
    test_config2_one_step_from_the_long_run.)"""
    hf = np.float32(w.h())

    def cell_box():
        p = np.concatenate([np.asarray(h.positions, np.float32) for h in fls])
        c = np.floor(p / hf)
        return tuple(c.min(axis=0).tolist() + c.max(axis=0).tolist())
    boxes = [None, None]
    while k < last:
        k = run_to(w, k, k + 1)
        box = cell_box()
        if k >= first and box == boxes[-1] == boxes[-2]:
            return k
        boxes = [boxes[-1], box]
    raise AssertionError(f"the cell box changed in every step from {first} to {last}")


def folds(err):
    """Fold periods (cells per axis, 0 = unfolded) of the SALVA_HIP_TILE_TRACE lines in `err`."""
    return [tuple(int(x) for x in m.groups()) for m in TRACE.finditer(err)]


def test_config2_one_step_from_the_long_run(defaults, capfd):
    """Config 2 (the bench scene, DFSPH + XSPH, 10^6) for 1000 steps: the first capped divergence solves (~step 40), the settled
    tank on the two-tiles-per-CU plane layouts (~350), and the strays of the leaking tank on a folded grid with launches of their
    own (~1000).  A twin world run to the same step without any read in between ends bit-identical: the checkpoints did not
    change the path under test."""
    scene = config_scene(2)
    defaults.setenv("SALVA_HIP_TILE_TRACE", "1")  # (read when the world is built: the twin below runs without it)
    w, fls, bds = scene.make_hip()
    defaults.delenv("SALVA_HIP_TILE_TRACE")
    res, log = {}, []

    def compare(K):
        capfd.readouterr()
        r = one_step_against_oracle(w, fls, bds, scene, f"config 2, step {K + 1}")
        cap = capfd.readouterr()
        r["fold"] = folds(cap.err)
        log.append(cap.out + f"config 2, step {K + 1}: fold periods {r['fold']}, chain breaks so far {w.counters.chain_breaks}\n")
        return r
    try:
        _config2_checkpoints(w, fls, scene, compare, res)
    finally:
        print("".join(log), end="")


def _config2_checkpoints(w, fls, scene, compare, res):
    k = run_to(w, 0, 40)
    res[40] = compare(40)
    k += 1
    assert w.counters.chain_breaks > 0, f"no chain has broken by step {k}: {w.counters}"
    # the first step after the impact that adopts the pre-enqueued grid
    k = run_to_stable_box(w, fls, k, 100, 340)
    res["pregrid"] = compare(k)
    k += 1
    assert res["pregrid"]["counters"]["pregrid_adopted"] > 0, f"step {k} did not adopt the pre-enqueued grid: {res['pregrid']}"
    for K in (350, 999):
        k = run_to(w, k, K)
        res[K] = compare(K)
        k += 1
    assert res[350]["reserved"][0] > 2080, f"step 351 did not run the two-tile layouts: {res[350]['reserved']}"
    assert res[999]["counters"]["sparse_class_passes"] > 0 and res[999]["strays"] > 0, res[999]
    assert res[999]["fold"] and all(any(p) for p in res[999]["fold"]), f"the grid is not folded at step 1000: {res[999]['fold']}"

    twin, tfls, _ = scene.make_hip()
    run_to(twin, 0, k)
    for a, b in zip(fls, tfls):
        assert np.array_equal(a.positions, b.positions) and np.array_equal(a.velocities, b.velocities)
        assert np.array_equal(w.velocity_changes(a), twin.velocity_changes(b))


def test_config2_look_first_then_step(defaults):
    """A ContactManager user reads the contacts of step K before it asks for step K+1, and step K+1 adopts the grid part step K
    enqueued: the export leaves the error flags dirty (`flags_clean` = false) in front of an adopted grid (second item).
    K is the first step from 200 on after two steps that kept the cell box; the adopting step after the export against the oracle."""
    scene = config_scene(2)
    w, fls, bds = scene.make_hip()
    k = run_to(w, 0, 199)
    k = run_to_stable_box(w, fls, k, 200, 340)
    for h in fls:
        off, jm, j = w.fluid_contacts(h)
        assert int(off[-1]) == len(j) > 0
        w.fluid_contacts(h, True)
    r = one_step_against_oracle(w, fls, bds, scene, f"config 2, step {k + 1} after a contact export")
    assert r["counters"]["pregrid_adopted"] > 0, f"step {k + 1} did not adopt the pre-enqueued grid: {r['counters']}"


def test_config2_speculative_step(defaults):
    """Speculative table sizing is opt-in (SALVA_HIP_SPECULATE=1): a world that has it on, compared at step 301, where the
    compared pass must have been speculative."""
    scene = config_scene(2)
    defaults.setenv("SALVA_HIP_SPECULATE", "1")
    w, fls, bds = scene.make_hip()
    defaults.delenv("SALVA_HIP_SPECULATE")
    run_to(w, 0, 300)
    r = one_step_against_oracle(w, fls, bds, scene, "config 2 (speculative sizing), step 301")
    assert r["counters"]["speculative_passes"] > 0, r["counters"]


def test_config3_iisph_akinci_one_step_after_500(defaults, capfd):
    """Config 3 (IISPH + Akinci2013(1, 10) in the open tank, 10^6) at step 500: the burst block — strays outside the tank in every
    direction, launches of their own for the sparse slots, a folded grid — with the pressures carried over.  Akinci's normalised
    terms move by ~1e-3 m/s between f32 and f64 in one step at this size: the noise-floor rule decides."""
    scene = config_scene(3)
    defaults.setenv("SALVA_HIP_TILE_TRACE", "1")
    w, fls, bds = scene.make_hip()
    defaults.delenv("SALVA_HIP_TILE_TRACE")
    run_to(w, 0, 499)
    run = folds(capfd.readouterr().err)
    first = next((i for i, p in enumerate(run) if any(p)), None)
    r = one_step_against_oracle(w, fls, bds, scene, "config 3, step 500")
    cap = capfd.readouterr()
    print(cap.out, end="")
    fold = folds(cap.err)
    print(f"config 3, step 500: fold periods {fold} (first folded pass of the run: {first})")
    assert r["iters"][1] >= 2, f"the pressure solve did not iterate: {r['iters']}"
    assert r["strays"] > 0, "no particle has left the tank by step 500"
    assert r["counters"]["sparse_class_passes"] > 0, f"step 500 ran no sparse-class launch: {r['counters']}"
    assert fold and all(any(p) for p in fold), f"the grid is not folded at step 500: {fold}"


def test_config4_two_fluids_one_step_after_300(defaults):
    """Config 4 (two fluids of 10^6, rho0 1000 / 500, DFSPH + XSPH) at step 300, settled and compressed.  The world ran the
    two-mass plane layouts: a twin with SALVA_HIP_NO_TWO_MASS=1 (the general kernels) does not end bit-identical."""
    scene = config_scene(4)
    w, fls, bds = scene.make_hip()
    run_to(w, 0, 299)
    one_step_against_oracle(w, fls, bds, scene, "config 4, step 300")
    defaults.setenv("SALVA_HIP_NO_TWO_MASS", "1")
    twin, tfls, _ = scene.make_hip()
    defaults.delenv("SALVA_HIP_NO_TWO_MASS")
    run_to(twin, 0, 300)
    assert not all(np.array_equal(a.velocities, b.velocities) for a, b in zip(fls, tfls)), "the two-mass path never switched on"


def _mem_available_gib():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / (1024.0 * 1024.0)
    except OSError:
        pass
    return 0.0


def test_undivided_8m_world_against_the_f32_oracle(defaults):
    """The undivided config-5-sized world (bench.build_config(2, 200), 8 x 10^6 particles): step 1 and step 31 against the f32
    oracle (no f64 or reordered twin: the oracle's contacts take 48 B each, ~13 GB here).  Measured on an MI355X box with 16
    oracle threads, this test alone: 29 s wall, 18.2 GiB peak RSS (each oracle step ~9 s)."""
    if _mem_available_gib() < 32.0:
        pytest.skip(f"MemAvailable {_mem_available_gib():.1f} GiB < 32 GiB: the 8 x 10^6 oracle does not fit")
    import resource

    t0 = time.perf_counter()
    scene = config_scene(2, 200)
    w, fls, bds = scene.make_hip()
    one_step_against_oracle(w, fls, bds, scene, "8M, step 1", sample=20000, f64=False)
    run_to(w, 1, 30)
    one_step_against_oracle(w, fls, bds, scene, "8M, step 31", sample=20000, f64=False)
    print(f"8M: wall {time.perf_counter() - t0:.0f} s, peak RSS {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GiB")


@pytest.mark.parametrize("solver", ["dfsph", "iisph"])
def test_two_fluid_scene_one_step_after_200_against_the_numpy_reading(hip_lib, defaults, solver):
    """HIP -> independent f64 reading (tests/numpy_reading.py) in a long-run state, with no oracle in between: the two-fluid scene of
    tests/test_numpy_reading_gpu.py after 200 device steps, loaded into the reading (x, v, dv, p, dt, inv_dt), one step compared
    at that file's bounds with the contact count exact."""
    from test_numpy_reading_gpu import DT32, G32, TOL_RHO, TOL_V, TOL_X, two_fluid_worlds

    w, fa, fb, dw = two_fluid_worlds(solver)
    for _ in range(200):
        w.step(DT, GRAVITY)
    ck = w.checkpoint()
    for f in range(2):
        rows = dw.fluid_rows(f)
        dw.x[rows] = ck[f"fluid{f}_positions"]
        dw.v[rows] = ck[f"fluid{f}_velocities"]
        dw.dv[rows] = ck[f"fluid{f}_velocity_changes"]
        dw.p[rows] = ck[f"fluid{f}_pressures"]
        dw.vol[rows] = ck[f"fluid{f}_volumes"]
    dw.dt, dw.inv_dt = float(ck["timestep"][0]), float(ck["timestep"][1])
    st = w.step(DT, GRAVITY)
    dw.step(DT32, G32)
    assert int(st.ncontacts) == dw.ncontacts, f"contacts {st.ncontacts} vs {dw.ncontacts}"
    h = dw.h
    for fl, rows in ((fa, dw.fluid_rows(0)), (fb, dw.fluid_rows(1))):
        dx = np.abs(np.asarray(fl.positions, np.float64) - dw.x[rows]).max()
        dv = np.abs(np.asarray(fl.velocities, np.float64) - dw.v[rows]).max()
        assert dx < TOL_X * h, f"positions differ by {dx / h:.2e} h"
        assert dv < TOL_V, f"velocities differ by {dv:.2e} m/s"
    rho = np.concatenate([w.densities(fa), w.densities(fb)])
    drho = np.abs(rho - dw.rho).max() / dw.rho.max()
    assert drho < TOL_RHO, f"densities differ by {drho:.2e} relative"
    print(f"numpy reading after 200 steps ({solver}): |dx| {dx / h:.2e} h, |dv| {dv:.2e} m/s, |drho| / rho {drho:.2e}, "
          f"contacts {dw.ncontacts}, iters {st.n_divergence_iters} {st.n_pressure_iters}")
