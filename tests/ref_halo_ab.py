"""The A/B harness of the referenced-only halo tests (test_referenced_halo_gpu.py, test_referenced_halo_matrix_gpu.py,
test_time_kernel_gpu.py): the same scene with SALVA_HIP_FULL_HALO=1 (the full 6x6x6 box in every step) and with
SALVA_HIP_REF_HALO=1 (the referenced slots only, in every step), compared bit for bit.

The switches are read in the World constructor: they are set around world creation only and restored afterwards.  For in-process
ranks (threads) they are set before the threads start and restored after the last one has joined — the environment is process-wide."""
import os
from contextlib import contextmanager

import numpy as np

from parity import DT, GRAVITY, Scene
from salva_amd import scenes

R = 0.025
SWITCHES = ("SALVA_HIP_FULL_HALO", "SALVA_HIP_REF_HALO", "SALVA_HIP_NO_SPLIT", "SALVA_HIP_FOLD_CELLS", "SALVA_HIP_CLASSES", "SALVA_HIP_NO_PLANES",
            "SALVA_HIP_REF_TIGHT", "SALVA_HIP_SPLIT_S", "SALVA_HIP_LIGHT", "SALVA_HIP_DS_LEVEL", "SALVA_HIP_MAX_MASSES", "SALVA_HIP_NO_CHAIN",
            "SALVA_HIP_NO_PREGRID", "SALVA_HIP_NO_DEFER_LISTS", "SALVA_HIP_SPECULATE", "SALVA_HIP_NO_SPECULATION", "SALVA_HIP_NO_CLASSES",
            "SALVA_HIP_NO_FOLD", "SALVA_HIP_SPEC_TIGHT")
ON, OFF = {"SALVA_HIP_REF_HALO": "1"}, {"SALVA_HIP_FULL_HALO": "1"}
# what a step's launches were cut for and what was built, from LiquidWorld.tile_tables (salva_hip_get_tile_tables): info[5] / [6] / [7] =
# the fluid | fluid + boundary | padded fluid + boundary halo that picks the layouts (pairs.h pick_ds_p3 / pick_ds_p2 / pick_ds),
# [8] the fullest box, [9] = 1 when the step kept the referenced slots only, [10] / [11] such passes so far / those repeated
P3_DS_THREE, P2_DS_THREE, FIXED_DS_SMALL = 2080, 2464, 2448  # tile.h


@contextmanager
def switches(env):
    """The environment a world is created in: every switch of SWITCHES cleared, then `env`; put back afterwards."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _make(env, scene):
    with switches(env):
        return scene.make_hip()


def _info(w):
    return w.tile_tables(0)[0]


def _run(env, scene, nsteps, look=(0, 1, -1)):
    w, fls, _ = _make(env, scene)
    look = {k % nsteps for k in look}
    trace, halos, seen, infos = [], [], [], []
    for k in range(nsteps):
        st = w.step(DT, GRAVITY)
        trace.append((st.n_divergence_iters, st.n_pressure_iters, int(st.ncontacts)))
        halos.append(int(st.reserved[0]))
        infos.append(_info(w))
        if k in look:
            seen.append([w.fluid_contacts(f) for f in fls] + [w.fluid_contacts(f, True) for f in fls])
    return w, fls, trace, halos, seen, infos


def _same(wa, fa, wb, fb):
    for x, y in zip(fa, fb):
        assert np.array_equal(x.positions, y.positions) and np.array_equal(x.velocities, y.velocities)
        assert np.array_equal(wa.densities(x), wb.densities(y))
        assert np.array_equal(wa.contact_counts(x), wb.contact_counts(y)) and np.array_equal(wa.contact_counts(x, True), wb.contact_counts(y, True))


def _same_exports(sa, sb):
    assert len(sa) == len(sb) > 0
    for a, b in zip(sa, sb):
        for (o1, m1, j1), (o2, m2, j2) in zip(a, b):
            assert np.array_equal(o1, o2) and np.array_equal(m1, m2) and np.array_equal(j1, j2)  # the same neighbours, in the same ORDER


def _bench_block(side, solver="dfsph", forces=(("xsph", 0.5, 0.0),), strays=0):
    """The bench scene at a reduced side: a jittered block in a tank, falling."""
    s = Scene(R, 2.0, solver)
    fluid, shell = scenes.tank(side, side, side, R)
    fluid = scenes.jitter(fluid, 0.1 * R, seed=11)
    if strays:  # single particles far from the block and from each other: one tile each (the sparse class)
        rng = np.random.default_rng(5)
        far = (fluid.max(axis=0) + np.float32(40 * R) + rng.uniform(0.0, 400 * R, size=(strays, 3))).astype(np.float32)
        fluid = np.ascontiguousarray(np.concatenate([fluid, far]))
    s.add_fluid(fluid, scenes.random_velocities(len(fluid), 0.2, seed=4), 1000.0, forces=list(forces))
    s.add_boundary(shell)
    return s


# ---- what every A/B case asserts (test_referenced_halo_matrix_gpu.py)
def check_switch(i_full, i_kept, declined=False):
    """The A/B switch itself: the full-box arm never kept, the other arm kept in EVERY step and dropped a slot in some step —
    otherwise the case compares a path with itself.  `declined`: a case of the decline table — neither arm keeps."""
    assert all(int(i[9]) == 0 and int(i[5]) == int(i[8]) for i in i_full), "the full-box arm staged something else than the full box"
    if declined:
        assert all(int(i[9]) == 0 for i in i_kept), [int(i[9]) for i in i_kept]
        return
    assert all(int(i[9]) == 1 for i in i_kept), [int(i[9]) for i in i_kept]
    assert any(int(i[5]) < int(i[8]) for i in i_kept), [(int(i[8]), int(i[5])) for i in i_kept]


def check_discards(w_full, w_kept, i_kept, may_miss=False):
    """counters.discarded_passes: the kept arm discards what the full-box arm discards plus the passes it repeated because a kept
    halo outgrew its bound (info[11]) — none, unless the case says its halos may grow faster than the margin (`may_miss`)."""
    d = int(w_kept.counters.discarded_passes) - int(w_full.counters.discarded_passes)
    assert d == int(i_kept[-1][11]), (d, int(i_kept[-1][11]))
    assert may_miss or d == 0, d


def _print_force_distance(name, e0, e1):
    """(measured before it is asserted) the largest difference between the arms' boundary forces, relative to the largest force"""
    worst = 0.0
    for a, b in zip(e0, e1):
        for x, y in zip(a, b):
            if isinstance(x, np.ndarray) and x.dtype == np.float32 and x.shape == np.shape(y) and x.size:
                worst = max(worst, float(np.abs(x - y).max()) / max(float(np.abs(x).max()), 1e-30))
    print(f"{name}: boundary forces of the two arms differ by at most {worst:.3e} of the largest force")


def report(name, nparticles, i_kept):
    """One line per case for the pull request text: scene size, (full, kept) halo maxima of the last step, repeated passes."""
    print(f"{name}: n = {nparticles}, last step (full, kept) = ({int(i_kept[-1][8])}, {int(i_kept[-1][5])}), kept passes {int(i_kept[-1][10])}, "
          f"repeated {int(i_kept[-1][11])}")


def ab(name, scene, nsteps, env=None, declined=False, may_miss=False, prepare=None, between=None, extra=None, dt=DT):
    """Both arms of one case over a `Scene`, every assertion of the set.  prepare(w, fluids, boundaries) runs once after creation,
    between(k, w, fluids, boundaries) after step k (the same seeded edits in both arms), extra(w, fluids, boundaries) -> anything
    comparable with == or np.array_equal, taken after every step (boundary forces, wrenches, query results)."""
    env = env or {}
    out = []
    for arm in (OFF, ON):
        print(name, "arm", arm)
        with switches(dict(env, **arm)):
            w, fls, bds = scene.make_hip()
        if prepare:
            prepare(w, fls, bds)
        look = {0, 1, nsteps - 1}
        trace, halos, seen, infos, extras = [], [], [], [], []
        for k in range(nsteps):
            st = w.step(dt, GRAVITY)
            trace.append((st.n_divergence_iters, st.n_pressure_iters, int(st.ncontacts)))
            halos.append(int(st.reserved[0]))
            infos.append(_info(w))
            live = [f for f in w.fluids()]
            if k in look:
                seen.append([w.fluid_contacts(f) for f in live] + [w.fluid_contacts(f, True) for f in live])
            ex = [np.array(b.forces) for b in w.boundaries() if b.wants_forces and b.forces is not None]
            if extra:
                ex.append(extra(w, live, list(w.boundaries())))
            extras.append(ex)
            if between and k + 1 < nsteps:
                between(k, w, fls, bds)
        out.append((w, [f for f in w.fluids()], trace, halos, seen, infos, extras))
    (w0, f0, t0, h0, s0, i0, e0), (w1, f1, t1, h1, s1, i1, e1) = out
    report(name, sum(f.num_particles() for f in f1), i1)
    check_switch(i0, i1, declined)
    assert t1 == t0, [(k, a, b) for k, (a, b) in enumerate(zip(t0, t1)) if a != b][:3]
    assert h1 == h0
    assert len(f0) == len(f1)
    _same(w1, f1, w0, f0)
    _same_exports(s1, s0)
    _print_force_distance(name, e0, e1)
    assert same_tree(e1, e0), "boundary forces / wrenches / query results differ"
    check_discards(w0, w1, i1, may_miss)
    return out


def same_tree(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b
