"""salva_hip_time_kernel (bench.py --full takes every roofline figure from it) leaves the world alone: twin worlds stepped k times,
one of them timed with every kernel id its solver accepts, then both run five more steps — the same bits in every field and the
same iteration / contact trace.

Kernel 4 (the list build) is the one id that rewrites state a reader can see: it rebuilds the lists — and, behind a step that kept
the referenced halo, the slot tables — from the positions as they are AFTER the step (include/salva_hip.h says so).  Until the next
step the contact counts, the contact exports and the tile tables describe those lists: every exported pair lies within h of each
other at the current positions, and the counts agree with the export.  The particle state and the run that follows are untouched."""
import numpy as np
import pytest

from parity import DT, GRAVITY, Scene
from ref_halo_ab import OFF, ON, R, _bench_block, _info, switches
from salva_amd import Becker2009Elasticity, scenes
from salva_amd._lib import SalvaHipError

pytestmark = pytest.mark.gpu
H = 4 * R
IDS = {"dfsph": (0, 1, 6, 4), "iisph": (2, 3, 4)}
OTHER = {"dfsph": (2, 3), "iisph": (1, 6)}


def _state(w, fls):
    return [(np.array(f.positions), np.array(f.velocities), w.densities(f)) for f in fls]


def _counts(w, fls):
    return [(w.contact_counts(f), w.contact_counts(f, True)) for f in fls]


def _equal(a, b):
    return all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


def _steps(w, n):
    out = []
    for _ in range(n):
        st = w.step(DT, GRAVITY)
        out.append((st.n_divergence_iters, st.n_pressure_iters, int(st.ncontacts), int(st.reserved[0])))
    return out


def _lists_describe_the_current_positions(w, fls):
    """After kernel 4: counts == export, and every fluid-fluid pair is within h at the positions as they are now."""
    pos = [np.array(f.positions) for f in fls]
    for k, f in enumerate(fls):
        off, jm, j = w.fluid_contacts(f)
        cnt = (off[1:] - off[:-1]).astype(np.uint32)
        assert np.array_equal(cnt, w.contact_counts(f)) and int(off[-1]) == len(j) > 0
        i = np.repeat(np.arange(len(cnt)), cnt.astype(np.int64))
        pj = np.stack([pos[int(m)][int(q)] for m, q in zip(jm[::97], j[::97])])
        d = np.linalg.norm(pos[k][i[::97]].astype(np.float64) - pj, axis=1)
        assert d.max() <= H * (1 + 1e-6), d.max()
        assert (cnt >= 1).all()  # the self contact


def _twins(scene, env, k, ids, others, prepare=None):
    worlds = []
    for _ in range(2):
        with switches(env):
            w, fls, _ = scene.make_hip()
        if prepare:
            prepare(w, fls)
        worlds.append((w, fls, _steps(w, k)))
    (wa, fa, ta), (wb, fb, tb) = worlds
    assert ta == tb and _equal(_state(wa, fa), _state(wb, fb))
    kept = int(_info(wa)[9])
    for kid in ids:
        us = wa.time_kernel(kid, reps=2)
        print("kernel", kid, f"{us:.1f} us", "(behind a kept-halo step)" if kept else "")
        assert np.isfinite(us) and us > 0.0, (kid, us)
        assert _equal(_state(wa, fa), _state(wb, fb)), f"kernel {kid} changed the particle state"
        if kid != 4:
            assert _equal(_counts(wa, fa), _counts(wb, fb)), f"kernel {kid} changed the contact counts"
        else:
            _lists_describe_the_current_positions(wa, fa)
    for kid in tuple(others) + (99,):
        with pytest.raises(SalvaHipError):
            wa.time_kernel(kid, reps=2)
    assert _equal(_state(wa, fa), _state(wb, fb))
    ta, tb = _steps(wa, 5), _steps(wb, 5)
    assert ta == tb, (ta, tb)
    assert _equal(_state(wa, fa), _state(wb, fb)) and _equal(_counts(wa, fa), _counts(wb, fb))
    assert int(wa.counters.discarded_passes) == int(wb.counters.discarded_passes)
    return wa, wb, kept


@pytest.mark.parametrize("solver", ["dfsph", "iisph"])
@pytest.mark.parametrize("halo", ["kept", "full"])
def test_time_kernel_leaves_the_world_alone(solver, halo):
    """Behind a step that kept the referenced halo (the `ref_last` branch of kernel 4) and behind one that did not."""
    wa, wb, kept = _twins(_bench_block(14, solver=solver), ON if halo == "kept" else OFF, 6, IDS[solver], OTHER[solver])
    assert kept == (1 if halo == "kept" else 0)
    assert int(_info(wa)[9]) == kept


def test_time_kernel_with_the_next_step_chained_and_its_grid_pre_enqueued():
    """A settled DFSPH block chains its steps and enqueues the next step's grid behind the publication (test_chain_gpu.py): the
    timed launches run between a step and the grid that is already waiting for the next one."""
    from test_chain_gpu import _drop_scene

    wa, wb, kept = _twins(_drop_scene(16), ON, 20, IDS["dfsph"], OTHER["dfsph"])
    c = wa.counters
    print("chained passes", int(c.chained_passes), "pre-enqueued grids adopted", int(c.pregrid_adopted), "dropped", int(c.pregrid_dropped))
    assert int(c.chained_passes) > 0 and int(c.pregrid_adopted) > 0, "the scene was meant to take the fast paths"
    assert (int(c.chained_passes), int(c.pregrid_adopted)) == (int(wb.counters.chained_passes), int(wb.counters.pregrid_adopted))


@pytest.mark.parametrize("halo", ["kept", "full"])
def test_time_kernel_elastic_passes(halo):
    """Kernels 7 and 8 (rotation + stress, force) of a Becker2009 block beside a fluid; the elastic state keeps what the step computed."""
    s = Scene(R, 2.0, "dfsph")
    fluid, shell = scenes.tank(22, 12, 12, R)
    fluid = scenes.jitter(fluid, 0.05 * R, seed=9)
    left = fluid[:, 0] < np.median(fluid[:, 0])
    s.add_fluid(np.ascontiguousarray(fluid[left]), None, 1000.0, forces=[("xsph", 0.5, 0.0)])
    s.add_fluid(np.ascontiguousarray(fluid[~left]), None, 1000.0)
    s.add_boundary(shell)

    def prepare(w, fls):
        fls[1].nonpressure_forces.append(Becker2009Elasticity(5e5, 0.3, True))

    wa, wb, kept = _twins(s, ON if halo == "kept" else OFF, 5, (7, 8, 0, 1, 6, 4), (2, 3), prepare=prepare)
    ea, eb = wa.elasticity_state(wa.fluids()._items[1], 0), wb.elasticity_state(wb.fluids()._items[1], 0)
    for key in ("rotations", "stress", "grad_tr", "positions0"):
        assert np.array_equal(ea[key], eb[key]), key


def test_time_kernel_needs_a_completed_step():
    with switches({}):
        w, fls, _ = _bench_block(8).make_hip()
    with pytest.raises(SalvaHipError):
        w.time_kernel(0, reps=1)
