"""The referenced-only halo (device_types.h StepCtx::tile_off, grid.hip k_nbr_tile_ref / k_ref_offsets).

A tile stages the 6x6x6-cell box around its 4x4x4 own cells, but a list can only name a halo particle within h of the own cube.  The
list builder therefore drops the slots no list names, compacts the tile's slot table in place and rewrites the list entries through
the rank of the kept slots.  The map is monotone, so every particle meets the same neighbours in the same order: nothing a particle
sees may change — the same bits in every field, the same iteration counts, the same exported lists (an export maps every entry back
through the compacted table: the same source particle, in the same place, as with the full box).

SALVA_HIP_REF_HALO=1 builds it in every step (by default only where some halo is beyond a three-per-CU layout), SALVA_HIP_FULL_HALO=1
never."""
import numpy as np
import pytest

from parity import Scene
from ref_halo_ab import (FIXED_DS_SMALL, OFF, ON, P2_DS_THREE, P3_DS_THREE, R, _bench_block, _make, _run, _same,  # noqa: F401 - the shared A/B harness
                         _same_exports)
from salva_amd import scenes

pytestmark = pytest.mark.gpu


def _two_fluids():
    s = Scene(R, 2.0, "dfsph")
    fluid, shell = scenes.tank(16, 24, 16, R)
    fluid = scenes.jitter(fluid, 0.1 * R, seed=3)
    mid = 0.5 * (float(fluid[:, 1].min()) + float(fluid[:, 1].max()))
    s.add_fluid(np.ascontiguousarray(fluid[fluid[:, 1] < mid]), None, 1000.0, forces=[("xsph", 0.5, 0.0)])
    s.add_fluid(np.ascontiguousarray(fluid[fluid[:, 1] >= mid]), None, 500.0, forces=[("xsph", 0.5, 0.0)])
    s.add_boundary(shell)
    return s


CASES = {
    "dfsph": (lambda: _bench_block(20), {}),
    "iisph_akinci": (lambda: _bench_block(16, solver="iisph", forces=(("akinci", 1.0, 10.0),)), {}),
    "two_mass": (_two_fluids, {}),
    "folded": (lambda: _bench_block(14), {"SALVA_HIP_FOLD_CELLS": "8"}),
    "strays": (lambda: _bench_block(14, strays=40), {"SALVA_HIP_CLASSES": "1"}),
    "general_kernels": (lambda: _bench_block(14), {"SALVA_HIP_NO_PLANES": "1"}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_kept_halo_changes_nothing_a_particle_sees(case):
    """30 steps with the switch on and off: positions, velocities, densities, list lengths, iteration counts and contact counts of every
    step, and the exported lists (fluid and boundary) of steps 1, 2 and 30, entry by entry."""
    make, env = CASES[case]
    sc = make()
    w0, f0, t0, h0, s0, i0 = _run(dict(env, **OFF), sc, 30)
    assert all(i[9] == 0 and i[5] == i[8] for i in i0), "the A/B switch: the full box everywhere"
    w1, f1, t1, h1, s1, i1 = _run(dict(env, **ON), sc, 30)
    print(case, "full box:", h0[:3], h0[-1], "(full, staged):", [(int(i[8]), int(i[5])) for i in i1[:3] + i1[-1:]])
    assert t1 == t0 and h1 == h0
    _same(w1, f1, w0, f0)
    _same_exports(s1, s0)
    # something was dropped in every step, and the launches were cut for less than the full box
    assert all(i[9] == 1 and i[5] < i[8] for i in i1), i1
    # no kept halo outgrew the bound its step was cut for (the previous step's maximum plus an eighth): nothing was computed twice
    # (a pass repeated because a list outgrew its capacity — with either switch — is built twice: at least one build per step)
    assert int(i1[-1][10]) >= 30 and int(i1[-1][11]) == 0, i1[-1]
    assert int(w1.counters.discarded_passes) == int(w0.counters.discarded_passes)


def test_a_kept_halo_beyond_its_bound_repeats_the_pass():
    """SALVA_HIP_REF_TIGHT=1 cuts the launches for an eighth LESS than the previous step's kept maxima: the list builder holds every
    tile to that cap, raises its flag where one does not fit, and the host repeats the pass with the full box's bounds — what a step
    whose halo grew faster than the margin goes through.  The run computes what the full box computes."""
    sc = _bench_block(20)
    w0, f0, t0, h0, s0, i0 = _run(OFF, sc, 12)
    w1, f1, t1, h1, s1, i1 = _run(dict(ON, SALVA_HIP_REF_TIGHT="1"), sc, 12)
    missed = int(i1[-1][11])
    print("passes repeated:", missed, "of", int(i1[-1][10]))
    assert missed >= 8, i1[-1]  # (the first step sizes its launches exactly; a repeated pass leaves no prediction for the next)
    assert int(w1.counters.discarded_passes) - int(w0.counters.discarded_passes) == missed
    assert t1 == t0 and h1 == h0
    _same(w1, f1, w0, f0)
    _same_exports(s1, s0)


def test_every_entry_names_the_same_particle_and_every_kept_slot_is_named():
    """One step's tables, tile by tile (all of them: the block has a few dozen), read back with the switch on and off: the tile's own
    range and list lengths agree; every list entry, mapped through the tile's slot table, names the same sorted particle; the kept
    table is the full one without the slots nobody names, in the same order; and every kept slot is named by some list or is an
    own particle — the builder keeps no superset."""
    sc = _bench_block(20)
    w0, *_ = _run(OFF, sc, 3, look=())
    w1, *_ = _run(ON, sc, 3, look=())
    nslots = int(w0.tile_tables(0)[0][0])
    assert nslots == int(w1.tile_tables(0)[0][0]) and nslots >= 27
    full = kept = 0
    for slot in range(nslots):
        a, row0, c0, e0 = w0.tile_tables(slot)
        b, row1, c1, e1 = w1.tile_tables(slot)
        assert (a[1], a[2], a[4]) == (b[1], b[2], b[4]) and np.array_equal(c0, c1)
        assert len(e0) == int(c0.sum()) == len(e1)
        assert e0.max() < len(row0) and e1.max() < len(row1)
        assert np.array_equal(row0[e0], row1[e1])  # entry by entry: the same source particle
        named0 = np.zeros(len(row0), bool)
        named0[e0] = True
        named0 |= (row0 >= a[1]) & (row0 < a[2])  # own particles stay
        assert np.array_equal(row1, row0[named0])  # what is left, in the same relative order
        named1 = np.zeros(len(row1), bool)
        named1[e1] = True
        named1 |= (row1 >= b[1]) & (row1 < b[2])
        assert named1.all(), (slot, int((~named1).sum()))  # no slot is staged that nobody names
        full += len(row0); kept += len(row1)
    print("halo slots of the step: full boxes", full, "kept", kept)
    assert kept < full


def _column(squeeze):
    """The compressed column of test_split_gpu.py, squeezed throughout: halos just beyond the three-per-CU plane layout."""
    s = Scene(R, 2.0, "dfsph")
    fluid, shell = scenes.tank(24, 30, 24, R)
    fluid = scenes.jitter(fluid, 0.1 * R, seed=2)
    y0 = float(fluid[:, 1].min())
    fluid[:, 1] = (y0 + (fluid[:, 1] - y0) * np.float32(squeeze)).astype(np.float32)
    s.add_fluid(fluid, None, 1000.0, forces=[("xsph", 0.5, 0.0)])
    s.add_boundary(shell)
    return s


def test_a_compressed_column_takes_the_three_per_cu_layout_with_the_kept_halo():
    """Halos of ~2160 particles in the full box (beyond the 2080 slots of the three-per-CU plane layout: the two-per-CU
    instantiation), fewer once the unnamed slots are dropped: every kernel family then takes its smallest layout — the evaluate
    kernels by the fluid halo, the apply kernels by fluid + boundary, the 16-byte layouts by the padded sum.  No switch but the A/B
    one: the default decides by itself that the scene is worth it."""
    sc = _column(0.84)
    w0, f0, t0, h0, _, i0 = _run({"SALVA_HIP_NO_SPLIT": "1", "SALVA_HIP_FULL_HALO": "1"}, sc, 4, look=())
    w1, f1, t1, h1, _, i1 = _run({"SALVA_HIP_NO_SPLIT": "1"}, sc, 4, look=())
    print("full box:", h0, "cut for (fluid, raw, sum):", [(int(i[5]), int(i[6]), int(i[7])) for i in i1])
    assert min(h0) > P3_DS_THREE and h1 == h0, (h0, h1)
    assert all(i[9] == 0 and i[5] > P3_DS_THREE for i in i0), i0  # two tiles per CU with the full box ...
    # ... three with the kept halo, from the first step on, in every family
    assert all(i[9] == 1 and i[5] <= P3_DS_THREE and i[6] <= P2_DS_THREE and i[7] <= FIXED_DS_SMALL for i in i1), i1
    assert t1 == t0
    _same(w1, f1, w0, f0)
