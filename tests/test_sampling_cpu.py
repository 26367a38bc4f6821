"""The ray sampler's specification without a GPU: tests/sampling_reading.py (an independent numpy f32 reading of DESIGN.md §13)
against the two restatements salva_amd/scenes.py already has, the cuboid's full lattice block in volume mode, the thin-chord rule
and the rounding mode."""
import numpy as np

import sampling_reading as R

F = np.float32


def test_reading_agrees_with_scenes_ball():
    from salva_amd import scenes

    q, pos, _ = R.sample(("ball", 0.15), 0.0125, R.SURFACE)
    ref = scenes.ball_surface_ray_sample(0.15, 0.0125)
    rays, s, _, _ = R.ray_chords(("ball", 0.15), 0.0125)
    assert len(rays) == 336
    assert min(float(b - a) for _, _, _, a, b in rays) > 10 * float(s / F(10.0))  # no thin chord: the two readings must agree
    assert pos.dtype == ref.dtype == np.float32 and pos.shape == ref.shape
    assert np.array_equal(pos.view(np.uint32), ref.view(np.uint32))


def test_reading_agrees_with_scenes_cuboid():
    from salva_amd import scenes

    q, pos, _ = R.sample(("cuboid", (0.2, 0.7, 2.5)), 0.05, R.SURFACE)
    ref = scenes.cuboid_surface_ray_sample([0.2, 0.7, 2.5], 0.05)
    assert len(pos) == 1648 and pos.shape == ref.shape
    assert np.array_equal(pos.view(np.uint32), ref.view(np.uint32))


def test_cuboid_volume_is_the_full_block():
    """A cuboid's faces sit exactly half a spacing from the lattice planes next to them (origin = mins - s / 2): the entry index is
    round(0.5) in exact arithmetic, and whatever f32 makes of it otherwise (the basic3 wall at r = 0.05 gets 0.49999997 -> 0 and with it
    a plane outside the box, in the reference as here).  With a power-of-two spacing and dyadic half extents every operation is
    exact: the entry is round(0.5) = 1, the exit round(N - 2 + 0.25) = N - 2, the samples the full block of lattice points inside."""
    for he, r in (((0.359375, 0.484375, 0.609375), 0.0625), ((2.359375, 2.359375, 4.234375), 0.0625)):
        q, pos, N = R.sample(("cuboid", he), r, R.VOLUME)
        assert len(q) == (N[0] - 2) * (N[1] - 2) * (N[2] - 2)
        block = np.array([(x, y, z) for x in range(1, N[0] - 1) for y in range(1, N[1] - 1) for z in range(1, N[2] - 1)], np.int64)
        assert np.array_equal(q, block)


def test_line_and_ray_counts_of_the_gpu_cases():
    """The lattices the GPU test names (tests/test_sampling_gpu.py): line counts and hitting rays."""
    _, _, N = R.sample(("capsule", 0.2, 0.1), 0.0125, R.SURFACE)
    assert N == [10, 26, 10] and len(R.ray_chords(("capsule", 0.2, 0.1), 0.0125)[0]) == 412
    _, _, N = R.sample(("cylinder", 0.15, 0.12), 0.0125, R.SURFACE)
    assert N == [12, 14, 12] and len(R.ray_chords(("cylinder", 0.15, 0.12), 0.0125)[0]) == 313


def test_thin_chord_yields_the_entry_only():
    radius = R.find_thin_chord_ball()
    shape = ("ball", radius)
    rays, s, origin, coords = R.ray_chords(shape, 0.0125)
    thin = [ray for ray in rays if 0 < F(ray[4] - ray[3]) < F(s / F(10.0))]
    assert thin, "the search must have found a ray with 0 < chord < s / 10"
    N = [len(c) for c in coords]
    for i, cj, ck, a, b in thin:
        j, k = (i + 1) % 3, (i + 2) % 3
        q_in, q_out = [0, 0, 0], [0, 0, 0]
        for q, v, fn in ((q_in, a, np.ceil), (q_out, b, np.floor)):
            q[i] = int(fn(F(F(v - origin[i]) / s)))
            q[j] = int(R.roundf(F(F(cj - origin[j]) / s)))
            q[k] = int(R.roundf(F(F(ck - origin[k]) / s)))
        assert q_in[i] == q_out[i] + 1  # a chord inside one lattice cell: ceil(entry) lies beyond floor(exit)
        per = {}
        R.sample(shape, 0.0125, R.SURFACE, per_axis=per)
        assert tuple(q_in) in per[i] and tuple(q_out) not in per[i]
        per = {}
        R.sample(shape, 0.0125, R.VOLUME, per_axis=per)
        on_line = [q for q in per[i] if q[j] == q_in[j] and q[k] == q_in[k]]
        assert on_line == []


def test_round_is_half_away_from_zero():
    assert R.roundf(F(2.5)) == 3 and R.roundf(F(0.5)) == 1 and R.roundf(F(-2.5)) == -3 and R.roundf(F(1.5)) == 2
    assert np.round(F(2.5)) == 2 and np.round(F(0.5)) == 0  # numpy's half-to-even is the wrong mode
    assert R.as_u32(R.roundf(F(-0.5))) == 0 and R.as_u32(F("nan")) == 0 and R.as_u32(-3.0) == 0
    # a hand-made .5 in the sampler's own arithmetic: (origin + 2.5 s - origin) / s with s = 0.25 is exactly 2.5
    s, o = F(0.25), F(-1.0)
    assert R.as_u32(R.roundf(F(F(F(o + F(2.5) * s) - o) / s))) == 3
