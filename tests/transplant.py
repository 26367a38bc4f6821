"""One oracle step from a device state: `one_step_against_oracle` ("One step from the device's own state").

Lockstep oracle runs diverge chaotically long before the states the bench and real runs live in (settled tanks, folded grids,
strays tens of metres below the bulk).  Here the device world runs on by itself; at a chosen step its `checkpoint()` — everything a
step carries over — is loaded into fresh oracle worlds (f32, and f64 for the noise floor), and the NEXT step of the continuing
device world is compared with one oracle step.  The inputs are identical bit for bit, so the contact sets must be equal and every
field is held to the step-0 bounds of tests/test_parity_gpu.py::compare, at any step of any run."""
from __future__ import annotations

import os
import time

import numpy as np

from parity import DT, GRAVITY, host_threads

COUNTERS = ("speculative_passes", "chained_passes", "chain_breaks", "pregrid_adopted", "discarded_passes", "light_class_passes",
            "sparse_class_passes")




def oracle_threads():
    try:
        omp = int(os.environ.get("OMP_NUM_THREADS", "16"))
    except ValueError:
        omp = 16
    return max(1, min(host_threads(), omp if omp > 0 else 16))


def _counters(w):
    c = w.counters
    return {k: int(getattr(c, k)) for k in COUNTERS}


def tank_box(scene):
    """Axis-aligned box of all boundary particles (the tank); None without boundaries."""
    if not scene.boundaries:
        return None
    p = np.concatenate([b["pos"] for b in scene.boundaries])
    return p.min(axis=0), p.max(axis=0)


def _worst(name, f, idx, pos, cnt_dev, cnt_ora, detail):
    return (f"{name} of fluid {f}: worst particle {idx} at {np.asarray(pos[idx]).tolist()}, contacts (ff, fb) device "
            f"{cnt_dev[0][idx]}, {cnt_dev[1][idx]} / oracle {cnt_ora[0][idx]}, {cnt_ora[1][idx]}: {detail}")


def one_step_against_oracle(w, fls, bds, scene, label, sample=20000, f64=True, gravity=GRAVITY, dt=DT, seed=0):
    """Compare the next step of device world `w` (fluid handles `fls`, boundary handles `bds`, built from `scene`) with one step
    of oracle worlds restored from `w.checkpoint()`.  Asserts contact counts (per particle, total) and the contact sets of a
    sample exactly, densities / alphas / boundary volumes at rel 1e-5 / 1e-4 / 1e-5, velocity_changes / velocities / positions
    after the step at max(1e-4 r or 1e-4 v_ref, 2 x the oracle's own noise), IISPH pressures at max(1e-3 max(1, p_max), the same
    noise floor), iteration counts within 1 of the f32 oracle's (or both at the cap).  The noise is the larger of |oracle f32 -
    oracle f64| and |oracle f32 - oracle f32 in another contact order| (`shuffle_seed`): the reference's contact order is
    unspecified, and the threaded oracle's own order changes from run to run (contacts are pushed by whichever thread gets there
    first), which a capped 50-iteration divergence solve amplifies to ~5e-4 v_ref in velocity_changes.
    `f64=False`: the f32 oracle only (the stated bounds, no noise floor).  Returns what the compared step did: counter deltas,
    StepStats.reserved[0..2] (largest fluid / boundary halo, threads), the stray count, worst errors, oracle wall time."""
    R = scene.radius
    ck = w.checkpoint()
    c0 = _counters(w)
    nthreads = oracle_threads()
    t0 = time.perf_counter()
    o = scene.make_oracle(threads=nthreads)
    o.restore(ck)
    noise = []  # the oracle's own noise: f64, and f32 in another contact order
    if f64:
        noise = [scene.make_oracle(f64=True, threads=nthreads), scene.make_oracle(threads=nthreads, shuffle_seed=7)]
        for x in noise:
            x.restore(ck)
    t_build = time.perf_counter() - t0

    st = w.step(dt, gravity)
    c1 = _counters(w)
    t0 = time.perf_counter()
    so = o.step(dt, gravity)
    s64 = [x.step(dt, gravity) for x in noise][0] if f64 else None
    t_oracle = time.perf_counter() - t0

    out = {"label": label, "counters": {k: c1[k] - c0[k] for k in COUNTERS}, "reserved": [float(st.reserved[i]) for i in range(3)],
           "iters": (st.n_divergence_iters, st.n_pressure_iters, so.n_div_iters, so.n_press_iters,
                     s64.n_div_iters if f64 else None, s64.n_press_iters if f64 else None),
           "ncontacts": int(st.ncontacts), "oracle_build_s": t_build, "oracle_step_s": t_oracle, "worst": {}, "strays": 0}
    worst = out["worst"]

    def note(key, v):
        worst[key] = max(worst.get(key, 0.0), float(v))

    # ---- contacts: the inputs are bit-identical, so nothing may differ
    assert int(st.ncontacts) == int(so.ncontacts), f"{label}: ncontacts {st.ncontacts} vs oracle {so.ncontacts}"
    box = tank_box(scene)
    rng = np.random.default_rng(seed)
    ps = scene.solver_params
    for f, h in enumerate(fls):
        pos0 = np.asarray(ck[f"fluid{f}_positions"], np.float32)
        cd = (w.contact_counts(h), w.contact_counts(h, True))
        co = (o.contact_counts(f), o.contact_counts(f, True))
        for k, kind in enumerate(("fluid-fluid", "fluid-boundary")):
            bad = np.nonzero(cd[k] != co[k])[0]
            assert bad.size == 0, _worst(f"{kind} contact counts", f, bad[0], pos0, cd, co, f"{bad.size} particles differ")
        # contact sets of a sample: the strays, the most crowded particles, a seeded random rest
        n = len(pos0)
        strays = np.zeros(0, np.int64)
        if box is not None:
            strays = np.nonzero(((pos0 < box[0]) | (pos0 > box[1])).any(axis=1))[0]
        out["strays"] += int(strays.size)
        crowded = np.argsort(cd[0].astype(np.int64) + cd[1], kind="stable")[-min(2000, n):]
        pick = np.unique(np.concatenate([strays, crowded]))
        if sample > pick.size:
            rest = np.setdiff1d(np.arange(n), pick, assume_unique=True)
            pick = np.union1d(pick, rng.choice(rest, size=min(sample - pick.size, rest.size), replace=False))
        for boundary in (False, True):
            off, jm, j = w.fluid_contacts(h, boundary)
            for i in pick:
                a, b = int(off[i]), int(off[i + 1])
                got = sorted(zip(jm[a:b].tolist(), j[a:b].tolist()))
                ref = o.contacts_of(f, int(i), boundary)
                assert got == ref, _worst("fluid-boundary contact set" if boundary else "fluid-fluid contact set", f, i, pos0, cd, co,
                                          f"device only {sorted(set(got) - set(ref))[:8]}, oracle only {sorted(set(ref) - set(got))[:8]}")
        out.setdefault("sampled", 0)
        out["sampled"] += int(pick.size)

        # ---- per-step scalars, computed from the identical inputs
        rho, rho_o = w.densities(h).astype(np.float64), o.fluid_scalar(f, "densities")
        e = np.abs(rho - rho_o) / np.abs(rho_o)
        note("densities", e.max(initial=0))
        assert e.max(initial=0) < 1e-5, _worst("densities", f, int(np.argmax(e)), pos0, cd, co, f"rel {e.max():.2e}")
        if scene.solver == "dfsph":
            # (per particle, the noise-floor rule: a stray whose few neighbours all sit near r = h has gradients of (1 - q)^2, whose
            # relative rounding error the kernels' own evaluation order amplifies — there the f64 oracle moves as far)
            al, al_o = w.alphas(h).astype(np.float64), o.fluid_scalar(f, "alphas")
            den = np.maximum(np.abs(al_o), 1e-3 * float(np.abs(al_o).max(initial=0)))
            e = np.abs(al - al_o) / den
            tol = np.full(e.shape, 1e-4)
            for x in noise:
                tol = np.maximum(tol, 2 * np.abs(al_o - x.fluid_scalar(f, "alphas")) / den)
            note("alphas", e.max(initial=0))
            q = int(np.argmax(e / tol)) if e.size else 0
            assert (e < tol).all(), _worst("alphas", f, q, pos0, cd, co, f"rel {e[q]:.2e} (bound {tol[q]:.2e}), "
                                           f"{int((e >= tol).sum())} particles over")

        # ---- the state after the step: stated bound or twice the oracle's own f32-vs-f64 distance
        vo = o.fluid_vec(f, "velocities")
        vref = max(2 * R / dt * 1e-2, float(np.abs(vo).max(initial=0)))
        for name, got, scale in (("positions", h.positions, R), ("velocities", h.velocities, vref),
                                 ("velocity_changes", w.velocity_changes(h), vref)):
            ref = o.fluid_vec(f, name)
            d = np.linalg.norm(np.asarray(got, np.float64) - ref, axis=1)
            tol = 1e-4 * scale
            for x in noise:
                tol = max(tol, 2 * float(np.linalg.norm(ref - x.fluid_vec(f, name), axis=1).max(initial=0)))
            note(name, d.max(initial=0) / scale)
            assert d.max(initial=0) < tol, _worst(name, f, int(np.argmax(d)), pos0, cd, co,
                                                  f"|d| {d.max():.3e} = {d.max() / scale:.2e} of {'r' if scale == R else 'v_ref'} "
                                                  f"(bound {tol / scale:.2e})")
        if scene.solver == "iisph":
            pr = o.fluid_scalar(f, "pressures")
            d = np.abs(w.pressures(h).astype(np.float64) - pr)
            tol = 1e-3 * max(1.0, float(pr.max(initial=0)))
            for x in noise:
                tol = max(tol, 2 * float(np.abs(pr - x.fluid_scalar(f, "pressures")).max(initial=0)))
            note("pressures", d.max(initial=0) / max(1.0, float(pr.max(initial=0))))
            assert d.max(initial=0) < tol, _worst("pressures", f, int(np.argmax(d)), pos0, cd, co, f"|dp| {d.max():.3e} (bound {tol:.3e})")

    for b, hb in enumerate(bds):
        vb, vb_o = np.asarray(hb.volumes, np.float64), o.boundary_volumes(b)
        e = np.abs(vb - vb_o) / np.abs(vb_o)
        note("boundary volumes", e.max(initial=0))
        assert e.max(initial=0) < 1e-5, f"{label}: boundary {b} volumes, worst particle {int(np.argmax(e))}: rel {e.max():.2e}"

    # ---- iteration counts
    def iters_ok(dev, ref, cap):
        return abs(dev - ref) <= 1 or (dev >= cap and ref >= cap)
    assert iters_ok(st.n_pressure_iters, so.n_press_iters, ps["max_pressure_iter"]), f"{label}: pressure iterations {out['iters']}"
    if scene.solver == "dfsph":
        assert iters_ok(st.n_divergence_iters, so.n_div_iters, ps["max_divergence_iter"]), f"{label}: divergence iterations {out['iters']}"
    print(f"{label}: counters {out['counters']} halo (fluid, boundary, threads) {out['reserved']} iters (dev div, press / oracle / "
          f"f64) {out['iters']} contacts {out['ncontacts']} strays {out['strays']} sampled {out['sampled']} | worst "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f" | oracle build {t_build:.1f} s, step {t_oracle:.1f} s ({nthreads} threads)")
    return out
