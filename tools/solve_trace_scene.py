"""Run ONE named scene of the solve driver's launch comparison (profiles/solve_driver_trace.json) and nothing else, so that a kernel
trace of the process (`rocprofv3 --kernel-trace -- python tools/solve_trace_scene.py NAME`) lists that scene's launches only.
The scenes are the suite's own: tests/test_chain_gpu.py, test_speculation_gpu.py, test_dist_gpu.py and the two golden scenes whose
solves go through every arm of the driver.  The library is the default one, or SALVA_HIP_LIB_VARIANT's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
# name -> (switches set before the world is made, steps)
SCENES = {"drop24": ({}, 64), "drop24_nochain": ({"SALVA_HIP_NO_CHAIN": "1"}, 64), "break": ({"SALVA_HIP_NO_SPEC_APPLY": "1"}, 60),
          "spec": ({}, 40), "dfsph_viscous": ({}, 6), "iisph_akinci": ({}, 6), "slabs3": ({}, 12)}


def main(name):
    env, nsteps = SCENES[name]
    os.environ.update(env)
    from parity import DT, GRAVITY, Scene
    from salva_amd import scenes
    if name == "slabs3":  # test_decomposed_solves_run_their_applies_beside_the_all_reduce: three loopback slabs
        import test_dist_gpu as td
        pos, vel, bpos = td.make_scene(nx=44, ny=12, nz=10, seed=21)
        vel[:, 1] -= np.float32(2.5)
        stats = td.run_slabs(pos, vel, bpos, nsteps, 3, False)[2]
        print(name, [s.n_divergence_iters for s in stats[0]])
        return
    if name in ("dfsph_viscous", "iisph_akinci"):
        from golden_scenes import SCENES as GOLDEN
        sc = GOLDEN[name][0]()
    elif name == "spec":  # test_speculative_applies_change_nothing_but_the_launch_count
        sc = Scene(0.025, 2.0, "dfsph")
        fluid, shell = scenes.tank(24, 24, 24, 0.025)
        sc.add_fluid(scenes.jitter(fluid, 0.1 * 0.025, seed=42), None, 1000.0, forces=[("xsph", 0.5, 0.0)])
        sc.add_boundary(shell)
    else:
        from test_chain_gpu import _drop_scene
        sc = _drop_scene(16, lift=0.1) if name == "break" else _drop_scene(24)
        if name == "break":  # test_chains_that_break_in_either_solve_continue_there
            sc.solver_params["max_density_error"] = 5e-5
    w = sc.make_hip()[0]
    trace = []
    for _ in range(nsteps):
        st = w.step(DT, GRAVITY)
        trace.append((st.n_divergence_iters, st.n_pressure_iters))
    print(name, trace, w.counters.chained_passes, w.counters.chain_breaks)


if __name__ == "__main__":
    main(sys.argv[1])
