"""ms per step over a window of steps of the bench scene (config 2; default: steps 300-399, the settled regime), wall clock around
the window; state stays on the device.  --first / --count choose the window."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("--first", type=int, default=300)
ap.add_argument("--count", type=int, default=100)
ap.add_argument("--side", type=int, default=100)
a = ap.parse_args()
fl, sh = bench.build_scene(a.side)
w, f = bench.make_world(fl, sh, 0)
for k in range(a.first):
    w.step(bench.DT, bench.GRAVITY)
t0 = time.perf_counter()
for k in range(a.count):
    st = w.step(bench.DT, bench.GRAVITY)
dt = time.perf_counter() - t0
print("soak%d_%d ms_per_step %.4f full_halo %d discarded %d variant %s full_env %s" % (a.first, a.first + a.count - 1, 1e3 * dt / a.count, int(st.reserved[0]), int(w.counters.discarded_passes),
      os.environ.get("SALVA_HIP_LIB_VARIANT", "new"), os.environ.get("SALVA_HIP_FULL_HALO", "-")), flush=True)
