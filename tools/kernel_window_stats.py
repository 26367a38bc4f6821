"""Per-kernel averages over the LAST `--steps` steps of a `rocprofv3 --kernel-trace` run (its *_kernel_trace.csv): the window starts
at the --steps-th last dispatch of k_update_positions, which runs once per step.  Prints dispatches per step, average us and us per
step for the kernels that take the most time."""
import argparse, csv, glob, os, re, sys
ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--top", type=int, default=16)
a = ap.parse_args()
files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
if not files:
    sys.exit("no kernel trace under " + a.dir)
rows = []
for f in files:
    for r in csv.DictReader(open(f)):
        name = re.sub(r"^(void )?(salva(_ok)?::)?", "", r["Kernel_Name"])
        m = re.match(r"([A-Za-z_0-9:]+)(<[^>(]*>)?", name)
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), (m.group(1) + (m.group(2) or "")) if m else name))
rows.sort()
marks = [s for s, e, n in rows if n.startswith("k_update_positions")]
if len(marks) < a.steps:
    sys.exit("fewer than --steps steps in the trace")
t0 = marks[-a.steps]
acc = {}
for s, e, n in rows:
    if s >= t0:
        c = acc.setdefault(n, [0, 0])
        c[0] += 1; c[1] += e - s
tot = sum(v[1] for v in acc.values())
print("window: last %d steps, %.1f us of kernels per step" % (a.steps, tot / 1e3 / a.steps))
for n, (c, t) in sorted(acc.items(), key=lambda kv: -kv[1][1])[:a.top]:
    print("%-60s %7.2f per step  avg %8.2f us  %8.1f us per step" % (n[:60], c / a.steps, t / 1e3 / c, t / 1e3 / a.steps))
