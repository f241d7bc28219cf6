"""The steady still step of a rocprofv3 --kernel-trace (csv): k_pair_begin, then the solver that does the still solve, xform ahead and pair ahead.
Every place where solver, k_pair_begin, solver follow each other with no other launch in between is one steady sub-step.  An nh_step call of K sub-steps is one
unbroken run of 2 (K - 2) + 2 such launches (its first sub-step launches a narrowphase, its last another solver).  Every run of at least 150 launches is tabulated, in
the order of the trace -- for `bench.py --steps 100` that is each 100-step call made with the timing filter on (198 launches; the filter's two events around every solver) and, last,
the 200-step landed window (398 launches; timing off, the ring event alone behind the solver): (a) solver end -> k_pair_begin start, (b) k_pair_begin,
(c) k_pair_begin end -> solver start, (d) solver; and the launch geometry of every k_pair_begin of the run.
usage: python profiles/export_steady_step.py <dir with *_kernel_trace.csv, or the csv> [label]   (prints the tables)"""
import collections, csv, glob, sys
import numpy as np

d = sys.argv[1]
label = sys.argv[2] if len(sys.argv) > 2 else d
f = d if d.endswith(".csv") else sorted(glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True))[-1]
rows = []
for r in csv.DictReader(open(f)):
    n = r["Kernel_Name"]
    kind = "P" if n.startswith("k_pair_begin") else "S" if "k_solve_one_body<4, true, true, 1, true, true, true, false>" in n else "x"
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, int(r.get("Workgroup_Size_X", 0) or 0), int(r.get("Grid_Size_X", 0) or 0)))
rows.sort()
kinds = "".join(r[2] for r in rows)
runs, i = [], 0
while i < len(kinds):
    if kinds[i] == "x": i += 1; continue
    j = i
    while j < len(kinds) and kinds[j] != "x": j += 1
    if j - i >= 150: runs.append((i, j))
    i = j

def line(name, v):
    v = np.asarray(v, dtype=np.float64) / 1e3
    return f"  {name:44s} mean {v.mean():8.2f}  sd {v.std():6.2f}  min {v.min():8.2f}  p50 {np.median(v):8.2f}  p95 {np.percentile(v, 95):8.2f}  max {v.max():8.2f}   us"

print(f"== {label}: {len(rows)} launches in the trace, {len(runs)} unbroken runs of the two steady launches")
for k, (i, j) in enumerate(runs):
    run = rows[i:j]
    a, b, c, dd, step = [], [], [], [], []
    for q in range(len(run) - 2):
        s0, p, s1 = run[q], run[q + 1], run[q + 2]
        if (s0[2], p[2], s1[2]) != ("S", "P", "S"): continue
        a.append(p[0] - s0[1]); b.append(p[1] - p[0]); c.append(s1[0] - p[1]); dd.append(s1[1] - s1[0]); step.append(s1[1] - s0[1])
    grids = collections.Counter((r[4] // max(r[3], 1), r[3]) for r in run if r[2] == "P")
    print(f"-- run {k + 1} of {len(runs)}: {len(run)} launches, {len(a)} steady sub-steps")
    print("  k_pair_begin launches by geometry: " + ", ".join(f"{n} x ({g} workgroups of {w})" for (g, w), n in sorted(grids.items())))
    print(line("(a) solver end -> k_pair_begin start", a))
    print(line("(b) k_pair_begin", b))
    print(line("(c) k_pair_begin end -> solver start", c))
    print(line("(d) solver", dd))
    print(line("whole sub-step (solver end -> solver end)", step))
