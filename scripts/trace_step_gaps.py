"""Idle time between the launches of each step, from a rocprofv3 kernel_trace.csv of `scripts/fixed_costs.py N trace`:
python scripts/trace_step_gaps.py <kernel_trace.csv> [steps]   (the last `steps` steps, default 40; a step begins at k_native_hash)
One line per step: span from its first launch's start to the next step's, busy time, idle time, kernels, and the
launches other than the step's own (a stamp kernel, say).  Sampled steps stand out by their idle time."""
import csv, sys
rows = []
with open(sys.argv[1]) as fh:
    for r in csv.DictReader(fh):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", "")))
rows.sort()
want = int(sys.argv[2]) if len(sys.argv) > 2 else 40
starts = [i for i, r in enumerate(rows) if "k_native_hash" in r[2]]
starts = starts[-want:]
ends = starts[1:] + [len(rows)]
spans = []
for si, (a, b) in enumerate(zip(starts, ends)):
    ks = rows[a:b]
    busy = sum(e - s for s, e, _ in ks)
    nxt = rows[b][0] if b < len(rows) else ks[-1][1]
    span = nxt - ks[0][0]
    small = sum(1 for _, _, k in ks if "stamp" in k)
    spans.append((span, busy))
    print("step %3d: span %7.2f us  busy %7.2f us  idle %6.2f us  %2d kernels (%d stamps)" %
          (si, span / 1e3, busy / 1e3, (span - busy) / 1e3, len(ks), small))
