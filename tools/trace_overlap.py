"""Per-step idle and overlap figures from a `rocprofv3 --kernel-trace --output-format csv` run of bench.py:
    python tools/trace_overlap.py <name>_kernel_trace.csv [steps]
A step starts at a patch_im2col dispatch (two of them, one per lane, when the encoder runs as two lanes).  For the last `steps` (default 20)
steps it prints, per step on average: the wall time from the step's first dispatch to the next step's, the sum of the kernel durations,
the time at least one kernel was running (the union of the intervals), the idle time (wall - union) and the time two or more kernels were
running at once (the measure of the points that at least two intervals cover)."""
import csv
import sys

path = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rows = []
for r in csv.DictReader(open(path)):
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Queue_Id"]))
rows.sort()
starts = [i for i, r in enumerate(rows) if "patch_im2col" in r[2]]
# two lanes: the second lane's im2col follows the first one's within the same step; keep the first of each step
marks = [starts[0]]
for i in starts[1:]:
    if rows[i][0] - rows[marks[-1]][0] > 1_000_000:      # steps are > 3 ms apart, the lanes' first launches < 0.2 ms
        marks.append(i)
marks = marks[-(steps + 1):]
n = len(marks) - 1
wall = (rows[marks[-1]][0] - rows[marks[0]][0]) / n
seg = rows[marks[0]:marks[-1]]
total = sum(e - s for s, e, _, _ in seg) / n
ev = sorted([(s, 1) for s, e, _, _ in seg] + [(e, -1) for s, e, _, _ in seg])
busy = twice = depth = 0
last = ev[0][0]
for t, d in ev:
    if depth >= 1:
        busy += t - last
    if depth >= 2:
        twice += t - last
    depth += d
    last = t
queues = sorted({q for _, _, _, q in seg})
print(f"{path}: {n} steps, {len(seg) / n:.1f} dispatches per step on queues {queues}")
print(f"  wall per step              {wall / 1e6:.3f} ms")
print(f"  sum of kernel durations    {total / 1e6:.3f} ms")
print(f"  some kernel running        {busy / n / 1e6:.3f} ms")
print(f"  idle (wall - running)      {(wall - busy / n) / 1e6:.3f} ms")
print(f"  two or more running        {twice / n / 1e6:.3f} ms")
