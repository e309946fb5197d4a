"""Per-kernel table of a rocprofv3 --kernel-trace run of bench.py --serialize, per optimizer step, with the spread of each
kernel's own per-launch times (the yardstick a kernel-level gain is held against): tools/kstat_table.py <trace dir> [min us/step]
One fused-Adam launch per optimizer step gives the step count of the trace."""
import csv, glob, sys
from collections import defaultdict

d = sys.argv[1]
floor = float(sys.argv[2]) if len(sys.argv) > 2 else 20.0
f = glob.glob(d + "/**/*_kernel_trace.csv", recursive=True)[0]
dur = defaultdict(list)
for r in csv.DictReader(open(f)):
    dur[r["Kernel_Name"].replace("(anonymous namespace)::", "")].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
steps = float(max((len(v) for k, v in dur.items() if k.startswith("adam_kernel")), default=1))
total = sum(sum(v) for v in dur.values())
print(f"{sum(len(v) for v in dur.values()) / steps:.2f} launches per step, {total / steps:.1f} us of kernel time per step ({steps:g} optimizer steps in the trace)")
print(f"{'kernel':84s} {'calls/step':>10s} {'us/step':>10s} {'avg us':>8s} {'min us':>8s} {'max us':>8s}")
for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
    if sum(v) / steps < floor and "bn_bwd" not in k and "sample_reduce" not in k:
        continue
    print(f"{k[:84]:84s} {len(v) / steps:10.2f} {sum(v) / steps:10.1f} {sum(v) / len(v):8.1f} {min(v):8.1f} {max(v):8.1f}")
# a kernel launched at several shapes per step: its launches come in the same order every step, so launch i belongs to
# position i mod calls-per-step; per position, the spread over the steps (third argument on: comma-separated name substrings)
for sub in (sys.argv[3].split(",") if len(sys.argv) > 3 else ()):
    for k, v in sorted(dur.items()):
        n = int(len(v) / steps)
        if sub not in k or n * steps != len(v):
            continue
        print(f"-- {k[:100]}: {n} launches per step, by position")
        for p in range(n):
            w = v[p::n]
            print(f"   position {p:2d}: avg {sum(w) / len(w):7.1f} us  min {min(w):7.1f}  max {max(w):7.1f}  spread {max(w) - min(w):6.1f}")
