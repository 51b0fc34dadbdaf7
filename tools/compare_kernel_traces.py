"""Compare two rocprofv3 --kernel-trace CSVs launch by launch: kernel name, grid, workgroup and LDS bytes, in dispatch
order.  Usage: python tools/compare_kernel_traces.py A_kernel_trace.csv B_kernel_trace.csv.  Exit status 1 if they differ."""
import collections
import csv
import sys


def records(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"] if "Dispatch_Id" in r else r["Start_Timestamp"]))
    lds = [c for c in rows[0] if "LDS" in c.upper()][0]

    def dims(r, stem):
        return tuple(int(r[f"{stem}_{a}"]) for a in "XYZ") if f"{stem}_X" in r else (int(r[stem]),)
    return [(r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), int(r[lds])) for r in rows]


a, b = records(sys.argv[1]), records(sys.argv[2])
print(f"A: {len(a)} launches, {len(set(r[0] for r in a))} kernels ({sys.argv[1]})")
print(f"B: {len(b)} launches, {len(set(r[0] for r in b))} kernels ({sys.argv[2]})")
diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
for i, x, y in diff[:10]:
    print(f"launch {i}:\n  A {x}\n  B {y}")
same = not diff and len(a) == len(b)
print("sequences of (kernel, grid, workgroup, LDS):", "EQUAL" if same else f"DIFFERENT ({len(diff)} launches, lengths {len(a)} / {len(b)})")
count = collections.Counter((r[0].replace("cough::(anonymous namespace)::", ""), r[3]) for r in a)
for (name, lds), n in sorted(count.items()):
    print(f"  {n:4d} x  LDS {lds:7d}  {name[:110]}")
sys.exit(0 if same else 1)
