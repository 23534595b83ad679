"""Per-launch table of chosen kernels from two rocprofv3 --kernel-trace runs of scripts/prof_step.py (before / after).
  prof_launches.py <before dir> <after dir> <out.md> <title> <name part>[,<name part>...]
Steady state as prof_summary.py steady takes it: the trace is cut at the stem's forward launch, the first step is dropped.  Every
launch whose kernel name contains one of the name parts is listed in the order it runs within a step, its duration averaged over
the steps; the two runs must list the same number of such launches per step (their names may differ: a launch that changed kernel)."""
import csv, glob, os, sys


def launches(d, parts):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not f:
        sys.exit(f"no *kernel_trace.csv under {d}")
    rows = list(csv.DictReader(open(f[-1])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cuts = [i for i, r in enumerate(rows) if "k_stem" in r["Kernel_Name"] and "fwd" in r["Kernel_Name"]]
    if len(cuts) < 3:
        sys.exit(f"need >= 3 steps, found {len(cuts)} stem launches")
    steps = []
    for a, b in zip(cuts[1:-1], cuts[2:]):
        steps.append([r for r in rows[a:b] if any(p in r["Kernel_Name"] for p in parts)])
    names = [[r["Kernel_Name"] for r in s] for s in steps]
    if any(n != names[0] for n in names):
        sys.exit(f"{d}: the steps do not launch the same kernels")
    out = []
    for j, r in enumerate(steps[0]):
        us = [(int(s[j]["End_Timestamp"]) - int(s[j]["Start_Timestamp"])) / 1e3 for s in steps]
        gx = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
        wx = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1)
        out.append((r["Kernel_Name"].replace("void ", "").split("(")[0], gx // max(wx, 1), sum(us) / len(us), min(us), max(us)))
    return out, len(steps)


def main():
    before, after, out, title, parts = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5].split(",")
    a, na = launches(before, parts)
    b, nb = launches(after, parts)
    if len(a) != len(b):      # another launch sequence: the two lists one after the other
        with open(out, "w") as f:
            for tag, lst in (("before", a), ("after", b)):
                f.write(f"# {title}: {tag}, {len(lst)} launches per step\n\n| # | kernel | workgroups | µs |\n|---|---|---|---|\n")
                for j, x in enumerate(lst):
                    f.write(f"| {j} | `{x[0]}` | {x[1]} | {x[2]:.1f} ({x[3]:.1f}..{x[4]:.1f}) |\n")
                f.write("\n")
        print(open(out).read())
        return
    with open(out, "w") as f:
        f.write(f"# {title}\n\nsteady state, first step dropped, {na} steps averaged before and {nb} after; min..max over the steps in brackets\n\n"
                "| # | kernel before | workgroups | µs before | kernel after | workgroups | µs after | after / before |\n|---|---|---|---|---|---|---|---|\n")
        for j, (x, y) in enumerate(zip(a, b)):
            f.write(f"| {j} | `{x[0]}` | {x[1]} | {x[2]:.1f} ({x[3]:.1f}..{x[4]:.1f}) | `{y[0]}` | {y[1]} | {y[2]:.1f} ({y[3]:.1f}..{y[4]:.1f}) | "
                    f"{y[2] / x[2]:.2f} |\n")
        f.write(f"\nSum: {sum(x[2] for x in a):.1f} µs per step before, {sum(y[2] for y in b):.1f} µs after.\n")
    print(open(out).read())


if __name__ == "__main__":
    main()
