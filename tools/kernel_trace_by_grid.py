#!/usr/bin/env python3
"""Per-launch durations out of a rocprofv3 --kernel-trace CSV, keyed by (kernel, grid, workgroup).

`--stats` sums every dispatch of one template instantiation, so fp2 / fp3 / fp4 forward (all fp_fwd_kernel<32, 8, false>) and
the per-point launches of the three split SA levels fall into one row each.  Their grids differ; this prints one row per
(kernel name, grid in workgroups, workgroup size): calls, mean / median / min duration in microseconds.

usage: tools/kernel_trace_by_grid.py DIR_OR_CSV [name substring ...] > table.csv
"""
import csv
import os
import statistics
import sys


def find_trace(path):
    if os.path.isfile(path):
        return path
    for root, _, files in os.walk(path):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                return os.path.join(root, f)
    raise SystemExit("no *kernel_trace.csv under %s" % path)


def short(name):
    """kernel name without its argument list and the `void psg::` prefix"""
    for p in ("void ", "psg::", "(anonymous namespace)::"):      # (before the cut: the namespace's own parenthesis)
        name = name.replace(p, "")
    return name.split("(")[0].strip()


def main():
    path = find_trace(sys.argv[1])
    want = sys.argv[2:]
    rows = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = short(r["Kernel_Name"])
            if want and not any(w in name for w in want):
                continue
            wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
            grid = [int(r["Grid_Size_" + a]) // max(w, 1) for a, w in zip("XYZ", wg)]
            key = (name, "x".join(map(str, grid)), wg[0] * wg[1] * wg[2])
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    out = csv.writer(sys.stdout)
    out.writerow(["kernel", "grid_wgs", "wg_threads", "calls", "mean_us", "median_us", "min_us", "total_ms"])
    for key, d in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
        out.writerow(list(key) + [len(d), "%.2f" % statistics.fmean(d), "%.2f" % statistics.median(d), "%.2f" % min(d),
                                  "%.3f" % (sum(d) / 1000.0)])


if __name__ == "__main__":
    main()
