"""Time the grid sub-sampling (psg_grid_assign + psg_grid_reduce) and the sub-cloud projection (psg_grid_index +
psg_grid_nearest) on a synthetic room the size of a raw S3DIS room: --points (4 M) raw points on the six planes of a
10 x 8 x 3 m box (2 mm of noise) and on the faces of a dozen boxes inside it, three colour channels, labels, dl = 0.04.

    python tools/grid_time.py [--points 4000000] [--runs 5] [--knn-runs 3] [--out profiles/r23_grid.json]

One box, one run.  After a warm-up of every shape: --runs timed passes of each call (device events around the call; the two
calls that read back synchronise inside, which is part of their cost), median / min / max in ms.  Part A: points per second
of assign + reduce, and the bytes the algorithm needs (every input once, every output once) over the median time as a
fraction of the measured HBM copy rate (6.29 TB/s).  Part B: the table search against knn_points(k = 1) - the brute-force
scan it replaces - on the same inputs in the same run, alternated, at (Q, M) = (all raw points, their sub-cloud) and at
(40 960, 10 240), the pyramid's first up-sampling shape (there also with cells of --coarse, nearer that sub-cloud's spacing);
the index vectors are compared, and a mismatch is an error.

--kernel-trace DIR_OR_CSV folds in the per-kernel durations of a `rocprofv3 --kernel-trace --output-format csv -- python tools/grid_time.py
--runs 2 --knn-runs 0` run made BEFORE (timings taken under the profiler are not figures for the calls); --trace-only prints
those and stops.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_MEASURED = 6.29e12      # bytes / s, float4 copy
OURS = ("minmax_kernel", "keys_kernel", "heads_kernel", "segments_kernel", "sums_kernel", "label_keys_kernel", "vote_kernel",
        "cell_points_kernel", "nearest_kernel")
LIBRARY = (("radix_sort_onesweep", "radix sort, onesweep"), ("radix_sort_block_sort", "radix sort, block sort"),
           ("merge_sort", "radix sort, block merge"), ("histogram", "radix sort, histogram"), ("scan", "scan"))


def synthetic_room(n, seed=23):
    """points [n,3] f32, colours [n,3] f32 (0..255), labels [n] i32"""
    rng = np.random.default_rng(seed)
    box = np.array([10.0, 8.0, 3.0], np.float32)
    p = rng.random((n, 3), dtype=np.float32) * box
    n_plane = int(n * 0.8)
    face = rng.integers(0, 6, n_plane)
    axis, side = face // 2, face % 2
    p[np.arange(n_plane), axis] = side * box[axis] + rng.normal(0, 0.002, n_plane).astype(np.float32)
    lab = np.zeros(n, np.int32)
    lab[:n_plane] = face
    rest = n - n_plane
    k = rng.integers(0, 12, rest)
    lo = (rng.random((12, 3), dtype=np.float32) * (box - 1.5)).astype(np.float32)
    size = (0.3 + rng.random((12, 3), dtype=np.float32) * 1.2).astype(np.float32)
    q = lo[k] + rng.random((rest, 3), dtype=np.float32) * size[k]
    ax = rng.integers(0, 3, rest)
    q[np.arange(rest), ax] = lo[k, ax] + rng.integers(0, 2, rest) * size[k, ax]
    p[n_plane:] = q
    lab[n_plane:] = 6 + k % 7
    perm = rng.permutation(n)
    col = rng.integers(0, 256, (n, 3)).astype(np.float32)
    return np.ascontiguousarray(p[perm], np.float32), col, lab[perm]


def kernel_durations(path):
    """{kernel @ workgroups: {calls, median_us, total_us}} of this unit's kernels and of the sort / scan kernels of the library it calls (split by
    payload: `pairs` carries the point index, `keys` sorts the label keys alone) out of a rocprofv3 --kernel-trace CSV"""
    import csv
    from kernel_trace_by_grid import find_trace
    rows = {}
    with open(find_trace(path), newline="") as fh:
        for r in csv.DictReader(fh):
            full = r["Kernel_Name"]
            name = next((k for k in OURS if "::" + k + "(" in full), None)
            if name is None and "rocprim" in full:
                kind = next((label for key, label in LIBRARY if key in full), None)
                if kind is not None:
                    name = kind + (" (keys)" if "empty_type" in full else " (pairs)" if "sort" in kind else "")
            if name is not None:
                name = "%s @ %d" % (name, int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1))
                rows.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {k: dict(calls=len(d), median_us=statistics.median(d), total_us=sum(d)) for k, d in sorted(rows.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--grid-size", type=float, default=0.04)
    ap.add_argument("--coarse", type=float, default=0.16, help="cell size of the second (40 960, 10 240) measurement")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--knn-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.trace_only:
        print(json.dumps(dict(kernels_us=kernel_durations(a.kernel_trace))))
        return
    import ctypes
    import torch
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.randla import grid
    from pointsecguard_amd.randla.helper_tool import knn_points
    assert torch.cuda.is_available(), "grid_time.py measures on the MI355X; there is nothing to time without it"
    p, col, lab = synthetic_room(a.points)
    P, C, L = (torch.from_numpy(x).cuda() for x in (p, col, lab))
    n, dl = a.points, a.grid_size
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        r = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), r

    def stats(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), runs=len(v)) if v else None

    # ---- part A: the two calls apart (the handle of randla/grid.py), and the public function as a whole
    sub = grid.grid_sub_sampling_device(P, C, L, dl, return_index=True)                 # warm-up, sizes the handle
    m = sub[0].shape[0]
    g = grid._grid(P.device, n)
    vox = torch.empty(n, dtype=torch.int32, device=P.device)
    sp, sf, sl = torch.empty_like(sub[0]), torch.empty_like(sub[1]), torch.empty_like(sub[2])
    mm = ctypes.c_int(0)
    t = dict(assign=[], reduce=[], whole=[], index=[], nearest=[], knn=[], nearest_small=[], nearest_small_coarse=[], knn_small=[])
    for _ in range(a.runs):
        t["assign"].append(timed(lambda: _lib.call("psg_grid_assign", g.handle, runtime.ptr(P), n, dl, runtime.ptr(vox), ctypes.byref(mm),
                                                   runtime.stream()))[0])
        t["reduce"].append(timed(lambda: _lib.call("psg_grid_reduce", g.handle, runtime.ptr(P), runtime.ptr(C), 3, runtime.ptr(L), 1,
                                                   runtime.ptr(sp), runtime.ptr(sf), runtime.ptr(sl), runtime.stream()))[0])
        t["whole"].append(timed(lambda: grid.grid_sub_sampling_device(P, C, L, dl, return_index=True))[0])
    assert mm.value == m and torch.equal(sp, sub[0]) and torch.equal(sf, sub[1]) and torch.equal(sl, sub[2]) and torch.equal(vox, sub[3])
    bytes_a = n * (12 + 12 + 4) + m * (12 + 12 + 4) + n * 4
    med_a = statistics.median(t["assign"]) + statistics.median(t["reduce"])

    # ---- part B
    S = sub[0]
    shapes = {"": (S, P), "_small": (P[:10240].contiguous(), P[:40960].contiguous())}
    same = {}
    for tag, (s_, q_) in shapes.items():
        ms_, qs_ = s_.shape[0], q_.shape[0]
        a_idx = grid.nearest_sub_point(s_, q_, dl)                                      # warm-up
        gq = grid._grid(s_.device, ms_)
        out = torch.empty(qs_, dtype=torch.int32, device=q_.device)
        k_idx = None
        for i in range(max(a.runs, a.knn_runs + 1 if a.knn_runs else 0)):                # the two methods alternate
            if i < a.runs and not tag:
                t["index"].append(timed(lambda: _lib.call("psg_grid_index", gq.handle, runtime.ptr(s_), ms_, dl, runtime.stream()))[0])
                t["nearest"].append(timed(lambda: _lib.call("psg_grid_nearest", gq.handle, runtime.ptr(q_), qs_, runtime.ptr(out),
                                                            runtime.stream()))[0])
            elif i < a.runs:
                t["nearest_small"].append(timed(lambda: grid.nearest_sub_point(s_, q_, dl))[0])            # index + nearest
                # the same with cells of the sub-cloud's own spacing: 10 240 points of this room lie about 0.15 m apart
                ms, c_idx = timed(lambda: grid.nearest_sub_point(s_, q_, a.coarse))
                t["nearest_small_coarse"].append(ms)
                assert torch.equal(c_idx, a_idx)
            if a.knn_runs and i < a.knn_runs + 1:
                ms, k_idx = timed(lambda: knn_points(s_[None], q_[None], 1))
                if i:                                                                    # (the first one is the warm-up)
                    t["knn" + tag].append(ms)
        if k_idx is not None:
            same["small" if tag else "large"] = bool(torch.equal(k_idx[0, :, 0], a_idx))
    assert all(same.values()), "the table search and knn_points(k = 1) disagree: %r" % (same,)

    out = dict(tool="grid_time", device=torch.cuda.get_device_name(0), n_points=n, grid_size=dl, n_voxels=m, features=3, labels=1,
               ms={k: stats(v) for k, v in t.items()},
               part_a=dict(points_per_s=n / (med_a * 1e-3), assign_plus_reduce_ms=med_a, algorithmic_bytes=bytes_a,
                           bytes_per_s=bytes_a / (med_a * 1e-3), fraction_of_measured_hbm=bytes_a / (med_a * 1e-3) / HBM_MEASURED),
               part_b=dict(large=dict(Q=n, M=m, table_ms=statistics.median(t["index"]) + statistics.median(t["nearest"]),
                                      knn_ms=statistics.median(t["knn"]) if t["knn"] else None),
                           small=dict(Q=40960, M=10240, table_ms=statistics.median(t["nearest_small"]),
                                      table_coarse_cells_ms=statistics.median(t["nearest_small_coarse"]), coarse_grid_size=a.coarse,
                                      knn_ms=statistics.median(t["knn_small"]) if t["knn_small"] else None),
                           indices_equal=same))
    if a.kernel_trace:
        out["kernels_us"] = kernel_durations(a.kernel_trace)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
