"""Time tar_NU_attack on ResGCN-28 (4096-point rooms, the fitted fixture weights of bench.py's resgcn workload) with the
settings of bench.py's `tarnu` workload (c=1, kappa=0, lr=0.01, target=6, mask = label == 11, steps capped at 40):
(a) one `forward` per room with a fresh attack object, as the reference's harness applies it - the host loop of
    attacks/nu.py: gcn_nu_attack, one library call per operation and one read-back per step;
(b) the same rooms through forward_rooms (psg_gcn_nu_window: lockstep, device-side windows) at R = 1, 4 and 8.
Every figure works on the same --rooms rooms (R = 4: two calls, R = 1: eight).  The legs ALTERNATE: after one warm-up pass
over all of them (workspaces, first eager windows, graph capture) every run times (a), R = 1, R = 4, R = 8 in turn, --runs
times (at least 3), on a side stream, synchronised around each timed region.  Prints min / median / max rooms per second, the
optimiser steps that ran, ms per optimiser step and room, and the hipGraph bookkeeping of each lockstep shape as one JSON line.

    python tools/gcn_nu_time.py [--runs 3] [--rooms 8] [--steps 40] [--out profiles/r15_gcn_nu.json]

--field coord | both (default color: the legs and the output above, unchanged) adds, in the same alternation on the same box,
the forward_rooms legs of the coordinate-field attack (psg_gcn_nu_field_window) at the same sizes, with
coord_lr = lr, and prints their rooms per second beside the colour legs' (`field_over_color`).  --kernel-trace DIR_OR_CSV reads
the CSV of a `rocprofv3 --kernel-trace -- python tools/gcn_nu_time.py --field coord ...` run made BEFORE (timings taken under
the profiler are not figures) and adds the durations of the coordinate Smooth term's two kernels and of the coordinate Adam
step per grid.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pointsecguard_amd import _lib, synthetic  # noqa: E402
from pointsecguard_amd.resgcn.sem_seg_dense.architecture import DenseDeepGCN  # noqa: E402
from pointsecguard_amd.resgcn.sem_seg_dense.attacks import torchattacks  # noqa: E402


NEW_KERNELS = ("smooth_knn_xyz_kernel", "smooth_xyz_sym_incoming_kernel", "nu_coord_adam_w_kernel")


def new_kernel_durations(path):
    """{kernel @ grid: {calls, median_us, min_us}} of the coordinate-field kernels out of a rocprofv3 --kernel-trace CSV"""
    import csv
    import statistics
    import re
    from kernel_trace_by_grid import find_trace
    rows = {}
    with open(find_trace(path), newline="") as fh:
        for r in csv.DictReader(fh):
            hit = re.search(r"(%s)(<[^>]*>)?" % "|".join(NEW_KERNELS), r["Kernel_Name"])
            if not hit:
                continue
            name = hit.group(0)
            wg = [max(int(r["Workgroup_Size_" + c]), 1) for c in "XYZ"]
            grid = "x".join(str(int(r["Grid_Size_" + c]) // w) for c, w in zip("XYZ", wg))
            rows.setdefault("%s @ %s" % (name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {k: dict(calls=len(d), median_us=statistics.median(d), min_us=min(d)) for k, d in sorted(rows.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rooms", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=28)
    ap.add_argument("--sizes", default="1,4,8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--field", default="color", choices=("color", "coord", "both"))
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-only", action="store_true", help="print the --kernel-trace durations and stop (no GPU work)")
    a = ap.parse_args()
    if a.trace_only:
        print(json.dumps(dict(kernels_us=new_kernel_durations(a.kernel_trace))))
        return
    runs, rooms, target = max(3, a.runs), a.rooms, 6
    kw = dict(c=1, kappa=0, steps=a.steps, lr=0.01, target=target)
    opt = SimpleNamespace(n_filters=64, k=16, act="relu", norm="batch", bias=True, epsilon=0.0, stochastic=False, conv="edge",
                          n_blocks=a.blocks, block="res", in_channels=9, dropout=0.0, n_classes=13)
    net = DenseDeepGCN(opt)
    sd = synthetic.gcn28_state_dict() if a.blocks == 28 else synthetic.gcn_state_dict(7, a.blocks)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net = net.cuda().eval()
    r = synthetic.make_rooms(rooms, 1)
    lab_i = synthetic.rule_labels(r)
    x = torch.from_numpy(np.ascontiguousarray(r.transpose(0, 2, 1)[:, :, :, None])).cuda()
    lab, masks = torch.from_numpy(lab_i.astype(np.int64)).cuda(), lab_i == 11
    assert masks.any(axis=1).all(), "a room without a point of class 11: tar_NU_attack divides by the mask count"
    side = torch.cuda.Stream()
    x.record_stream(side)
    lab.record_stream(side)
    done = {}

    def per_room():
        for i in range(rooms):
            torchattacks.tar_NU_attack(net, mask=masks[i], **kw)(x[i:i + 1], lab[i:i + 1])

    def lockstep(R):
        def leg():
            n = 0
            for i in range(0, rooms, R):
                n += int(torchattacks.tar_NU_attack(net, mask=None, **kw).forward_rooms(x[i:i + R], lab[i:i + R], masks[i:i + R])[1].sum())
            done["forward_rooms_R%d" % R] = n
        leg.__name__ = "forward_rooms_R%d" % R
        return leg

    def lockstep_field(R):
        def leg():
            n = 0
            for i in range(0, rooms, R):
                atk = torchattacks.tar_NU_attack(net, mask=None, field=a.field, **kw)
                n += int(atk.forward_rooms(x[i:i + R], lab[i:i + R], masks[i:i + R])[1].sum())
            done[leg.__name__] = n
        leg.__name__ = "forward_rooms_R%d_%s" % (R, a.field)
        return leg

    sizes = [int(v) for v in a.sizes.split(",")]
    assert all(rooms % R == 0 for R in sizes)
    legs = [per_room] + [lockstep(R) for R in sizes]
    if a.field != "color":
        legs += [lockstep_field(R) for R in sizes]
    times = {f.__name__: [] for f in legs}
    with torch.cuda.stream(side):
        for f in legs:                                   # warm-up: workspaces, eager first windows, the capture
            f()
            f()
        for _ in range(runs):                            # alternated: a drift of the machine reaches every leg alike
            for f in legs:
                side.synchronize()
                t = time.perf_counter()
                f()
                side.synchronize()
                times[f.__name__].append(time.perf_counter() - t)
        side.synchronize()
    done["per_room"] = done.get("forward_rooms_R1")      # the same rooms one at a time: the same optimiser steps
    res = dict(network="ResGCN-%d" % a.blocks, n_point=4096, rooms=rooms, steps_cap=a.steps, runs=runs, figures={}, graphs={})
    for name, ts in times.items():
        rps = sorted(rooms / t for t in ts)
        fig = dict(rooms_per_s_min=rps[0], rooms_per_s_median=float(np.median(rps)), rooms_per_s_max=rps[-1], seconds=ts,
                   optimiser_steps=done.get(name))
        if done.get(name):
            fig["ms_per_room_step_median"] = float(np.median(ts)) / done[name] * 1e3
        res["figures"][name] = fig
    for key, S in getattr(net, "_psg_gcn_nu_states", {}).items():
        res["graphs"]["R%d" % key[1]] = _lib.capture_stats(S.graph)
    if a.field != "color":
        res["field"] = a.field
        res["field_over_color"] = {
            "R%d" % R: res["figures"]["forward_rooms_R%d_%s" % (R, a.field)]["rooms_per_s_median"] /
            res["figures"]["forward_rooms_R%d" % R]["rooms_per_s_median"] for R in sizes}
        for key, S in getattr(net, "_psg_gcn_nu_field_states", {}).items():
            res["graphs"]["R%d_%s" % (key[1], key[4])] = _lib.capture_stats(S.graph)
    if a.kernel_trace:
        res["kernels_us"] = new_kernel_durations(a.kernel_trace)
    res["capture_stats_process"] = _lib.capture_stats()
    spread = max(max(v["rooms_per_s_max"] / v["rooms_per_s_min"] for v in res["figures"].values()) - 1.0, 0.0)
    res["largest_spread_of_a_figure"] = spread
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
