"""Time the vanilla PointNet path on 8-room batches: the module forward, and NB_attack(eps=0.1, alpha=0.05, iters=10)
(the reference script's settings, NB_nontarget_test_semseg.py:169).  Prints one JSON line.

    python tools/pointnet_time.py [--rooms 8] [--reps 20] [--out profiles/pointnet_time.json]

--nu times tar_NU_attack instead, with the settings of bench.py's `tarnu` workload (c=1, kappa=0, lr=0.01, target=6, mask =
label == 11, steps capped at 40) at 8 and 32 rooms: (a) one call per room with a fresh attack object, as the reference's
harness applies it, (b) the same rooms through forward_rooms (lockstep; skipped where the tree has none for this network),
(c) lockstep with the three-kernel head instead of pn_nu_head_kernel.  Every figure is run --runs times (at least 3) on a
side stream, each figure in a block of its own after its own warm-up, synchronised around the timed region; prints min / median / max rooms per second, the optimiser steps that
actually ran, and the hipGraph bookkeeping of the process (psg_capture_stats) as one JSON line.

    python tools/pointnet_time.py --nu [--runs 3] [--sizes 8,32] [--out profiles/r10_pointnet_nu_run.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pointsecguard_amd import synthetic  # noqa: E402
from pointsecguard_amd.attacks import torchattacks  # noqa: E402
from pointsecguard_amd.models.pointnet_sem_seg import get_model  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def nu_main(a):
    import inspect
    from pointsecguard_amd import _lib
    from pointsecguard_amd.attacks.torchattacks.attacks import pointnet as pn
    steps, target = 40, 6
    kw = dict(c=1, kappa=0, steps=steps, lr=0.01, target=target)
    net = get_model(13)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.pointnet_state_dict(3).items()})
    net = net.cuda().eval()
    has_rooms = "return_steps" in inspect.signature(pn.nu_attack).parameters       # the window path of this network
    side = torch.cuda.Stream()
    res = dict(mode="nu", steps_cap=steps, runs=max(3, a.runs), lockstep_available=has_rooms, figures={})

    def stats(ts, rooms):
        rps = sorted(rooms / t for t in ts)
        return dict(rooms_per_s_min=rps[0], rooms_per_s_median=float(np.median(rps)), rooms_per_s_max=rps[-1], seconds=ts)

    for rooms in [int(v) for v in a.sizes.split(",")]:
        r = synthetic.make_rooms(rooms, 1)
        lab_i = synthetic.rule_labels(r)
        x = torch.from_numpy(np.ascontiguousarray(r.transpose(0, 2, 1))).cuda()
        x.record_stream(side)
        lab, masks = lab_i.astype(np.float64), lab_i == 11
        done = {}

        def per_room():                                          # the harness's call, the same on every tree
            for i in range(rooms):
                torchattacks.tar_NU_attack(net, mask=masks[i], **kw)(x[i:i + 1], lab[i:i + 1])

        def per_room_steps():                                    # (outside the timed region)
            if not has_rooms:
                return None                                      # this tree's forward does not report them
            return int(sum(pn.nu_attack(torchattacks.tar_NU_attack(net, mask=masks[i], **kw), x[i:i + 1], lab[i:i + 1], mask=masks[i],
                                        target=target, neighbour=5, targeted_variant=True, return_steps=True)[1] for i in range(rooms)))

        def lockstep():
            done["lockstep"] = int(torchattacks.tar_NU_attack(net, mask=None, **kw).forward_rooms(x, lab, masks)[1].sum())

        def lockstep_three_kernel_head():
            done["lockstep_three_kernel_head"] = int(torchattacks.tar_NU_attack(net, mask=None, **kw).forward_rooms(x, lab, masks)[1].sum())

        legs = [per_room] + ([lockstep, lockstep_three_kernel_head] if has_rooms else [])
        times = {f.__name__: [] for f in legs}
        with torch.cuda.stream(side):
            # every leg in a block of its own after its own warm-up (workspaces, first eager windows, graph capture): the head
            # variant is part of a window's graph key, so alternating the two lockstep legs would re-capture in every call
            for f in legs:
                pn.fused_head = f is not lockstep_three_kernel_head
                try:
                    f()
                    f()
                    for _ in range(max(3, a.runs)):
                        side.synchronize()
                        t = time.perf_counter()
                        f()
                        side.synchronize()
                        times[f.__name__].append(time.perf_counter() - t)
                finally:
                    pn.fused_head = True
            done["per_room"] = per_room_steps()
            side.synchronize()
        for name, ts in times.items():
            res["figures"]["%s_%d" % (name, rooms)] = dict(stats(ts, rooms), optimiser_steps=done[name])
    res["capture_stats"] = _lib.capture_stats()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nu", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", default="8,32")
    a = ap.parse_args()
    if a.nu:
        return nu_main(a)
    net = get_model(13)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.pointnet_state_dict(3).items()})
    net = net.cuda().eval()
    r = synthetic.make_rooms(a.rooms, 1)
    x = torch.from_numpy(np.ascontiguousarray(r.transpose(0, 2, 1))).cuda()
    lab = synthetic.rule_labels(r).astype(np.float64)
    atk = torchattacks.NB_attack(net, eps=0.1, alpha=0.05, iters=10)

    def fwd():
        with torch.no_grad():
            net(x)

    t_fwd = timed(fwd, a.reps)
    t_nb = timed(lambda: atk(x, lab), max(1, a.reps // 4))
    mac_exec, mac_ref = 621e3, 1149321       # per point
    n = a.rooms * 4096
    res = dict(rooms=a.rooms, forward_ms=t_fwd * 1e3, forward_rooms_per_s=a.rooms / t_fwd,
               forward_tflops_executed=2 * mac_exec * n / t_fwd / 1e12, forward_tflops_reference=2 * mac_ref * n / t_fwd / 1e12,
               nb10_ms=t_nb * 1e3, nb10_rooms_per_s=a.rooms / t_nb)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
