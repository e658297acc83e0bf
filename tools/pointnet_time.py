"""Time the vanilla PointNet path on 8-room batches: the module forward, and NB_attack(eps=0.1, alpha=0.05, iters=10)
(the reference script's settings, NB_nontarget_test_semseg.py:169).  Prints one JSON line.

    python tools/pointnet_time.py [--rooms 8] [--reps 20] [--out profiles/pointnet_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
