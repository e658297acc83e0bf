#!/usr/bin/env python3
"""Per-launch time of the SSG module kernels on rooms shrunk by a factor (GPU; HIP events of psg_pn2_prof_read).

At --shrink 0.25 every level-0 ball of a 4096-point room is full: the packed SA forward (PSG_PN2_PACK, default on) has nothing
to skip there and must cost what the unpacked kernel does.  Run once per value of PSG_PN2_PACK (read once per process) and
compare the sa*_fwd rows; the other rows are kernels the switch does not touch and show the run-to-run spread.  The same holds
for the packed SA backward (PSG_PN2_PACK_BWD, default on where a level has the kernel): run under PSG_PN2_PACK_BWD=0 and unset,
alternated, and compare the sa*_bwd rows - full workgroups run the unpacked backward body there.

usage: [PSG_PN2_PACK=0] [PSG_PN2_PACK_BWD=0] tools/sa_pack_probe.py [--rooms 64] [--shrink 0.25] [--iters 20] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=64)
    ap.add_argument("--shrink", type=float, default=0.25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import make_rooms, rule_labels
    R, N = a.rooms, 4096
    rooms = make_rooms(R, 1000)
    rooms[..., 0:3] *= np.float32(a.shrink)
    model = runtime.PN2Model(runtime.fold_state_dict(dict(np.load(os.path.join(ROOT, "tests", "golden", "pn2_weights.npz")))))
    ws = runtime.PN2Workspace(R, N, 1)
    x0 = torch.from_numpy(rooms).cuda()
    labels = torch.from_numpy(rule_labels(rooms).astype(np.int32)).cuda()
    rng = np.random.default_rng(0)
    starts = np.stack([rng.integers(0, n, (1, R)) for n in (4096, 1024, 256, 64)], axis=1).astype(np.int32)
    ws.plan_build(x0, torch.from_numpy(starts).cuda(), 1)
    logp = torch.empty(R, N, 13, device="cuda")
    dlogp = torch.empty_like(logp)

    def iteration():
        ws.forward(model, 0, x0, logp=logp, lean=True)
        _lib.call("psg_ce_logp_grad", runtime.ptr(logp), runtime.ptr(labels), 0, R * N, R * N, 13, 1.0 / N, runtime.ptr(dlogp),
                  None, runtime.stream())
        ws.backward(model, 0, dlogp, colour_only=True)

    for _ in range(5):
        iteration()
    torch.cuda.synchronize()
    ws.prof_enable(True)
    for _ in range(a.iters):
        iteration()
    torch.cuda.synchronize()
    prof = ws.prof_read()
    us = {k: round(1000.0 * ms / n, 2) for k, (ms, n) in sorted(prof.items())}
    res = {"PSG_PN2_PACK": os.environ.get("PSG_PN2_PACK", "1"), "PSG_PN2_PACK_BWD": os.environ.get("PSG_PN2_PACK_BWD", "1"),
           "rooms": R, "shrink": a.shrink, "us_per_launch": us}
    print(json.dumps(res))
    print("sa backward:", " ".join("%s %.2f" % (k, v) for k, v in us.items() if k.startswith("sa") and k.endswith("_bwd")))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
