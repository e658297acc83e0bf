"""Time tar_NBattack on RandLA-Net (40 960-point clouds, synthetic weights) with the settings tester_S3DIS.py:277-280 gives it
(l_2, magnitude 10, alpha 1) under a fixed iteration cap and exits that cannot fire:
(a) one `batch_attack` per cloud - the host loop of randla/attack.py: forward, hinge, backward and update per iteration, the
    40 960-int arg-max read back and evaluated on the host every iteration;
(b) the same clouds through `batch_attack_clouds` (psg_rla_tbim_window: lockstep, device-side windows, one read-back per
    window) at G = 1, 4 and 8.
The mask is one class: labels = the clean prediction, origin = the class predicted most, target = the class predicted least.
The lockstep legs get EXIT_RATIO = (1, 1) (n_hits > n_mask never holds); the host loop's `sr > 0.9` is checked not to have
held: every `batch_attack` must return sr <= 0.9 (an earlier exit returns the sr that caused it), or the tool stops.
Every figure works on the same --clouds clouds (G = 4: two calls, G = 1: eight).  The legs ALTERNATE: after a warm-up pass over
all of them (workspaces, first eager windows, graph capture) every run times (a), G = 1, G = 4, G = 8 in turn, --runs times
(at least 3), on a side stream, synchronised around each timed region.  Prints min / median / max clouds per second, ms per
iteration and cloud, and the hipGraph bookkeeping of each lockstep shape as one JSON line.

    python tools/rla_tbim_time.py [--runs 3] [--clouds 8] [--steps 20] [--points 40960] [--out profiles/r21_rla_tbim.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pointsecguard_amd import _lib  # noqa: E402
from pointsecguard_amd.randla import attack, network  # noqa: E402
from pointsecguard_amd.synthetic import randla_params  # noqa: E402

MAGNITUDE, ALPHA = 10.0, 1.0     # tester_S3DIS.py:277-280


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--points", type=int, default=40960)
    ap.add_argument("--sizes", default="1,4,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    runs, clouds, n = max(3, a.runs), a.clouds, a.points
    sizes = [int(v) for v in a.sizes.split(",")]
    assert all(clouds % G == 0 for G in sizes)
    model = network.RandLAModel(randla_params(3))
    rng = np.random.default_rng(0)
    xyz = (rng.random((clouds, n, 3), dtype=np.float32) * np.array([4, 3, 3], np.float32)).astype(np.float32)
    feats_h = np.concatenate([xyz, rng.random((clouds, n, 3), dtype=np.float32)], -1)
    side = torch.cuda.Stream()

    def new_attack():
        cls = attack.tar_NBattack(model, 1, goal="t", distance_metric="l_2")
        cls.config(magnitude=MAGNITUDE, alpha=ALPHA, iteration=a.steps)
        return cls

    one = new_attack()
    lock = {}
    for G in sizes:
        lock[G] = new_attack()
        lock[G].EXIT_RATIO = (1, 1)                      # n_hits > n_mask never holds
    iters_run, worst_sr = {}, [0.0]
    with torch.cuda.stream(side):
        feats = torch.from_numpy(feats_h).cuda()
        ws = network.RandLAWorkspace(n)
        labels = []
        for i in range(clouds):
            ws.set_cloud(feats[i, :, 0:3].contiguous())
            labels.append(ws.forward(model, feats[i]).argmax(1))
        labels = torch.stack(labels)
        del ws
        counts = np.stack([np.bincount(l, minlength=13) for l in labels.cpu().numpy()])
        ori = int(counts.min(0).argmax())                # every cloud has points of it
        assert counts[:, ori].min() > 0, "no class is predicted in every cloud"
        target = int(np.argsort(counts.sum(0) + (np.arange(13) == ori) * counts.sum(), kind="stable")[0])

        def per_cloud():
            for i in range(clouds):
                out = one.batch_attack(feats[i], labels[i], target=target, ori=ori)
                worst_sr[0] = max(worst_sr[0], out[1])
                if not out[1] <= 0.9:
                    raise SystemExit("the host loop's exit fired (sr = %r on cloud %d): the legs would not do the same work" % (out[1], i))
            iters_run["per_cloud"] = clouds * (a.steps + 1)

        def lockstep(G):
            def leg():
                done = 0
                for i in range(0, clouds, G):
                    lock[G].batch_attack_clouds(feats[i:i + G], labels[i:i + G], target=target, ori=ori)
                    done += int(lock[G].last_steps.sum())
                assert done == clouds * (a.steps + 1), done
                iters_run[leg.__name__] = done
            leg.__name__ = "batch_attack_clouds_G%d" % G
            return leg

        legs = [per_cloud] + [lockstep(G) for G in sizes]
        times = {f.__name__: [] for f in legs}
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
    res = dict(network="RandLA-Net", attack="tar_NBattack", metric="l_2", magnitude=MAGNITUDE, alpha=ALPHA, n_point=n, clouds=clouds,
               iteration_cap=a.steps, runs=runs, ori=ori, target=target, mask_points=counts[:, ori].tolist(), host_loop_worst_sr=worst_sr[0],
               figures={}, graphs={})
    for name, ts in times.items():
        cps = sorted(clouds / t for t in ts)
        res["figures"][name] = dict(clouds_per_s_min=cps[0], clouds_per_s_median=float(np.median(cps)), clouds_per_s_max=cps[-1],
                                    seconds=ts, iterations=iters_run[name],
                                    ms_per_cloud_iteration_median=float(np.median(ts)) / iters_run[name] * 1e3)
    for G in sizes:
        S = lock[G]._clouds[(n, G)]
        res["graphs"]["G%d" % G] = dict(full=_lib.capture_stats(S.graph), full_and_final=_lib.capture_stats(S.graph_tail))
    res["capture_stats_process"] = _lib.capture_stats()
    res["largest_spread_of_a_figure"] = max(max(v["clouds_per_s_max"] / v["clouds_per_s_min"] for v in res["figures"].values()) - 1.0, 0.0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
