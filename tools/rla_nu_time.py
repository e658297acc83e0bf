"""Time NUattack on RandLA-Net (40 960-point clouds, synthetic weights) with a fixed step cap and exits that cannot fire
(labels = the clean prediction, so the accuracy stays near 1; the lockstep legs also get the threshold 0 / 1):
(a) one `batch_attack` per cloud - the host loop of randla/attack.py: two forwards and one backward per optimiser step, one
    blocking read-back per step;
(b) the same clouds through `batch_attack_clouds` (psg_rla_nu_window: lockstep, device-side windows, one forward and one
    backward per step) at G = 1, 4 and 8.
Every figure works on the same --clouds clouds (G = 4: two calls, G = 1: eight).  The legs ALTERNATE: after a warm-up pass over
all of them (workspaces, first eager windows, graph capture) every run times (a), G = 1, G = 4, G = 8 in turn, --runs times
(at least 3), on a side stream, synchronised around each timed region.  Prints min / median / max clouds per second, ms per
optimiser step and cloud, and the hipGraph bookkeeping of each lockstep shape as one JSON line.

--field coord | both times the coordinate-field attack instead (randla/nu_field.py, psg_rla_nu_field_window: the pyramid of
every cloud rebuilt in every step, the full backward, no hipGraph): there is no host loop for that field, so leg (a) is left out
and the colour lockstep legs stay as the baseline the field legs alternate with; the JSON line then also carries `field` and the
bytes of each full workspace.  With the default, --field color, nothing changes.

    python tools/rla_nu_time.py [--runs 3] [--clouds 8] [--steps 20] [--points 40960] [--field color] [--out profiles/r18_rla_nu.json]
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
from pointsecguard_amd.randla import attack, network, nu_field  # noqa: E402
from pointsecguard_amd.synthetic import randla_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--points", type=int, default=40960)
    ap.add_argument("--sizes", default="1,4,8")
    ap.add_argument("--field", default="color", choices=("color", "coord", "both"))
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
    one = attack.NUattack(model, 1, "ut", "l_2")
    one.config(cs=1.0, iteration=a.steps)
    lock = {}
    for G in sizes:
        lock[G] = attack.NUattack(model, 1, "ut", "l_2")
        lock[G].config(cs=1.0, iteration=a.steps)
        lock[G].EXIT_RATIO = (0, 1)                      # den * n_correct < 0 never holds
    moved = {}
    if a.field != "color":
        for G in sizes:
            moved[G] = nu_field.NUattackField(model, 1, "ut", "l_2", field=a.field)
            moved[G].config(cs=1.0, iteration=a.steps)
            moved[G].EXIT_RATIO = (0, 1)
    steps_run = {}
    with torch.cuda.stream(side):
        feats = torch.from_numpy(feats_h).cuda()
        ws = network.RandLAWorkspace(n)
        labels = []
        for i in range(clouds):                          # labels = the clean prediction: the host loop's `acc < 1/13` cannot fire
            ws.set_cloud(feats[i, :, 0:3].contiguous())
            labels.append(ws.forward(model, feats[i]).argmax(1))
        labels = torch.stack(labels)
        del ws

        def per_cloud():
            for i in range(clouds):
                one.batch_attack(feats[i], labels[i])
            steps_run["per_cloud"] = clouds * a.steps

        def lockstep(G):
            def leg():
                done = 0
                for i in range(0, clouds, G):
                    lock[G].batch_attack_clouds(feats[i:i + G], labels[i:i + G])
                    done += int(lock[G].last_steps.sum())
                steps_run[leg.__name__] = done
            leg.__name__ = "batch_attack_clouds_G%d" % G
            return leg

        def field_leg(G):
            def leg():
                done = 0
                for i in range(0, clouds, G):
                    moved[G].batch_attack_clouds(feats[i:i + G], labels[i:i + G])
                    done += int(moved[G].last_steps.sum())
                steps_run[leg.__name__] = done
            leg.__name__ = "field_%s_G%d" % (a.field, G)
            return leg

        legs = [per_cloud] + [lockstep(G) for G in sizes]
        if a.field != "color":
            legs = [f for G in sizes for f in (lockstep(G), field_leg(G))]
        times = {f.__name__: [] for f in legs}
        np.random.seed(0)
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
    res = dict(network="RandLA-Net", n_point=n, clouds=clouds, steps_cap=a.steps, runs=runs, figures={}, graphs={})
    for name, ts in times.items():
        cps = sorted(clouds / t for t in ts)
        res["figures"][name] = dict(clouds_per_s_min=cps[0], clouds_per_s_median=float(np.median(cps)), clouds_per_s_max=cps[-1],
                                    seconds=ts, optimiser_steps=steps_run[name],
                                    ms_per_cloud_step_median=float(np.median(ts)) / steps_run[name] * 1e3)
    for G in sizes:
        S = lock[G]._clouds[(n, G)]
        res["graphs"]["G%d" % G] = dict(full=_lib.capture_stats(S.graph), full_with_tail=_lib.capture_stats(S.graph_tail))
    if a.field != "color":
        res["field"] = a.field
        res["full_workspace_bytes"] = {"G%d" % G: int(moved[G]._field_clouds[(n, G)].ws.nbytes) for G in sizes}
    res["capture_stats_process"] = _lib.capture_stats()
    res["largest_spread_of_a_figure"] = max(max(v["clouds_per_s_max"] / v["clouds_per_s_min"] for v in res["figures"].values()) - 1.0, 0.0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
