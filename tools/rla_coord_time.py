"""Time RandLA-Net's NBattack at 40 960 points with the tester's l_2 settings (magnitude 17, alpha 1.7, bench.py's `randla`
workload) on the colour field - the fused device loop psg_rla_bim_attack, one cloud - beside the coordinate field, the host loop
of DESIGN section 5q (pyramid of the moved positions, forward, hinge gradient, psg_rla_backward_full, field step per
iteration).  One box, one run: after a warm-up of both legs, --runs (at least 3) ALTERNATED timed passes of `color`, `coord`
(and `both` with --both), each over --clouds clouds of --iters iterations, synchronised around every timed region.  Prints
min / median / max clouds per second per leg, `coord_over_color`, and the event-timed cost of one psg_rla_set_cloud
(build_pyramid: five kNN levels, three radix sorts per level) as one JSON line.

    python tools/rla_coord_time.py [--runs 3] [--clouds 2] [--iters 20] [--out profiles/r22_rla_coord.json]

--kernel-trace DIR_OR_CSV reads the CSV of a `rocprofv3 --kernel-trace -- python tools/rla_coord_time.py ...` run made BEFORE
(timings taken under the profiler are not figures) and adds the durations of the new kernels per grid; --trace-only prints
those and stops.

--lockstep times the coordinate field's lockstep form (randla/nb_field.py) instead: eight clouds (--clouds),
the same l_2 settings, a 20-iteration cap; after a warm-up of all legs, --runs (at least 3) ALTERNATED passes of (a) one
`NBattack(field="coord").batch_attack` per cloud - the host loop above, code this form does not change - and (b)
`NBattackField.batch_attack_clouds` at G = 1, 4 and 8 (--sizes).  --targeted does the same for tar_NBattack /
tar_NBattackField with tools/rla_tbim_time.py's settings (magnitude 10, alpha 1, labels = the clean prediction, origin = the class
predicted most, target = the one predicted least) and EXIT_RATIO = (1, 1), the host loop checked not to have left early.
Prints min / median / max clouds per second and ms per cloud and iteration per leg, and the two ratios the section states.

    python tools/rla_coord_time.py --lockstep [--targeted] [--field coord] [--out profiles/r25_rla_nb_field.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NEW_KERNELS = ("relpos_bwd_kernel", "point_sum_kernel", "att_pool_split_dir_xyz_kernel", "field_sq_norm_kernel", "field_l2_delta_kernel",
               "field_l2_apply_kernel", "field_linf_kernel", "tbim_retire_field_kernel")
N_PTS, MAGNITUDE, ALPHA = 40960, 17.0, 1.7


def new_kernel_durations(path):
    """{kernel @ grid: {calls, median_us, min_us}} of the coordinate-gradient kernels out of a rocprofv3 --kernel-trace CSV"""
    import csv
    import re
    from kernel_trace_by_grid import find_trace
    rows = {}
    with open(find_trace(path), newline="") as fh:
        for r in csv.DictReader(fh):
            hit = re.search("|".join(NEW_KERNELS), r["Kernel_Name"])
            if not hit:
                continue
            wg = max(int(r["Workgroup_Size_X"]), 1)
            key = "%s @ %d" % (hit.group(0), int(r["Grid_Size_X"]) // wg)
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {k: dict(calls=len(d), median_us=statistics.median(d), min_us=min(d)) for k, d in sorted(rows.items())}


def lockstep_main(a):
    import torch
    from pointsecguard_amd.randla import attack, nb_field, network
    from pointsecguard_amd.synthetic import randla_params
    runs, clouds, n = max(3, a.runs), a.clouds, N_PTS
    sizes = [int(v) for v in a.sizes.split(",")]
    assert all(clouds % G == 0 for G in sizes)
    magnitude, alpha = (10.0, 1.0) if a.targeted else (MAGNITUDE, ALPHA)
    model = network.RandLAModel(randla_params(3))
    rng = np.random.default_rng(0)
    xyz = (rng.random((clouds, n, 3), dtype=np.float32) * np.array([4, 3, 3], np.float32)).astype(np.float32)
    feats = torch.from_numpy(np.concatenate([xyz, rng.random((clouds, n, 3), dtype=np.float32)], -1)).cuda()
    kw, extra = {}, {}
    if a.targeted:
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
        kw = dict(target=int(np.argsort(counts.sum(0) + (np.arange(13) == ori) * counts.sum(), kind="stable")[0]), ori=ori)
        extra = dict(kw, mask_points=counts[:, ori].tolist())
        parent, sub = attack.tar_NBattack, nb_field.tar_NBattackField
    else:
        labels = torch.from_numpy(rng.integers(0, 13, (clouds, n)).astype(np.int32)).cuda()
        parent, sub = attack.NBattack, nb_field.NBattackField

    def new_attack(cls):
        atk = cls(model, distance_metric="l_2", field=a.field)
        atk.config(magnitude=magnitude, alpha=alpha, iteration=a.iters)
        return atk

    one, lock, worst_sr = new_attack(parent), {G: new_attack(sub) for G in sizes}, [0.0]
    for atk in lock.values():
        atk.EXIT_RATIO = (1, 1)                          # targeted: n_hits > n_mask never holds

    def per_cloud():
        for i in range(clouds):
            out = one.batch_attack(feats[i], labels[i], **kw)
            if a.targeted:
                worst_sr[0] = max(worst_sr[0], out[1])
                if not out[1] <= 0.9:
                    raise SystemExit("the host loop's exit fired (sr = %r on cloud %d): the legs would not do the same work" % (out[1], i))

    def lockstep(G):
        def leg():
            for i in range(0, clouds, G):
                lock[G].batch_attack_clouds(feats[i:i + G], labels[i:i + G], **kw)
                assert not a.targeted or (lock[G].last_steps == a.iters + 1).all()
        leg.__name__ = "batch_attack_clouds_G%d" % G
        return leg

    legs = [per_cloud] + [lockstep(G) for G in sizes]
    times = {f.__name__: [] for f in legs}
    for f in legs:                                       # warm-up: workspaces, kernel attributes
        f()
    for _ in range(runs):                                # alternated: a drift of the machine reaches every leg alike
        for f in legs:
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[f.__name__].append(time.perf_counter() - t)
    res = dict(tool="rla_coord_time --lockstep", network="RandLA-Net", attack="tar_NBattack" if a.targeted else "NBattack", field=a.field,
               metric="l_2", magnitude=magnitude, alpha=alpha, n_points=n, clouds=clouds, iteration_cap=a.iters, gradient_steps=a.iters + 1,
               runs=runs, figures={}, device=torch.cuda.get_device_name(0), **extra)
    if a.targeted:
        res["host_loop_worst_sr"] = worst_sr[0]
    for name, ts in times.items():
        cps = sorted(clouds / t for t in ts)
        res["figures"][name] = dict(clouds_per_s_min=cps[0], clouds_per_s_median=statistics.median(cps), clouds_per_s_max=cps[-1], seconds=ts,
                                    ms_per_cloud_iteration_median=statistics.median(ts) / (clouds * (a.iters + 1)) * 1e3)
    med = {k: v["clouds_per_s_median"] for k, v in res["figures"].items()}
    res["largest_spread_of_a_figure"] = max(v["clouds_per_s_max"] / v["clouds_per_s_min"] for v in res["figures"].values()) - 1.0
    for G in sizes:
        res["G%d_over_per_cloud" % G] = med["batch_attack_clouds_G%d" % G] / med["per_cloud"]
    if a.kernel_trace:
        res["kernels_us"] = new_kernel_durations(a.kernel_trace)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a" if a.append else "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--both", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--lockstep", action="store_true")
    ap.add_argument("--targeted", action="store_true")
    ap.add_argument("--field", default="coord", choices=("coord", "both"))
    ap.add_argument("--sizes", default="1,4,8")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    if a.trace_only:
        print(json.dumps(dict(kernels_us=new_kernel_durations(a.kernel_trace))))
        return
    if a.clouds is None:
        a.clouds = 8 if a.lockstep or a.targeted else 2
    if a.lockstep or a.targeted:
        lockstep_main(a)
        return
    import torch
    from pointsecguard_amd.randla import attack, network
    from pointsecguard_amd.synthetic import randla_params
    model = network.RandLAModel(randla_params(3))
    rng = np.random.default_rng(4)
    clouds = []
    for _ in range(a.clouds):
        xyz = (rng.random((N_PTS, 3), dtype=np.float32) * np.array([8, 6, 3], np.float32)).astype(np.float32)
        f = np.concatenate([xyz, rng.random((N_PTS, 3), dtype=np.float32)], 1)
        clouds.append((torch.from_numpy(f).cuda(), torch.from_numpy(rng.integers(0, 13, N_PTS).astype(np.int32)).cuda()))
    legs = {}
    for field in ("color", "coord") + (("both",) if a.both else ()):
        atk = attack.NBattack(model, distance_metric="l_2", field=field)
        atk.config(magnitude=MAGNITUDE, alpha=ALPHA, iteration=a.iters)
        legs[field] = atk

    def one_pass(atk):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f, y in clouds:
            atk.batch_attack(f, y)
        torch.cuda.synchronize()
        return len(clouds) / (time.perf_counter() - t0)

    for atk in legs.values():                                   # warm-up: workspaces, the colour loop's graph capture
        one_pass(atk)
    rates = {k: [] for k in legs}
    for _ in range(max(3, a.runs)):
        for k, atk in legs.items():
            rates[k].append(one_pass(atk))
    ws = legs["coord"]._ws[("field", N_PTS)].ws
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    pyramid = []
    for _ in range(5):
        ev[0].record()
        ws.set_cloud(clouds[0][0][:, 0:3].contiguous())
        ev[1].record()
        torch.cuda.synchronize()
        pyramid.append(ev[0].elapsed_time(ev[1]))
    out = dict(tool="rla_coord_time", n_points=N_PTS, metric="l_2", magnitude=MAGNITUDE, alpha=ALPHA, iterations=a.iters,
               gradient_steps=a.iters + 1, clouds_per_pass=a.clouds, runs=max(3, a.runs),
               clouds_per_s={k: dict(min=min(v), median=statistics.median(v), max=max(v)) for k, v in rates.items()},
               coord_over_color=statistics.median(rates["coord"]) / statistics.median(rates["color"]),
               ms_per_gradient_step={k: 1e3 / statistics.median(v) / (a.iters + 1) for k, v in rates.items()},
               set_cloud_ms=dict(min=min(pyramid), median=statistics.median(pyramid), max=max(pyramid)),
               full_workspace_bytes=ws.nbytes, device=torch.cuda.get_device_name(0))
    if a.kernel_trace:
        out["kernels_us"] = new_kernel_durations(a.kernel_trace)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
