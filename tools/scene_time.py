"""Time the whole-scene NB attack (harness.evaluate_whole_scene_consistent) against the per-block loop
(harness.evaluate_whole_scene with torchattacks.NB_attack) on a synthetic room at the user's size: --points (300 000) points
in a --size (6 x 5 m) room, block_points = 4096, eps 0.1 / alpha 0.05 / iters 10 (NB_nontarget_test_semseg.py:169),
batch_size 8, one scene.

    python tools/scene_time.py [--points 300000] [--size 6 5] [--runs 5] [--out profiles/r28_scene_attack.json]

One box, one process.  After one warm-up of every variant: --runs rounds, and in every round the three variants one after the
other - the consistent loop, the per-block loop with streams = 1, the per-block loop with its default streams -, each call from
np.random.seed / torch.manual_seed to a device synchronise (the host-side slicing of the room is inside every figure: all
three pay the same one).  Median, min and max in blocks/s (blocks of the room / wall time of the call) and the ratios of the medians.
The per-block loop is the yardstick; the consistent loop rebuilds the geometry plan for every (iteration, batch) and coalesces
nothing, so it is expected to be slower.

--field coord | both adds the coordinate field to the same rounds: after `consistent` (colours, as above)
come `consistent_field` (SceneNBAttack(field=...), one displacement per scene point) and the per-block loop with
NB_attack(field=...) at streams = 1 and at its default streams; coord_eps / coord_alpha follow eps / alpha.  The ratios are then
consistent_field over each of the three.

--kernel-trace DIR_OR_CSV folds in, from a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/scene_time.py --only consistent --runs 1` (with --field: `--only consistent_field`) run made BEFORE, the share of the device time of that run spent in the kernels
of csrc/psg_scene.hip, and in the two coordinate-field kernels among them (timings taken under the profiler are not figures for the calls); --trace-only prints that and stops.

--attack nu times the whole-scene NU attack (attacks.scene.SceneNUAttack) instead; --attack nb (default)
is everything above, unchanged.  Same synthetic room, sliced ONCE outside the timed calls; steps = --iters (10), exit_below =
(0, 1) so that the exit cannot fire; two variants alternated in one process after a warm-up of each: `scene_nu` - one
SceneNUAttack call on the room's blocks - and `per_block_nu` - NU_attack.forward_rooms over the same blocks in groups of
batch_size (a last group of one block: NU_attack's plain call).  Both attack the network's own clean predictions, which keeps the
per-block attack's exit (correct / 4096 < 1 / 13) from firing; the steps every block ran are checked and reported.  Each call
from torch.manual_seed to a device synchronise.  No speed bar: the scene attack rebuilds the geometry plan per (step, batch) on
one stream and replays nothing, the per-block path plans ten steps at once and replays captured windows.  With --attack nu
--kernel-trace / --trace-only report the share of the kernels of csrc/psg_scene_nu.hip (and of the psg_scene.hip kernels the
attack launches) in a `--only scene_nu --runs 1` profiler run.

--attack nu --field coord | both alternates three variants in the same way: `scene_nu_field` -
SceneNUAttack(field=...), Adam on one displacement per scene point -, `scene_nu` - the colour field of the same loop - and
`per_block_nu_field` - NU_attack(field=...).forward_rooms over the same blocks in groups of batch_size.  The ratios are
scene_nu_field over each of the other two; the kernel-trace share (a `--only scene_nu_field --runs 1` profiler run) lists
scene_nu_field_step_kernel on its own.  No speed bar.
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

OURS = ("occ_count_kernel", "occ_scan_kernel", "occ_fill_kernel", "occ_rank_kernel", "colour_to_blocks_kernel",
        "rows_mask_kernel", "scene_pgd_step_kernel", "delta_to_blocks_kernel", "scene_field_step_kernel")
FIELD_KERNELS = ("delta_to_blocks_kernel", "scene_field_step_kernel")
VARIANTS = ("consistent", "per_block_streams1", "per_block_default")
FIELD_VARIANTS = ("consistent", "consistent_field", "per_block_field_streams1", "per_block_field_default")


def synthetic_room(n, size_x, size_y, seed=28):
    """S3DIS-format room [n, 7]: xyz in metres, rgb 0..255, label"""
    rng = np.random.default_rng(seed)
    xyz = rng.random((n, 3)) * np.array([size_x, size_y, 2.8])
    rgb = np.floor(rng.random((n, 3)) * 256.0)
    label = rng.integers(0, 13, n).astype(np.float64)
    return np.concatenate([xyz, rgb, label[:, None]], axis=1)


def scene_kernel_share(path):
    """device time of the psg_scene.hip kernels over the device time of all kernels of a rocprofv3 --kernel-trace CSV"""
    import csv
    from kernel_trace_by_grid import find_trace
    ours, total, per = 0.0, 0.0, {}
    with open(find_trace(path), newline="") as fh:
        for r in csv.DictReader(fh):
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
            total += us
            name = next((k for k in OURS if k + "(" in r["Kernel_Name"]), None)
            if name is not None:
                ours += us
                d = per.setdefault(name, dict(calls=0, total_us=0.0))
                d["calls"] += 1
                d["total_us"] += us
    field = sum(per[k]["total_us"] for k in FIELD_KERNELS if k in per)
    return dict(scene_kernels_us=ours, field_kernels_us=field, all_kernels_us=total, share=ours / total if total else None,
                field_share=field / total if total else None, kernels=per)


NU_KERNELS = ("scene_nu_init_kernel", "scene_nu_colour_kernel", "scene_nu_step_kernel", "scene_nu_count_kernel",
              "scene_nu_decide_kernel", "scene_nu_field_step_kernel")
NU_VARIANTS = ("scene_nu", "per_block_nu")
NU_FIELD_VARIANTS = ("scene_nu_field", "scene_nu", "per_block_nu_field")


def nu_kernel_share(path):
    """device time of the psg_scene_nu.hip kernels (and of the psg_scene.hip kernels beside them) over all kernels of a trace"""
    import csv
    from kernel_trace_by_grid import find_trace
    total, per = 0.0, {}
    with open(find_trace(path), newline="") as fh:
        for r in csv.DictReader(fh):
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
            total += us
            name = next((k for k in NU_KERNELS + OURS if k + "(" in r["Kernel_Name"]), None)
            if name is not None:
                d = per.setdefault(name, dict(calls=0, total_us=0.0))
                d["calls"] += 1
                d["total_us"] += us
    nu = sum(d["total_us"] for k, d in per.items() if k in NU_KERNELS)
    scene = sum(d["total_us"] for k, d in per.items() if k in OURS)
    step = per.get("scene_nu_field_step_kernel", {}).get("total_us", 0.0)
    return dict(nu_kernels_us=nu, scene_kernels_us=scene, all_kernels_us=total, nu_share=nu / total if total else None,
                scene_share=scene / total if total else None, field_step_share=step / total if total else None, kernels=per)


def main_nu(a, ap):
    """--attack nu: SceneNUAttack beside NU_attack.forward_rooms over the same blocks (see the module docstring)"""
    if a.trace_only:
        print(json.dumps(dict(kernel_trace=nu_kernel_share(a.kernel_trace))))
        return
    import torch
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model, upload
    assert torch.cuda.is_available(), "scene_time.py measures on the MI355X; there is nothing to time without it"
    all_variants = NU_VARIANTS if a.field == "color" else NU_FIELD_VARIANTS
    if a.only and a.only not in all_variants:
        ap.error("--only %s does not exist under --attack nu --field %s" % (a.only, a.field))
    room = synthetic_room(a.points, a.size[0], a.size[1])
    ds = harness.ScannetDatasetWholeScene(None, block_points=a.block_points, scenes={"Area_5_room.npy": room})
    np.random.seed(3)
    data, _, _, index = ds[0]
    n_blocks = int(data.shape[0])
    counts = np.bincount(index.reshape(-1), minlength=a.points)
    torch.manual_seed(1)
    net = get_model(13).cuda().eval()          # random weights: the time of an attack does not depend on what the network predicts
    dev = torch.device("cuda")
    x = upload(torch.from_numpy(data.astype(np.float32)), dev, pin=True)
    idx = upload(torch.from_numpy(index.astype(np.int32)), dev, pin=True)
    images = x.transpose(2, 1).contiguous()                                    # [nb, 9, bp], what the per-block attack takes
    groups = [(lo, min(lo + a.batch_size, n_blocks)) for lo in range(0, n_blocks, a.batch_size)]
    with torch.no_grad():                      # labels: the clean predictions (an exit on accuracy cannot fire at the start)
        gt = torch.cat([net(images[lo:hi])[0].argmax(dim=2).to(torch.int32) for lo, hi in groups]).contiguous()
    rgb, scene_labels = room[:, 3:6], room[:, 6]
    ran = {}

    def call(variant):
        torch.manual_seed(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if variant in ("scene_nu", "scene_nu_field"):
            atk = SceneNUAttack(net, steps=a.iters, batch_size=a.batch_size, exit_below=(0, 1),
                                field=a.field if variant == "scene_nu_field" else "color")
            atk(x, idx, gt, rgb, scene_labels)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ran[variant] = [a.iters if atk.last_exit_step < 0 else atk.last_exit_step + 1]
        else:
            field = a.field if variant == "per_block_nu_field" else "color"
            atk = torchattacks.NU_attack(net, steps=a.iters, field=field)
            steps_run = []
            for lo, hi in groups:
                if hi - lo > 1 or field != "color":       # (the field form attacks one room per call: rooms form throughout)
                    steps_run += [int(s) for s in atk.forward_rooms(images[lo:hi], gt[lo:hi])[1]]
                else:
                    atk(images[lo:hi], gt[lo:hi])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ran[variant] = steps_run
        return n_blocks / dt

    variants = [a.only] if a.only else list(all_variants)
    for v in variants:                          # warm-up: workspaces, packed weights, captured windows
        call(v)
    rate = {v: [] for v in variants}
    for _ in range(a.runs):
        for v in variants:
            rate[v].append(call(v))
    med = {v: statistics.median(r) for v, r in rate.items()}
    out = dict(tool="scene_time", attack="nu", device=torch.cuda.get_device_name(0), n_points=a.points, size=list(a.size),
               block_points=a.block_points, n_blocks=n_blocks, batch_size=a.batch_size, steps=a.iters, exit_below=[0, 1], runs=a.runs,
               field=a.field, occurrences=dict(mean=float(counts.mean()), max=int(counts.max()), multi_share=float((counts > 1).mean())),
               blocks_per_s={v: dict(median=med[v], min=min(r), max=max(r), spread=(max(r) - min(r)) / med[v]) for v, r in rate.items()},
               steps_run={v: dict(min=min(r), max=max(r)) for v, r in ran.items() if r})
    if not a.only and a.field != "color":
        out["scene_nu_field_over"] = {v: med["scene_nu_field"] / med[v] for v in variants if v != "scene_nu_field"}
    elif not a.only:
        out["scene_nu_over_per_block_nu"] = med["scene_nu"] / med["per_block_nu"]
    if a.kernel_trace:
        out["kernel_trace"] = nu_kernel_share(a.kernel_trace)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attack", choices=("nb", "nu"), default="nb")
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--size", type=float, nargs=2, default=(6.0, 5.0))
    ap.add_argument("--block-points", type=int, default=4096)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--field", choices=("color", "coord", "both"), default="color")
    ap.add_argument("--only", choices=sorted(set(VARIANTS + FIELD_VARIANTS + NU_VARIANTS + NU_FIELD_VARIANTS)), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.attack == "nu":
        return main_nu(a, ap)
    if a.trace_only:
        print(json.dumps(dict(kernel_trace=scene_kernel_share(a.kernel_trace))))
        return
    import torch
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.attacks.scene import SceneNBAttack
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model
    assert torch.cuda.is_available(), "scene_time.py measures on the MI355X; there is nothing to time without it"
    eps, alpha = 0.1, 0.05
    room = synthetic_room(a.points, a.size[0], a.size[1])
    ds = harness.ScannetDatasetWholeScene(None, block_points=a.block_points, scenes={"Area_5_room.npy": room})
    np.random.seed(3)
    n_blocks = int(ds[0][0].shape[0])
    counts = np.bincount(ds[0][3].reshape(-1), minlength=a.points)
    torch.manual_seed(1)
    net = get_model(13).cuda().eval()          # random weights: the time of an attack does not depend on what the network predicts
    quiet = lambda *_: None

    def call(variant):
        np.random.seed(3)
        torch.manual_seed(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if variant == "consistent":
            harness.evaluate_whole_scene_consistent(net, ds, lambda m: SceneNBAttack(m, eps, alpha, a.iters),
                                                    batch_size=a.batch_size, log=quiet)
        elif variant == "consistent_field":
            harness.evaluate_whole_scene_consistent(net, ds, lambda m: SceneNBAttack(m, eps, alpha, a.iters, field=a.field),
                                                    batch_size=a.batch_size, log=quiet)
        elif variant.startswith("per_block_field"):
            kw = {"streams": 1} if variant == "per_block_field_streams1" else {}
            harness.evaluate_whole_scene(net, ds, lambda m: torchattacks.NB_attack(m, eps=eps, alpha=alpha, iters=a.iters,
                                                                                     field=a.field),
                                         batch_size=a.batch_size, log=quiet, **kw)
        else:
            kw = {"streams": 1} if variant == "per_block_streams1" else {}
            harness.evaluate_whole_scene(net, ds, lambda m: torchattacks.NB_attack(m, eps=eps, alpha=alpha, iters=a.iters),
                                         batch_size=a.batch_size, log=quiet, **kw)
        torch.cuda.synchronize()
        return n_blocks / (time.perf_counter() - t0)

    all_variants = VARIANTS if a.field == "color" else FIELD_VARIANTS
    if a.only and a.only not in all_variants:
        ap.error("--only %s does not exist under --field %s" % (a.only, a.field))
    variants = [a.only] if a.only else list(all_variants)
    for v in variants:                          # warm-up: workspaces, packed weights, replicas' first launches
        call(v)
    rate = {v: [] for v in variants}
    for _ in range(a.runs):
        for v in variants:
            rate[v].append(call(v))
    med = {v: statistics.median(r) for v, r in rate.items()}
    out = dict(tool="scene_time", device=torch.cuda.get_device_name(0), n_points=a.points, size=list(a.size), block_points=a.block_points,
               n_blocks=n_blocks, batch_size=a.batch_size, eps=eps, alpha=alpha, iters=a.iters, runs=a.runs, field=a.field,
               occurrences=dict(mean=float(counts.mean()), max=int(counts.max()), multi_share=float((counts > 1).mean())),
               blocks_per_s={v: dict(median=med[v], min=min(r), max=max(r), spread=(max(r) - min(r)) / med[v]) for v, r in rate.items()})
    if not a.only and a.field != "color":
        out["consistent_field_over"] = {v: med["consistent_field"] / med[v] for v in variants if v != "consistent_field"}
    elif not a.only:
        out["consistent_over_per_block"] = dict(streams1=med["consistent"] / med["per_block_streams1"],
                                                default=med["consistent"] / med["per_block_default"])
    if a.kernel_trace:
        out["kernel_trace"] = scene_kernel_share(a.kernel_trace)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
