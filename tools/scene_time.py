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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--size", type=float, nargs=2, default=(6.0, 5.0))
    ap.add_argument("--block-points", type=int, default=4096)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--field", choices=("color", "coord", "both"), default="color")
    ap.add_argument("--only", choices=sorted(set(VARIANTS + FIELD_VARIANTS)), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
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
