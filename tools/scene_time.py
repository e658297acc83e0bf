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

--slicer host | device picks the block slicer of every evaluation call above: the numpy loop of
ScannetDatasetWholeScene.__getitem__ (default) or device_item; --slicer both (--attack nb) runs every variant with either,
`variant@host` and `variant@device` alternated in the same rounds, and reports device over host per variant and whether the
two ranges overlap.  --slicing-only times the slicing alone instead: one slicing of
the room per variant - `host` = ds[0] plus the float32 / int32 casts and the uploads the loops make of it, `device` =
ds.device_item(0) -, alternated in one process after a warm-up of each, np.random.seed(3) before every call, each call from the
seed to a device synchronise; median / min / max in ms, whether the two ranges overlap, and the device slicing's shares: the
host plan (harness.slice_plan on the room's counts, timed alone), the read-back of the counts (from the launch of the count
pass to the counts on the host) and the three passes' kernels (HIP events, in a run of their own).
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


def main_slicing(a):
    """--slicing-only: one slicing of the room per variant, host against device (see the module docstring)"""
    import torch
    from pointsecguard_amd import harness
    from pointsecguard_amd.models.pointnet2_sem_seg import upload
    assert torch.cuda.is_available(), "scene_time.py measures on the MI355X; there is nothing to time without it"
    dev = torch.device("cuda")
    room = synthetic_room(a.points, a.size[0], a.size[1])
    ds = harness.ScannetDatasetWholeScene(None, block_points=a.block_points, scenes={"Area_5_room.npy": room})
    shape = {}

    def call(variant):
        np.random.seed(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if variant == "device":
            out = ds.device_item(0)
        else:                                       # what evaluate_whole_scene_consistent does with the host slicer's arrays
            data, label, smpw, index = ds[0]
            out = (upload(torch.from_numpy(data.astype(np.float32)), dev, pin=True),
                   upload(torch.from_numpy(label.astype(np.int32)), dev, pin=True),
                   upload(torch.from_numpy(smpw.astype(np.float32)), dev, pin=True),
                   upload(torch.from_numpy(index.astype(np.int32)), dev, pin=True))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        shape[variant] = tuple(out[0].shape)
        return dt * 1e3

    variants = ("host", "device")
    for v in variants:
        call(v)
    ms = {v: [] for v in variants}
    for _ in range(a.runs):
        for v in variants:
            ms[v].append(call(v))
    assert shape["host"] == shape["device"]
    stat = {v: dict(median=statistics.median(r), min=min(r), max=max(r)) for v, r in ms.items()}
    overlap = not (stat["device"]["max"] < stat["host"]["min"] or stat["host"]["max"] < stat["device"]["min"])
    out = dict(tool="scene_time", leg="slicing_only", device=torch.cuda.get_device_name(0), n_points=a.points, size=list(a.size),
               block_points=a.block_points, n_blocks=shape["device"][0], runs=a.runs, ms=stat, ranges_overlap=overlap,
               host_over_device=stat["host"]["median"] / stat["device"]["median"], device_shares=slicing_shares(ds, a.runs))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def slicing_shares(ds, runs):
    """where a device slicing's time goes, each part timed in a run of its own: the host plan, the count pass up to the counts on
    the host, and the kernels of the three passes by HIP events (medians, ms)"""
    import torch
    from pointsecguard_amd import _lib, harness, runtime
    dev = torch.device("cuda")
    scene, labels, weights = ds._device_scene(0, dev)
    points = ds.scene_points_list[0]
    n, bp = scene.shape[0], ds.block_points
    cmin, cmax = np.amin(points, axis=0)[:3], np.amax(points, axis=0)[:3]
    windows, centres, _, _ = harness.slice_cells(cmin, cmax, ds.block_size, ds.stride, ds.padding)
    n_cells = windows.shape[0]
    items = n_cells * (-(-n // _lib.SLICE_TILE)) + 1
    win = torch.from_numpy(windows).to(dev)
    cen = torch.from_numpy(centres).to(dev)
    tile_off = torch.empty(items, dtype=torch.int32, device=dev)
    counts_dev = torch.empty(n_cells, dtype=torch.int32, device=dev)
    cell_off = torch.empty(n_cells + 1, dtype=torch.int32, device=dev)
    rgb = runtime.ptr(scene[:, 3:])

    def count():
        _lib.call("psg_slice_count", runtime.ptr(scene), 6, n, runtime.ptr(win), n_cells, runtime.ptr(tile_off), items,
                  runtime.ptr(counts_dev), runtime.ptr(cell_off), runtime.stream())

    count()
    counts = counts_dev.cpu().numpy()
    total = int(counts.sum())
    np.random.seed(3)
    src_pos, _, nb = harness.slice_plan(counts, bp)
    inside = torch.empty(total, dtype=torch.int32, device=dev)
    src = torch.from_numpy(src_pos).to(dev)
    block_cell = torch.from_numpy(np.repeat(np.arange(n_cells, dtype=np.int32), -(-counts.astype(np.int64) // bp))).to(dev)
    data = torch.empty(nb, bp, 9, dtype=torch.float32, device=dev)
    label = torch.empty(nb, bp, dtype=torch.int32, device=dev)
    smpw = torch.empty(nb, bp, dtype=torch.float32, device=dev)
    index = torch.empty(nb, bp, dtype=torch.int32, device=dev)

    def members():
        _lib.call("psg_slice_members", runtime.ptr(scene), 6, n, runtime.ptr(win), n_cells, runtime.ptr(tile_off), items,
                  runtime.ptr(inside), total, runtime.stream())

    def gather():
        _lib.call("psg_slice_gather", runtime.ptr(scene), 6, rgb, 6, runtime.ptr(labels), n, runtime.ptr(inside), total,
                  runtime.ptr(cell_off), runtime.ptr(block_cell), runtime.ptr(cen), n_cells, runtime.ptr(src), nb, bp, float(cmax[0]),
                  float(cmax[1]), float(cmax[2]), runtime.ptr(weights), runtime.ptr(data), runtime.ptr(label), runtime.ptr(smpw),
                  runtime.ptr(index), runtime.stream())

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    plan_ms, readback_ms, kern = [], [], dict(count=[], members=[], gather=[])
    for _ in range(max(runs, 3)):
        np.random.seed(3)
        t0 = time.perf_counter()
        harness.slice_plan(counts, bp)
        plan_ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count()
        counts_dev.cpu()
        readback_ms.append((time.perf_counter() - t0) * 1e3)
        for name, fn in (("count", count), ("members", members), ("gather", gather)):
            kern[name].append(events(fn))
    med = statistics.median
    return dict(n_cells=n_cells, members=total, host_plan_ms=med(plan_ms), count_and_readback_ms=med(readback_ms),
                kernels_ms={k: med(v) for k, v in kern.items()})


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
    ap.add_argument("--slicer", choices=("host", "device", "both"), default="host")
    ap.add_argument("--slicing-only", action="store_true")
    a = ap.parse_args()
    if a.slicing_only:
        return main_slicing(a)
    if a.attack == "nu":
        if a.slicer != "host":
            ap.error("--attack nu slices the room once, outside the timed calls: --slicer does not apply")
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
        variant, _, slicer = variant.partition("@")
        slicer = slicer or a.slicer
        np.random.seed(3)
        torch.manual_seed(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if variant == "consistent":
            harness.evaluate_whole_scene_consistent(net, ds, lambda m: SceneNBAttack(m, eps, alpha, a.iters),
                                                    batch_size=a.batch_size, log=quiet, slicer=slicer)
        elif variant == "consistent_field":
            harness.evaluate_whole_scene_consistent(net, ds, lambda m: SceneNBAttack(m, eps, alpha, a.iters, field=a.field),
                                                    batch_size=a.batch_size, log=quiet, slicer=slicer)
        elif variant.startswith("per_block_field"):
            kw = {"streams": 1} if variant == "per_block_field_streams1" else {}
            harness.evaluate_whole_scene(net, ds, lambda m: torchattacks.NB_attack(m, eps=eps, alpha=alpha, iters=a.iters,
                                                                                     field=a.field),
                                         batch_size=a.batch_size, log=quiet, slicer=slicer, **kw)
        else:
            kw = {"streams": 1} if variant == "per_block_streams1" else {}
            harness.evaluate_whole_scene(net, ds, lambda m: torchattacks.NB_attack(m, eps=eps, alpha=alpha, iters=a.iters),
                                         batch_size=a.batch_size, log=quiet, slicer=slicer, **kw)
        torch.cuda.synchronize()
        return n_blocks / (time.perf_counter() - t0)

    all_variants = VARIANTS if a.field == "color" else FIELD_VARIANTS
    if a.only and a.only not in all_variants:
        ap.error("--only %s does not exist under --field %s" % (a.only, a.field))
    variants = [a.only] if a.only else list(all_variants)
    if a.slicer == "both":
        variants = ["%s@%s" % (v, sl) for v in variants for sl in ("host", "device")]
    for v in variants:                          # warm-up: workspaces, packed weights, replicas' first launches
        call(v)
    rate = {v: [] for v in variants}
    for _ in range(a.runs):
        for v in variants:
            rate[v].append(call(v))
    med = {v: statistics.median(r) for v, r in rate.items()}
    out = dict(tool="scene_time", device=torch.cuda.get_device_name(0), n_points=a.points, size=list(a.size), block_points=a.block_points,
               n_blocks=n_blocks, batch_size=a.batch_size, eps=eps, alpha=alpha, iters=a.iters, runs=a.runs, field=a.field,
               slicer=a.slicer,
               occurrences=dict(mean=float(counts.mean()), max=int(counts.max()), multi_share=float((counts > 1).mean())),
               blocks_per_s={v: dict(median=med[v], min=min(r), max=max(r), spread=(max(r) - min(r)) / med[v]) for v, r in rate.items()})
    if a.slicer == "both":
        out["device_over_host"] = {
            v[:-5]: dict(ratio=med[v[:-5] + "@device"] / med[v],
                         ranges_overlap=not (max(rate[v]) < min(rate[v[:-5] + "@device"]) or max(rate[v[:-5] + "@device"]) < min(rate[v])))
            for v in variants if v.endswith("@host")}
    elif not a.only and a.field != "color":
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
