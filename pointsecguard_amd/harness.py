"""Whole-scene evaluation harness on the device.

Mirrors, relative to /root/reference/PointNet:
  data_utils/S3DISDataLoader.py:81-178      ScannetDatasetWholeScene  (host-side block slicing: numpy, like the reference;
                                            device_item / slicer="device": the same blocks cut on the device)
  NB_nontarget_test_semseg.py:55-62         add_vote                  (device: psg_vote_add)
  NB_nontarget_test_semseg.py:126-291       the per-scene loop: clean / adversarial predictions of every block batch,
                                            vote pools, per-batch TSV log rows, per-scene and total IoU / accuracy
What moves to the GPU is everything the reference does per point on the host: the add_vote double loop
(4096 x B Python iterations per batch), the arg-max / per-class counters and the L2 distance; only 13-entry
counter vectors and one scalar per batch come back.  Scenes are the sharding unit across GPUs (the vote pool
of a scene never leaves its rank); the counters are all-reduced once at the end.
"""
import math
import os

import numpy as np
import torch

from . import _lib, runtime
from .models.pointnet2_sem_seg import upload
from .sharding import reduce_counters, shard_scenes

NUM_CLASSES = runtime.NUM_CLASSES
CLASSES = ['ceiling', 'floor', 'wall', 'beam', 'column', 'window', 'door', 'table', 'chair', 'sofa', 'bookcase',
           'board', 'clutter']   # NB_nontarget_test_semseg.py:35
LOG_HEADER = "index\tL2_dis\tadv_acc\tacc\tadv_miou\tmiou\n"            # :110
LOG_ROW = "%d\t%.3f\t%.5f\t%.5f\t%.5f\t\t%.5f\n"                         # :213-215
TARGETED_LOG_HEADER = "ori\tindex\tL2_dis\tcount\t target acc\tadv_acc\tacc\tadv_miou\tmiou\n"      # NB_target_test_semseg.py:93
TARGETED_LOG_ROW = "%d\t%d\t%.3f\t%d\t%.5f\t%.5f\t%.5f\t%.5f\t\t%.5f\n"                          # :226-229


SLICERS = ("host", "device")


def check_slicer(slicer):
    if slicer not in SLICERS:
        raise ValueError("slicer must be one of %s, got %r" % (SLICERS, slicer))
    return slicer


def slice_plan(counts, block_points):
    """The random part of ScannetDatasetWholeScene.__getitem__ from the cells' member counts alone.

    counts: the number of points in every grid cell, in the slicer's cell order (iy outer, ix inner), empty cells included.
    Per non-empty cell, in that order, numpy's GLOBAL generator is consumed exactly as the slicer consumes it - the padding
    draw np.random.choice(cnt, extra, replace=extra > cnt) (also when extra == 0), then one permutation of the padded
    length - because both draws depend on the cell's count only, not on which points its members are; an empty cell draws
    nothing.  Returns (src_pos, first_block, nb): src_pos int32 [nb * block_points] = for every output slot its position in
    its cell's member list (np.where's ascending order), first_block int32 [n_cells] = the first block of every cell (a
    cell of cnt members fills ceil(cnt / block_points) blocks; an empty cell none), nb = the number of blocks.  A scene
    without a non-empty cell raises ValueError (the host slicer raises too, on its empty vstack)."""
    counts = np.asarray(counts).astype(np.int64).reshape(-1)
    bp = int(block_points)
    if bp < 1 or (counts < 0).any():
        raise ValueError("slice_plan: block_points=%d and the counts must not be negative" % bp)
    blocks = -(-counts // bp)
    first_block = np.concatenate(([0], np.cumsum(blocks)[:-1])) if counts.size else np.zeros(0, np.int64)
    nb = int(blocks.sum())
    if nb == 0:
        raise ValueError("slice_plan: no grid cell holds a point (need at least one array to concatenate)")
    src_pos = np.empty(nb * bp, dtype=np.int32)
    for c in np.flatnonzero(counts):
        cnt, total = int(counts[c]), int(blocks[c]) * bp
        extra = total - cnt
        fill = np.random.choice(cnt, extra, replace=extra > cnt)
        perm = np.random.permutation(total)
        lo = int(first_block[c]) * bp
        src_pos[lo:lo + total] = np.concatenate((np.arange(cnt), fill))[perm]
    return src_pos, first_block.astype(np.int32), nb


def slice_cells(cmin, cmax, block_size, stride, padding):
    """The grid of ScannetDatasetWholeScene.__getitem__ from a scene's corners, with that method's own float64 expressions:
    (windows float64 [n_cells, 4] = {s_x - pad, e_x + pad, s_y - pad, e_y + pad}, centres float64 [n_cells, 2] = {s_x + bs /
    2.0, s_y + bs / 2.0}, grid_x, grid_y), cells in the slicer's order (iy outer, ix inner)."""
    bs, st, pad = block_size, stride, padding
    grid_x = int(np.ceil(float(cmax[0] - cmin[0] - bs) / st) + 1)
    grid_y = int(np.ceil(float(cmax[1] - cmin[1] - bs) / st) + 1)
    windows, centres = [], []
    for iy in range(grid_y):
        for ix in range(grid_x):
            e_x = min(cmin[0] + ix * st + bs, cmax[0])
            s_x = e_x - bs
            e_y = min(cmin[1] + iy * st + bs, cmax[1])
            s_y = e_y - bs
            windows.append((s_x - pad, e_x + pad, s_y - pad, e_y + pad))
            centres.append((s_x + bs / 2.0, s_y + bs / 2.0))
    return (np.array(windows, dtype=np.float64).reshape(-1, 4), np.array(centres, dtype=np.float64).reshape(-1, 2),
            grid_x, grid_y)


class ScannetDatasetWholeScene:
    """Whole rooms cut into overlapping block_size x block_size columns of `block_points` points each
    (S3DISDataLoader.py:81-178).  `root` is a directory of S3DIS-format `Area_<k>_<room>.npy` arrays [n, 7]
    (xyz in metres, rgb 0..255, label); `scenes` (dict name -> array) supplies them directly instead.
    Random padding / shuffling draws come from numpy's global generator in the reference's order, so
    np.random.seed(s) reproduces the reference's blocks."""

    def __init__(self, root, block_points=4096, split='test', test_area=5, stride=0.5, block_size=1.0, padding=0.001,
                 scenes=None):
        assert split in ('train', 'test')
        self.block_points, self.block_size, self.padding = block_points, block_size, padding
        self.root, self.split, self.stride = root, split, stride
        names = list(scenes.keys()) if scenes is not None else os.listdir(root)
        tag = 'Area_%d' % test_area
        self.file_list = [d for d in names if (tag in d) == (split == 'test')]
        self.scene_points_list, self.semantic_labels_list = [], []
        self.room_coord_min, self.room_coord_max, self.scene_points_num = [], [], []
        counts = np.zeros(13)
        for name in self.file_list:
            data = scenes[name] if scenes is not None else np.load(os.path.join(root, name))
            self.scene_points_list.append(data[:, :6])
            self.semantic_labels_list.append(data[:, 6])
            self.room_coord_min.append(np.amin(data[:, :3], axis=0))
            self.room_coord_max.append(np.amax(data[:, :3], axis=0))
            self.scene_points_num.append(data.shape[0])
            counts += np.histogram(data[:, 6], range(14))[0]
        freq = counts.astype(np.float32)
        freq = freq / np.sum(freq)
        self.labelweights = np.power(np.amax(freq) / freq, 1 / 3.0)

    def __len__(self):
        return len(self.scene_points_list)

    def __getitem__(self, index):
        points = self.scene_points_list[index][:, :6]
        labels = self.semantic_labels_list[index]
        cmin, cmax = np.amin(points, axis=0)[:3], np.amax(points, axis=0)[:3]
        bs, st, pad, bp = self.block_size, self.stride, self.padding, self.block_points
        grid_x = int(np.ceil(float(cmax[0] - cmin[0] - bs) / st) + 1)
        grid_y = int(np.ceil(float(cmax[1] - cmin[1] - bs) / st) + 1)
        data_parts, label_parts, weight_parts, index_parts = [], [], [], []
        for iy in range(grid_y):
            for ix in range(grid_x):
                e_x = min(cmin[0] + ix * st + bs, cmax[0])
                s_x = e_x - bs
                e_y = min(cmin[1] + iy * st + bs, cmax[1])
                s_y = e_y - bs
                inside = np.where((points[:, 0] >= s_x - pad) & (points[:, 0] <= e_x + pad) &
                                  (points[:, 1] >= s_y - pad) & (points[:, 1] <= e_y + pad))[0]
                if inside.size == 0:
                    continue
                total = int(np.ceil(inside.size / bp)) * bp
                extra = total - inside.size
                fill = np.random.choice(inside, extra, replace=extra > inside.size)
                idx = np.concatenate((inside, fill))
                np.random.shuffle(idx)
                block = points[idx, :]                      # a copy: the scene itself is never modified
                norm_xyz = block[:, :3] / cmax              # "normalised" location in the room: divided by the max corner
                block[:, 0] = block[:, 0] - (s_x + bs / 2.0)
                block[:, 1] = block[:, 1] - (s_y + bs / 2.0)
                block[:, 3:6] /= 255.0
                lab = labels[idx].astype(int)
                data_parts.append(np.concatenate((block, norm_xyz), axis=1))
                label_parts.append(lab)
                weight_parts.append(self.labelweights[lab])
                index_parts.append(idx)
        data_room = np.vstack(data_parts).reshape((-1, bp, 9))
        label_room = np.hstack(label_parts).reshape((-1, bp))
        # the reference's hstack starts from an empty float64 array, which promotes the float32 class weights
        sample_weight = np.hstack(weight_parts).astype(np.float64).reshape((-1, bp))
        index_room = np.hstack(index_parts).reshape((-1, bp))
        return data_room, label_room, sample_weight, index_room

    def _device_scene(self, index, dev):
        """The scene's float64 [n, 6] array, its int32 labels and the float32 class weights on `dev`: uploaded once and kept
        until another scene (or device) is asked for."""
        cache = getattr(self, "_dev_cache", None)
        if cache is not None and cache[0] == (index, dev):
            return cache[1:]
        self._dev_cache = None
        points = self.scene_points_list[index]
        if points.dtype != np.float64:
            raise ValueError('device_item: the scene is %s, the device slicer computes in float64 only (the host path computes '
                             'in the array\'s own dtype); use slicer="host"' % points.dtype)
        lab = self.semantic_labels_list[index].astype(np.int32)
        if lab.size and (int(lab.min()) < 0 or int(lab.max()) >= NUM_CLASSES):
            raise IndexError("device_item: a label of the scene lies outside [0, %d)" % NUM_CLASSES)
        scene = torch.from_numpy(np.ascontiguousarray(points[:, :6])).to(dev)
        labels = torch.from_numpy(lab).to(dev)
        weights = torch.from_numpy(np.asarray(self.labelweights, dtype=np.float32)).to(dev)
        self._dev_cache = ((index, dev), scene, labels, weights)
        return scene, labels, weights

    def device_item(self, index, device=None, xyz=None):
        """__getitem__(index) cut on the device: device tensors (data float32 [nb, bp, 9], label int32
        [nb, bp], smpw float32 [nb, bp], index int32 [nb, bp]), bit for bit __getitem__'s four arrays after the casts the
        harness applies to them (float32, int32, float32, int32) under the same np.random state, and np.random stands
        afterwards where __getitem__ leaves it: the device counts and lists every cell's members, ONE read-back brings the
        counts, slice_plan draws from them what the reference draws, the device gathers.  Everything else is enqueued on the
        current stream.

        xyz: float64 [n, 3] (numpy or a device tensor) in place of the scene's coordinates - a moved scene, such as
        evaluate_whole_scene_consistent's adv_xyz: corners, grid and windows are those __getitem__ would use on a scene with
        these coordinates (a device tensor costs one more small read-back, for its corners).

        Refusals: a scene that is not float64 (ValueError; slicer="host" computes in the array's own dtype); a grid of more
        than 1024 cells (ValueError; their windows sit in LDS); a label outside [0, 13): IndexError - HERE THE TWO PATHS
        DIFFER: the host path indexes the class weights with the label, so it wraps a negative one."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise _lib.PsgError("device_item slices on the MI355X device (got %s); __getitem__ is the host path" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        scene, labels, weights = self._device_scene(index, dev)
        n = scene.shape[0]
        with torch.cuda.device(dev):
            if xyz is None:
                points = self.scene_points_list[index]
                coords, stride = scene, 6
                cmin, cmax = np.amin(points, axis=0)[:3], np.amax(points, axis=0)[:3]
            else:
                on_host = not isinstance(xyz, torch.Tensor)
                if on_host:
                    xyz = torch.from_numpy(np.ascontiguousarray(xyz))
                if xyz.dtype != torch.float64 or tuple(xyz.shape) != (n, 3):
                    raise ValueError("device_item: xyz must be float64 [%d, 3] (got %s %s)" % (n, xyz.dtype, tuple(xyz.shape)))
                coords, stride = xyz.to(dev).contiguous(), 3
                if on_host:
                    cmin, cmax = np.amin(xyz.numpy(), axis=0), np.amax(xyz.numpy(), axis=0)
                else:                                   # one small read-back for the corners (min / max are exact anywhere)
                    cmin, cmax = torch.stack([coords.amin(dim=0), coords.amax(dim=0)]).cpu().numpy()
            bp = self.block_points
            windows, centres, grid_x, grid_y = slice_cells(cmin, cmax, self.block_size, self.stride, self.padding)
            n_cells = windows.shape[0]
            if n_cells > _lib.SLICE_MAX_CELLS:
                raise ValueError('device_item: the grid has %d x %d = %d cells, the device slicer holds %d (their windows sit in '
                                 'LDS); use slicer="host"' % (grid_x, grid_y, n_cells, _lib.SLICE_MAX_CELLS))
            if n_cells < 1:
                raise ValueError("device_item: the scene's grid has no cell (need at least one array to concatenate)")
            st = runtime.stream()
            tile_items = n_cells * ((n + _lib.SLICE_TILE - 1) // _lib.SLICE_TILE) + 1
            win_dev = torch.from_numpy(windows).to(dev)
            tile_off = torch.empty(tile_items, dtype=torch.int32, device=dev)
            counts_dev = torch.empty(n_cells, dtype=torch.int32, device=dev)
            cell_off = torch.empty(n_cells + 1, dtype=torch.int32, device=dev)
            _lib.call("psg_slice_count", runtime.ptr(coords), stride, n, runtime.ptr(win_dev), n_cells, runtime.ptr(tile_off),
                      tile_items, runtime.ptr(counts_dev), runtime.ptr(cell_off), st)
            counts = counts_dev.cpu().numpy()                      # the one read-back: the host cannot draw the plan without it
            blocks = -(-counts.astype(np.int64) // bp)
            total = int(counts.astype(np.int64).sum())
            if total > 0x7FFFFFFF or int(blocks.sum()) * bp > 0x7FFFFFFF // 9:
                raise ValueError('device_item: %d cell members in %d blocks exceed the device slicer\'s 32-bit offsets; use '
                                 'slicer="host"' % (total, int(blocks.sum())))
            src_pos, _, nb = slice_plan(counts, bp)
            block_cell = np.repeat(np.arange(n_cells, dtype=np.int32), blocks)
            inside = torch.empty(total, dtype=torch.int32, device=dev)
            _lib.call("psg_slice_members", runtime.ptr(coords), stride, n, runtime.ptr(win_dev), n_cells, runtime.ptr(tile_off),
                      tile_items, runtime.ptr(inside), total, st)
            src_dev = upload(torch.from_numpy(src_pos), dev, pin=True)
            cell_dev = upload(torch.from_numpy(block_cell), dev, pin=True)
            cen_dev = upload(torch.from_numpy(centres), dev, pin=True)
            data = torch.empty(nb, bp, 9, dtype=torch.float32, device=dev)
            label = torch.empty(nb, bp, dtype=torch.int32, device=dev)
            smpw = torch.empty(nb, bp, dtype=torch.float32, device=dev)
            idx = torch.empty(nb, bp, dtype=torch.int32, device=dev)
            _lib.call("psg_slice_gather", runtime.ptr(coords), stride, runtime.ptr(scene[:, 3:]), 6, runtime.ptr(labels), n,
                      runtime.ptr(inside), total, runtime.ptr(cell_off), runtime.ptr(cell_dev), runtime.ptr(cen_dev), n_cells,
                      runtime.ptr(src_dev), nb, bp, float(cmax[0]), float(cmax[1]), float(cmax[2]), runtime.ptr(weights),
                      runtime.ptr(data), runtime.ptr(label), runtime.ptr(smpw), runtime.ptr(idx), st)
        return data, label, smpw, idx


def _cuda(t, name, dtype):
    return runtime.require_cuda(t, name, dtype)


def add_vote(vote_label_pool, point_idx, pred_label, weight, bad=None):
    """vote_label_pool[point_idx[b, n], pred_label[b, n]] += 1 where weight[b, n] != 0
    (NB_nontarget_test_semseg.py:55-62), on the device.  vote_label_pool int32 [n_points, 13]; point_idx int32
    [B, N]; weight float32 [B, N] or None; pred_label int32 [B, N], or the [B, N, 13] log-probs themselves (the
    arg-max, first index on ties, is then taken in the same kernel).  Returns vote_label_pool.  An index or label out of
    range raises IndexError - at once, or, when the caller passes its own device counter `bad` (int32 [1], zeroed), when the
    caller checks it with check_votes(bad): the loop over a scene's batches then runs without a host synchronisation."""
    _cuda(vote_label_pool, "vote_label_pool", torch.int32)
    _cuda(point_idx, "point_idx", torch.int32)
    if weight is not None:
        _cuda(weight, "weight", torch.float32)
    logp = pred = None
    if pred_label.dtype == torch.float32:
        logp = _cuda(pred_label, "pred_label", torch.float32)
        assert logp.shape[-1] == vote_label_pool.shape[1]
    else:
        pred = _cuda(pred_label, "pred_label", torch.int32)
    rows = point_idx.numel()
    deferred = bad is not None
    if not deferred:
        bad = torch.zeros(1, dtype=torch.int32, device=vote_label_pool.device)
    _lib.call("psg_vote_add", runtime.ptr(logp), runtime.ptr(pred), runtime.ptr(point_idx), runtime.ptr(weight), rows,
              vote_label_pool.shape[1], vote_label_pool.shape[0], runtime.ptr(vote_label_pool), runtime.ptr(bad),
              runtime.stream())
    if not deferred:
        check_votes(bad)
    return vote_label_pool


def check_votes(bad):
    if int(bad.item()):
        raise IndexError("add_vote: a point index or a label is out of range")


def vote_stats(vote_label_pool, labels, counters=None, want_pred=False):
    """Scene counters of :219-229: pred = argmax of the votes; returns int64 [3, 13] = seen, correct, union
    (accumulated into `counters` when given) and, optionally, the predicted labels."""
    _cuda(vote_label_pool, "vote_label_pool", torch.int32)
    _cuda(labels, "labels", torch.int32)
    if counters is None:
        counters = torch.zeros(3, vote_label_pool.shape[1], dtype=torch.int64, device=labels.device)
    pred = torch.empty(labels.numel(), dtype=torch.int32, device=labels.device) if want_pred else None
    _lib.call("psg_vote_stats", runtime.ptr(vote_label_pool), runtime.ptr(labels), labels.numel(),
              vote_label_pool.shape[1], runtime.ptr(counters), runtime.ptr(pred), runtime.stream())
    return (counters, pred) if want_pred else counters


def l2_distance(a, b):
    """torch.dist(a, b) of :184 as a device scalar (float32 tensor of one element)."""
    _cuda(a, "a", torch.float32)
    _cuda(b, "b", torch.float32)
    assert a.numel() == b.numel()
    scratch = torch.empty(256, dtype=torch.float64, device=a.device)
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    _lib.call("psg_l2_dist", runtime.ptr(a.contiguous()), runtime.ptr(b.contiguous()), a.numel(), runtime.ptr(scratch),
              runtime.ptr(out), runtime.stream())
    return out


def _miou(counters):
    c = counters.to(torch.float64).cpu().numpy()
    iou = c[1] / (c[2] + 1e-6)
    present = c[0] != 0
    return float(np.mean(iou[present])) if present.any() else 0.0


def _replica(classifier):
    """A second instance of the same network on the same device (own packed weights, workspaces and attack state): what lets
    batches of a scene run side by side on separate streams - one model instance serves one stream at a time."""
    with torch.random.fork_rng(devices=[]):          # (the constructor's weight init draws from the CPU generator: the
        rep = type(classifier)(NUM_CLASSES)          # FPS starts of the run must not depend on how many replicas exist)
    rep.load_state_dict(classifier.state_dict())
    return rep.to(next(classifier.parameters()).device).eval()


def evaluate_whole_scene(classifier, dataset, make_attack, batch_size=8, num_votes=1, log_path=None, rank=0, world=1,
                         log=print, targeted=None, streams=3, slicer="host"):
    """The reference's evaluation loop (NB_nontarget_test_semseg.py:126-291) with the per-point work on the GPU.

    classifier: an eval-mode `get_model` on the GPU; make_attack(classifier) -> a torchattacks attack object (e.g.
    lambda m: torchattacks.NB_attack(m, eps=0.1, alpha=0.05, iters=10), :169), or None for the clean evaluation of
    PointNet/test_semseg.py (the "adversarial" columns then repeat the clean ones); dataset: ScannetDatasetWholeScene.
    Scenes are dealt round-robin to ranks; the int64 counters are summed over ranks at the end.  Returns a dict with
    the totals the reference prints (:272-291) and per-scene mIoUs; TSV rows go to `log_path` (rank-suffixed when
    world > 1) in the reference's format.

    targeted = dict(origin=o, target=t) selects the protocol of the targeted scripts (NB_target_test_semseg.py:157-229,
    NU_target_test_semseg.py): per batch mask = (labels == origin), no attack when the batch holds no such point, the
    attack is built per batch as make_attack(classifier, target, mask[0]) (the reference passes the FIRST block's mask,
    :177), and the TSV rows carry origin, count and the target accuracy over the masked points (:226-229); rows are only
    written for attacked batches.

    streams (round 5): the batches of a scene are independent (the vote pools take commutative integer adds, the rows are
    written in batch order at the end of the scene), so batch i runs on HIP stream i % streams with its own replica of the
    network; the host still issues the batches - and draws their FPS starts from the CPU generator - in the reference's
    order, so the results are those of streams = 1 (tests/test_gpu_harness.py).  The host-side block slicing of the NEXT scene
    (`dataset[si]`: ~60 ms of numpy per 70-block scene, as much as the GPU needs for the scene's attacks) runs on a helper
    thread meanwhile - for this module's own ScannetDatasetWholeScene only, whose `__getitem__` touches nothing but
    numpy's generator: the slicing calls still happen one after the other in the reference's order (scene by scene, vote by
    vote), so `np.random` is consumed exactly as before; a caller's dataset class is sliced in line.  While the helper
    thread runs, `make_attack` / the attack must not draw from numpy's GLOBAL generator (the attacks of this package use torch's
    generators only); replicas that cannot be built (another constructor signature) fall back to one stream with a log line.

    slicer="device" (DESIGN.md section 5zb): `dataset.device_item(si, dev)` in the place and order of `dataset[si]` - the same
    blocks bit for bit and the same np.random draws, so the generator order above holds and the results are those of
    slicer="host"; no helper thread (nothing is left to hide), the batches take slices of the device tensors instead of
    uploading numpy slices, and the targeted protocol's masks and counts come from one read-back of the scene's block labels
    per slicing.  A dataset class without device_item is a TypeError."""
    _check_device_slicer(slicer, dataset)
    dev = next(classifier.parameters()).device
    n_streams = max(1, int(streams))
    nets = [classifier]
    try:
        nets += [_replica(classifier) for _ in range(n_streams - 1)]
    except Exception as exc:          # a caller's model class with another constructor, or state outside state_dict (advisor, round 5)
        log("evaluate_whole_scene: no replica of %s (%s: %s); running on one stream" % (type(classifier).__name__, type(exc).__name__, exc))
        nets, n_streams = [classifier], 1
    lanes = [torch.cuda.Stream(device=dev) for _ in range(n_streams)] if n_streams > 1 else [None]
    attacks = [make_attack(n) if (make_attack is not None and targeted is None) else None for n in nets]
    n_pt = dataset.block_points
    total = torch.zeros(2, 3, NUM_CLASSES, dtype=torch.int64, device=dev)   # [clean | adversarial][seen, correct, union]
    scene_rows = []
    fh = None
    if log_path is not None:
        path = log_path if world == 1 else "%s.rank%d" % (log_path, rank)
        fh = open(path, "w")
        fh.write(LOG_HEADER if targeted is None else TARGETED_LOG_HEADER)
    my_scenes = shard_scenes(list(range(len(dataset))), rank, world)
    fetch_order = [si for si in my_scenes for _ in range(num_votes)]
    fetcher = None
    if slicer == "host" and type(dataset) is ScannetDatasetWholeScene and len(fetch_order) > 1:
        from concurrent.futures import ThreadPoolExecutor
        fetcher = ThreadPoolExecutor(max_workers=1)
    n_fetched = [0]
    nxt = [fetcher.submit(dataset.__getitem__, fetch_order[0])] if fetcher else [None]

    def next_scene_data(si):
        k = n_fetched[0]
        n_fetched[0] += 1
        if slicer == "device":
            return _device_scene_data(dataset, si, dev, lanes, targeted is not None)
        if fetcher is None:
            return dataset[si] + (None,)
        data = nxt[0].result()
        nxt[0] = fetcher.submit(dataset.__getitem__, fetch_order[k + 1]) if k + 1 < len(fetch_order) else None
        return data + (None,)

    try:
      for si in my_scenes:
          labels_np = dataset.semantic_labels_list[si]
          n_scene = labels_np.shape[0]
          scene_labels = torch.from_numpy(labels_np.astype(np.int32)).to(dev)
          pool = torch.zeros(n_scene, NUM_CLASSES, dtype=torch.int32, device=dev)
          adv_pool = torch.zeros_like(pool)
          pending = []                                 # rows of this scene's log: device scalars, read back once per scene
          vote_bad = torch.zeros(1, dtype=torch.int32, device=dev)
          for ln in lanes:                             # the scene's pools were zeroed on the caller's stream
              if ln is not None:
                  ln.wait_stream(torch.cuda.current_stream(dev))
          n_issued = 0
          for _ in range(num_votes):
              scene_data, scene_label, scene_smpw, scene_point_index, label_host = next_scene_data(si)
              num_blocks = scene_data.shape[0]
              for sbatch in range((num_blocks + batch_size - 1) // batch_size):
                  lo, hi = sbatch * batch_size, min((sbatch + 1) * batch_size, num_blocks)
                  slot = n_issued % n_streams
                  n_issued += 1
                  pending.extend(_scene_batch(nets[slot], attacks[slot], make_attack, targeted, lanes[slot], dev, n_pt, sbatch, lo, hi,
                                              scene_data, scene_label, scene_smpw, scene_point_index, pool, adv_pool, vote_bad,
                                              label_host))
          for ln in lanes:
              if ln is not None:
                  torch.cuda.current_stream(dev).wait_stream(ln)
          check_votes(vote_bad)
          _write_rows(pending, targeted, fh)
          c_scene = vote_stats(pool, scene_labels)
          c_scene_adv = vote_stats(adv_pool, scene_labels)
          total[0] += c_scene
          total[1] += c_scene_adv
          name = dataset.file_list[si][:-4]
          scene_rows.append((name, _miou(c_scene), _miou(c_scene_adv)))
          log('Mean IoU of %s: %.4f' % (name, scene_rows[-1][1]))
          log('Mean IoU of %s: %.4f' % (name, scene_rows[-1][2]))
    finally:
        # (also when a batch raises: the helper thread and its pending slice must not outlive the call)
        if fh is not None:
            fh.close()
        if fetcher is not None:
            fetcher.shutdown(wait=True, cancel_futures=True)
    return _finish(total, scene_rows, rank, log)


def _check_device_slicer(slicer, dataset):
    if check_slicer(slicer) == "device" and not hasattr(dataset, "device_item"):
        raise TypeError('slicer="device" needs a dataset with device_item (ScannetDatasetWholeScene); %s has none'
                        % type(dataset).__name__)


def _device_scene_data(dataset, si, dev, lanes, want_host_labels):
    """One device slicing for evaluate_whole_scene: the four device tensors and - for the targeted protocol - the block labels
    on the host (one read-back per slicing).  The tensors are produced on the caller's stream and consumed on the lanes: the
    caller's stream first waits for the lanes (the previous slicing's tensors are released here and their memory may be
    handed out again at once), the lanes then wait for the slicing."""
    cur = torch.cuda.current_stream(dev)
    for ln in lanes:
        if ln is not None:
            cur.wait_stream(ln)
    data, label, smpw, index = dataset.device_item(si, dev)
    label_host = label.cpu().numpy() if want_host_labels else None
    for ln in lanes:
        if ln is not None:
            ln.wait_stream(cur)
    return data, label, smpw, index, label_host


def _scene_batch(classifier, attack, make_attack, targeted, lane, dev, n_pt, sbatch, lo, hi, scene_data, scene_label, scene_smpw,
                 scene_point_index, pool, adv_pool, vote_bad, label_host=None):
    """One batch of a scene on `lane` (a HIP stream, or None = the caller's): clean forward, attack, adversarial forward,
    votes, counters, L2 - everything stays on the device; returns the batch's pending log row (or nothing).  The scene's four
    arrays are the host slicer's numpy arrays, or the device slicer's tensors (label_host: their labels on the host, for the
    targeted protocol)."""
    import contextlib
    with (torch.cuda.stream(lane) if lane is not None else contextlib.nullcontext()):
        if isinstance(scene_data, torch.Tensor):
            torch_data = scene_data[lo:hi].transpose(2, 1).contiguous()
            gt, idx, smpw = scene_label[lo:hi], scene_point_index[lo:hi], scene_smpw[lo:hi]
            gt_np = label_host[lo:hi] if label_host is not None else gt
        else:
            # (numpy does the float64 -> float32 conversion: a torch CPU op of this size wakes the whole OpenMP pool)
            torch_data = upload(torch.from_numpy(scene_data[lo:hi].astype(np.float32)), dev, pin=True).transpose(2, 1).contiguous()
            gt_np = scene_label[lo:hi]
            gt = upload(torch.from_numpy(gt_np.astype(np.int32)), dev, pin=True)
            idx = upload(torch.from_numpy(scene_point_index[lo:hi].astype(np.int32)), dev, pin=True)
            smpw = upload(torch.from_numpy(scene_smpw[lo:hi].astype(np.float32)), dev, pin=True)
        seg_pred, _ = classifier(torch_data)
        seg_pred = seg_pred.detach().contiguous()
        count, mask_np = 0, None
        if targeted is not None:
            mask_np = gt_np == targeted["origin"]
            count = int(mask_np.sum())
            batch_attack = make_attack(classifier, targeted["target"], mask_np[0]) if count else None
        else:
            batch_attack = attack
        if batch_attack is not None:
            adv_images = batch_attack(torch_data, gt_np)
            adv_seg_pred, _ = classifier(adv_images)
            adv_seg_pred = adv_seg_pred.detach().contiguous()
        else:
            adv_images, adv_seg_pred = torch_data, seg_pred
        add_vote(pool, idx, seg_pred, smpw, bad=vote_bad)
        add_vote(adv_pool, idx, adv_seg_pred, smpw, bad=vote_bad)
        c_clean, _ = runtime.seg_stats(seg_pred, gt)
        c_adv, _ = runtime.seg_stats(adv_seg_pred, gt)
        dis = l2_distance(adv_images, torch_data)
        # The batch's TSV row needs five scalars; they stay on the device until the scene is done (ONE read-back per
        # scene instead of four or five host synchronisations per batch: the host slices the next blocks while
        # the GPU attacks these - the rows and their order are what the reference writes, :213-215)
        hits = None
        if targeted is not None and count:
            m = upload(torch.from_numpy(mask_np), dev, pin=True)
            hits = ((adv_seg_pred.argmax(dim=2) == targeted["target"]) & m).sum()
        if targeted is None or count:
            return [(sbatch, (hi - lo) * n_pt, count, dis, c_clean, c_adv, hits)]
    return []


def evaluate_whole_scene_consistent(classifier, dataset, make_scene_attack, batch_size=8, log_path=None, rank=0, world=1,
                                    log=print, targeted=None, on_scene=None, on_scene_field=None, slicer="host"):
    """evaluate_whole_scene with ONE adversarial scene per room: the attack moves one colour per
    physical scene point - attacks.scene.SceneNBAttack - instead of one per block slot, so the adversarial blocks that are
    voted on are slices of a point cloud that exists (and can be saved and re-sliced).

    make_scene_attack(classifier) -> a SceneNBAttack (for the targeted protocol one built with the same origin / target);
    its batch_size is set to this call's.  Per scene of the rank's shard, in this order - which is also the order in which the
    generators are consumed: np.random by the slicing, torch's CPU generator by the FPS starts of every forward -
      1. one slicing (dataset[si]; num_votes is 1, as in the reference's attack scripts);
      2. the clean forwards of all batches, in batch order;
      3. the scene attack (iteration outer, batch inner);
      4. the adversarial forwards of all batches, in batch order.
    Steps 3 and 4 draw, in that order, from a fork of the CPU generator (torch.random.fork_rng) taken after step 2: when the
    scene is done the generator stands where its clean forwards left it.  The clean forwards of EVERY scene therefore draw
    exactly what evaluate_whole_scene(classifier, dataset, None) draws under the same seeds - the clean counters of the two are
    the same numbers -, and a seeded run is reproducible; the price is that a scene's attack and the next scene's clean
    forwards start from the same generator state.
    Votes, counters, the per-batch TSV rows (same header and row format; L2_dis per batch of adversarial against clean
    blocks) and the totals are those of evaluate_whole_scene.  targeted = dict(origin=o, target=t): the ten-column rows,
    written for the batches that hold a point of `origin`; a scene without such a point is evaluated clean and logs no rows.
    on_scene(name, adv_rgb01): called once per scene with the adversarial colours as a float32 numpy array [n_scene, 3] in
    [0, 1] (the clean ones for a scene that was not attacked) - the reference's .xyzrgb dump.  One stream, no replicas.
    on_scene_field(name, adv_rgb01, adv_xyz): the same call with the moved geometry beside the colours, for a scene attack
    built with field="coord" | "both" (DESIGN.md section 5v): adv_xyz = the scene's xyz (float64, metres, [n_scene, 3]) + the
    attack's displacement delta; the clean arrays for a scene that was not attacked or an attack that moves colours only.
    slicer="device" (DESIGN.md section 5zb): step 1 is dataset.device_item(si, dev) - the same blocks and the same np.random
    draws, on the device; the results are those of slicer="host".  A dataset class without device_item is a TypeError."""
    from .attacks.scene import check_scene_model
    _check_device_slicer(slicer, dataset)
    check_scene_model(classifier)
    dev = next(classifier.parameters()).device
    if dev.type != "cuda":
        raise _lib.PsgError("the classifier must be on the MI355X device (got %s); there is no CPU path" % dev)
    attack = make_scene_attack(classifier)
    attack.batch_size = int(batch_size)
    if targeted is not None and (attack.origin != targeted["origin"] or attack.target != targeted["target"]):
        raise ValueError("the scene attack's origin / target differ from the targeted protocol's")
    n_pt = dataset.block_points
    total = torch.zeros(2, 3, NUM_CLASSES, dtype=torch.int64, device=dev)
    scene_rows = []
    fh = None
    if log_path is not None:
        path = log_path if world == 1 else "%s.rank%d" % (log_path, rank)
        fh = open(path, "w")
        fh.write(LOG_HEADER if targeted is None else TARGETED_LOG_HEADER)
    try:
        for si in shard_scenes(list(range(len(dataset))), rank, world):
            labels_np = dataset.semantic_labels_list[si]
            n_scene = labels_np.shape[0]
            scene_labels = torch.from_numpy(labels_np.astype(np.int32)).to(dev)
            pool = torch.zeros(n_scene, NUM_CLASSES, dtype=torch.int32, device=dev)
            adv_pool = torch.zeros_like(pool)
            vote_bad = torch.zeros(1, dtype=torch.int32, device=dev)
            if slicer == "device":
                x_all, gt_all, smpw_all, idx_all = dataset.device_item(si, dev)
                scene_label = gt_all.cpu().numpy() if targeted is not None else None      # (the targeted rows' counts)
            else:
                scene_data, scene_label, scene_smpw, scene_point_index = dataset[si]
                x_all = upload(torch.from_numpy(scene_data.astype(np.float32)), dev, pin=True)            # [nb, bp, 9] point-major
                gt_all = upload(torch.from_numpy(scene_label.astype(np.int32)), dev, pin=True)
                idx_all = upload(torch.from_numpy(scene_point_index.astype(np.int32)), dev, pin=True)
                smpw_all = upload(torch.from_numpy(scene_smpw.astype(np.float32)), dev, pin=True)
            num_blocks = x_all.shape[0]
            batches = [(lo, min(lo + batch_size, num_blocks)) for lo in range(0, num_blocks, batch_size)]
            attacked = targeted is None or bool((labels_np == targeted["origin"]).any())
            clean_stats = []
            for lo, hi in batches:
                torch_data = x_all[lo:hi].transpose(2, 1).contiguous()
                seg_pred, _ = classifier(torch_data)
                seg_pred = seg_pred.detach().contiguous()
                add_vote(pool, idx_all[lo:hi], seg_pred, smpw_all[lo:hi], bad=vote_bad)
                if not attacked:
                    add_vote(adv_pool, idx_all[lo:hi], seg_pred, smpw_all[lo:hi], bad=vote_bad)
                clean_stats.append(runtime.seg_stats(seg_pred, gt_all[lo:hi])[0])
            check_votes(vote_bad)
            pending, adv_rgb = [], None
            rgb_np = dataset.scene_points_list[si][:, 3:6]
            if attacked:
                # steps 3 and 4 draw from a FORK of the CPU generator: afterwards it stands where the clean forwards left it
                with torch.random.fork_rng(devices=[]):
                    adv_rgb, pending = _scene_attack_and_votes(classifier, attack, targeted, batches, n_pt, x_all, idx_all, gt_all,
                                                               smpw_all, scene_label, rgb_np, scene_labels, adv_pool, vote_bad,
                                                               clean_stats)
                check_votes(vote_bad)
            if on_scene is not None:
                on_scene(dataset.file_list[si][:-4],
                         adv_rgb.cpu().numpy() if attacked else (rgb_np / 255.0).astype(np.float32))
            if on_scene_field is not None:
                xyz = np.array(dataset.scene_points_list[si][:, 0:3], dtype=np.float64)
                delta = getattr(attack, "last_delta", None) if attacked else None
                if delta is not None:
                    xyz += delta.cpu().numpy().astype(np.float64)
                on_scene_field(dataset.file_list[si][:-4],
                               adv_rgb.cpu().numpy() if attacked else (rgb_np / 255.0).astype(np.float32), xyz)
            _write_rows(pending, targeted, fh)
            c_scene = vote_stats(pool, scene_labels)
            c_scene_adv = vote_stats(adv_pool, scene_labels)
            total[0] += c_scene
            total[1] += c_scene_adv
            name = dataset.file_list[si][:-4]
            scene_rows.append((name, _miou(c_scene), _miou(c_scene_adv)))
            log('Mean IoU of %s: %.4f' % (name, scene_rows[-1][1]))
            log('Mean IoU of %s: %.4f' % (name, scene_rows[-1][2]))
    finally:
        if fh is not None:
            fh.close()
    return _finish(total, scene_rows, rank, log)


def _scene_attack_and_votes(classifier, attack, targeted, batches, n_pt, x_all, idx_all, gt_all, smpw_all, scene_label, rgb_np,
                            scene_labels, adv_pool, vote_bad, clean_stats):
    """Steps 3 and 4 of evaluate_whole_scene_consistent for one scene: the scene attack, then the adversarial forwards, votes,
    counters and L2 of every batch in batch order; returns (adversarial colours [n_scene, 3], the scene's pending log rows)."""
    adv_rgb, adv_blocks = attack(x_all, idx_all, gt_all, rgb_np, scene_labels)
    pending = []
    for sbatch, (lo, hi) in enumerate(batches):
        adv_data = adv_blocks[lo:hi].transpose(2, 1).contiguous()
        adv_seg_pred, _ = classifier(adv_data)
        adv_seg_pred = adv_seg_pred.detach().contiguous()
        add_vote(adv_pool, idx_all[lo:hi], adv_seg_pred, smpw_all[lo:hi], bad=vote_bad)
        c_adv, _ = runtime.seg_stats(adv_seg_pred, gt_all[lo:hi])
        dis = l2_distance(adv_data, x_all[lo:hi].transpose(2, 1).contiguous())
        count, hits = 0, None
        if targeted is not None:
            count = int((scene_label[lo:hi] == targeted["origin"]).sum())
            hits = ((adv_seg_pred.argmax(dim=2) == targeted["target"]) & (gt_all[lo:hi] == targeted["origin"])).sum()
        if targeted is None or count:
            pending.append((sbatch, (hi - lo) * n_pt, count, dis, clean_stats[sbatch], c_adv, hits))
    return adv_rgb, pending


def _write_rows(pending, targeted, fh):
    """The scene's TSV rows in the order the batches were issued (NB_nontarget_test_semseg.py:213-215): ONE read-back for all."""
    if not pending:
        return
    scal = torch.stack([torch.cat([p[3].double().reshape(1), (p[6] if p[6] is not None else p[3].new_zeros(())).double().reshape(1)])
                        for p in pending]).cpu().numpy()
    ctr = torch.stack([torch.stack([p[4], p[5]]) for p in pending]).cpu()
    for k, (sbatch, rows, count, _, _, _, hits) in enumerate(pending):
        c_clean, c_adv = ctr[k, 0], ctr[k, 1]
        acc = float(c_clean[1].sum().item()) / float(rows)
        adv_acc = float(c_adv[1].sum().item()) / float(rows)
        dis_f = float(np.float32(scal[k, 0]))
        if targeted is None:
            line = LOG_ROW % (sbatch, dis_f, adv_acc, acc, _miou(c_adv), _miou(c_clean))
        else:
            line = TARGETED_LOG_ROW % (targeted["origin"], sbatch, dis_f, count, float(scal[k, 1]) / count, adv_acc, acc,
                                       _miou(c_adv), _miou(c_clean))
        if fh is not None:
            fh.write(line)


def _finish(total, scene_rows, rank, log):
    reduce_counters(total)
    t = total.to(torch.float64).cpu().numpy()
    out = {"scenes": scene_rows, "counters": total.cpu().numpy()}
    for tag, c in (("", t[0]), ("adv_", t[1])):
        seen = t[0][0]                                   # the reference divides the adversarial counters by the clean `seen`
        out[tag + "iou_per_class"] = (c[1] / (c[2] + 1e-6)).tolist()
        out[tag + "miou"] = float(np.mean(c[1] / (c[2] + 1e-6)))                          # :272-273, :282
        out[tag + "avg_class_acc"] = float(np.mean(c[1] / (seen + 1e-6)))                 # :283-284, :288-289
        out[tag + "accuracy"] = float(np.sum(c[1]) / float(np.sum(seen) + 1e-6))          # :285-286, :290-291
    if rank == 0:
        log('------- IoU --------')
        for l in range(NUM_CLASSES):
            denom = t[0][2][l]
            log('class %s, IoU: %.3f ' % (CLASSES[l] + ' ' * (14 - len(CLASSES[l])), t[0][1][l] / denom if denom else math.nan))
        log('eval point avg class IoU: %f' % out["miou"])
        log('eval whole scene point avg class acc: %f' % out["avg_class_acc"])
        log('eval whole scene point accuracy: %f' % out["accuracy"])
        log("-------attack--------")
        log('eval point avg class IoU: %f' % out["adv_miou"])
        log('eval whole scene point avg class acc: %f' % out["adv_avg_class_acc"])
        log('eval whole scene point accuracy: %f' % out["adv_accuracy"])
    return out
