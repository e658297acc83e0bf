"""Whole-scene evaluation harness on the device.

Mirrors, relative to /root/reference/PointNet:
  data_utils/S3DISDataLoader.py:81-178      ScannetDatasetWholeScene  (host-side block slicing: numpy, like the reference)
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
                         log=print, targeted=None, streams=3):
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
    generators only); replicas that cannot be built (another constructor signature) fall back to one stream with a log line."""
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
    if type(dataset) is ScannetDatasetWholeScene and len(fetch_order) > 1:
        from concurrent.futures import ThreadPoolExecutor
        fetcher = ThreadPoolExecutor(max_workers=1)
    n_fetched = [0]
    nxt = [fetcher.submit(dataset.__getitem__, fetch_order[0])] if fetcher else [None]

    def next_scene_data(si):
        k = n_fetched[0]
        n_fetched[0] += 1
        if fetcher is None:
            return dataset[si]
        data = nxt[0].result()
        nxt[0] = fetcher.submit(dataset.__getitem__, fetch_order[k + 1]) if k + 1 < len(fetch_order) else None
        return data

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
              scene_data, scene_label, scene_smpw, scene_point_index = next_scene_data(si)
              num_blocks = scene_data.shape[0]
              for sbatch in range((num_blocks + batch_size - 1) // batch_size):
                  lo, hi = sbatch * batch_size, min((sbatch + 1) * batch_size, num_blocks)
                  slot = n_issued % n_streams
                  n_issued += 1
                  pending.extend(_scene_batch(nets[slot], attacks[slot], make_attack, targeted, lanes[slot], dev, n_pt, sbatch, lo, hi,
                                              scene_data, scene_label, scene_smpw, scene_point_index, pool, adv_pool, vote_bad))
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


def _scene_batch(classifier, attack, make_attack, targeted, lane, dev, n_pt, sbatch, lo, hi, scene_data, scene_label, scene_smpw,
                 scene_point_index, pool, adv_pool, vote_bad):
    """One batch of a scene on `lane` (a HIP stream, or None = the caller's): clean forward, attack, adversarial forward,
    votes, counters, L2 - everything stays on the device; returns the batch's pending log row (or nothing)."""
    import contextlib
    with (torch.cuda.stream(lane) if lane is not None else contextlib.nullcontext()):
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
                                    log=print, targeted=None, on_scene=None, on_scene_field=None):
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
    attack's displacement delta; the clean arrays for a scene that was not attacked or an attack that moves colours only."""
    from .attacks.scene import check_scene_model
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
            scene_data, scene_label, scene_smpw, scene_point_index = dataset[si]
            num_blocks = scene_data.shape[0]
            x_all = upload(torch.from_numpy(scene_data.astype(np.float32)), dev, pin=True)            # [nb, bp, 9] point-major
            gt_all = upload(torch.from_numpy(scene_label.astype(np.int32)), dev, pin=True)
            idx_all = upload(torch.from_numpy(scene_point_index.astype(np.int32)), dev, pin=True)
            smpw_all = upload(torch.from_numpy(scene_smpw.astype(np.float32)), dev, pin=True)
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
