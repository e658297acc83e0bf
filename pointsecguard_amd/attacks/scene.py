"""Whole-scene NB attack: PGD on ONE colour per physical scene point.

The per-block attacks (torchattacks.NB_attack / tar_NB_attack under harness.evaluate_whole_scene) follow the reference: every
batch of blocks is attacked on its own, and since the 1 m x 1 m blocks overlap at stride 0.5 m the same scene point ends up
with a different colour in every block that holds it.  Here the variable is the scene's colour array c [n_scene][3]; every
iteration writes c into all block slots, runs the network's forward / CE gradient / colour backward batch by batch, sums the
block gradients over each point's slots in ascending slot order (fp32, no atomics) and takes one sign step on c.  The
result is a point cloud: one colour per point, bounded by eps once.
"""
import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.models import pointnet2_sem_seg, pointnet2_sem_seg_msg
from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts, upload

NUM_CLASSES = runtime.NUM_CLASSES


def check_scene_model(model):
    """The networks this attack drives: both PointNet++ sem-seg variants (one set of psg_pn2_* entry points)."""
    if not isinstance(model, (pointnet2_sem_seg.get_model, pointnet2_sem_seg_msg.get_model)):
        raise NotImplementedError("the whole-scene attack is implemented for pointnet2_sem_seg and pointnet2_sem_seg_msg "
                                  "(got %s.%s)" % (type(model).__module__, type(model).__name__))
    return model


def _device_array(a, dtype, np_dtype, name, device):
    """numpy -> device (converted by numpy, uploaded through pinned memory); a tensor must already be on the device."""
    if isinstance(a, np.ndarray):
        return upload(torch.from_numpy(np.ascontiguousarray(a.astype(np_dtype))), device, pin=True)
    return runtime.require_cuda(a, name, dtype)


class SceneNBAttack:
    """PGD (sign steps, L-inf ball of radius eps around the clean colours, box [0, 1]) on the colours of a whole scene.

    __call__(blocks, point_idx, block_labels, scene_rgb, scene_labels) -> (adv_rgb01 [n_scene, 3], adv_blocks [nb, bp, 9]),
    both float32 device tensors.  The inputs are one scene as ScannetDatasetWholeScene.__getitem__ returns it: blocks
    [nb][bp][9] (point-major), point_idx [nb][bp], block labels [nb][bp] - numpy arrays, or device tensors (float32 / int32 /
    int32) -, scene_rgb: the scene's colours 0..255 as a numpy array [n_scene][3] (c0 = float32(rgb / 255.0), the bits the
    slicer puts into channels 3:6), scene_labels [n_scene] (read by the targeted attack only).

    Per iteration t: for every batch k of `batch_size` consecutive blocks in slicer order (the last one may be smaller)
    colours of c into the batch's slots, FPS starts from the CPU generator (draw_fps_starts(B_k, bp, 1); t outer, k inner),
    psg_pn2_plan_build, psg_pn2_forward_lean, psg_ce_logp_grad (scale 1 / bp, all rows), psg_pn2_backward_colour into the
    batch's slice of the scene-wide gradient buffer; then psg_scene_pgd_step.  Nothing is read back inside the loop.

    Non-targeted: ascent on the CE to the block labels.  Targeted (target and origin both given): mask = (scene_labels ==
    origin); descent on the CE to `target` summed over the slots of masked points, divided by bp; only masked points move.
    This is deliberately NOT tar_NB_attack's batch quirk (the first block's mask applied to every block of the batch, the CE
    mean of room 0 only): a scene point is masked by its own label wherever it occurs.

    project_last=True (default): the final step is projected like every other, so the returned scene lies in the eps ball and
    in [0, 1].  project_last=False returns the reference's un-projected last step, which makes the attack
    bit-identical to torchattacks.NB_attack on a scene whose blocks do not overlap.

    trace: optional callback, called after every iteration with (t, starts of every batch [list of int32 device tensors],
    dx0 [nb, bp, 9], c before the step, c after it, dlogp [nb, bp, 13]) - device tensors; dx0 is the attack's own buffer."""

    def __init__(self, model, eps, alpha, iters, batch_size=8, target=None, origin=None, project_last=True, trace=None):
        self.model = check_scene_model(model)
        if (target is None) != (origin is None):
            raise ValueError("the targeted scene attack needs both `target` and `origin`")
        if target is not None and not 0 <= int(target) < NUM_CLASSES:
            raise ValueError("target class %r out of range" % (target,))
        if int(iters) < 1 or int(batch_size) < 1:
            raise ValueError("iters and batch_size must be positive")
        self.eps, self.alpha, self.iters, self.batch_size = float(eps), float(alpha), int(iters), int(batch_size)
        self.target, self.origin, self.project_last, self.trace = target, origin, bool(project_last), trace

    def __call__(self, blocks, point_idx, block_labels, scene_rgb, scene_labels):
        net = self.model
        params = next(net.parameters())
        if not params.is_cuda:
            raise _lib.PsgError("the model must be on the MI355X device (got %s); there is no CPU path" % params.device)
        dev = params.device
        x = _device_array(blocks, torch.float32, np.float32, "blocks", dev)
        idx = _device_array(point_idx, torch.int32, np.int32, "point_idx", dev)
        gt = _device_array(block_labels, torch.int32, np.int32, "block_labels", dev)
        if x.dim() != 3 or x.shape[2] != 9 or idx.shape != x.shape[:2] or gt.shape != x.shape[:2]:
            raise ValueError("expected blocks [nb, bp, 9] with point_idx / block_labels [nb, bp], got %s, %s, %s" % (
                tuple(x.shape), tuple(idx.shape), tuple(gt.shape)))
        if not isinstance(scene_rgb, np.ndarray) or scene_rgb.ndim != 2 or scene_rgb.shape[1] != 3:
            raise ValueError("scene_rgb must be a numpy array [n_scene, 3] of colours 0..255")
        nb, bp = x.shape[0], x.shape[1]
        n_scene = scene_rgb.shape[0]
        c0 = upload(torch.from_numpy(np.ascontiguousarray((scene_rgb / 255.0).astype(np.float32))), dev, pin=True)
        targeted = self.target is not None
        mask = None
        if targeted:
            if isinstance(scene_labels, torch.Tensor):
                mask = (runtime.require_cuda(scene_labels, "scene_labels") == int(self.origin)).to(torch.uint8).contiguous()
            else:
                mask = upload(torch.from_numpy((np.asarray(scene_labels) == self.origin).astype(np.uint8)), dev, pin=True)
            if mask.numel() != n_scene:
                raise ValueError("scene_labels must hold %d labels" % n_scene)

        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        occ_off, occ_ent = runtime.scene_occ_build(idx, n_scene, bad)
        if int(bad.item()):        # (the one read-back, before the loop: once per scene)
            raise IndexError("SceneNBAttack: a point index is outside [0, %d)" % n_scene)

        x = x.clone()              # the caller's blocks stay clean
        c = c0.clone()
        dx0_all = torch.zeros(nb, bp, 9, dtype=torch.float32, device=dev)     # backward_colour writes channels 3:6 only
        model = net._packed()
        batches = [(lo, min(lo + self.batch_size, nb)) for lo in range(0, nb, self.batch_size)]
        sizes = sorted({hi - lo for lo, hi in batches})
        ws = {b: net._workspace(b, bp, 1) for b in sizes}
        net._generation += 1       # the workspace activations no longer belong to an earlier autograd forward
        logp = {b: torch.empty(b, bp, NUM_CLASSES, dtype=torch.float32, device=dev) for b in sizes}
        trace = self.trace
        if trace is not None:      # the tests read every batch's dlogp: kept scene-wide only then
            dlogp_all = torch.zeros(nb, bp, NUM_CLASSES, dtype=torch.float32, device=dev)
        else:
            dlogp = {b: torch.empty(b, bp, NUM_CLASSES, dtype=torch.float32, device=dev) for b in sizes}
        direction = -1.0 if targeted else 1.0
        st = runtime.stream
        for t in range(self.iters):
            starts_t = []
            for lo, hi in batches:
                b = hi - lo
                xb, ib, w = x[lo:hi], idx[lo:hi], ws[b]
                runtime.scene_colour_to_blocks(c, ib, xb, bad)
                starts = upload(draw_fps_starts(b, bp, 1, pinned=True), dev, pin=True)
                dl = dlogp_all[lo:hi] if trace is not None else dlogp[b]
                _lib.call("psg_pn2_plan_build", w.handle, runtime.ptr(xb), runtime.ptr(starts), 1, st())
                _lib.call("psg_pn2_forward_lean", model.handle, w.handle, 0, runtime.ptr(xb), runtime.ptr(logp[b]), st())
                _lib.call("psg_ce_logp_grad", runtime.ptr(logp[b]), None if targeted else runtime.ptr(gt[lo:hi]),
                          int(self.target) if targeted else 0, b * bp, b * bp, NUM_CLASSES, 1.0 / bp, runtime.ptr(dl), None, st())
                if targeted:
                    runtime.scene_rows_mask(dl, ib, mask)
                _lib.call("psg_pn2_backward_colour", model.handle, w.handle, 0, runtime.ptr(dl), runtime.ptr(dx0_all[lo:hi]), st())
                if trace is not None:
                    starts_t.append(starts)
            last = t == self.iters - 1 and not self.project_last
            c_before = c.clone() if trace is not None else None
            runtime.scene_pgd_step(c, c0, mask, occ_off, occ_ent, dx0_all, self.alpha, self.eps, direction, last)
            if trace is not None:
                trace(t, starts_t, dx0_all, c_before, c.clone(), dlogp_all)
        runtime.scene_colour_to_blocks(c, idx, x, bad)
        return c, x
