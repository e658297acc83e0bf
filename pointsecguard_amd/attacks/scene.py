"""Whole-scene NB attack: PGD on ONE colour per physical scene point.

The per-block attacks (torchattacks.NB_attack / tar_NB_attack under harness.evaluate_whole_scene) follow the reference: every
batch of blocks is attacked on its own, and since the 1 m x 1 m blocks overlap at stride 0.5 m the same scene point ends up
with a different colour in every block that holds it.  Here the variable is the scene's colour array c [n_scene][3]; every
iteration writes c into all block slots, runs the network's forward / CE gradient / colour backward batch by batch, sums the
block gradients over each point's slots in ascending slot order (fp32, no atomics) and takes one sign step on c.  The
result is a point cloud: one colour per point, bounded by eps once.

SceneNUAttack is the norm-unbounded counterpart: Adam in tanh space on the same one-colour-per-point
variable, with the f-loss and Smooth gradients of the blocks summed the same way and the L2 term counted once per point.
"""
import collections
import ctypes

import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks.torchattacks.attacks._common import check_field
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


def _check_target(target, origin):
    if (target is None) != (origin is None):
        raise ValueError("the targeted scene attack needs both `target` and `origin`")
    if target is not None and not 0 <= int(target) < NUM_CLASSES:
        raise ValueError("target class %r out of range" % (target,))


_Scene = collections.namedtuple("_Scene", "dev x_clean idx gt c0 mask occ_off occ_ent bad nb bp n_scene")


def _open_scene(who, net, blocks, point_idx, block_labels, scene_rgb, scene_labels, origin):
    """One scene as both attacks take it (the class docstrings), checked and on the device: the clean blocks, c0 =
    float32(rgb / 255.0), mask = (scene_labels == origin) as uint8 (None without an origin) and the occurrence lists of every
    scene point.  `who` names the calling class in the index error."""
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
    n_scene = scene_rgb.shape[0]
    c0 = upload(torch.from_numpy(np.ascontiguousarray((scene_rgb / 255.0).astype(np.float32))), dev, pin=True)
    mask = None
    if origin is not None:
        if isinstance(scene_labels, torch.Tensor):
            mask = (runtime.require_cuda(scene_labels, "scene_labels") == int(origin)).to(torch.uint8).contiguous()
        else:
            mask = upload(torch.from_numpy((np.asarray(scene_labels) == origin).astype(np.uint8)), dev, pin=True)
        if mask.numel() != n_scene:
            raise ValueError("scene_labels must hold %d labels" % n_scene)

    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    occ_off, occ_ent = runtime.scene_occ_build(idx, n_scene, bad)
    if int(bad.item()):        # (the one read-back of the prologue, before the loop: once per scene)
        raise IndexError("%s: a point index is outside [0, %d)" % (who, n_scene))
    return _Scene(dev, x, idx, gt, c0, mask, occ_off, occ_ent, bad, x.shape[0], x.shape[1], n_scene)


class _Batches:
    """The scene's blocks in batches of `batch_size` consecutive blocks, slicer order (the last one may be smaller): `spans`
    [(lo, hi)], one workspace and one logp buffer per batch size, and the front and the back of a batch's pass."""

    def __init__(self, net, scene, batch_size):
        self.dev, self.bp = scene.dev, scene.bp
        self.model = net._packed()
        self.spans = [(lo, min(lo + batch_size, scene.nb)) for lo in range(0, scene.nb, batch_size)]
        self.sizes = sorted({hi - lo for lo, hi in self.spans})
        self.ws = {b: net._workspace(b, scene.bp, 1) for b in self.sizes}
        net._generation += 1       # the workspace activations no longer belong to an earlier autograd forward
        self.logp = self.per_size(torch.empty, scene.bp, NUM_CLASSES)

    def per_size(self, make, *tail):
        """{B: float32 device tensor [B, *tail]} for every batch size; make = torch.empty | torch.zeros."""
        return {b: make(b, *tail, dtype=torch.float32, device=self.dev) for b in self.sizes}

    def forward(self, xb):
        """FPS starts from the CPU generator (one draw per batch), plan, lean forward -> (starts, logp [B, bp, 13])."""
        b = xb.shape[0]
        starts = upload(draw_fps_starts(b, self.bp, 1, pinned=True), self.dev, pin=True)
        self.ws[b].plan_build(xb, starts, 1)
        return starts, self.ws[b].forward(self.model, 0, xb, self.logp[b], lean=True)

    def backward(self, dlogp, dx0, full=False):
        """dx0 [B, bp, 9] <- channels 3:6 (psg_pn2_backward_colour), or all nine under full (psg_pn2_backward_full)."""
        self.ws[dlogp.shape[0]].backward(self.model, 0, dlogp, dx0, colour_only=not full, full=full)


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
    dx0 [nb, bp, 9], c before the step, c after it, dlogp [nb, bp, 13]) - device tensors; dx0 is the attack's own buffer.

    field (an extension of the reference API, like NB_attack's): "color" (default) is the attack above,
    launch for launch.  "coord" moves channels 0:3, "both" the two fields together; PointNet++ SSG only (the exact coordinate
    gradient psg_pn2_backward_full).  The variable is ONE displacement delta [n_scene][3] (float32, metres, starting at zero)
    per scene point, |delta| <= coord_eps and no box; coord_eps / coord_alpha fall back to eps / alpha.  Every slot holds
    x[e][0:3] = fl32(x_clean[e][0:3] + delta[point_idx[e]]) - one fp32 add onto the slot's clean, block-centred coordinates -,
    so all copies of a point carry the same displacement to within half an ulp of each slot's coordinate; channels 6:9 stay
    as given (the per-block coordinate field's convention).  Block membership is the ORIGINAL slicing's: a point that moves
    across a block's border stays in the blocks that held it, the moved scene is not re-sliced.  Per iteration every batch
    runs psg_scene_delta_to_blocks (both: + psg_scene_colour_to_blocks), the FPS starts, psg_pn2_plan_build (geometry moves),
    psg_pn2_forward_lean, psg_ce_logp_grad, (targeted) psg_scene_rows_mask and psg_pn2_backward_full; then
    psg_scene_field_step sums channels 0:3 of the block gradients over each point's slots in ascending slot order and takes
    delta = clamp(delta + dir * coord_alpha * sign(g), -coord_eps, coord_eps) (un-clamped on the last iteration under
    project_last=False); "both" also runs psg_scene_pgd_step on channels 3:6 of the same gradients.  __call__ still returns
    (adv_rgb01, adv_blocks) - adv_rgb01 is the clean c0 under "coord" -; the final delta is left in self.last_delta (device
    tensor [n_scene, 3]; None after a colour run).
    trace_field: the field path's callback (`trace` is the colour path's and is not called here), called after every iteration
    with a dict: t, starts, dx0 [nb, bp, 9], delta_before, delta_after, c_before, c_after (None under "coord"), dlogp."""

    def __init__(self, model, eps, alpha, iters, batch_size=8, target=None, origin=None, project_last=True, trace=None,
                 field="color", coord_eps=None, coord_alpha=None, trace_field=None):
        self.model = check_scene_model(model)
        self.field = check_field(field)
        if self.field != "color" and not isinstance(model, pointnet2_sem_seg.get_model):
            raise NotImplementedError("field=%r is implemented for the PointNet++ SSG network (pointnet2_sem_seg): the exact "
                                      "coordinate gradient psg_pn2_backward_full refuses MSG" % self.field)
        _check_target(target, origin)
        if int(iters) < 1 or int(batch_size) < 1:
            raise ValueError("iters and batch_size must be positive")
        self.eps, self.alpha, self.iters, self.batch_size = float(eps), float(alpha), int(iters), int(batch_size)
        self.coord_eps = self.eps if coord_eps is None else float(coord_eps)
        self.coord_alpha = self.alpha if coord_alpha is None else float(coord_alpha)
        self.target, self.origin, self.project_last, self.trace = target, origin, bool(project_last), trace
        self.trace_field = trace_field
        self.last_delta = None

    def __call__(self, blocks, point_idx, block_labels, scene_rgb, scene_labels):
        net = self.model
        sc = _open_scene("SceneNBAttack", net, blocks, point_idx, block_labels, scene_rgb, scene_labels, self.origin)
        dev, x_clean, idx, gt, c0, mask, occ_off, occ_ent, bad, nb, bp, n_scene = sc
        colour, coord = self.field != "coord", self.field != "color"
        targeted = self.target is not None
        x = x_clean.clone()     # the caller's blocks stay clean: every iteration adds delta onto THEM
        c = c0.clone() if colour else c0
        delta = torch.zeros(n_scene, 3, dtype=torch.float32, device=dev) if coord else None
        # backward_full writes all nine channels, backward_colour channels 3:6 only
        dx0_all = (torch.empty if coord else torch.zeros)(nb, bp, 9, dtype=torch.float32, device=dev)
        bt = _Batches(net, sc, self.batch_size)
        trace = self.trace_field if coord else self.trace
        if trace is not None:      # the tests read every batch's dlogp: kept scene-wide only then
            dlogp_all = torch.zeros(nb, bp, NUM_CLASSES, dtype=torch.float32, device=dev)
        else:
            dlogp = bt.per_size(torch.empty, bp, NUM_CLASSES)
        direction = -1.0 if targeted else 1.0
        for t in range(self.iters):
            starts_t = []
            for lo, hi in bt.spans:
                b = hi - lo
                xb, ib = x[lo:hi], idx[lo:hi]
                if coord:
                    runtime.scene_delta_to_blocks(delta, ib, x_clean[lo:hi], xb, bad)
                if colour:
                    runtime.scene_colour_to_blocks(c, ib, xb, bad)
                starts, logp = bt.forward(xb)
                dl = dlogp_all[lo:hi] if trace is not None else dlogp[b]
                _lib.call("psg_ce_logp_grad", runtime.ptr(logp), None if targeted else runtime.ptr(gt[lo:hi]),
                          int(self.target) if targeted else 0, b * bp, b * bp, NUM_CLASSES, 1.0 / bp, runtime.ptr(dl), None,
                          runtime.stream())
                if targeted:
                    runtime.scene_rows_mask(dl, ib, mask)
                bt.backward(dl, dx0_all[lo:hi], full=coord)
                if trace is not None:
                    starts_t.append(starts)
            last = t == self.iters - 1 and not self.project_last
            if trace is not None:
                delta_before, c_before = delta.clone() if coord else None, c.clone() if colour else None
            if coord:
                runtime.scene_field_step(delta, mask, occ_off, occ_ent, dx0_all, self.coord_alpha, self.coord_eps, direction, last)
            if colour:
                runtime.scene_pgd_step(c, c0, mask, occ_off, occ_ent, dx0_all, self.alpha, self.eps, direction, last)
            if trace is not None and coord:
                trace(dict(t=t, starts=starts_t, dx0=dx0_all, delta_before=delta_before, delta_after=delta.clone(),
                           c_before=c_before, c_after=c.clone() if colour else None, dlogp=dlogp_all))
            elif trace is not None:
                trace(t, starts_t, dx0_all, c_before, c.clone(), dlogp_all)
        if coord:
            runtime.scene_delta_to_blocks(delta, idx, x_clean, x, bad)
        if colour:
            runtime.scene_colour_to_blocks(c, idx, x, bad)
        self.last_delta = delta
        return c, x


BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8          # torch.optim.Adam's defaults, as nu.py passes them


def _ratio(name, r):
    num, den = int(r[0]), int(r[1])
    if den < 1 or num < 0:
        raise ValueError("%s = (num, den) needs num >= 0 and den > 0, got %r" % (name, (r,)))
    return num, den


class SceneNUAttack:
    """The norm-unbounded attack (Adam in tanh space, the reference's NU column) on the colours of a whole scene: ONE
    colour per physical scene point.  Same models, same call and same batch_size / target / origin
    attributes as SceneNBAttack, so it drops into harness.evaluate_whole_scene_consistent.

    The variable is w [n_scene][3] = inverse_tanh_space(c0), c0 = float32(rgb / 255.0); the colours are c = 1/2 (tanh w + 1).
    Minimised:  cost = sum_blocks f_b + c * sum_blocks Smooth_b + c * sum_points |c_p - c0_p|^2
    f_b: the reference's f-loss over the block's slots (psg_nu_f_loss_grad_rooms, kappa) - non-targeted y = block labels,
    tsign = +1; targeted (target and origin both given) y = target, tsign = -1 and the dlogp rows of slots whose point is
    not of class `origin` zeroed (psg_scene_rows_mask).  This is the plain targeted f-loss, deliberately NOT tar_NU_attack's
    quirks (`_targeted` left at +1, mask and Smooth of batch row 0).  Smooth_b: per block, the `neighbour` (default 10,
    targeted 5) smallest distances from every adversarial colour of the block to the clean colours of the same block
    (psg_smooth_knn_rooms, N <= 8192).  The L2 term counts once per scene point.  Points that move: non-targeted every point
    with a slot, targeted those of class `origin` with a slot (none: ValueError); the others keep the bytes of c0.

    Step s (outer), batch k (inner, slicer order): psg_scene_nu_colour, psg_scene_colour_to_blocks; per batch the FPS
    starts (draw_fps_starts(B_k, bp, 1), CPU generator), psg_pn2_plan_build, psg_pn2_forward_lean,
    psg_nu_f_loss_grad_rooms, (targeted) psg_scene_rows_mask, psg_pn2_backward_colour, psg_smooth_knn_rooms; then
    psg_scene_nu_latch and - not after the last step - psg_scene_nu_step (Adam step s + 1, betas 0.9 / 0.999, eps 1e-8).
    No restart rule, no learning-rate halving, no graph capture.

    Exit, in integers: non-targeted n_hits = slots with pred == label, fires at the first step with n_hits * den < num *
    rows, (num, den) = exit_below; targeted n_hits = masked slots with pred == target, fires with n_hits * den > num *
    masked slots, (num, den) = exit_above.  exit_below = (0, 1) never fires.  The firing step snapshots the colours its
    forward saw and clears the device's `active` word; later launches leave every byte alone.  The host reads that word every
    `check_every` steps (every step under `trace`) and nothing else inside the loop; results do not depend on check_every.

    Returns (adv_rgb01 [n_scene, 3], adv_blocks [nb, bp, 9]): the colours of the exit step's forward, or of step
    steps - 1's, in every slot; channels 0:3 and 6:9 and the caller's blocks stay clean.  Afterwards last_exit_step (-1 at
    the cap), last_history (int64 numpy [steps_run][2]: n_hits, n_counted) and last_w (device tensor).
    trace(dict), after every step: s, starts, dx0 [nb, bp, 9], sgrad [nb, bp, 3], pred [nb, bp], w_before, w_after, m_after,
    v_after, c (the colours of the step's forward), gsum_f, gsum_s (None where no Adam step ran: after the last step or the
    exit), active (0 / 1 after the step's latch) - device tensors; dx0 / sgrad / pred are the attack's own buffers.

    field (an extension of the reference API, like SceneNBAttack's): "color" (default) is the attack
    above, launch for launch.  "coord" moves channels 0:3, "both" the two fields together; PointNet++ SSG only
    (psg_pn2_backward_full).  The coordinate variable is ONE displacement delta [n_scene][3] (float32, metres, zero at the
    start) per scene point, optimised by Adam directly - no tanh space, coordinates have no box -, moments mx = vx = 0; every
    slot holds x[e][0:3] = fl32(x_clean[e][0:3] + delta[point_idx[e]]) (psg_scene_delta_to_blocks, always onto the clean
    blocks), channels 6:9 stay as given and block membership is the original slicing's, as in SceneNBAttack.  Minimised:
      sum_blocks f_b + coord_c * sum_blocks SmoothXyz_b + coord_c * sum_points |delta_p|^2     ("both": + the two colour terms)
    SmoothXyz_b: the Smooth term on channels 0:3 of the block's moved slots against its CLEAN slots (psg_smooth_knn_xyz_rooms,
    direct differences); coord_c / coord_lr fall back to c / lr.  Per batch: psg_scene_delta_to_blocks (both: +
    psg_scene_colour_to_blocks), the FPS starts, psg_pn2_plan_build (geometry moves), psg_pn2_forward_lean,
    psg_nu_f_loss_grad_rooms, (targeted) psg_scene_rows_mask, psg_pn2_backward_full, psg_smooth_knn_xyz_rooms (both: +
    psg_smooth_knn_rooms); then psg_scene_nu_latch (its snapshot is of the colours: c0 under "coord") and - not after the last
    step - psg_scene_nu_field_step (both: + psg_scene_nu_step on channels 3:6 of the same gradients).  The exit leaves delta as
    the firing step's forward saw it.  __call__ still returns (adv_rgb01, adv_blocks) - adv_rgb01 is the clean c0 under
    "coord" -; afterwards last_delta (device tensor [n_scene, 3]; None after a colour run), last_mx, last_vx.  The trace dict
    then also carries delta_before, delta_after, mx_after, vx_after, sgrad_xyz [nb, bp, 3], gsum_x, gsum_sx (None where no
    Adam step ran); under "coord" the colour state's entries (w_*, m_after, v_after, sgrad, gsum_f, gsum_s) are None."""

    def __init__(self, model, c=1e-4, kappa=0, steps=1000, lr=0.01, batch_size=8, neighbour=None, target=None, origin=None,
                 exit_below=(1, 13), exit_above=(9, 10), check_every=10, trace=None, field="color", coord_c=None, coord_lr=None):
        self.model = check_scene_model(model)
        self.field = check_field(field)
        if self.field != "color" and not isinstance(model, pointnet2_sem_seg.get_model):
            raise NotImplementedError("field=%r is implemented for the PointNet++ SSG network (pointnet2_sem_seg): the exact "
                                      "coordinate gradient psg_pn2_backward_full refuses MSG" % self.field)
        _check_target(target, origin)
        if int(steps) < 1 or int(batch_size) < 1 or int(check_every) < 1:
            raise ValueError("steps, batch_size and check_every must be positive")
        self.exit_below, self.exit_above = _ratio("exit_below", exit_below), _ratio("exit_above", exit_above)
        if neighbour is None:
            neighbour = 5 if target is not None else 10          # the reference's: nontarget.py / target.py
        if not 1 <= int(neighbour) <= 16:
            raise ValueError("neighbour = %r outside 1 .. 16 (psg_smooth_knn_rooms)" % (neighbour,))
        self.c, self.kappa, self.steps, self.lr = float(c), float(kappa), int(steps), float(lr)
        self.coord_c = self.c if coord_c is None else float(coord_c)
        self.coord_lr = self.lr if coord_lr is None else float(coord_lr)
        given = self.field != "color"          # the colour attack never reads them: only what the caller passed is checked
        if (given or coord_lr is not None) and not self.coord_lr > 0:
            raise ValueError("coord_lr = %r must be positive" % (self.coord_lr,))
        if (given or coord_c is not None) and not self.coord_c >= 0:
            raise ValueError("coord_c = %r must not be negative" % (self.coord_c,))
        self.batch_size, self.neighbour, self.check_every = int(batch_size), int(neighbour), int(check_every)
        self.target, self.origin, self.trace = target, origin, trace
        self.last_exit_step, self.last_history, self.last_w = None, None, None
        self.last_delta, self.last_mx, self.last_vx = None, None, None

    def __call__(self, blocks, point_idx, block_labels, scene_rgb, scene_labels):
        net = self.model
        sc = _open_scene("SceneNUAttack", net, blocks, point_idx, block_labels, scene_rgb, scene_labels, self.origin)
        dev, x_clean, idx, gt, c0, mask, occ_off, occ_ent, bad, nb, bp, n_scene = sc
        colour, coord = self.field != "coord", self.field != "color"
        targeted = self.target is not None
        if targeted and not bool(mask[idx.reshape(-1).long()].any().item()):       # (a read-back, once per scene)
            raise ValueError("SceneNUAttack: no slot of this scene holds a point of the origin class %r" % (self.origin,))

        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)      # noqa: E731
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)        # noqa: E731
        x = x_clean.clone()        # the caller's blocks stay clean, and are the Smooth terms' reference slots
        c = c0.clone() if colour else c0
        w = m = v = sgrad_all = nn_state = None
        if colour:
            w = runtime.scene_nu_init(c0)
            m, v = f32(n_scene, 3), f32(n_scene, 3)
            sgrad_all = f32(nb, bp, 3)
            nn_state = i32(nb, bp, self.neighbour)
        delta = mx = vx = sgrad_xyz = None
        if coord:
            delta, mx, vx = f32(n_scene, 3), f32(n_scene, 3), f32(n_scene, 3)
            sgrad_xyz = f32(nb, bp, 3)
        snap = f32(n_scene, 3)
        active = torch.ones(1, dtype=torch.int32, device=dev)
        exit_step = torch.full((1,), -1, dtype=torch.int32, device=dev)
        counters = i32(2)
        hist = torch.zeros(self.steps, 2, dtype=torch.int64, device=dev)
        dx0_all = f32(nb, bp, 9)   # backward_colour writes channels 3:6 only, backward_full all nine
        pred_all = i32(nb, bp)
        bt = _Batches(net, sc, self.batch_size)
        dlogp = bt.per_size(torch.zeros, bp, NUM_CLASSES)
        f_sum = bt.per_size(torch.zeros)               # psg_nu_f_loss_grad_rooms adds the rooms' f sums here: not read
        trace = self.trace
        gsum_f = gsum_s = gsum_x = gsum_sx = None
        if trace is not None and colour:
            gsum_f, gsum_s = f32(n_scene, 3), f32(n_scene, 3)
        if trace is not None and coord:
            gsum_x, gsum_sx = f32(n_scene, 3), f32(n_scene, 3)
        tsign = -1.0 if targeted else 1.0
        num, den = self.exit_above if targeted else self.exit_below
        off3 = lambda t: ctypes.c_void_p(t.data_ptr() + 3 * 4)                          # noqa: E731  (channel 3 of row 0)
        st = runtime.stream
        for s in range(self.steps):
            if colour:
                runtime.scene_nu_colour(w, mask, occ_off, active, c)
            if not coord:
                runtime.scene_colour_to_blocks(c, idx, x, bad)
            starts_s = []
            for lo, hi in bt.spans:
                b = hi - lo
                xb = x[lo:hi]
                if coord:
                    runtime.scene_delta_to_blocks(delta, idx[lo:hi], x_clean[lo:hi], xb, bad)
                    if colour:
                        runtime.scene_colour_to_blocks(c, idx[lo:hi], xb, bad)
                starts, logp = bt.forward(xb)
                _lib.call("psg_nu_f_loss_grad_rooms", runtime.ptr(logp), None if targeted else runtime.ptr(gt[lo:hi]),
                          int(self.target) if targeted else 0, b, bp, NUM_CLASSES, self.kappa, tsign, runtime.ptr(dlogp[b]),
                          runtime.ptr(f_sum[b]), runtime.ptr(pred_all[lo:hi]), st())
                if targeted:
                    runtime.scene_rows_mask(dlogp[b], idx[lo:hi], mask)
                bt.backward(dlogp[b], dx0_all[lo:hi], full=coord)
                if coord:
                    _lib.call("psg_smooth_knn_xyz_rooms", runtime.ptr(xb), 9, bp * 9, runtime.ptr(x_clean[lo:hi]), 9, bp * 9, b, bp,
                              self.neighbour, None, runtime.ptr(sgrad_xyz[lo:hi]), None, None, st())
                if colour:
                    _lib.call("psg_smooth_knn_rooms", off3(xb), 9, bp * 9, off3(x_clean[lo:hi]), 9, bp * 9, b, bp, self.neighbour,
                              None, runtime.ptr(sgrad_all[lo:hi]), runtime.ptr(nn_state[lo:hi]), 1 if s > 0 else 0, st())
                if trace is not None:
                    starts_s.append(starts)
            runtime.scene_nu_latch(pred_all, None if targeted else gt, int(self.target) if targeted else 0, idx, mask, num, den, s,
                                   c, snap, counters, hist[s], exit_step, active)
            stepping = s < self.steps - 1
            if trace is not None:
                w_before = w.clone() if colour else None
                delta_before = delta.clone() if coord else None
                running = bool(active.item())
            if stepping and coord:
                runtime.scene_nu_field_step(delta, mx, vx, mask, occ_off, occ_ent, dx0_all, sgrad_xyz, self.coord_c, self.coord_lr,
                                            BETA1, BETA2, ADAM_EPS, s + 1, active, gsum_x, gsum_sx)
            if stepping and colour:
                runtime.scene_nu_step(w, m, v, c, c0, mask, occ_off, occ_ent, dx0_all, sgrad_all, self.c, self.lr, BETA1, BETA2,
                                      ADAM_EPS, s + 1, active, gsum_f, gsum_s)
            if trace is not None:
                stepped = stepping and running
                kept = lambda t, on=True: t.clone() if on and t is not None else None      # noqa: E731
                row = dict(s=s, starts=starts_s, dx0=dx0_all, sgrad=sgrad_all, pred=pred_all, w_before=w_before, w_after=kept(w),
                           m_after=kept(m), v_after=kept(v), c=c.clone(), gsum_f=kept(gsum_f, stepped), gsum_s=kept(gsum_s, stepped),
                           active=int(running))
                if coord:
                    row.update(delta_before=delta_before, delta_after=delta.clone(), mx_after=mx.clone(), vx_after=vx.clone(),
                               sgrad_xyz=sgrad_xyz, gsum_x=kept(gsum_x, stepped), gsum_sx=kept(gsum_sx, stepped))
                trace(row)
                if not running:
                    break
            elif (s + 1) % self.check_every == 0 and not int(active.item()):
                break
        exited = int(exit_step.item())
        self.last_exit_step = exited
        self.last_history = hist[:exited + 1 if exited >= 0 else self.steps].cpu().numpy()
        self.last_w = w
        self.last_delta, self.last_mx, self.last_vx = delta, mx, vx
        adv = snap if exited >= 0 and colour else c
        if coord:
            runtime.scene_delta_to_blocks(delta, idx, x_clean, x, bad)
        if colour:
            runtime.scene_colour_to_blocks(adv, idx, x, bad)
        return adv, x

