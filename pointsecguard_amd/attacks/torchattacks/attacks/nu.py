"""Host loop of the NU (norm-unbounded, Adam in tanh space) attacks over the libpsg kernels.

Reference: PointNet/attacks/torchattacks/attacks/nontarget.py:52-135 (NU_attack.forward/f/smooth) and
target.py:62-175 (tar_NU_attack.forward/non_f/tar_f/smooth).  Per step:
  colour = 1/2 (tanh w + 1) -> model forward -> f-loss on softmax(log-probs) + c*Smooth + c*L2 ->
  input-gradient backward -> Adam step on w.
Everything numeric runs in HIP kernels (psg_nu_*, psg_smooth_knn, psg_pn2_forward/backward), and since round 4 so
does the per-step part of the reference's control flow: `psg_nu_step_latch` counts the correct points / target hits,
files them with the step's loss sums in a device-side history and evaluates the accuracy exit test in double
precision exactly as the host did; the first step whose test fires snapshots the image and clears the attack's
active flag.  The host reads the history only where the reference itself must touch the host - after step 0
(at batch 32 the targeted attack always exits there), after every 10th step (restart test + noise draw,
learning-rate halving with a fresh optimiser every 50) and at the end: an attack that exits at step s returns
its step-s image, at most 9 later steps are speculation that is thrown away.  With a `trace` callback (tests)
the history is read after every step, like the reference's `.item()` calls.

Reference behaviours kept on purpose: the Smooth term and `other_acc`
use batch row 0 only; `acc` divides by 4096 whatever the batch; the returned image lags the optimiser by
one step; `_targeted` stays +1 unless set_attack_mode() is called; the restart adds uniform noise to the
masked colours (overwritten by tanh_space on the next step) and clamps ALL nine channels to [0,1], which
moves the xyz coordinates -- the geometry plan is rebuilt from the current coordinates after it.
"""
import ctypes

import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks.nu_windows import CHUNK, RoomsState, _bind, room_masks, to_restart, window_end, window_loop
from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts, upload

from . import pointnet as pointnet_net
from ._common import labels_to_device, mask_to_device, psg_model

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
# Geometry plan horizon (round 6).  A plan may run up to PLAN_AHEAD forwards ahead of the control-flow windows (`plan_ahead`
# forwards at once; what a restart or an early exit leaves unused of it is re-drawn / given back to the generator: the FPS
# draws come from the CPU generator in forward order, pointnet_util.py:75, the restart noise of target.py:131 from the
# device's - the two streams do not interleave).  The round-5 review expected that to pay (a 640-problem plan per window is
# bound by FPS latency: 17.1 of a window's 40.9 ms in the profiled call) and it does not: rooms/s of the configs[2] bench at
# plan_ahead = 10 / 20 / 30 / 50: 614 / 591 / 587 / 572 with four calls in flight, 478 / 468 / 461 / 456 with one
# (tools/r06_g.sh) - the small plans run in the shadow of the network kernels around them, a 2 496-problem plan is a
# 24-ms block that nothing overlaps.  So the default stays one plan per window (= rounds 3-5); the knob and its bookkeeping
# stay, tested at 50 (tests/test_gpu_nu.py), for callers whose attacks run one at a time with long step caps.
PLAN_AHEAD = 50          # capacity: forwards a geometry plan may hold (graph handles, workspace slots)
plan_ahead = CHUNK       # forwards actually planned at once (a multiple of CHUNK, <= PLAN_AHEAD): module-level knob


class _NuState(RoomsState):
    """RoomsState of G attacks of `rows` batch rows with the colour loops' scratch, and one graph handle per window position
    inside a geometry plan (a captured window holds its plan slots)."""

    def __init__(self, dev, G, rows, N, neighbour):
        super().__init__(dev, G, rows, N, neighbour, n_scal=3, n_graphs=PLAN_AHEAD // CHUNK)     # scal rows: f, smooth, l2
        B = G * rows
        self.key = (G, rows, N, int(neighbour))
        self.x0_orig = self._f32(B, N, 9)
        self.logp, self.dlogp = self._f32(B, N, 13), self._f32(B, N, 13)
        self.restart_l2 = self._f32(G)                               # psg_nu_restart_rooms: sum((x - x_orig)^2), channels 0:3 and 6:9


def _state(net, dev, G, rows, N, neighbour):
    return _NuState.of(net, "_psg_nu_states", (str(dev), G, rows, N, int(neighbour)), dev, G, rows, N, neighbour)


def _pointnet_restart(S, x0, again, n_mask, G, rows, N, dev, extra_l2):
    """The restart of target.py:127-132 for the attacks `again` of a PointNet state: the noise is drawn as the PointNet++ code
    of _nu_core draws it - per attack, in ascending order, from the device generator - and placed by ONE psg_nu_restart_rooms
    launch for all of them (mask-order scatter, clamp of all nine channels, the extra L2 per attack into extra_l2)."""
    offs, flags, total = np.zeros(G, np.int64), np.zeros(G, np.uint8), 0
    blocks = []
    for g in again:
        blocks.append(torch.empty(rows, 3, int(n_mask[g]), device=dev, dtype=torch.float32).uniform_(0, 1).reshape(-1))
        offs[g], flags[g] = total, 1
        total += blocks[-1].numel()
    noise = torch.cat(blocks)
    ctl = torch.from_numpy(np.concatenate([offs.view(np.uint8), flags])).to(dev)          # one upload: offsets, flags
    _lib.call("psg_nu_restart_rooms", runtime.ptr(x0), runtime.ptr(S.x0_orig), runtime.ptr(S.mask), runtime.ptr(S.n_mask),
              ctypes.c_void_p(ctl.data_ptr() + 8 * G), runtime.ptr(noise), runtime.ptr(ctl), G, rows, N, runtime.ptr(S.restart_l2),
              runtime.stream())
    extra_l2[again] = S.restart_l2.cpu().numpy().astype(np.float64)[again]               # one read-back for all of them


def _nu_core(atk, images, labels, masks, target, neighbour, targeted_variant, trace, starts_fn, G, rows, record=None, restore_lr=False):
    """G attacks of `rows` batch rows each, advanced together: (1, B) = the reference's call on a batch of B rows (its batch
    semantics: Smooth term and mask of batch row 0, counts over all rows), (R, 1) = R one-room calls in lockstep.
    masks: [G, N] or None.  Returns (out [G*rows, 9, N], steps_run [G]: the optimiser steps the reference's loop ran).

    The window loop is nu_windows.window_loop; this function supplies what is this network's.  The vanilla PointNet
    (pointnet.is_pointnet) goes the same way: its windows are psg_pointnet_nu_window calls, it has no geometry plan (no FPS
    starts, nothing drawn from or given back to the CPU generator) and its restart is one psg_nu_restart_rooms launch.
    `record(step, row [5, G], extra_l2 [G], was_active [G])` (tests) receives every step's history row without changing the
    windows (`trace` reads back after every step, so it cannot observe them), and `record(step, None, extra_l2, restarting [G])`
    when attacks restart after `step`."""
    B, _, N = images.shape
    assert B == G * rows
    masks, n_mask = room_masks(masks, G, N, targeted_variant, "target.py:104")
    pointnet = pointnet_net.is_pointnet(atk.model)
    net = psg_model(atk.model)
    dev = atk.device
    images = images.detach().to(dev).float().contiguous()
    st = runtime.stream
    S = _state(net, dev, G, rows, N, neighbour)
    model = net._packed()
    net._generation += 1
    if pointnet:
        ws = net._workspace(B, N)
    else:
        ws = net._workspace(B, N, max(CHUNK + 1, min(int(plan_ahead), PLAN_AHEAD)))  # plan slots: what a plan can hold, no more
    use_target = targeted_variant and target is not None
    mode = 0 if not targeted_variant else (2 if use_target else 1)
    S.labels.copy_(labels_to_device(labels, dev))
    mask_b = None
    if masks is not None:
        S.mask.copy_(torch.from_numpy(masks.astype(np.uint8)))
        mask_b = S.mask.bool()
    S.n_mask.copy_(torch.from_numpy(n_mask.astype(np.int32)))
    x0, w, m, v = S.x0, S.w, S.m, S.v
    _lib.call("psg_to_point_major", runtime.ptr(images), B, 9, N, runtime.ptr(x0), st())
    S.ori.copy_(x0[:, :, 3:6])
    S.x0_orig.copy_(x0)
    _lib.call("psg_nu_inverse_tanh", runtime.ptr(x0), B, N, runtime.ptr(w), st())
    m.zero_(); v.zero_(); S.scal.zero_()
    S.active.fill_(1); S.exit.fill_(-1)
    extra_l2 = np.zeros(G)  # (adv - images)^2 over the non-colour channels: non-zero only after a restart clamped them
    prev_cost = np.full((atk.steps, G), 1e10)
    cost = None
    win_args, win_entry = (_lib.PointnetNuWindowArgs, "psg_pointnet_nu_window") if pointnet else (_lib.NuWindowArgs, "psg_pn2_nu_window")
    win = win_args(
        model=model.handle.value, ws=ws.handle.value, G=G, rows=rows, N=N, mode=mode, use_target=int(use_target),
        target=int(target) if use_target else 0, neighbour=int(neighbour), kappa=float(atk.kappa), tsign=float(atk._targeted),
        c_smooth=float(atk.c), c_l2=float(atk.c), beta1=BETA1, beta2=BETA2, eps=ADAM_EPS)
    _bind(win, S, "w m v n_mask x0 ori labels logp dlogp dx0 sgrad pred scal nn_state hist out active exit_step=exit")
    win.mask = S.mask.data_ptr() if masks is not None else None
    if pointnet:
        win.fused_head = 1 if pointnet_net.fused_head else 0
        win.logp = None                                  # (scratch of the three-kernel head's log-probs: nobody reads a copy)
    planned_until, plan_base, rng_at = 0, 0, None

    def plan(step):
        """the geometry plan that covers `step`, built when there is none -> its end"""
        nonlocal planned_until, plan_base, rng_at
        if step >= planned_until:
            # Geometry windows end after steps 10, 20, 30, ..: a restart (which draws from the RNG and may move xyz) can
            # only follow a step that is a multiple of 10 greater than 10, so the FPS draws of a window come out of the
            # generator in the reference's order.  The first forward is planned ALONE: the accuracy exits can end the
            # attack right after it (at batch 32 the targeted one always does, target.py:105-121), and a plan for
            # eleven forwards would then be ten too many; the rest of the first window follows with step 1.
            # (the plan reads the coordinates only; the colours of a step are written inside the window call)
            # (round 6) ... the plan may run up to `plan_ahead` forwards ahead ([0], [1..50], [51..100], .. at 50); the draws are
            # made window by window with the generator's state kept at every window end, so that what is not consumed can
            # be given back (end of the attack) or drawn again (a restart moved the coordinates)
            n_plan = 1 if step == 0 else min(max(CHUNK, min(int(plan_ahead), PLAN_AHEAD)) // CHUNK * CHUNK, atk.steps - step)
            if starts_fn is not None:
                starts = upload(starts_fn(step, n_plan), dev)
                rng_at = None
            else:
                if rng_at is not None and step in rng_at:
                    torch.set_rng_state(rng_at[step])                # the unused draws of the plan this one replaces
                parts, rng_at, s_ = [], {}, step
                while s_ < step + n_plan:
                    e_ = min(window_end(s_, CHUNK), step + n_plan)
                    parts.append(draw_fps_starts(B, N, e_ - s_))
                    rng_at[e_] = torch.get_rng_state()
                    s_ = e_
                starts = upload(torch.cat(parts), dev)
            ws.plan_build(x0, starts, n_plan)
            plan_base, planned_until = step, step + n_plan
        return planned_until

    def enqueue(step, n_run, adam_t):
        # the steps of the window in ONE call: colours, forward, f-loss, backward, Smooth term, Adam step, statistics + exit
        # latch per step; full windows of the same shape are replayed as a hipGraph (psg_pn2_nu_window)
        win.step0, win.n_steps = step, n_run
        win.adam_t0, win.lr, win.warm_first = adam_t, float(atk.lr), 1 if step > 0 else 0
        if pointnet:
            graph = S.graphs[0] if n_run == CHUNK else None              # (no plan slots in the key: one handle serves every window)
        else:
            win.slot0 = step - plan_base
            graph = S.graphs[((step - plan_base) // CHUNK) % len(S.graphs)] if n_run == CHUNK and (step - plan_base) % CHUNK == 0 else None
        _lib.call(win_entry, ctypes.byref(win), graph, st())

    def on_step(s_i, row, was_active, exited):
        nonlocal cost
        f_loss, sm_loss, l2_loss = row[2], row[3], row[4] + extra_l2
        cost = f_loss + float(atk.c) * sm_loss + float(atk.c) * l2_loss
        prev_cost[s_i] = np.where(was_active, cost, prev_cost[s_i])
        if trace is not None:
            trace(s_i, cost, f_loss, sm_loss, l2_loss, was_active, S)
        if record is not None:
            record(s_i, row.copy(), extra_l2.copy(), was_active.copy())

    def between(last, step, active):                     # target.py:127-132, attack by attack
        nonlocal planned_until
        again = to_restart(last, active, cost, prev_cost)
        if not len(again):
            return
        if record is not None:
            record(last, None, extra_l2.copy(), np.isin(np.arange(G), again))        # a restart event: who restarts after `last`
        if pointnet:
            _pointnet_restart(S, x0, again, n_mask, G, rows, N, dev, extra_l2)
            return
        for g in again:                                  # the noise draws stay per attack, in order
            k = int(n_mask[g])
            noise = torch.empty(rows, 3, k, device=dev, dtype=torch.float32).uniform_(0, 1)
            col = x0[g * rows:(g + 1) * rows, :, 3:6].transpose(1, 2)        # view [rows, 3, N]
            col[:, :, mask_b[g]] = col[:, :, mask_b[g]] + noise
        ridx = torch.from_numpy(np.concatenate([np.arange(g * rows, (g + 1) * rows) for g in again])).to(dev)
        clamped = x0[ridx].clamp_(min=0, max=1)                   # ALL channels, like the reference
        x0[ridx] = clamped
        d = clamped - S.x0_orig[ridx]
        sums = ((d[:, :, 0:3] ** 2).sum(dim=(1, 2)) + (d[:, :, 6:9] ** 2).sum(dim=(1, 2))).reshape(len(again), rows)
        extra_l2[again] = sums.sum(dim=1).cpu().numpy().astype(np.float64)   # one read-back for all of them
        planned_until = step                             # xyz may have moved: rebuild the plan before the next forward

    out, steps_run, step = window_loop(atk, S, rows, enqueue, targeted_variant=targeted_variant, on_step=on_step, between=between,
                                       limit=None if pointnet else plan, one_step=trace is not None, moments=(m, v),
                                       restore_lr=restore_lr)
    if rng_at is not None and planned_until > step:
        # draws of forwards that never ran go back to the generator - all but those of the window the attack stopped in
        # (rounds 3-5 drew window by window: the generator is left where it was left then)
        e_ = step if step in rng_at else min(k for k in rng_at if k >= step)
        torch.set_rng_state(rng_at[e_])
    return out, steps_run


def nu_attack(atk, images, labels, mask, target, neighbour, targeted_variant=False, trace=None, starts_fn=None, return_steps=False,
              record=None):
    """NU_attack.forward / tar_NU_attack.forward on a batch (the reference's call).  `starts_fn(step, n_plan)` (tests) supplies
    the [n_plan, 4, B] FPS start indices of a geometry window instead of the generator draws; `trace` (tests) is called
    after every step with the step's scalars and the state tensors (and makes the loop read back after every step);
    `return_steps`: also return the number of optimiser steps the reference's loop ran."""
    B, _, N = images.shape
    masks = None
    if mask is not None:
        masks = mask_to_device(mask, N, "cpu").numpy().astype(bool)[None]
    tr = None
    if trace is not None:
        def tr(step, cost, f, sm, l2, was_active, S):
            trace(step=step, cost=float(cost[0]), f=float(f[0]), smooth=float(sm[0]), l2=float(l2[0]), w=S.w, m=S.m, v=S.v, dx0=S.dx0,
                  x0=S.x0, pred=S.pred)
    # (the reference leaves the halved lr on the attack object, target.py:123-125: a batch call does too)
    out, steps_run = _nu_core(atk, images, labels, masks, target, neighbour, targeted_variant, tr, starts_fn, 1, B, record=record)
    return (out, int(steps_run[0])) if return_steps else out


def nu_attack_rooms(atk, images, labels, masks, target, neighbour, targeted_variant=False, trace=None, starts_fn=None, record=None):
    """R independent ONE-ROOM attacks advanced in lockstep: what `nu_attack` does when it is called once per room
    (`images[r:r+1]`, `labels[r:r+1]`, `masks[r]`), with one launch per operation for all rooms instead of R
    (psg_*_rooms entry points; the network kernels simply see a batch of R).  This is how BASELINE configs[2] is applied
    per room: the reference's tar_NU semantics are batch-of-one (target.py:62-133: Smooth term, exit
    accuracies and the mask all read batch row 0).

    Per room exactly the per-call arithmetic: its own mask row, Smooth term, f / Smooth / L2 sums, cost history, exit test
    and restart; a room that has left the loop keeps the image it returned and is skipped by the optimiser.  Rooms share
    the step counter, so all of them re-plan their geometry at the same steps ([0], [1..10], [11..20], ..: where a single
    call re-plans too).  Two things differ from R sequential calls and are why this is a separate entry: (1) the FPS
    start indices of a window are drawn for all rooms at once ([n_plan, 4, R] from the CPU generator) instead of room
    after room, and restart noise is drawn room by room at the step it happens - the same distributions, another order of
    consumption; (2) the learning rate.  The reference halves `self.lr` every 50 steps and leaves it halved on the attack
    OBJECT (target.py:123-125); its harness constructs a NEW `tar_NU_attack` for every batch (NU_target_test_semseg.py:181,
    steps=1000), so every attack of the real protocol starts from the constructor's lr.  That is what lockstep rooms do:
    every room starts from the lr this object holds at the call - R fresh objects -, all rooms halve together (they
    share the step counter), and on return `self.lr` is put back to its value at the call (like the harness's throw-away
    objects; R sequential calls on ONE object would instead hand each room the previous room's left-over lr).  Rounds 3-4
    refused more than 50 steps for this reason; with the fresh-object semantics stated, the 1000-step protocol runs in
    lockstep (tests/test_gpu_nu.py::test_tar_nu_rooms_past_the_lr_halving_equals_fresh_objects_per_room).

    images [R, 9, N], labels [R, N], masks [R, N] bool (None for the non-targeted variant).  Returns (adv [R, 9, N],
    steps_run [R] int64 numpy: the optimiser steps each room executed).
    """
    R, _, N = images.shape
    if R < 2:
        raise ValueError("nu_attack_rooms advances several rooms in lockstep; call nu_attack for one room")
    tr = None
    if trace is not None:
        def tr(step, cost, f, sm, l2, was_active, S):
            trace(step=step, cost=cost, f=f, smooth=sm, l2=l2, w=S.w, m=S.m, v=S.v, dx0=S.dx0, x0=S.x0, pred=S.pred,
                  active=was_active.copy())
    return _nu_core(atk, images, labels, masks, target, neighbour, targeted_variant, tr, starts_fn, R, 1, record=record, restore_lr=True)


def ctypes_off(t, n_floats):
    """Device pointer to element `n_floats` of a float32 tensor."""
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * n_floats)
