"""Host loop of the ResGCN NU attacks over the libpsg kernels.

Reference: ResGCN/sem_seg_dense/attacks/torchattacks/attacks/colper.py:42-120 (NU_attack) and tcolper.py:51-170
(tar_NU_attack).  Differences from the PointNet variants that are reproduced here: the f-loss works on raw
logits with the reference's one-hot masking (a 0 takes part in every max); cost = c*f + 1e-4*Smooth + L2
(NU) / f + 1e-4*Smooth + c*L2 (tar_NU); Smooth compares the adversarial colours with THEMSELVES
(smooth(adv_images, images) ignores its second argument: colper.py:115-117), so its gradient flows through both
sides of every neighbour pair; NU_attack draws uniform noise every steps//10 steps without using it.
"""
import ctypes

import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks.torchattacks.attacks.nu import ADAM_EPS, BETA1, BETA2, _pointnet_restart, ctypes_off

from .colper import _gcn


def gcn_nu_attack(atk, images, labels, mask=None, target=None, neighbour=10, targeted_variant=False, trace=None):
    net = _gcn(atk.model)
    dev = atk.device
    images = images.detach().to(dev).float()
    B, C, N, _ = images.shape
    labels_d = labels.detach().to(dev).to(torch.int32).contiguous()
    mask_d = mask_b = None
    if mask is not None:
        m_np = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
        mask_d = torch.from_numpy(m_np.astype(np.uint8)).to(dev)
        mask_b = mask_d.bool()
    model, ws = net._packed(), net._workspace(B, N)
    net._generation += 1
    st = runtime.stream
    x0 = torch.empty(B, N, 9, device=dev, dtype=torch.float32)
    _lib.call("psg_to_point_major", runtime.ptr(images[:, :, :, 0].contiguous()), B, 9, N, runtime.ptr(x0), st())
    ori = x0[:, :, 3:6].contiguous()
    x0_orig = x0.clone()
    extra_l2 = 0.0
    w = torch.empty(B, N, 3, device=dev, dtype=torch.float32)
    _lib.call("psg_nu_inverse_tanh", runtime.ptr(x0), B, N, runtime.ptr(w), st())
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    dl = torch.empty(B, N, 13, device=dev, dtype=torch.float32)
    dx0 = torch.empty(B, N, 9, device=dev, dtype=torch.float32)
    sgrad = torch.empty(N, 3, device=dev, dtype=torch.float32)
    pred = torch.empty(B, N, device=dev, dtype=torch.int32)
    scal = torch.zeros(3, device=dev, dtype=torch.float32)
    lr, adam_t = float(atk.lr), 0
    prev_cost = [1e10] * atk.steps
    tsign = float(atk._targeted)
    use_target = targeted_variant and target is not None
    mode = 0 if not targeted_variant else (2 if use_target else 1)
    c_f = float(atk.c) if not targeted_variant else 1.0        # colper: c*f + 1e-4*S + L2 ; tcolper: f + 1e-4*S + c*L2
    c_l2 = 1.0 if not targeted_variant else float(atk.c)
    out = torch.empty(B, 9, N, device=dev, dtype=torch.float32)

    def snapshot():
        _lib.call("psg_to_channel_major", runtime.ptr(x0), B, 9, N, runtime.ptr(out), st())
        return out.unsqueeze(-1)

    for step in range(atk.steps):
        _lib.call("psg_nu_tanh_color", runtime.ptr(w), runtime.ptr(mask_d), B, N, runtime.ptr(x0), st())
        net.consume_rng(1)
        logits = ws.forward(model, x0)
        scal.zero_()
        _lib.call("psg_gcn_f_loss_grad", runtime.ptr(logits), runtime.ptr(labels_d), int(target) if use_target else 0,
                  runtime.ptr(mask_d), mode, B * N, N, 13, float(atk.kappa), tsign, c_f, runtime.ptr(dl),
                  runtime.ptr(scal[0:1]), runtime.ptr(pred), st())
        ws.backward(model, dl, dx0)
        _lib.call("psg_smooth_knn", ctypes_off(x0, 3), 9, ctypes_off(x0, 3), 9, N, int(neighbour), runtime.ptr(scal[1:2]),
                  runtime.ptr(sgrad), st())
        adam_t += 1
        _lib.call("psg_nu_adam_step", runtime.ptr(w), runtime.ptr(m), runtime.ptr(v), runtime.ptr(mask_d), runtime.ptr(dx0),
                  runtime.ptr(x0), runtime.ptr(ori), runtime.ptr(sgrad), 1e-4, c_l2, lr, BETA1, BETA2, ADAM_EPS, adam_t, B, N,
                  runtime.ptr(scal[2:3]), st())
        correct = pred.eq(labels_d)
        if targeted_variant:
            hits = (pred.eq(int(target)) if use_target else correct)[:, mask_b].sum()
            stats = torch.stack([correct.sum().float(), hits.float(), scal[0], scal[1], scal[2]]).cpu()
        else:
            stats = torch.stack([correct.sum().float(), scal[0], scal[0], scal[1], scal[2]]).cpu()
        n_correct, n_tgt, f_loss, sm_loss, l2_loss = (float(z) for z in stats)
        l2_loss += extra_l2
        cost = c_f * f_loss + 1e-4 * sm_loss + c_l2 * l2_loss
        prev_cost[step] = cost
        if trace is not None:
            trace(step=step, cost=cost, f=f_loss, smooth=sm_loss, l2=l2_loss, w=w, m=m, v=v, x0=x0, pred=pred)
        if not targeted_variant:
            if n_correct / 4096 < 1 / 13:                       # colper.py:88-89
                return snapshot()
            if step % max(atk.steps // 10, 1) == 0:            # colper.py:90-93: noise drawn, never used
                torch.empty(B, 9, N, 1, device=dev).uniform_(0, 0.01)
            continue
        target_acc = n_tgt / float(mask_b.sum().item())
        if (not use_target and target_acc < 1 / 13) or (use_target and target_acc > 0.9):   # tcolper.py:118-123
            return snapshot()
        if step > 0 and step % 50 == 0:                         # tcolper.py:125-127
            atk.lr = atk.lr / 2
            lr, adam_t = float(atk.lr), 0
            m.zero_()
            v.zero_()
        if step > 10 and step % 10 == 0 and cost >= prev_cost[step - 10]:   # tcolper.py:129-132
            noise = torch.empty(B, 3, int(mask_b.sum().item()), device=dev, dtype=torch.float32).uniform_(0, 1)
            col = x0[:, :, 3:6].transpose(1, 2)
            col[:, :, mask_b] = col[:, :, mask_b] + noise
            x0.clamp_(min=0, max=1)
            dd = x0 - x0_orig
            extra_l2 = float((dd[:, :, 0:3] ** 2).sum().item() + (dd[:, :, 6:9] ** 2).sum().item())
    return snapshot()


# ---------------------------------------------------------------------------------------------------------------------
# Rooms in lockstep, steps in device-side windows (psg_gcn_nu_window): R one-room attacks advanced together.
CHUNK = 10  # control-flow window: tcolper's restart test and lr halving can only follow steps that are multiples of 10


class _GcnNuState:
    """Device buffers of one lockstep shape (R rooms of N points, `neighbour` Smooth neighbours), kept with the model instance
    between calls: the addresses stay the same, so a 10-step window captured as a hipGraph by one call is replayed by the
    next (one model instance serves one host thread / stream at a time, like its network workspace)."""

    def __init__(self, dev, R, N, neighbour):
        f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
        self.x0, self.x0_orig, self.ori = f32(R, N, 9), f32(R, N, 9), f32(R, N, 3)
        self.w, self.m, self.v = f32(R, N, 3), f32(R, N, 3), f32(R, N, 3)
        self.logits, self.dlogits, self.dx0 = f32(R, N, 13), f32(R, N, 13), f32(R, N, 9)
        self.sgrad = f32(R, N, 3)
        self.pred, self.labels = i32(R, N), i32(R, N)
        self.mask = torch.empty(R, N, device=dev, dtype=torch.uint8)
        self.scal = f32(3, R)                                        # rows: f, smooth, l2
        self.nn_state = i32(R, N, int(neighbour))                    # Smooth term: every colour's neighbours in rank order
        self.hist = f32(CHUNK, 5, R)                                 # one window of history rows: n_correct, n_hits, f, smooth, l2
        self.active = torch.empty(R, device=dev, dtype=torch.uint8)
        self.exit, self.n_mask = i32(R), i32(R)
        self.restart_l2 = f32(R)                                     # psg_nu_restart_rooms: sum((x - x_orig)^2), channels 0:3 and 6:9
        self.out = f32(R, 9, N)
        self.graph = ctypes.c_void_p()                               # one handle: every full window has the same shape
        _lib.call("psg_nu_graph_create", ctypes.byref(self.graph))

    def __del__(self):
        try:
            if self.graph:
                _lib.load().psg_nu_graph_destroy(self.graph)
        except Exception:
            pass


def _rooms_state(net, dev, R, N, neighbour):
    cache = net.__dict__.setdefault("_psg_gcn_nu_states", {})
    key = (str(dev), R, N, int(neighbour))
    if key not in cache:
        cache[key] = _GcnNuState(dev, R, N, neighbour)
    return cache[key]


def gcn_nu_attack_rooms(atk, images, labels, masks=None, target=None, neighbour=10, targeted_variant=False, trace=None,
                        record=None):
    """R independent ONE-ROOM attacks advanced in lockstep: what `gcn_nu_attack` does when it is called once per room
    (`images[r:r+1]`, `labels[r:r+1]`, `masks[r]`), with one launch per operation for all rooms and the optimiser steps
    enqueued window by window (psg_gcn_nu_window: [0], [1..10], [11..20], ..; full windows are replayed as a hipGraph), with
    one read-back per window of its history rows and exit steps.  The reference's control flow (colper.py:88-95,
    tcolper.py:118-132) sits between windows, per room: a room whose accuracy test fires at step s returns its step-s image
    (the device latch holds the snapshot; what the window ran past s is speculation and is discarded), the learning rate is
    halved with zeroed moments after every 50th step, and after every 10th step the rooms whose cost has not fallen restart
    (psg_nu_restart_rooms; the noise is drawn room by room in ascending order from the device generator; the L2 the clamp
    leaves on the other channels is kept per room).

    The fresh-object semantics of the PointNet `nu_attack_rooms` apply: every room starts from the lr this object holds at
    the call, all rooms halve together (they share the step counter), and `atk.lr` is put back on return - R sequential
    `forward` calls on ONE object would hand each room the previous room's left-over lr, the reference's harness builds a
    new attack object per batch.

    Random numbers.  With R = 1 both generators stand on return exactly where `forward` on that room leaves them: the CPU
    generator has made the draws of the forwards the reference's loop ran (`consume_rng`; what speculative steps consumed
    is given back), the device generator the unused noise of colper.py:93-94 and the restart noise of the steps that ran.
    With R > 1 the CPU generator advances as for the longest-running room, and the device draws of a step are made room by
    room in ascending order.

    images [R, 9, N, 1], labels [R, N], masks [R, N] bool (None for NU_attack).  `trace(step=, cost=, f=, smooth=, l2=
    [R] arrays, w=, m=, v=, x0=, pred= state tensors, active= [R])` (tests) reads back after every step; `record(step,
    row [5, R], extra_l2 [R], was_active [R])` receives every step's history row without changing the windows, and
    `record(step, None, extra_l2, restarting [R])` when rooms restart after `step`.
    Returns (adv [R, 9, N, 1], steps_run [R] int64 numpy: the optimiser steps each room executed)."""
    net = _gcn(atk.model)
    if images.dim() != 4 or images.shape[1] != 9 or images.shape[3] != 1:
        raise ValueError("expected images [R, 9, N, 1], got %s" % (tuple(images.shape),))
    R, _, N, _ = images.shape
    mk = None
    if masks is not None:
        mk = masks.detach().to(torch.bool).cpu().numpy() if isinstance(masks, torch.Tensor) else np.asarray(masks).astype(bool)
        if mk.shape != (R, N):
            raise ValueError("masks must be boolean [%d, %d], got shape %s" % (R, N, mk.shape))
        n_mask = mk.sum(axis=1).astype(np.float64)
        if targeted_variant and (n_mask == 0).any():
            # the reference divides the hits by the mask count (tcolper.py:109): an empty mask raises there too
            raise ZeroDivisionError("tar_NU_attack: rooms %s have an empty mask (tcolper.py:109: division by the mask count)"
                                    % np.nonzero(n_mask == 0)[0].tolist())
    elif targeted_variant:
        raise ValueError("the targeted variant needs one mask per room")
    else:
        n_mask = np.zeros(R)
    dev = atk.device
    lr_at_call = atk.lr
    images = images.detach().to(dev).float()
    st = runtime.stream
    S = _rooms_state(net, dev, R, N, neighbour)
    model, ws = net._packed(), net._workspace(R, N)
    net._generation += 1
    use_target = targeted_variant and target is not None
    mode = 0 if not targeted_variant else (2 if use_target else 1)
    c_f = float(atk.c) if not targeted_variant else 1.0        # colper: c*f + 1e-4*S + L2 ; tcolper: f + 1e-4*S + c*L2
    c_l2 = 1.0 if not targeted_variant else float(atk.c)
    S.labels.copy_(labels.detach().to(dev).to(torch.int32))
    if mk is not None:
        S.mask.copy_(torch.from_numpy(mk.astype(np.uint8)))
    S.n_mask.copy_(torch.from_numpy(n_mask.astype(np.int32)))
    x0, w, m, v = S.x0, S.w, S.m, S.v
    _lib.call("psg_to_point_major", runtime.ptr(images[:, :, :, 0].contiguous()), R, 9, N, runtime.ptr(x0), st())
    S.ori.copy_(x0[:, :, 3:6])
    S.x0_orig.copy_(x0)
    _lib.call("psg_nu_inverse_tanh", runtime.ptr(x0), R, N, runtime.ptr(w), st())
    m.zero_(); v.zero_(); S.scal.zero_()
    S.active.fill_(1); S.exit.fill_(-1)
    extra_l2 = np.zeros(R)      # (adv - images)^2 over the non-colour channels: non-zero only after a restart clamped them
    prev_cost = np.full((atk.steps, R), 1e10)
    lr, adam_t = float(atk.lr), 0
    exited = np.full(R, -1, np.int64)
    noise_every = max(atk.steps // 10, 1)
    win = _lib.GcnNuWindowArgs(
        model=model.handle.value, ws=ws.handle.value, G=R, N=N, mode=mode, use_target=int(use_target),
        target=int(target) if use_target else 0, neighbour=int(neighbour), kappa=float(atk.kappa), tsign=float(atk._targeted),
        c_f=c_f, c_smooth=1e-4, c_l2=c_l2, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, w=w.data_ptr(), m=m.data_ptr(), v=v.data_ptr(),
        mask=S.mask.data_ptr() if mk is not None else None, n_mask=S.n_mask.data_ptr(), x0=x0.data_ptr(), ori=S.ori.data_ptr(),
        labels=S.labels.data_ptr(), logits=S.logits.data_ptr(), dlogits=S.dlogits.data_ptr(), dx0=S.dx0.data_ptr(),
        sgrad=S.sgrad.data_ptr(), pred=S.pred.data_ptr(), scal=S.scal.data_ptr(), nn_state=S.nn_state.data_ptr(),
        hist=S.hist.data_ptr(), out=S.out.data_ptr(), active=S.active.data_ptr(), exit_step=S.exit.data_ptr())
    rng_after = {}              # CPU generator after the forward of step s: what speculative steps drew is given back
    step = 0
    try:
        while step < atk.steps:
            window_end = 1 if step == 0 else ((step - 1) // CHUNK + 1) * CHUNK + 1          # [0], [1..10], [11..20], ..
            n_run = 1 if trace is not None else min(atk.steps, window_end) - step
            for s_i in range(step, step + n_run):        # one stochastic-graph draw set per forward (torch_edge.py:21)
                net.consume_rng(1)
                rng_after[s_i] = torch.get_rng_state()
            win.step0, win.n_steps, win.adam_t0, win.lr = step, n_run, adam_t, lr
            ws.nu_window(win, S.graph if n_run == CHUNK else None)
            adam_t += n_run
            last = step + n_run - 1
            # ---- the reference's control flow, per room, where the reference's host work needs the values (ONE read-back)
            got = torch.cat([S.hist[:n_run].reshape(-1), S.exit.float()]).cpu().numpy().astype(np.float64)
            hrows, exited = got[:-R].reshape(n_run, 5, R), got[-R:].astype(np.int64)
            for s_i in range(step, last + 1):
                was_active = (exited < 0) | (exited >= s_i)              # rooms whose loop was still running at step s_i
                f_loss, sm_loss = hrows[s_i - step, 2], hrows[s_i - step, 3]
                l2_loss = hrows[s_i - step, 4] + extra_l2
                cost = c_f * f_loss + 1e-4 * sm_loss + c_l2 * l2_loss
                prev_cost[s_i] = np.where(was_active, cost, prev_cost[s_i])
                if trace is not None:
                    trace(step=s_i, cost=cost, f=f_loss, smooth=sm_loss, l2=l2_loss, w=w, m=m, v=v, x0=x0, pred=S.pred,
                          active=was_active.copy())
                if record is not None:
                    record(s_i, hrows[s_i - step].copy(), extra_l2.copy(), was_active.copy())
                if not targeted_variant and s_i % noise_every == 0:     # colper.py:90-94: noise drawn, never used
                    for _ in np.nonzero((exited < 0) | (exited > s_i))[0]:
                        torch.empty(1, 9, N, 1, device=dev).uniform_(0, 0.01)
            step = last + 1
            active = exited < 0                          # after this window's exits (colper.py:88-89, tcolper.py:118-123)
            if not active.any():
                break
            if not targeted_variant:
                continue
            if last > 0 and last % 50 == 0:              # tcolper.py:125-127: halve lr, NEW optimiser (moments reset)
                atk.lr = atk.lr / 2
                lr, adam_t = float(atk.lr), 0
                m.zero_()
                v.zero_()
            if last > 10 and last % 10 == 0:             # tcolper.py:129-132, room by room
                again = np.nonzero(active & (cost >= prev_cost[last - 10]))[0]
                if len(again):
                    if record is not None:
                        record(last, None, extra_l2.copy(), np.isin(np.arange(R), again))
                    _pointnet_restart(S, x0, again, n_mask, R, 1, N, dev, extra_l2)
    finally:
        atk.lr = lr_at_call
    steps_run = np.where(exited >= 0, exited + 1, step).astype(np.int64)
    if step:
        torch.set_rng_state(rng_after[int(steps_run.max()) - 1])        # as for the longest-running room
    out = S.out.clone()                                  # (the caller owns what it gets; the state buffer is reused)
    for r in np.nonzero(exited < 0)[0]:                  # rooms that ran to the cap: the current image
        _lib.call("psg_to_channel_major", runtime.ptr(x0[r:r + 1]), 1, 9, N, runtime.ptr(out[r:r + 1]), st())
    return out.unsqueeze(-1), steps_run
