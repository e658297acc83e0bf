"""Host loop of the ResGCN NU attacks over the libpsg kernels.

Reference: ResGCN/sem_seg_dense/attacks/torchattacks/attacks/colper.py:42-120 (NU_attack) and tcolper.py:51-170
(tar_NU_attack).  Differences from the PointNet variants that are reproduced here: the f-loss works on raw
logits with the reference's one-hot masking (a 0 takes part in every max); cost = c*f + 1e-4*Smooth + L2
(NU) / f + 1e-4*Smooth + c*L2 (tar_NU); Smooth compares the adversarial colours with THEMSELVES
(smooth(adv_images, images) ignores its second argument: colper.py:115-117), so its gradient flows through both
sides of every neighbour pair; NU_attack draws uniform noise every steps//10 steps without using it.
"""
import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks.nu_windows import CHUNK, RoomsState, _bind, room_masks, to_restart, window_loop
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
class _GcnNuState(RoomsState):
    """RoomsState of R rooms with this network's scratch; one graph handle: every full window has the same shape."""

    def __init__(self, dev, R, N, neighbour):
        super().__init__(dev, R, 1, N, neighbour, n_scal=3, n_graphs=1)      # scal rows: f, smooth, l2
        self.x0_orig = self._f32(R, N, 9)
        self.logits, self.dlogits = self._f32(R, N, 13), self._f32(R, N, 13)
        self.restart_l2 = self._f32(R)                               # psg_nu_restart_rooms: sum((x - x_orig)^2), channels 0:3 and 6:9


def _rooms_state(net, dev, R, N, neighbour):
    return _GcnNuState.of(net, "_psg_gcn_nu_states", (str(dev), R, N, int(neighbour)), dev, R, N, neighbour)


def gcn_nu_attack_rooms(atk, images, labels, masks=None, target=None, neighbour=10, targeted_variant=False, trace=None,
                        record=None):
    """R independent ONE-ROOM attacks advanced in lockstep: what `gcn_nu_attack` does when it is called once per room
    (`images[r:r+1]`, `labels[r:r+1]`, `masks[r]`), with one launch per operation for all rooms and the optimiser steps
    enqueued window by window (psg_gcn_nu_window: [0], [1..10], [11..20], ..; full windows are replayed as a hipGraph), with
    one read-back per window of its history rows and exit steps (nu_windows.window_loop).  The reference's control flow
    (colper.py:88-95, tcolper.py:118-132) sits between windows, per room: a room whose accuracy test fires at step s returns its
    step-s image (the device latch holds the snapshot; what the window ran past s is speculation and is discarded), the
    learning rate is halved with zeroed moments after every 50th step, and after every 10th step the rooms whose cost has not
    fallen restart (psg_nu_restart_rooms; the noise is drawn room by room in ascending order from the device generator; the L2
    the clamp leaves on the other channels is kept per room).

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
    mk, n_mask = room_masks(masks, R, N, targeted_variant, "tcolper.py:109")
    dev = atk.device
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
    cost = None
    noise_every = max(atk.steps // 10, 1)
    win = _lib.GcnNuWindowArgs(
        model=model.handle.value, ws=ws.handle.value, G=R, N=N, mode=mode, use_target=int(use_target),
        target=int(target) if use_target else 0, neighbour=int(neighbour), kappa=float(atk.kappa), tsign=float(atk._targeted),
        c_f=c_f, c_smooth=1e-4, c_l2=c_l2, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS)
    _bind(win, S, "w m v n_mask x0 ori labels logits dlogits dx0 sgrad pred scal nn_state hist out active exit_step=exit")
    win.mask = S.mask.data_ptr() if mk is not None else None
    rng_after = {}              # CPU generator after the forward of step s: what speculative steps drew is given back

    def enqueue(step, n_run, adam_t):
        for s_i in range(step, step + n_run):            # one stochastic-graph draw set per forward (torch_edge.py:21)
            net.consume_rng(1)
            rng_after[s_i] = torch.get_rng_state()
        win.step0, win.n_steps, win.adam_t0, win.lr = step, n_run, adam_t, float(atk.lr)
        ws.nu_window(win, S.graph if n_run == CHUNK else None)

    def on_step(s_i, row, was_active, exited):
        nonlocal cost
        f_loss, sm_loss, l2_loss = row[2], row[3], row[4] + extra_l2
        cost = c_f * f_loss + 1e-4 * sm_loss + c_l2 * l2_loss
        prev_cost[s_i] = np.where(was_active, cost, prev_cost[s_i])
        if trace is not None:
            trace(step=s_i, cost=cost, f=f_loss, smooth=sm_loss, l2=l2_loss, w=w, m=m, v=v, x0=x0, pred=S.pred,
                  active=was_active.copy())
        if record is not None:
            record(s_i, row.copy(), extra_l2.copy(), was_active.copy())
        if not targeted_variant and s_i % noise_every == 0:     # colper.py:90-94: noise drawn, never used
            for _ in np.nonzero((exited < 0) | (exited > s_i))[0]:      # (a room that exits at s_i returns before the draw)
                torch.empty(1, 9, N, 1, device=dev).uniform_(0, 0.01)

    def between(last, step, active):                     # tcolper.py:129-132, room by room
        again = to_restart(last, active, cost, prev_cost)
        if len(again):
            if record is not None:
                record(last, None, extra_l2.copy(), np.isin(np.arange(R), again))
            _pointnet_restart(S, x0, again, n_mask, R, 1, N, dev, extra_l2)

    out, steps_run, step = window_loop(atk, S, 1, enqueue, targeted_variant=targeted_variant, on_step=on_step, between=between,
                                       one_step=trace is not None, moments=(m, v))
    if step:
        torch.set_rng_state(rng_after[int(steps_run.max()) - 1])        # as for the longest-running room
    return out.unsqueeze(-1), steps_run
