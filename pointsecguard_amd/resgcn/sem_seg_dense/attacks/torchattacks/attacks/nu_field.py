"""Host loop of the ResGCN NU attacks on the COORDINATE field (NU_attack / tar_NU_attack with field="coord" | "both"): an
extension of the reference API (the reference ships the colour half, nu.py), DESIGN section 5o.

Rooms form only: G independent one-room attacks advanced together (G >= 1); `forward` takes one room.  The variable is
delta [G][N][3] in metres, optimised directly by Adam (no tanh space: coordinates have no box), zero at the start;
xyz = ori_xyz + delta on masked points of active rooms; channels 6:9 stay as given.

  NU_attack      cost = c f + 1e-4 Smooth_xyz + L2_xyz                  (+ 1e-4 Smooth + L2 on colours with "both")
  tar_NU_attack  cost = f + 1e-4 Smooth_xyz + coord_c L2_xyz            (+ 1e-4 Smooth + c L2 on colours with "both")
  gradient into Adam on delta = dx0[0:3] + 2 c_l2x delta + c_sx sgrad_xyz, step size coord_lr (default lr)

Smooth_xyz is this network's own Smooth (colper.py:115-120) on channels 0:3: every point against the `neighbour` nearest
points of its own MOVED room, itself included, gradient through both ends of every pair (psg_smooth_knn_xyz_sym_rooms);
L2_xyz = sum delta^2.  The kNN graphs of the network are constants of the derivative, so dx0[0:3] is exact.

The optimiser steps run in device-side windows (psg_gcn_nu_field_window): [0], [1..10], [11..20], ..; full windows are
replayed as a hipGraph - this network has no FPS plan and draws nothing inside a step.  Exits are read back after step 0 and
then once per window; the exit snapshot carries the moved coordinates and lags the optimiser by one step.  tar_NU_attack
halves both learning rates and zeroes all moments every 50 steps (a window boundary).

NO RESTART and no restart draws: tcolper.py:128-131 clamps all nine channels to the colour box, which would wipe delta (and
the room); the restart of colper.py:92-95 writes a dead variable.  The CPU generator advances by one stochastic-graph draw
set per forward that the reference's loop would have run; the device generator is not touched.
"""
import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks.nu_windows import RoomsState, _bind, room_masks, window_loop
from pointsecguard_amd.attacks.torchattacks.attacks._common import check_field
from pointsecguard_amd.attacks.torchattacks.attacks.nu import ADAM_EPS, BETA1, BETA2

from .colper import FIELD_CODES, _gcn
from .nu import CHUNK


class _GcnFieldState(RoomsState):
    """RoomsState of G rooms with the coordinate variable and this network's scratch; one graph handle: every full window has
    the same shape."""

    def __init__(self, dev, G, N, neighbour):
        super().__init__(dev, G, 1, N, neighbour, n_scal=5, n_graphs=1)      # scal rows: f, Smooth, L2, Smooth_xyz, L2_xyz
        f32 = self._f32
        self.ori_xyz, self.sgrad_xyz = f32(G, N, 3), f32(G, N, 3)
        self.delta, self.mx, self.vx = f32(G, N, 3), f32(G, N, 3), f32(G, N, 3)
        self.logits, self.dlogits = f32(G, N, 13), f32(G, N, 13)
        self.nn_xyz = self._i32(G, N, int(neighbour))


def _state(net, dev, G, N, neighbour, field):
    return _GcnFieldState.of(net, "_psg_gcn_nu_field_states", (str(dev), G, N, int(neighbour), field), dev, G, N, neighbour)


def window_args(S, model, ws, G, N, field, mode, use_target, target, neighbour, kappa, tsign, c_f, c_l2, c_l2_xyz, masked):
    """The argument block of psg_gcn_nu_field_window over the buffers of a _GcnFieldState (step0 / n_steps / adam_t0 / lr /
    coord_lr are set per window)."""
    win = _lib.GcnNuFieldWindowArgs(
        model=model.handle.value, ws=ws.handle.value, G=G, N=N, mode=mode, use_target=int(use_target),
        target=int(target) if use_target else 0, neighbour=int(neighbour), field=FIELD_CODES[field], kappa=float(kappa),
        tsign=float(tsign), c_f=c_f, c_smooth=1e-4, c_l2=c_l2, c_smooth_xyz=1e-4, c_l2_xyz=c_l2_xyz, beta1=BETA1, beta2=BETA2,
        eps=ADAM_EPS)
    _bind(win, S, "w m v delta mx vx ori_xyz n_mask x0 ori labels logits dlogits dx0 sgrad sgrad_xyz pred scal nn_state nn_xyz hist "
                  "out active exit_step=exit")
    win.mask = S.mask.data_ptr() if masked else None
    return win


def init_state(S, images, labels, masks, both):
    """Clean rooms into the state: x0 point-major, the clean fields, delta and all moments zero, every room active."""
    G, _, N = images.shape
    st = runtime.stream
    S.labels.copy_(labels.detach().to(S.labels.device).to(torch.int32).reshape(G, N))
    n_mask = np.zeros(G)
    if masks is not None:
        S.mask.copy_(torch.from_numpy(masks.astype(np.uint8)))
        n_mask = masks.sum(axis=1).astype(np.float64)
    S.n_mask.copy_(torch.from_numpy(n_mask.astype(np.int32)))
    _lib.call("psg_to_point_major", runtime.ptr(images), G, 9, N, runtime.ptr(S.x0), st())
    S.ori_xyz.copy_(S.x0[:, :, 0:3])
    S.ori.copy_(S.x0[:, :, 3:6])
    if both:
        _lib.call("psg_nu_inverse_tanh", runtime.ptr(S.x0), G, N, runtime.ptr(S.w), st())
    for t in (S.m, S.v, S.delta, S.mx, S.vx, S.scal):
        t.zero_()
    S.active.fill_(1)
    S.exit.fill_(-1)


def gcn_nu_field_attack_rooms(atk, images, labels, masks=None, target=None, neighbour=10, targeted_variant=False, trace=None,
                              record=None):
    """G one-room attacks in lockstep; images [G, 9, N, 1], labels [G, N], masks [G, N] bool (None: NU_attack).  Returns
    (adv [G, 9, N, 1], optimiser steps run per room [G] int64 numpy).  Every room starts from the learning rates the object
    holds at the call, all rooms halve together, and `atk.lr` / `atk.coord_lr` are put back on return.

    `trace(step=, cost=, f=, smooth=, l2=, smooth_xyz=, l2_xyz=, active=, S=)` (tests) is called after every step - the
    windows are then one step long - with the step's per-room scalars and the state; `record(step, row [7, G], was_active
    [G])` receives every step's history row without changing the windows."""
    field = check_field(atk.field)
    assert field != "color"
    net = _gcn(atk.model)
    if images.dim() != 4 or images.shape[1] != 9 or images.shape[3] != 1:
        raise ValueError("expected images [R, 9, N, 1], got %s" % (tuple(images.shape),))
    G, _, N, _ = images.shape
    mk, _ = room_masks(masks, G, N, targeted_variant, "tcolper.py:109")
    return _field_core(atk, net, images, labels, mk, target, neighbour, targeted_variant, trace, record, field)


def gcn_nu_field_attack(atk, images, labels, mask=None, target=None, neighbour=10, targeted_variant=False):
    """NU_attack.forward / tar_NU_attack.forward with field != "color": one room per call."""
    check_field(atk.field)
    if images.shape[0] != 1:
        raise ValueError("field=%r attacks one room per call (the reference's batch semantics are a colour-path property and are "
                         "not extended); use forward_rooms for %d rooms in lockstep" % (atk.field, images.shape[0]))
    masks = None if mask is None else (mask if isinstance(mask, torch.Tensor) else np.asarray(mask)).reshape(1, -1)
    return gcn_nu_field_attack_rooms(atk, images, labels, masks, target, neighbour, targeted_variant)[0]


def _field_core(atk, net, images, labels, mk, target, neighbour, targeted_variant, trace, record, field):
    dev = atk.device
    images = images.detach().to(dev).float()[:, :, :, 0].contiguous()
    G, _, N = images.shape
    S = _state(net, dev, G, N, neighbour, field)
    model, ws = net._packed(), net._workspace(G, N)
    net._generation += 1
    both = field == "both"
    use_target = targeted_variant and target is not None
    mode = 0 if not targeted_variant else (2 if use_target else 1)
    c_f = float(atk.c) if not targeted_variant else 1.0          # colper: c*f + 1e-4*S + L2 ; tcolper: f + 1e-4*S + c*L2
    c_l2 = 1.0 if not targeted_variant else float(atk.c)
    coord_c = getattr(atk, "coord_c", None)
    c_l2_xyz = 1.0 if not targeted_variant else float(atk.c if coord_c is None else coord_c)
    init_state(S, images, labels, mk, both)
    win = window_args(S, model, ws, G, N, field, mode, use_target, target, neighbour, atk.kappa, atk._targeted, c_f, c_l2, c_l2_xyz,
                      mk is not None)
    rng_after = {}              # CPU generator after the forward of step s: what speculative steps drew is given back

    def enqueue(step, n_run, adam_t):
        for s_i in range(step, step + n_run):            # one stochastic-graph draw set per forward (torch_edge.py:21)
            net.consume_rng(1)
            rng_after[s_i] = torch.get_rng_state()
        lr = float(atk.lr)
        win.step0, win.n_steps, win.adam_t0 = step, n_run, adam_t
        win.lr, win.coord_lr = lr, lr if atk.coord_lr is None else float(atk.coord_lr)
        ws.nu_field_window(win, S.graph if n_run == CHUNK else None)

    def on_step(s_i, row, was_active, exited):
        if trace is not None:
            cost = c_f * row[2] + 1e-4 * row[5] + c_l2_xyz * row[6] + (1e-4 * row[3] + c_l2 * row[4] if both else 0.0)
            trace(step=s_i, cost=cost, f=row[2], smooth=row[3], l2=row[4], smooth_xyz=row[5], l2_xyz=row[6],
                  active=was_active.copy(), S=S)
        if record is not None:
            record(s_i, row.copy(), was_active.copy())

    out, steps_run, step = window_loop(atk, S, 1, enqueue, targeted_variant=targeted_variant,
                                       on_step=on_step if trace is not None or record is not None else None,
                                       one_step=trace is not None, lr_names=("lr", "coord_lr"), moments=(S.m, S.v, S.mx, S.vx))
    if step:
        torch.set_rng_state(rng_after[int(steps_run.max()) - 1])        # as for the longest-running room
    return out.unsqueeze(-1), steps_run
