"""Host loop of the NU attacks on the COORDINATE field (NU_attack / tar_NU_attack with field="coord" | "both") of the
PointNet++ SSG network: an extension of the reference API (the reference ships the colour half, nu.py), DESIGN section 5l.

Rooms form only: G independent one-room attacks advanced together (G >= 1) - how the real protocol calls tar_NU_attack,
with batches of one.  The batch quirks of the colour path (Smooth term and mask of batch row 0) are not extended.

The variable is delta [G][N][3] in metres, optimised directly by Adam (no tanh space: coordinates have no box), zero at the
start; xyz = ori_xyz + delta on masked points of active rooms; channels 6:9 stay as given, as in the NB coordinate attack.
Per step, one psg_pn2_nu_field_step call: delta applied to x0 (both: + the colours from w), geometry plan rebuilt from the
moved points (four FPS draws per room and step from the CPU generator in forward order; `starts_fn(step, 1)` supplies them
in tests), forward, f-loss gradient, the exact coordinate backward, the Smooth term(s), the Adam step(s), the exit latch.
  cost = f + c (Smooth_rgb + L2_rgb) + coord_c (Smooth_xyz + L2_xyz)        (the colour terms with "both" only)
  gradient into Adam on delta = dx0[0:3] + 2 coord_c delta + coord_c sgrad_xyz,  step size coord_lr
Smooth_xyz is the reference's Smooth (nontarget.py:131-135) on channels 0:3 against the room's ORIGINAL points, evaluated on
direct differences (psg_smooth_knn_xyz_rooms); neighbour = 10 (NU_attack) / 5 (tar_NU_attack), as for colours.

Exits are the reference's tests through the unchanged latch: the exit snapshot carries the moved coordinates and lags the
optimiser by one step.  The history is read back after step 0 and then after every 10th step ([0], [1..10], [11..20], ..;
the FPS draws of a window are made together); what ran after an attack's exit is discarded.  With `trace` / `record` every
step is read back.  tar_NU_attack keeps halving the learning rate(s) with a fresh optimiser (all moments zeroed) every 50
steps.

NO RESTART: the restart of target.py:127-132 is uniform [0, 1] noise on the colours followed by a clamp of ALL nine
channels to the colour box; it has no coordinate counterpart and would wipe the perturbation (and the room), so
field != "color" never applies it.
"""
import ctypes

import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks.nu_windows import RoomsState, _bind, room_masks, window_loop
from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts, upload

from ._common import check_field, labels_to_device, psg_model
from .nu import ADAM_EPS, BETA1, BETA2
from .pointnet import is_pointnet

FIELD_CODES = {"coord": 1, "both": 2}          # PSG_NU_FIELD_COORD / PSG_NU_FIELD_BOTH of include/psg.h


class _FieldState(RoomsState):
    """RoomsState of G rooms with the coordinate variable; no graph handle: the plan is rebuilt by every step."""

    def __init__(self, dev, G, N, neighbour):
        super().__init__(dev, G, 1, N, neighbour, n_scal=5, n_graphs=0)     # scal rows: f, Smooth_rgb, L2_rgb, Smooth_xyz, L2_xyz
        f32 = self._f32
        self.ori_xyz, self.sgrad_xyz = f32(G, N, 3), f32(G, N, 3)
        self.delta, self.m_xyz, self.v_xyz = f32(G, N, 3), f32(G, N, 3), f32(G, N, 3)
        self.logp, self.dlogp = f32(G, N, 13), f32(G, N, 13)


def _state(net, dev, G, N, neighbour):
    return _FieldState.of(net, "_psg_nu_field_states", (str(dev), G, N, int(neighbour)), dev, G, N, neighbour)


def check_network(model, field):
    """field != "color" runs on the PointNet++ SSG network only (psg_pn2_backward_full)."""
    if is_pointnet(model) or getattr(model, "ARCH", runtime.ARCH_SSG) != runtime.ARCH_SSG:
        raise NotImplementedError("field=%r is implemented for the PointNet++ SSG network" % field)
    return psg_model(model)


def nu_field_attack_rooms(atk, images, labels, masks, target, neighbour, targeted_variant=False, trace=None, starts_fn=None,
                          record=None):
    """G one-room attacks in lockstep; images [G, 9, N], labels [G, N], masks [G, N] bool (None: NU_attack).  Returns
    (adv [G, 9, N], optimiser steps run per room [G] int64 numpy).  Every room starts from the learning rates the object
    holds at the call, all rooms halve together, and `atk.lr` / `atk.coord_lr` are put back on return (nu.nu_attack_rooms).

    `trace(step=, cost=, f=, smooth=, l2=, smooth_xyz=, l2_xyz=, active=, S=)` (tests) is called after every step with the
    step's per-room scalars and the state buffers; `record(step, row [7, G], was_active [G])` likewise."""
    field = check_field(atk.field)
    assert field != "color"
    net = check_network(atk.model, field)
    G, C, N = images.shape
    if C != 9:
        raise ValueError("images must be [rooms, 9, points], got %s" % (tuple(images.shape),))
    if N % 64:
        raise ValueError("the lockstep f-loss sums need a point count that is a multiple of 64, got %d" % N)
    mk, n_mask = room_masks(masks, G, N, targeted_variant, "target.py:104")
    return _field_core(atk, net, images, labels, mk, n_mask, target, neighbour, targeted_variant, trace, starts_fn, record, field)


def nu_field_attack(atk, images, labels, mask, target, neighbour, targeted_variant=False, trace=None, starts_fn=None):
    """NU_attack.forward / tar_NU_attack.forward with field != "color": one room per call (the protocol's batches of one)."""
    check_network(atk.model, check_field(atk.field))
    if images.shape[0] != 1:
        raise ValueError("field=%r attacks one room per call (the reference's batch semantics are a colour-path property and are "
                         "not extended); use forward_rooms for %d rooms in lockstep" % (atk.field, images.shape[0]))
    masks = None if mask is None else (mask if isinstance(mask, torch.Tensor) else np.asarray(mask))[None]
    return nu_field_attack_rooms(atk, images, labels, masks, target, neighbour, targeted_variant, trace, starts_fn)[0]


def _field_core(atk, net, images, labels, masks, n_mask, target, neighbour, targeted_variant, trace, starts_fn, record, field):
    dev = atk.device
    images = images.detach().to(dev).float().contiguous()
    G, _, N = images.shape
    st = runtime.stream
    S = _state(net, dev, G, N, neighbour)
    model = net._packed()
    net._generation += 1
    ws = net._workspace(G, N, 1)                                     # one plan slot, rebuilt by every step
    both = field == "both"
    use_target = targeted_variant and target is not None
    mode = 0 if not targeted_variant else (2 if use_target else 1)
    S.labels.copy_(labels_to_device(labels, dev).reshape(G, N))
    if masks is not None:
        S.mask.copy_(torch.from_numpy(masks.astype(np.uint8)))
    S.n_mask.copy_(torch.from_numpy(n_mask.astype(np.int32)))
    _lib.call("psg_to_point_major", runtime.ptr(images), G, 9, N, runtime.ptr(S.x0), st())
    S.ori_xyz.copy_(S.x0[:, :, 0:3])
    S.ori.copy_(S.x0[:, :, 3:6])
    if both:
        _lib.call("psg_nu_inverse_tanh", runtime.ptr(S.x0), G, N, runtime.ptr(S.w), st())
    for t in (S.m, S.v, S.delta, S.m_xyz, S.v_xyz, S.scal):
        t.zero_()
    S.active.fill_(1)
    S.exit.fill_(-1)
    c, coord_c = float(atk.c), float(atk.c if atk.coord_c is None else atk.coord_c)
    a = _lib.NuFieldArgs(
        model=model.handle.value, ws=ws.handle.value, G=G, N=N, mode=mode, use_target=int(use_target),
        target=int(target) if use_target else 0, neighbour=int(neighbour), field=FIELD_CODES[field], kappa=float(atk.kappa),
        tsign=float(atk._targeted), c=c, coord_c=coord_c, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS)
    _bind(a, S, "w m v delta m_xyz v_xyz ori_xyz n_mask x0 ori labels logp dlogp dx0 sgrad sgrad_xyz pred scal nn_state out active "
                "exit_step=exit")
    a.mask = S.mask.data_ptr() if masks is not None else None

    def enqueue(step, n_run, adam_t):
        # the FPS draws of a window are made together; then one psg_pn2_nu_field_step call per step (the plan follows the points)
        if starts_fn is not None:
            starts = upload(torch.cat([torch.as_tensor(starts_fn(step + i, 1), dtype=torch.int32).reshape(1, 4, G) for i in range(n_run)]), dev)
        else:
            starts = upload(draw_fps_starts(G, N, n_run), dev)
        a.lr = float(atk.lr)
        a.coord_lr = a.lr if atk.coord_lr is None else float(atk.coord_lr)
        for i in range(n_run):
            a.step, a.adam_t, a.warm = step + i, adam_t + i + 1, 1 if step + i > 0 else 0
            a.starts = starts.data_ptr() + 4 * 4 * G * i
            a.hist = S.hist.data_ptr() + 4 * 7 * G * i
            _lib.call("psg_pn2_nu_field_step", ctypes.byref(a), st())

    def on_step(s_i, row, was_active, exited):
        if trace is not None:
            cost = row[2] + c * (row[3] + row[4]) + coord_c * (row[5] + row[6])
            trace(step=s_i, cost=cost, f=row[2], smooth=row[3], l2=row[4], smooth_xyz=row[5], l2_xyz=row[6],
                  active=was_active.copy(), S=S)
        if record is not None:
            record(s_i, row.copy(), was_active.copy())

    every_step = trace is not None or record is not None             # (here `record` shortens the windows too)
    out, steps_run, _ = window_loop(atk, S, 1, enqueue, targeted_variant=targeted_variant, on_step=on_step if every_step else None,
                                    one_step=every_step, lr_names=("lr", "coord_lr"), moments=(S.m, S.v, S.m_xyz, S.v_xyz))
    return out, steps_run
