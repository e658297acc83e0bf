"""The colour attacks on the vanilla PointNet (pointsecguard_amd.models.pointnet_sem_seg.get_model).

Dispatch is by a class marker (`PSG_NETWORK = "pointnet"`), not by class identity: the reference harness imports the
model module by file name (`importlib.import_module('pointnet_sem_seg')` with models/ on sys.path, INTEGRATION
section 1), which makes a second class object of the same file.

NB_attack / tar_NB_attack: one fused, stream-ordered libpsg call (psg_pointnet_nb_attack), iters x (forward,
CE-on-log-probs gradient, input-gradient backward, sign step + L-inf projection).  This network draws no random
numbers, so unlike the PointNet++ path there are no FPS starts.

NU_attack / tar_NU_attack: the window loop of attacks/nu_windows.py with nu.py's callables (`_nu_core`, shared with
PointNet++: no geometry plan here, the restart is one psg_nu_restart_rooms launch): steps [0], [1..10], [11..20], ..
are one psg_pointnet_nu_window call each, replayed as a hipGraph from the third full window on, with one read-back per
window; `forward` is one attack on the batch (G = 1, rows = B), `forward_rooms` R one-room attacks in lockstep.  The
reference's control flow (PointNet/attacks/torchattacks/attacks/nontarget.py:52-105, target.py:62-133) sits between the
windows: the accuracy exits, and for tar_NU the learning-rate halving with a fresh optimiser every 50 steps and the restart
noise after every 10th step whose cost did not fall (psg_nu_restart_rooms).  This network has no FPS plan, so nothing is
drawn from the CPU generator.

`nu_step` / `nu_attack(trace=...)` below is the per-step host loop over the single entry points (psg_nu_tanh_color,
psg_pointnet_forward, psg_nu_f_loss_grad, psg_pointnet_backward, psg_smooth_knn, psg_nu_adam_step, psg_nu_step_latch) with a
read-back after every step: what a `trace` callback gets, and the checker the window path is tested against.
"""
import ctypes

import numpy as np
import torch

from pointsecguard_amd import _lib, runtime

from ._common import labels_to_device, mask_to_device

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
# The windows run the seam between forward and backward as one kernel (pn_nu_head_kernel); False selects the three-kernel
# sequence instead (log-softmax, f-loss gradient, log-softmax backward): same images, for tools/pointnet_time.py's comparison.
fused_head = True


def is_pointnet(model):
    return getattr(type(model), "PSG_NETWORK", None) == "pointnet"


def nb_attack(atk, images, labels=None, mask=None, target=None):
    net = atk.model
    images = images.detach().to(atk.device).float().contiguous()
    B, C, N = images.shape
    lab = None if target is not None else labels_to_device(labels, atk.device, pin=True)
    m = None if mask is None else mask_to_device(mask, N, atk.device)
    ws = net._workspace(B, N)
    net._generation += 1  # the workspace activations no longer belong to an earlier autograd forward
    return ws.nb_attack(net._packed(), images, lab, atk.eps, atk.alpha, atk.iters, mask=m,
                        target=None if target is None else int(target))


def _off(t, n_floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * n_floats)


class NuState:
    """Device buffers of one NU attack on B rooms of N points (point-major x0 [B][N][9], w / m / v [B][N][3])."""

    def __init__(self, B, N, dev):
        f = dict(device=dev, dtype=torch.float32)
        self.B, self.N = B, N
        self.x0, self.dx0 = torch.empty(B, N, 9, **f), torch.empty(B, N, 9, **f)
        self.w, self.m, self.v = torch.empty(B, N, 3, **f), torch.zeros(B, N, 3, **f), torch.zeros(B, N, 3, **f)
        self.ori = torch.empty(B, N, 3, **f)
        self.dlogp = torch.empty(B, N, runtime.NUM_CLASSES, **f)
        self.sgrad = torch.empty(N, 3, **f)
        self.pred = torch.empty(B, N, device=dev, dtype=torch.int32)
        self.scal = torch.zeros(3, **f)
        self.hist = torch.zeros(5, **f)
        self.out = torch.empty(B, 9, N, **f)
        self.active = torch.ones(1, device=dev, dtype=torch.uint8)
        self.exit = torch.full((1,), -1, device=dev, dtype=torch.int32)


def nu_step(net, S, labels, mask, n_mask, target, mode, kappa, tsign, c, neighbour, lr, adam_t, step):
    """One optimiser step of the reference's loop body on the state S (nontarget.py:70-93, target.py:79-113): colours from
    w, forward, f-loss gradient, input-gradient backward, Smooth term of batch row 0, Adam step, statistics and exit latch.
    Leaves {n_correct, n_hits, f, Smooth, L2} of the step in S.hist."""
    st = runtime.stream
    B, N = S.B, S.N
    model, ws = net._packed(), net._workspace(B, N)
    p = runtime.ptr
    _lib.call("psg_nu_tanh_color", p(S.w), p(mask), B, N, p(S.x0), st())
    logp, _ = ws.forward(model, S.x0)
    use_target = mode == 2
    _lib.call("psg_nu_f_loss_grad", p(logp), None if use_target else p(labels), int(target) if use_target else 0, B * N,
              runtime.NUM_CLASSES, float(kappa), float(tsign), p(S.dlogp), p(S.scal[0:1]), p(S.pred), st())
    ws.backward(model, S.dlogp, None, S.dx0)
    _lib.call("psg_smooth_knn", _off(S.x0, 3), 9, p(S.ori), 3, N, int(neighbour), p(S.scal[1:2]), p(S.sgrad), st())
    _lib.call("psg_nu_adam_step", p(S.w), p(S.m), p(S.v), p(mask), p(S.dx0), p(S.x0), p(S.ori), p(S.sgrad), float(c), float(c),
              float(lr), BETA1, BETA2, ADAM_EPS, int(adam_t), B, N, p(S.scal[2:3]), st())
    _lib.call("psg_nu_step_latch", p(S.pred), p(labels), int(target) if use_target else 0, p(mask) if mode else None,
              p(n_mask) if mode else None, 1, B, N, int(mode), p(S.scal), p(S.hist), p(S.x0), p(S.out), p(S.active), p(S.exit),
              int(step), st())


def nu_attack(atk, images, labels, mask=None, target=None, neighbour=10, targeted_variant=False, trace=None, return_steps=False,
              record=None):
    """NU_attack.forward (targeted_variant=False) / tar_NU_attack.forward on a batch, the reference's call: through the
    windows of nu.py, or with a `trace` callback through the per-step loop below (a read-back after every step)."""
    if trace is None:
        from . import nu
        return nu.nu_attack(atk, images, labels, mask, target, neighbour, targeted_variant=targeted_variant, return_steps=return_steps,
                            record=record)
    net = atk.model
    dev = atk.device
    images = images.detach().to(dev).float().contiguous()
    B, C, N = images.shape
    net._generation += 1
    S = NuState(B, N, dev)
    st = runtime.stream
    labels_d = labels_to_device(labels, dev)
    mask_d = n_mask = mask_b = None
    if mask is not None:
        mask_d = mask_to_device(mask, N, dev)
        mask_b = mask_d.bool()
        k = int(mask_b.sum().item())
        if targeted_variant and k == 0:
            raise ZeroDivisionError("tar_NU_attack: empty mask (target.py:104 divides by the mask count)")
        n_mask = torch.tensor([k], device=dev, dtype=torch.int32)
    elif targeted_variant:
        raise ValueError("tar_NU_attack needs a mask")
    use_target = targeted_variant and target is not None
    mode = 0 if not targeted_variant else (2 if use_target else 1)
    _lib.call("psg_to_point_major", runtime.ptr(images), B, 9, N, runtime.ptr(S.x0), st())
    S.ori.copy_(S.x0[:, :, 3:6])
    x0_orig = S.x0.clone()
    _lib.call("psg_nu_inverse_tanh", runtime.ptr(S.x0), B, N, runtime.ptr(S.w), st())
    lr, adam_t, extra_l2 = float(atk.lr), 0, 0.0
    prev_cost = [1e10] * atk.steps
    c = float(atk.c)
    for step in range(atk.steps):
        adam_t += 1
        nu_step(net, S, labels_d, mask_d, n_mask, target, mode, atk.kappa, atk._targeted, c, neighbour, lr, adam_t, step)
        h = torch.cat([S.hist, S.exit.float()]).cpu().numpy().astype(np.float64)
        cost = h[2] + c * h[3] + c * (h[4] + extra_l2)
        prev_cost[step] = cost
        if trace is not None:
            trace(step=step, cost=cost, f=h[2], smooth=h[3], l2=h[4] + extra_l2, S=S)
        if h[5] >= 0:                                    # the exit test fired: S.out holds this step's image
            return S.out.clone()
        if not targeted_variant:
            continue
        if step > 0 and step % 50 == 0:                  # target.py:123-125: halve lr, new optimiser
            atk.lr = atk.lr / 2
            lr, adam_t = float(atk.lr), 0
            S.m.zero_()
            S.v.zero_()
        if step > 10 and step % 10 == 0 and cost >= prev_cost[step - 10]:     # target.py:127-132
            noise = torch.empty(B, 3, int(n_mask.item()), device=dev, dtype=torch.float32).uniform_(0, 1)
            col = S.x0[:, :, 3:6].transpose(1, 2)
            col[:, :, mask_b] = col[:, :, mask_b] + noise
            S.x0.clamp_(min=0, max=1)                    # ALL channels, like the reference
            d = S.x0 - x0_orig
            extra_l2 = float((d[:, :, 0:3] ** 2).sum().item() + (d[:, :, 6:9] ** 2).sum().item())
    _lib.call("psg_to_channel_major", runtime.ptr(S.x0), B, 9, N, runtime.ptr(S.out), st())
    return S.out.clone()
