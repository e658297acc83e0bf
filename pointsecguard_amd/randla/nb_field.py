"""BIM / NBattack and TBIM / tar_NBattack of RandLA-Net on the point positions (`field="coord"`) or on positions and colours
(`"both"`), G clouds in lockstep: DESIGN.md section 5t.  The parents in `attack.py` run these fields one cloud per call, every
iteration driven from the host (`attack._field_iteration`); these subclasses add `batch_attack_clouds`: G clouds on one full
cloud-batch workspace, `chunk` iterations per library call (`psg_rla_bim_field_window`), every iteration rebuilding the index
pyramid of all clouds on the device from the positions the field step just wrote.  The targeted pair reads back once per window
(history rows and exit steps; the `sr > 0.9` exit is taken per cloud on the device, in integers, the exiting iteration's
update still applied); the untargeted pair reads nothing back before the end.  No hipGraph: the window runs eagerly.

`batch_attack` is inherited untouched: the one-cloud host loop, which a G = 1 call here reproduces bit for bit.  `field="color"`
runs the parents' code and returns the parents' bytes.

After a run: `last_adv_xyz` [G, N, 3] the moved positions, `last_dist_xyz` [G] their l_2 distances, `last_adv` [G, N, 3] the
colours (targeted pair; the untargeted one returns them), `last_steps` [G] the gradient steps taken (targeted pair).  The tuples'
`new_dists` stays the colour distance (0.0 under "coord"), as for `batch_attack`.  The state's workspace is left on
`last_adv_xyz`, so a forward on the adversarial features evaluates the attack."""
import numpy as np
import torch

from pointsecguard_amd import _lib
from pointsecguard_amd.randla import attack, network

CHUNK = attack.CHUNK
_FIELD_CODE = {"coord": 1, "both": 2}        # PSG_NU_FIELD_COORD / PSG_NU_FIELD_BOTH of include/psg.h


class _FieldCloudsState:
    """Device buffers of G clouds of N points attacked in lockstep on the coordinate field, and their full workspace."""

    def __init__(self, n, G):
        self.ws = network.RandLAWorkspace(n, batch=G, full=True)
        dev = self.ws.device
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
        R = G * n
        self.feat, self.dfeat = f32(R, 6), f32(R, 6)
        self.logits, self.dlogits = f32(R, 13), f32(R, 13)
        self.xs, self.ori_xyz, self.xyz, self.dxyz = f32(R, 3), f32(R, 3), f32(R, 3), f32(R, 3)
        self.delta = f32(R, 3)                               # scratch of the field step, then of the colour step
        self.norms, self.norms_xyz = f32(2, G), f32(2, G)
        self.labels, self.ys, self.hit_ys, self.pred, self.out_pred = i32(R), i32(R), i32(R), i32(R), i32(R)
        self.mask = torch.zeros(R, dtype=torch.uint8, device=dev)
        self.n_mask = i32(G)
        self.scratch = i32(G, 2 * _lib.RLA_NU_PARTS + 1)
        self.hist = f32(CHUNK, G, 3)
        self.out_adv, self.out_adv_xyz, self.out_stats = f32(R, 3), f32(R, 3), f32(G, 3)
        self.active, self.leaving = (torch.zeros(G, dtype=torch.uint8, device=dev) for _ in range(2))
        self.exit = i32(G)


class _NbField:
    """What the four classes share: the checks, the per-shape state, the lockstep loop."""

    chunk = CHUNK           # iterations per window (tests shorten it; at most CHUNK)
    window_hook = None      # targeted pair: called after every window's read-back (first iteration, iterations, final, state, rows)

    def _check(self, features, labels):
        """features [G, N, 6] and labels [G, N] on the host side, the settings: every refusal before any device work
        -> (f, lab int32 [G, N], G, n)"""
        if self.eps is None or self.alpha is None or self.iteration is None:
            raise ValueError("call config(magnitude=..., alpha=..., iteration=...) first")
        if self.iteration < 1:
            raise ValueError("iteration must be positive")
        f = attack._features(features, clouds=True, device=False)
        G, n = int(f.shape[0]), int(f.shape[1])
        lab = attack._labels(labels, np.int32)
        if lab.shape != (G, n):
            raise ValueError("labels must be [G, N] = %s, got %s" % ((G, n), lab.shape))
        return f, lab, G, n

    def _run_field(self, f, G, n, lab, mode, loss_ys=None, hit_ys=None, mask_h=None, sign=1.0):
        """The lockstep loop on the checked inputs -> (the state, the clean prediction [G, N]); sets last_adv, last_adv_xyz,
        last_dist_xyz and (mode 1) last_steps; leaves the workspace on the moved positions."""
        clouds = self.__dict__.setdefault("_field_clouds", {})
        if (n, G) not in clouds:
            clouds[(n, G)] = _FieldCloudsState(n, G)
        S, both = clouds[(n, G)], self.field == "both"
        S.feat.copy_(f.float().reshape(G * n, 6))
        S.xs.copy_(S.feat[:, 3:6])
        S.ori_xyz.copy_(S.feat[:, 0:3])
        S.xyz.copy_(S.ori_xyz)
        pred0 = None
        if mode:                                             # the clean prediction of the tuples (the window builds its own pyramids)
            S.ws.set_cloud(S.ori_xyz)
            pred0 = S.ws.forward(self.model, S.feat).argmax(1).cpu().numpy().reshape(G, n)
        S.labels.copy_(torch.from_numpy(np.ascontiguousarray(lab.reshape(-1))))
        if mode:
            S.ys.copy_(torch.from_numpy(np.ascontiguousarray(loss_ys, np.int32).reshape(-1)))
            S.hit_ys.copy_(torch.from_numpy(np.ascontiguousarray(hit_ys, np.int32).reshape(-1)))
            S.mask.copy_(torch.from_numpy(mask_h.astype(np.uint8).reshape(-1)))
            S.n_mask.copy_(torch.from_numpy(mask_h.sum(1).astype(np.int32)))
        for t in (S.norms, S.norms_xyz, S.out_stats, S.out_adv, S.out_adv_xyz, S.out_pred, S.leaving):
            t.zero_()
        S.active.fill_(1)
        S.exit.fill_(-1)
        win = _lib.RlaBimFieldWindowArgs()
        win.model, win.ws = self.model.handle, S.ws.handle
        win.G, win.N, win.l2_metric = G, n, 1 if self.distance_metric == "l_2" else 0
        win.mode, win.field = mode, _FIELD_CODE[self.field]
        win.num, win.den = (int(self.EXIT_RATIO[0]), int(self.EXIT_RATIO[1])) if mode else (0, 1)
        win.eps, win.alpha, win.sign = self.eps, self.alpha, sign
        win.coord_eps = self.eps if self.coord_eps is None else self.coord_eps
        win.coord_alpha = self.alpha if self.coord_alpha is None else self.coord_alpha
        attack._bind(win, S, "labels feat logits dlogits dfeat norms_xyz delta pred scratch out_adv out_adv_xyz out_pred out_stats active "
                             "ori_xyz xyz dxyz")
        if both:
            attack._bind(win, S, "ori=xs norms")
        if mode:
            attack._bind(win, S, "mask n_mask hit_ys loss_ys=ys hist leaving exit_step=exit")

        def set_window(it0, n_run, final):               # final, the cap: its last step snapshots the clouds still running
            win.n_steps, win.it0, win.final = n_run, it0, 1 if final else 0
            return n_run

        # iterations 0 .. iteration; the targeted pair (mode 1) reads back once per window, the untargeted pair nothing
        _, steps = attack._run_windows("psg_rla_bim_field_window", win, S, 0, self.iteration, self.chunk, set_window, self.window_hook,
                                       read_back=bool(mode))
        if mode:
            self.last_steps = steps
        self.last_adv = S.out_adv.reshape(G, n, 3).clone()
        self.last_adv_xyz = S.out_adv_xyz.reshape(G, n, 3).clone()
        ori_xyz = S.ori_xyz.reshape(G, n, 3)
        # per cloud, the reduction attack._field_finish makes
        self.last_dist_xyz = torch.stack([torch.linalg.vector_norm(self.last_adv_xyz[g] - ori_xyz[g]) for g in range(G)]).cpu().numpy()
        S.ws.set_cloud(S.out_adv_xyz)
        return S, pred0


class _BimField(_NbField):
    """The untargeted pair's lockstep form."""

    def batch_attack_clouds(self, features, labels):
        """features [G, N, 6], labels [G, N] -> adversarial rgb [G, N, 3] after `iteration + 1` updates (bim.py:204-232: one
        before the loop); every cloud takes every step.  Raises ValueError, before any device work, on unset config, bad shapes
        or iteration < 1."""
        f, lab, G, n = self._check(features, labels)
        if self.field == "color":
            cache = self.__dict__.setdefault("_color_clouds", {})
            if G not in cache:
                cache[G] = attack.BIM(self.model, batch_size=G, distance_metric=self.distance_metric)
            cache[G].eps, cache[G].alpha, cache[G].iteration = self.eps, self.alpha, self.iteration
            return cache[G].batch_attack(f, lab).reshape(G, n, 3) if G > 1 else cache[G].batch_attack(f[0], lab[0])[None]
        self._run_field(f, G, n, lab, 0)
        return self.last_adv


class _TbimField(_NbField):
    """The targeted pair's lockstep form."""

    def batch_attack_clouds(self, features, labels, target=None, ori=2):
        """features [G, N, 6], labels [G, N] -> a list of G tuples (target_points, sr, other_acc, original_other_accuracy,
        new_dists, other_mIoU, original_other_mIoU), the fields `batch_attack` returns.  Every cloud has its own exit; like
        there, the update of the exiting iteration is still applied: `last_adv_xyz` / `last_adv` hold the positions and colours
        after it, the tuple the prediction before it.  Raises ValueError, before any device work, on unset config, bad shapes,
        iteration < 1, a missing target or a cloud without a point of `ori`."""
        if self.field == "color":
            return super().batch_attack_clouds(features, labels, target, ori)
        f, lab, G, n = self._check(features, labels)
        if target is None:
            raise ValueError("target: the class the points of class `ori` are pushed to")
        mask_h = attack._origin_points(lab, ori, "311-314")
        ys_target = np.where(mask_h, target, lab).astype(np.int32)
        targeted = self.goal in ("t", "tm")
        S, pred0 = self._run_field(f, G, n, lab, 1, ys_target if targeted else lab, ys_target, mask_h, -1.0 if targeted else 1.0)
        pred = S.out_pred.cpu().numpy().reshape(G, n)
        ori_rgb = S.xs.reshape(G, n, 3)
        return [attack._targeted_out(self.logger, pred[g], pred0[g], lab[g], ys_target[g], mask_h[g],
                                     float(torch.linalg.vector_norm(self.last_adv[g] - ori_rgb[g]))) for g in range(G)]


class BIMField(_BimField, attack.BIM):
    """attack.BIM (field "coord" by default) with the lockstep `batch_attack_clouds`."""

    def __init__(self, model, batch_size=1, loss="colper", goal="ut", distance_metric="l_inf", session=None, iteration_callback=None,
                 field="coord"):
        attack.BIM.__init__(self, model, batch_size, loss, goal, distance_metric, session, iteration_callback, field)


class NBattackField(_BimField, attack.NBattack):
    """attack.NBattack (field "coord" by default) with the lockstep `batch_attack_clouds`."""

    def __init__(self, model, batch_size=1, loss="colper", goal="ut", distance_metric="l_2", session=None, iteration_callback=None,
                 field="coord"):
        attack.NBattack.__init__(self, model, batch_size, loss, goal, distance_metric, session, iteration_callback, field)


class TBIMField(_TbimField, attack.TBIM):
    """attack.TBIM (field "coord" by default) with `batch_attack_clouds` on the coordinate field."""

    def __init__(self, model, batch_size=1, loss="colper", goal="t", distance_metric="l_2", session=None, iteration_callback=None,
                 field="coord"):
        attack.TBIM.__init__(self, model, batch_size, loss, goal, distance_metric, session, iteration_callback, field)


class tar_NBattackField(_TbimField, attack.tar_NBattack):
    """attack.tar_NBattack (field "coord" by default) with `batch_attack_clouds` on the coordinate field."""

    def __init__(self, model, batch_size=1, loss="colper", goal="t", distance_metric="l_2", session=None, iteration_callback=None,
                 field="coord"):
        attack.tar_NBattack.__init__(self, model, batch_size, loss, goal, distance_metric, session, iteration_callback, field)
