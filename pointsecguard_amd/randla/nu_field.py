"""NUattack / tar_NUattack of RandLA-Net on the point positions (`field="coord"`) or on positions and colours (`"both"`):
DESIGN.md section 5s.  `attack.NUattack` / `attack.tar_NUattack` move colours only and refuse the other fields at
construction; these subclasses add them, `field="color"` running the parents' code and returning the parents' bytes.

The optimiser variable of the positions is `delta` [G, N, 3] in metres, optimised directly by Adam (coordinates have no box,
so there is no tanh space); xyz = ori_xyz + delta on the moving points - all of them for NUattackField, the points of class
`ori` for tar_NUattackField.  loss = |xyz - ori_xyz|_2 + cs * hinge, under "both" plus the unchanged colour term with the
colour variable of the parents (its own distance and moments, one `cs`).  There is one loop, the lockstep one: G clouds on
one full cloud-batch workspace, CHUNK steps per library call (`psg_rla_nu_field_window`), every step rebuilding the index
pyramid of all clouds on the device from the positions just written; one read-back per window, the accuracy exits per cloud
on the device in integers.  `batch_attack` is that loop at G = 1.  No hipGraph: the window runs eagerly.

After a run: `last_adv_xyz` [G, N, 3] the moved positions, `last_dist_xyz` [G] their l_2 distances, `last_adv` [G, N, 3] the
colours, `last_steps` [G] the steps taken (`batch_attack`: the two position / colour tensors without the cloud axis).  The
tuples' `new_dists` stays the colour distance (0.0 under "coord"), as for the BIM family."""
import numpy as np
import torch

from pointsecguard_amd import _lib
from pointsecguard_amd.attacks.torchattacks.attacks._common import check_field
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
        self.dws, self.m, self.v, self.xs = f32(R, 3), f32(R, 3), f32(R, 3), f32(R, 3)                  # the colour variable ("both")
        self.delta, self.m_xyz, self.v_xyz, self.ori_xyz = f32(R, 3), f32(R, 3), f32(R, 3), f32(R, 3)
        self.xyz, self.dxyz = f32(R, 3), f32(R, 3)
        self.feat, self.dfeat = f32(R, 6), f32(R, 6)
        self.logits, self.dlogits = f32(R, 13), f32(R, 13)
        self.labels, self.ys, self.pred, self.out_pred = i32(R), i32(R), i32(R), i32(R)
        self.mask = torch.zeros(R, dtype=torch.uint8, device=dev)
        self.n_mask = i32(G)
        self.dist2, self.dist2_xyz, self.out_stats = f32(G), f32(G), f32(G, 4)
        self.out_adv, self.out_adv_xyz = f32(R, 3), f32(R, 3)
        self.partials, self.partials_xyz = (torch.zeros(G, _lib.RLA_NU_PARTS, dtype=torch.float64, device=dev) for _ in range(2))
        self.scratch = i32(G, 2 * _lib.RLA_NU_PARTS + 1)
        self.hist = f32(CHUNK + 1, G, 4)
        self.active = torch.zeros(G, dtype=torch.uint8, device=dev)
        self.exit = i32(G)


class _NuField:
    """What the two classes share: the field settings, the per-shape state, the lockstep loop."""

    def _init_field(self, field, coord_learning_rate):
        self.field = field
        self.coord_lr = self.lr if coord_learning_rate is None else float(coord_learning_rate)
        self._field_clouds = {}

    def _check(self, features, lab):
        """features [G, N, 6] and labels [G, N] on the host side: every refusal before any device work -> (f, G, n)"""
        f = attack._features(features, clouds=True, device=False)
        G, n = int(f.shape[0]), int(f.shape[1])
        if tuple(lab.shape) != (G, n):
            raise ValueError("labels must be [G, N] = %s, got %s" % ((G, n), tuple(lab.shape)))
        if self.iteration < 1:
            raise ValueError("iteration must be positive")
        return f, G, n

    def _run_field(self, f, G, n, lab, ys_h, mask_h):
        """The lockstep loop on the checked inputs.  -> the state, pred0 [G, N], the snapshot's pred [G, N] and
        {n_correct, n_hits, dist2_rgb, dist2_xyz} [G, 4]."""
        if (n, G) not in self._field_clouds:
            self._field_clouds[(n, G)] = _FieldCloudsState(n, G)
        S, both = self._field_clouds[(n, G)], self.field == "both"
        S.feat.copy_(f.float().reshape(G * n, 6))
        S.xs.copy_(S.feat[:, 3:6])
        S.ori_xyz.copy_(S.feat[:, 0:3])
        S.ws.set_cloud(S.ori_xyz)
        pred0 = S.ws.forward(self.model, S.feat).argmax(1).cpu().numpy().reshape(G, n)
        S.labels.copy_(torch.from_numpy(np.ascontiguousarray(lab, np.int32).reshape(-1)))
        S.ys.copy_(torch.from_numpy(np.ascontiguousarray(ys_h, np.int32).reshape(-1)))
        if mask_h is not None:
            S.mask.copy_(torch.from_numpy(np.ascontiguousarray(mask_h, np.uint8).reshape(-1)))
            S.n_mask.copy_(torch.from_numpy(mask_h.reshape(G, n).sum(1).astype(np.int32)))
        for t in (S.dws, S.m, S.v, S.delta, S.m_xyz, S.v_xyz, S.dist2, S.dist2_xyz, S.out_stats, S.out_adv, S.out_adv_xyz, S.out_pred):
            t.zero_()
        S.active.fill_(1)
        S.exit.fill_(-1)
        win = _lib.RlaNuFieldWindowArgs()
        win.model, win.ws = self.model.handle, S.ws.handle
        win.G, win.N, win.mode, win.field = G, n, self.EXIT_MODE, _FIELD_CODE[self.field]
        win.num, win.den = int(self.EXIT_RATIO[0]), int(self.EXIT_RATIO[1])
        win.cs, win.lr, win.coord_lr = self.cs, self.lr, self.coord_lr
        attack._bind(win, S, "delta m_xyz v_xyz ori_xyz xyz dxyz labels ys feat logits dlogits dfeat dist2_xyz partials_xyz pred scratch "
                             "hist out_adv out_adv_xyz out_pred out_stats active exit_step=exit")
        if both:
            attack._bind(win, S, "xs dws m v dist2 partials")
        win.mask = S.mask.data_ptr() if mask_h is not None else None
        win.n_mask = S.n_mask.data_ptr() if mask_h is not None else None

        def set_window(t0, n_run, tail):                 # tail, the cap: it also evaluates its last step, snapshotting the clouds still running
            win.n_steps, win.adam_t0, win.tail_eval = n_run, t0, 1 if tail else 0
            return n_run + (1 if tail else 0)

        # (4-column history rows; the state has no graph handle and the entry point takes none)
        _, self.last_steps = attack._run_windows("psg_rla_nu_field_window", win, S, 1, self.iteration, self.chunk, set_window,
                                                 self.window_hook)
        self.last_adv = S.out_adv.reshape(G, n, 3).clone()
        self.last_adv_xyz = S.out_adv_xyz.reshape(G, n, 3).clone()
        stats = S.out_stats.cpu().numpy().astype(np.float64)
        self.last_dist_xyz = np.sqrt(stats[:, 3])
        return S, pred0, S.out_pred.cpu().numpy().reshape(G, n), stats

    def _one_cloud(self, features, labels):
        """[N, 6] / [N] -> the G = 1 inputs; a bad shape is refused here, before any device work"""
        f = attack._features(features, clouds=False, device=False)
        lab = attack._labels(labels, np.int64)
        if lab.shape != (int(f.shape[0]),):
            raise ValueError("labels must be [N] = %s, got %s" % ((int(f.shape[0]),), lab.shape))
        return f[None], lab[None]

    def _squeeze(self):
        self.last_adv, self.last_adv_xyz = self.last_adv[0], self.last_adv_xyz[0]


class NUattackField(_NuField, attack.NUattack):
    """attack.NUattack with `field="coord" | "both"`: every point moves; goal 'ut' keeps the reference's un-negated hinge
    (DESIGN.md 5n), the loop stops per cloud when the accuracy falls below 1/13; then the random-noise baseline, every field
    that moved with noise of its own l_2 size."""

    def __init__(self, model, batch_size=1, goal="ut", distance_metric="l_2", cw_loss_c=99999.0, confidence=0.0, learning_rate=0.01,
                 field="coord", coord_learning_rate=None):
        field = check_field(field)
        attack.NUattack.__init__(self, model, batch_size, goal, distance_metric, cw_loss_c, confidence, learning_rate)
        self._init_field(field, coord_learning_rate)

    def batch_attack(self, features, labels):
        """One cloud, features [N, 6], labels [N]: the lockstep loop at G = 1 -> the reference's 7-tuple (NUattack.py:233)."""
        if self.field == "color":
            return attack.NUattack.batch_attack(self, features, labels)
        out = self.batch_attack_clouds(*self._one_cloud(features, labels))[0]
        self._squeeze()
        return out

    def batch_attack_clouds(self, features, labels):
        """features [G, N, 6], labels [G, N] -> a list of G tuples (acc, original_accuracy, new_dists, mIoU, original_mIoU,
        rand_acc, rand_mIoU)."""
        if self.field == "color":
            return attack.NUattack.batch_attack_clouds(self, features, labels)
        lab = attack._labels(labels, np.int64)
        f, G, n = self._check(features, lab)
        S, pred0, pred, stats = self._run_field(f, G, n, lab, lab, None)
        dist_rgb = np.sqrt(stats[:, 2])
        rpred = self._field_noise_pred(S, dist_rgb, self.last_dist_xyz, G, n)
        return [attack._untargeted_out(self.logger, pred[g], pred0[g], rpred[g], lab[g], float(dist_rgb[g])) for g in range(G)]

    def _field_noise_pred(self, S, dist_rgb, dist_xyz, G, n):
        """Prediction [G, N] under random noise (NUattack.py:236-252) of every field that moved, each of its own l_2 size: numpy's
        global generator, per cloud in cloud order, under "both" the colours first, then the positions - a seeded run consumes
        the stream as G consecutive one-cloud calls do.  Positions are not clipped.  One pyramid build and one forward for the
        G noisy clouds (the workspace is left on them)."""
        both = self.field == "both"
        noise_rgb, noise_xyz = np.zeros((G, n, 3), np.float32), np.empty((G, n, 3), np.float32)
        for g in range(G):
            if both:
                z = np.random.uniform(0, 1, size=(n, 3))
                noise_rgb[g] = (z / np.linalg.norm(z) * dist_rgb[g]).astype(np.float32)
            z = np.random.uniform(0, 1, size=(n, 3))
            noise_xyz[g] = (z / np.linalg.norm(z) * dist_xyz[g]).astype(np.float32)
        rnd = torch.empty_like(S.feat)
        rnd[:, 0:3] = S.ori_xyz + torch.from_numpy(noise_xyz.reshape(G * n, 3)).cuda()
        rnd[:, 3:6] = torch.clamp(S.xs + torch.from_numpy(noise_rgb.reshape(G * n, 3)).cuda(), 0, 1) if both else S.xs
        S.ws.set_cloud(rnd[:, 0:3].contiguous())
        return S.ws.forward(self.model, rnd).argmax(1).cpu().numpy().reshape(G, n)


class tar_NUattackField(_NuField, attack.tar_NUattack):
    """attack.tar_NUattack with `field="coord" | "both"`: only the points of class `ori` move, the hinge is taken against the
    target labels on those points, the loop stops per cloud when more than 95 % of them are predicted as the target."""

    def __init__(self, model, batch_size=1, goal="t", distance_metric="l_2", confidence=0.0, learning_rate=0.01, field="coord",
                 coord_learning_rate=None):
        field = check_field(field)
        attack.tar_NUattack.__init__(self, model, batch_size, goal, distance_metric, confidence, learning_rate)
        self._init_field(field, coord_learning_rate)

    def batch_attack(self, features, labels, target=None, ori=2):
        """One cloud: the lockstep loop at G = 1 -> (target_points, sr, other_acc, original_other_accuracy, new_dists,
        other_mIoU, original_other_mIoU)."""
        if self.field == "color":
            return attack.tar_NUattack.batch_attack(self, features, labels, target, ori)
        out = self.batch_attack_clouds(*self._one_cloud(features, labels), target=target, ori=ori)[0]
        self._squeeze()
        return out

    def batch_attack_clouds(self, features, labels, target=None, ori=2):
        """features [G, N, 6], labels [G, N] -> a list of G tuples, the fields `batch_attack` returns.  Raises ValueError,
        before any device work, on bad shapes, a missing target or a cloud without a point of class `ori`."""
        if self.field == "color":
            return attack.tar_NUattack.batch_attack_clouds(self, features, labels, target, ori)
        lab = attack._labels(labels, np.int64)
        if lab.ndim != 2:
            raise ValueError("labels must be [G, N], got %s" % (lab.shape,))
        if target is None:
            raise ValueError("target: the class the points of class `ori` are pushed to")
        f, G, n = self._check(features, lab)
        mask_h = attack._origin_points(lab, ori, "253-256")
        ys_target = np.where(mask_h, target, lab)
        S, pred0, pred, stats = self._run_field(f, G, n, lab, ys_target, mask_h)
        return [attack._targeted_out(self.logger, pred[g], pred0[g], lab[g], ys_target[g], mask_h[g], float(np.sqrt(stats[g, 2])))
                for g in range(G)]
