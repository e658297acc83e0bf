"""The colour attacks of the reference's RandLA-Net tester (tester_S3DIS.py:36-44) behind the call shapes of its ares
classes: BIM / NBattack (bim.py:10-236, NBattack.py:8-48: non-targeted), TBIM / tar_NBattack (bim.py:277-505,
NBattack.py:53-65: targeted, origin class -> target class), NUattack / tar_NUattack (NUattack.py, tar_NUattack.py: Adam in
tanh space on distance + c * hinge).

The reference builds TensorFlow graphs around a session; here BIM is one fused device loop (`psg_rla_bim_attack`) and the
attacks whose loop reads an accuracy back every iteration (TBIM's `sr > 0.9`, NU's `acc < 1/13`, tar_NU's `sr > 0.95`)
keep that loop on the host over the step entry points (forward, masked hinge gradient, backward, update step): exactly
one small read-back per iteration, like the reference's session.run.  `batch_attack` takes the cloud's features [N, 6]
(xyz, rgb) and labels [N] instead of the reference's flattened data_batch list; the returned metric tuples are the
reference's, the adversarial colours stay available as `.last_adv`.  Network parity is UNPINNED (oracle/randla_net.py).

`NUattack.batch_attack_clouds` / `tar_NUattack.batch_attack_clouds` are the lockstep form of the two NU attacks: G clouds
advance together on one cloud-batch workspace, CHUNK optimiser steps per library call (`psg_rla_nu_window`), one read-back
per window; the accuracy exits are taken per cloud on the device, in integers.  `batch_attack` stays the one-cloud path.
`TBIM.batch_attack_clouds` (and `tar_NBattack`'s) is the same for the targeted BIM: CHUNK iterations per library call
(`psg_rla_tbim_window`), the `sr > 0.9` exit per cloud on the device, the exiting iteration's update still applied.

`field="coord" | "both"` (BIM, NBattack, TBIM, tar_NBattack; `batch_attack`, one cloud): the same attacks on the point positions
(DESIGN.md section 5q).  Every iteration rebuilds the index pyramid on the moved positions (`psg_rla_set_cloud`), runs the
forward on [positions | rgb], the hinge gradient, `psg_rla_backward_full` (feature path + relative-position branch) and the
field step `psg_rla_bim_step_field` - under "both" followed by the unchanged colour step, each field normalised and clipped
on its own with its own (magnitude, alpha); coordinates have no box.  `field="color"` is the code above, byte for byte.
NUattack / tar_NUattack refuse the other fields here; their coordinate-field forms are the subclasses of `randla/nu_field.py`.
The lockstep form of these fields for BIM / NBattack / TBIM / tar_NBattack is the subclasses of `randla/nb_field.py`.
"""
import ctypes

import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks.nu_windows import _bind, destroy_graphs, new_graphs  # noqa: F401  (_bind: the field modules' too)
from pointsecguard_amd.attacks.torchattacks.attacks._common import check_field
from pointsecguard_amd.randla import network

_FIELD_ONLY = ("field=%r: the coordinate field runs in BIM / NBattack / TBIM / tar_NBattack.batch_attack with batch_size == 1 "
               "(one cloud per call); %s moves colours only (the NU attacks on this field: randla.nu_field.NUattackField / "
               "tar_NUattackField; G clouds in lockstep: randla.nb_field.BIMField / NBattackField / TBIMField / tar_NBattackField)")

CHUNK = 10  # optimiser steps per device-side window (the CHUNK of the other networks' NU attacks)


def _features(features, clouds=None, device=True):
    """features (tensor or numpy) -> float32 device tensor (device=False: a tensor where it is); clouds False: [N, 6] of one
    cloud, True: [G, N, 6], None: either (the caller checks).  A bad shape is refused before any device work."""
    f = features if isinstance(features, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(features, np.float32))
    if clouds is False and (f.dim() != 2 or f.shape[1] != 6):
        raise ValueError("features must be [N, 6] (xyz, rgb) of one cloud, got %s" % (tuple(f.shape),))
    if clouds and (f.dim() != 3 or f.shape[2] != 6 or f.shape[0] < 1):
        raise ValueError("features must be [G, N, 6] (xyz, rgb) of G >= 1 clouds, got %s" % (tuple(f.shape),))
    return f.float().cuda().contiguous() if device else f


def _labels(labels, host=None):
    """labels (tensor or numpy) -> int32 device tensor, or (host = a numpy dtype) a host array of that type"""
    if host is not None:
        return (labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)).astype(host)
    y = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
    return y.to(torch.int32).cuda().contiguous()


_SETTINGS = {"magnitude": "eps", "alpha": "alpha", "cs": "cs", "rand_init_magnitude": "rand_init_eps",
             # the coordinate field's own (eps, alpha); unset, they follow magnitude / alpha
             "coord_magnitude": "coord_eps", "coord_alpha": "coord_alpha"}


def _config(atk, kwargs, *names):
    """Takes from kwargs the settings in `names` that it gives: iteration as int, logger as it is, the others as floats (the
    reference passes numbers or 1-element arrays)."""
    for name in names:
        if name not in kwargs:
            continue
        if name == "iteration":
            atk.iteration = int(kwargs[name])
        elif name == "logger":
            atk.logger = kwargs[name]
        else:
            setattr(atk, _SETTINGS[name], float(np.asarray(kwargs[name]).reshape(-1)[0]))


def _mean_iou(pred, true):
    """compute_iou of the reference's attack classes (bim.py:153-165)."""
    pred, true = np.asarray(pred).ravel(), np.asarray(true).ravel()
    iou = []
    for l in np.unique(np.concatenate([pred, true])):
        inter = np.sum((pred == l) & (true == l))
        iou.append(inter / np.float32(np.sum(true == l) + np.sum(pred == l) - inter))
    return float(np.mean(iou))


def _targeted_out(logger, pred, pred0, lab, ys_target, mask_h, new_dists):
    """One cloud's tuple of the targeted attacks (bim.py:508), logged: (target_points, sr, other_acc, original_other_accuracy,
    new_dists, other_mIoU, original_other_mIoU) from the last prediction, the clean one, the labels, the target labels and the
    origin-class mask [N]."""
    n, tp = lab.shape[0], float(mask_h.sum())
    out = (tp, float(np.sum(pred[mask_h] == ys_target[mask_h]) / tp), float(np.sum(pred[~mask_h] == ys_target[~mask_h]) / (n - tp)),
           float(np.sum(pred0[~mask_h] == lab[~mask_h]) / (n - tp)), new_dists, _mean_iou(pred[~mask_h], lab[~mask_h]),
           _mean_iou(pred0[~mask_h], lab[~mask_h]))
    if logger is not None:
        logger.info("points={}, sr={},  other_acc={}, original_other_accuracy={}, new_dists={}, other_mIoU={}, "
                    "original_other_mIoU={}".format(*out))
    return out


def _untargeted_out(logger, pred, pred0, rpred, lab, new_dists):
    """One cloud's tuple of NUattack (NUattack.py:233), logged: (acc, original_accuracy, new_dists, mIoU, original_mIoU,
    rand_acc, rand_mIoU) from the last prediction, the clean one and the one under random noise of the same size."""
    n = lab.shape[0]
    out = (float(np.sum(pred == lab) / n), float(np.sum(pred0 == lab) / n), new_dists, _mean_iou(pred, lab), _mean_iou(pred0, lab),
           float(np.sum(rpred == lab) / n), _mean_iou(rpred, lab))
    if logger is not None:
        logger.info("acc={}, original_acc={}, new_dists={}, mIoU={}, original_mIoU={}, rand_acc={}, rand_mIoU={}".format(*out))
    return out


def _origin_points(lab, ori, tester_lines):
    """mask of the origin class [N] or [G, N]; every cloud needs a point of it"""
    mask_h = lab == ori
    empty = np.flatnonzero(mask_h.reshape(-1, mask_h.shape[-1]).sum(1) == 0)
    if empty.size:
        where = "this cloud" if lab.ndim == 1 else "cloud(s) %s" % ", ".join(str(g) for g in empty)
        raise ValueError("no point of the origin class %d in %s (tester_S3DIS.py:%s skips such clouds)" % (ori, where, tester_lines))
    return mask_h


class _FieldState:
    """Device buffers of the coordinate-field loop of one cloud and its full workspace (network.RandLAWorkspace(full=True))."""

    def __init__(self, n):
        self.ws = network.RandLAWorkspace(n, full=True)
        dev = self.ws.device
        self.norms, self.norms_xyz = (torch.zeros(2, dtype=torch.float32, device=dev) for _ in range(2))
        self.delta = torch.empty(n, 3, dtype=torch.float32, device=dev)
        self.dlogits = torch.empty(n, network.NUM_CLASSES, dtype=torch.float32, device=dev)
        self.ori_xyz = self.ori_rgb = None

    def start(self, feat):
        self.ori_xyz, self.ori_rgb = feat[:, 0:3].contiguous(), feat[:, 3:6].contiguous()


def _field_iteration(atk, S, feat, ys, mask, sign):
    """One iteration on feat [N, 6] in place, stream-ordered, no read-back: pyramid of the moved positions, forward, hinge
    gradient against ys (mask, sign: psg_rla_colper_grad_masked), full backward, field step(s).  -> the logits it stepped from."""
    ws, n, l2 = S.ws, feat.shape[0], 1 if atk.distance_metric == "l_2" else 0
    ws.set_cloud(feat[:, 0:3].contiguous())
    logits = ws.forward(atk.model, feat)
    _lib.call("psg_rla_colper_grad_masked", runtime.ptr(logits), runtime.ptr(ys), None if mask is None else runtime.ptr(mask),
              float(sign), n, runtime.ptr(S.dlogits), None, runtime.stream())
    dfeat, dxyz = ws.backward(atk.model, S.dlogits, full=True)
    coord_eps = atk.eps if atk.coord_eps is None else atk.coord_eps
    coord_alpha = atk.alpha if atk.coord_alpha is None else atk.coord_alpha
    _lib.call("psg_rla_bim_step_field", runtime.ptr(feat), runtime.ptr(dfeat), runtime.ptr(dxyz), runtime.ptr(S.ori_xyz), n,
              coord_eps, coord_alpha, l2, runtime.ptr(S.norms_xyz), runtime.ptr(S.delta), runtime.stream())
    if atk.field == "both":
        _lib.call("psg_rla_bim_step", runtime.ptr(feat), runtime.ptr(dfeat), runtime.ptr(S.ori_rgb), n, atk.eps, atk.alpha, l2,
                  runtime.ptr(S.norms), runtime.ptr(S.delta), runtime.stream())
    return logits


def _field_finish(atk, S, feat):
    """the moved positions, their l_2 distance (a 0-dim device tensor: float() reads it back), and the workspace left on them,
    so that a forward on the adversarial features evaluates the attack"""
    atk.last_adv_xyz = feat[:, 0:3].contiguous()
    atk.last_dist_xyz = torch.linalg.vector_norm(atk.last_adv_xyz - S.ori_xyz)
    S.ws.set_cloud(atk.last_adv_xyz)


class _CloudsState:
    """Device buffers of G clouds of N points attacked in lockstep, their cloud-batch workspace and the graph handle of the
    full windows (every full window of one call shape has the same argument block).  For TBIM xs are the clean colours, dws the
    l_2 step's delta, ys the labels of the hinge and hit_ys the labels the hits are counted against."""

    def __init__(self, n, G):
        self.ws = network.RandLAWorkspace(n, batch=G)
        dev = self.ws.device
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
        R = G * n
        self.dws, self.m, self.v = f32(R, 3), f32(R, 3), f32(R, 3)
        self.xs, self.feat, self.dfeat = f32(R, 3), f32(R, 6), f32(R, 6)
        self.logits, self.dlogits = f32(R, 13), f32(R, 13)
        self.labels, self.ys, self.hit_ys, self.pred, self.out_pred = i32(R), i32(R), i32(R), i32(R), i32(R)
        self.mask = torch.zeros(R, dtype=torch.uint8, device=dev)
        self.n_mask = i32(G)
        self.dist2, self.norms, self.out_stats, self.out_adv = f32(G), f32(2, G), f32(G, 3), f32(R, 3)
        self.partials = torch.zeros(G, _lib.RLA_NU_PARTS, dtype=torch.float64, device=dev)
        self.scratch = i32(G, 2 * _lib.RLA_NU_PARTS + 1)
        self.hist = f32(CHUNK + 1, G, 3)
        self.active, self.leaving = (torch.zeros(G, dtype=torch.uint8, device=dev) for _ in range(2))
        self.exit = i32(G)
        # two handles: the full windows, and a full window that is also the last one (it carries the tail evaluation)
        self.graph, self.graph_tail = new_graphs(2)

    def __del__(self):
        destroy_graphs((getattr(self, "graph", None), getattr(self, "graph_tail", None)))


def _run_windows(entry, win, S, first, cap, chunk, set_window, hook, read_back=True):
    """The window loop of the lockstep attacks: steps first .. cap in windows of `chunk` (at most CHUNK), the last one cut at
    the cap, through the library's `entry`.  set_window(first step, steps, last) sets the window's fields of `win` and returns
    the number of history rows it writes; after the window's one read-back (those rows and the exit steps)
    hook(first step, steps, last, S, rows [rows, G, columns of S.hist]) is called; the loop ends after the window in which
    the last cloud exits.  read_back=False (the untargeted field BIM: every cloud takes every step): nothing returns to the
    host, no hook.  A state with graph handles passes one to the entry point, for a full CHUNK window only (cut windows run
    eagerly): S.graph, or S.graph_tail when it is also the last; the field windows' states have none and their entry points
    take none.  -> (the row count of every window, steps taken per cloud [G]: the exit step, or the cap, counted from
    `first`)."""
    chunk = max(1, min(int(chunk), CHUNK))
    G, cols = S.exit.shape[0], S.hist.shape[2]
    exited, rows_run = np.full(G, -1, np.int64), []
    t0 = first
    while t0 <= cap:
        n_run = min(chunk, cap - t0 + 1)
        last = t0 + n_run - 1 == cap
        rows = set_window(t0, n_run, last)
        if hasattr(S, "graph"):
            _lib.call(entry, ctypes.byref(win), None if n_run != CHUNK else (S.graph_tail if last else S.graph), runtime.stream())
        else:
            _lib.call(entry, ctypes.byref(win), runtime.stream())
        rows_run.append(rows)
        if read_back:
            back = torch.cat([S.hist[:rows].reshape(-1), S.exit.float()]).cpu().numpy()     # the window's one read-back
            exited = back[rows * G * cols:].astype(np.int64)
            if hook is not None:
                hook(t0, n_run, last, S, back[:rows * G * cols].reshape(rows, G, cols))
        t0 += n_run
        if (exited >= 0).all():
            break
    return rows_run, np.where(exited >= 0, exited, cap) + 1 - first


class _Attack:
    """What the constructors share: the field, the model, the per-shape workspaces."""

    step_hook = None        # tests, tools (non-colour fields): called after every iteration with (iteration, features [N, 6])

    def __init__(self, model, batch_size, field, field_one_cloud=False):
        self.field = check_field(field)
        if field_one_cloud and self.field != "color" and batch_size != 1:
            raise NotImplementedError(_FIELD_ONLY % (field, "batch_size > 1"))
        self.coord_eps = self.coord_alpha = self.last_adv_xyz = self.last_dist_xyz = None
        if not isinstance(model, network.RandLAModel):
            raise TypeError("model must be a pointsecguard_amd.randla.network.RandLAModel")
        self.model, self.batch_size = model, batch_size
        self.iteration = None
        self._ws = {}

    def _field_state(self, n):
        if ("field", n) not in self._ws:
            self._ws[("field", n)] = _FieldState(n)
        return self._ws[("field", n)]


class _RandInit:
    """NBattack.py's `rand_init_magnitude`: accepted and, like there, without effect"""

    rand_init_eps = None

    def config(self, **kwargs):
        super().config(**kwargs)
        _config(self, kwargs, "rand_init_magnitude")


class BIM(_Attack):
    def __init__(self, model, batch_size=1, loss="colper", goal="ut", distance_metric="l_inf", session=None,
                 iteration_callback=None, field="color"):
        super().__init__(model, batch_size, field, field_one_cloud=True)
        if goal != "ut" or distance_metric not in ("l_inf", "l_2") or iteration_callback is not None:
            raise NotImplementedError("BIM / NBattack: goal='ut', l_inf / l_2 (the targeted attack is TBIM / tar_NBattack)")
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.distance_metric = distance_metric
        self.eps = self.alpha = None

    def config(self, **kwargs):
        """magnitude (max distortion), alpha (step size), iteration (bim.py:118-150)."""
        _config(self, kwargs, "magnitude", "alpha", "iteration", "coord_magnitude", "coord_alpha")

    def batch_attack(self, features, labels):
        """features [N,6] (xyz, rgb) and labels [N] of one cloud - or [batch_size, N, 6] and [batch_size, N] - (device
        tensors or numpy) -> adversarial rgb [N,3] / [batch_size, N, 3] after `iteration` updates (device tensor).
        field "coord" / "both" (one cloud): the moved positions are `last_adv_xyz` [N,3], `last_dist_xyz` their l_2 distance."""
        if self.eps is None or self.alpha is None or self.iteration is None:
            raise RuntimeError("call config(magnitude=..., alpha=..., iteration=...) first")
        f, y = _features(features), _labels(labels)
        batched = f.dim() == 3
        if batched != (self.batch_size > 1) or (batched and f.shape[0] != self.batch_size):
            raise ValueError("features must be [N,6] for batch_size=1, [batch_size,N,6] otherwise (batch_size=%d, got %s)" %
                             (self.batch_size, tuple(f.shape)))
        n = f.shape[-2]
        if self.field != "color":
            S, feat = self._field_state(n), f.clone()
            S.start(feat)
            for it in range(self.iteration + 1):                 # bim.py:204-232, as below
                _field_iteration(self, S, feat, y, None, 1.0)
                if self.step_hook is not None:
                    self.step_hook(it, feat)
            _field_finish(self, S, feat)
            return feat[:, 3:6].contiguous()
        if n not in self._ws:
            self._ws[n] = network.RandLAWorkspace(n, batch=self.batch_size)
        # bim.py:204-232: one update before the loop, then `iteration` more
        adv = self._ws[n].bim_attack(self.model, f.reshape(-1, 6), y.reshape(-1), self.eps, self.alpha, self.iteration + 1,
                                     metric=self.distance_metric)
        rgb = adv[:, 3:6].contiguous()
        return rgb.reshape(self.batch_size, n, 3) if batched else rgb


class _StepAttack(_Attack):
    """Shared plumbing of the host-loop attacks: device buffers of one cloud and the step entry points."""

    def __init__(self, model, batch_size=1, field="color"):
        super().__init__(model, batch_size, field)
        if batch_size != 1:
            raise NotImplementedError("one cloud per call (ConfigS3DIS.val_batch_size = 1): the accuracy exits are per cloud")
        self.logger, self.last_adv = None, None
        self._clouds, self.last_steps = {}, None        # the lockstep attacks (batch_attack_clouds)

    def _setup(self, features, labels, full=False):
        f = _features(features, clouds=False)
        n = f.shape[0]
        if full:                                             # the coordinate field: a full workspace and its loop's buffers
            ws = self._field_state(n).ws
        else:
            if n not in self._ws:
                self._ws[n] = network.RandLAWorkspace(n)
            ws = self._ws[n]
        ws.set_cloud(f[:, 0:3].contiguous())
        return ws, f.clone(), _labels(labels), n

    @staticmethod
    def _grad(ws, model, feat, ys, mask, sign):
        logits = ws.forward(model, feat)
        dlogits = torch.empty_like(logits)
        _lib.call("psg_rla_colper_grad_masked", runtime.ptr(logits), runtime.ptr(ys), None if mask is None else runtime.ptr(mask),
                  float(sign), logits.shape[0], runtime.ptr(dlogits), None, runtime.stream())
        return logits, ws.backward(model, dlogits)

    def _start_clouds(self, f):
        """The lockstep state of f [G, N, 6] (built on the shape's first use) with the clouds loaded, every cloud active, and the
        clean prediction [G, N]."""
        G, n = int(f.shape[0]), int(f.shape[1])
        if (n, G) not in self._clouds:
            self._clouds[(n, G)] = _CloudsState(n, G)
        S = self._clouds[(n, G)]
        S.feat.copy_(f.reshape(G * n, 6))
        S.xs.copy_(S.feat[:, 3:6])                       # the clean colours
        S.ws.set_cloud(S.feat[:, 0:3].contiguous())
        pred0 = S.ws.forward(self.model, S.feat).argmax(1).cpu().numpy().reshape(G, n)
        S.active.fill_(1)
        S.exit.fill_(-1)
        return S, pred0


class TBIM(_StepAttack):
    """Targeted BIM (bim.py:277-505): the points of class `ori` are pushed to class `target`; the hinge is taken against
    the target labels on the masked points only, the gradient is negated (goal 't'), the update rule is BIM's; the loop
    stops when more than 90 % of the masked points are predicted as the target (bim.py:504-505).  Note the reference's
    `xs_adv_var = mask * xs_adv_var + (1 - mask) * xs_adv_var` (bim.py:318) is the identity: every colour may move."""

    def __init__(self, model, batch_size=1, loss="colper", goal="t", distance_metric="l_2", session=None, iteration_callback=None,
                 field="color"):
        super().__init__(model, batch_size, field)
        if goal not in ("t", "tm", "ut") or distance_metric not in ("l_inf", "l_2") or iteration_callback is not None:
            raise NotImplementedError("implemented: goal 't' / 'tm' / 'ut', l_inf / l_2")
        self.goal, self.distance_metric = goal, distance_metric
        self.eps = self.alpha = None

    def config(self, **kwargs):
        _config(self, kwargs, "magnitude", "alpha", "iteration", "logger", "coord_magnitude", "coord_alpha")

    def batch_attack(self, features, labels, target=None, ori=2):
        """-> (target_points, sr, other_acc, original_other_accuracy, new_dists, other_mIoU, original_other_mIoU),
        bim.py:508.  field "coord" / "both": the same loop on the positions (module docstring); new_dists stays the colour
        distance, the moved positions are `last_adv_xyz`, their l_2 distance `last_dist_xyz`."""
        if self.eps is None or self.alpha is None or self.iteration is None:
            raise RuntimeError("call config(magnitude=..., alpha=..., iteration=...) first")
        ws, feat, y, n = self._setup(features, labels, full=self.field != "color")
        S = self._field_state(n) if self.field != "color" else None
        if S is not None:
            S.start(feat)
        lab = y.cpu().numpy()
        mask_h = _origin_points(lab, ori, "311-314")
        target_points = float(mask_h.sum())
        ys_target = np.where(mask_h, target, lab).astype(np.int32)
        targeted = self.goal in ("t", "tm")
        ys = torch.from_numpy(ys_target if targeted else lab.astype(np.int32)).cuda()
        mask = torch.from_numpy(mask_h.astype(np.uint8)).cuda()
        ori_rgb = feat[:, 3:6].contiguous()
        norms = torch.zeros(2, dtype=torch.float32, device=feat.device)
        delta = torch.empty(n, 3, dtype=torch.float32, device=feat.device)
        pred = pred0 = ws.forward(self.model, feat).argmax(1).cpu().numpy()
        # bim.py:470-482 runs the update once before the loop; its result is the loop's starting point
        for it in range(self.iteration + 1):
            if S is not None:                                # the coordinate field: gradient and update(s) in one go
                logits = _field_iteration(self, S, feat, ys, mask, -1.0 if targeted else 1.0)
            else:
                logits, dfeat = self._grad(ws, self.model, feat, ys, mask, -1.0 if targeted else 1.0)
            pred = logits.argmax(1).cpu().numpy()            # the one read-back of the iteration (the reference's session.run)
            sr = float(np.sum(pred[mask_h] == ys_target[mask_h]) / target_points)
            if S is None:
                _lib.call("psg_rla_bim_step", runtime.ptr(feat), runtime.ptr(dfeat), runtime.ptr(ori_rgb), n, self.eps, self.alpha,
                          1 if self.distance_metric == "l_2" else 0, runtime.ptr(norms), runtime.ptr(delta), runtime.stream())
            elif self.step_hook is not None:
                self.step_hook(it, feat)
            if it > 0 and sr > 0.90:                         # (the update before the loop is not followed by the test)
                break
        if S is not None:
            _field_finish(self, S, feat)
        self.last_adv = feat[:, 3:6].contiguous()
        new_dists = float(torch.linalg.vector_norm(self.last_adv - ori_rgb))
        return _targeted_out(self.logger, pred, pred0, lab, ys_target, mask_h, new_dists)

    # the lockstep form: the exit `hits / points > 0.90` as an integer ratio, steps per window, the tests' and tools' hook
    EXIT_RATIO = (9, 10)
    chunk = 10              # iterations per window (tests shorten it; at most CHUNK)
    window_hook = None      # called after every window's read-back with (first iteration, iterations, final, state, history rows)

    def batch_attack_clouds(self, features, labels, target=None, ori=2):
        """G clouds in lockstep: features [G, N, 6], labels [G, N] -> a list of G tuples (target_points, sr, other_acc,
        original_other_accuracy, new_dists, other_mIoU, original_other_mIoU), the fields `batch_attack` returns.  Every cloud
        has its own exit; like there, the update of the exiting iteration is still applied: `last_adv` [G, N, 3] holds the
        colours after it, the tuple the prediction before it.  `last_steps` [G]: gradient steps taken per cloud.  Raises
        ValueError before any device work on unset config, bad shapes, iteration < 1 or a cloud without a point of `ori`."""
        if self.field != "color":
            raise NotImplementedError(_FIELD_ONLY % (self.field, "batch_attack_clouds"))
        if self.eps is None or self.alpha is None or self.iteration is None:
            raise ValueError("call config(magnitude=..., alpha=..., iteration=...) first")
        if self.iteration < 1:
            raise ValueError("iteration must be positive")
        if target is None:
            raise ValueError("target: the class the points of class `ori` are pushed to")
        f = _features(features, clouds=True, device=False)
        G, n = int(f.shape[0]), int(f.shape[1])
        lab = _labels(labels, np.int32)
        if lab.shape != (G, n):
            raise ValueError("labels must be [G, N] = %s, got %s" % ((G, n), lab.shape))
        mask_h = _origin_points(lab, ori, "311-314")
        f = f.float().cuda().contiguous()
        ys_target = np.where(mask_h, target, lab).astype(np.int32)
        targeted = self.goal in ("t", "tm")
        S, pred0 = self._start_clouds(f)
        S.labels.copy_(torch.from_numpy(lab.reshape(-1)))
        S.hit_ys.copy_(torch.from_numpy(ys_target.reshape(-1)))
        S.ys.copy_(torch.from_numpy((ys_target if targeted else lab).reshape(-1)))       # the labels of the hinge
        S.mask.copy_(torch.from_numpy(mask_h.astype(np.uint8).reshape(-1)))
        S.n_mask.copy_(torch.from_numpy(mask_h.sum(1).astype(np.int32)))
        for t in (S.norms, S.out_stats, S.out_adv, S.out_pred, S.leaving):
            t.zero_()
        win = _lib.RlaTbimWindowArgs()
        win.model, win.ws = self.model.handle, S.ws.handle
        win.G, win.N, win.l2_metric = G, n, 1 if self.distance_metric == "l_2" else 0
        win.num, win.den = int(self.EXIT_RATIO[0]), int(self.EXIT_RATIO[1])
        win.eps, win.alpha, win.sign = self.eps, self.alpha, -1.0 if targeted else 1.0
        _bind(win, S, "ori=xs mask n_mask labels hit_ys loss_ys=ys feat logits dlogits dfeat norms delta=dws pred scratch hist "
                      "out_adv out_pred out_stats active leaving exit_step=exit")

        def set_window(it0, n_run, final):               # final, the cap: its last step snapshots the clouds still running
            win.n_steps, win.it0, win.final = n_run, it0, 1 if final else 0
            return n_run

        # iterations 0 .. iteration (bim.py:470-482: one update before the loop)
        _, self.last_steps = _run_windows("psg_rla_tbim_window", win, S, 0, self.iteration, self.chunk, set_window, self.window_hook)
        self.last_adv = S.out_adv.reshape(G, n, 3).clone()
        pred = S.out_pred.cpu().numpy().reshape(G, n)
        ori_rgb = S.xs.reshape(G, n, 3)
        return [_targeted_out(self.logger, pred[g], pred0[g], lab[g], ys_target[g], mask_h[g],
                              float(torch.linalg.vector_norm(self.last_adv[g] - ori_rgb[g]))) for g in range(G)]


class NBattack(_RandInit, BIM):
    """NBattack.py:8-48: BIM plus a `rand_init_magnitude` setting.  The reference computes the random start point but never
    assigns it (`setup_xs` still assigns the clean colours, NBattack.py:27-29), so the attack IS BIM; the setting is
    accepted and, like there, has no effect."""

    def __init__(self, model, batch_size=1, loss="colper", goal="ut", distance_metric="l_2", session=None, iteration_callback=None,
                 field="color"):
        super().__init__(model, batch_size, loss, goal, distance_metric, session, iteration_callback, field)


class tar_NBattack(_RandInit, TBIM):
    """NBattack.py:53-65: TBIM plus the same unused `rand_init_magnitude` setting."""


class NUattack(_StepAttack):
    """NUattack.py:12-245: Adam (lr 0.01) on d_ws with adv = (tanh(atanh(2 b x - b) + d_ws) + 1) / 2, loss =
    |adv - x|_2 + cs * score, score = the colper hinge against the labels (goal 'ut': NUattack.py:47-48 keeps the un-negated
    hinge).  One search step of `iteration` Adam steps (the reference returns inside its first search step), stopping early
    when the accuracy falls below 1/13 (:213); then the random-noise baseline of the same l_2 size (:236-252)."""

    def __init__(self, model, batch_size=1, goal="ut", distance_metric="l_2", cw_loss_c=99999.0, confidence=0.0, learning_rate=0.01,
                 field="color"):
        if check_field(field) != "color":
            raise NotImplementedError(_FIELD_ONLY % (field, "NUattack"))
        super().__init__(model, batch_size)
        if goal != "ut" or distance_metric != "l_2":
            raise NotImplementedError("NUattack: goal 'ut', l_2 (tester_S3DIS.py:39)")
        self.lr, self.cs, self.iteration = float(learning_rate), 1.0, 1000

    def config(self, **kwargs):
        _config(self, kwargs, "cs", "iteration", "logger")

    def _run(self, features, labels, ys_h, mask_h, stop):
        ws, feat, y, n = self._setup(features, labels)
        dev = feat.device
        xs = feat[:, 3:6].contiguous()
        ys = torch.from_numpy(ys_h.astype(np.int32)).cuda()
        mask = None if mask_h is None else torch.from_numpy(mask_h.astype(np.uint8)).cuda()
        dws, m, v = (torch.zeros(n, 3, dtype=torch.float32, device=dev) for _ in range(3))
        dist2 = torch.zeros(1, dtype=torch.float32, device=dev)
        mptr = None if mask is None else runtime.ptr(mask)
        pred0 = ws.forward(self.model, feat).argmax(1).cpu().numpy()
        state = {"pred0": pred0, "n": n, "xs": xs, "ws": ws, "feat": feat}
        for t in range(1, self.iteration + 1):
            _lib.call("psg_rla_nu_color", runtime.ptr(xs), runtime.ptr(dws), mptr, n, runtime.ptr(feat), runtime.ptr(dist2), runtime.stream())
            _, dfeat = self._grad(ws, self.model, feat, ys, mask, 1.0)
            _lib.call("psg_rla_nu_adam_step", runtime.ptr(xs), runtime.ptr(dws), runtime.ptr(m), runtime.ptr(v), mptr, runtime.ptr(feat),
                      runtime.ptr(dfeat), runtime.ptr(dist2), n, self.cs, self.lr, t, runtime.stream())
            # the reference evaluates the UPDATED variable (NUattack.py:189-198): colours and logits after the step
            _lib.call("psg_rla_nu_color", runtime.ptr(xs), runtime.ptr(dws), mptr, n, runtime.ptr(feat), runtime.ptr(dist2), runtime.stream())
            pred = ws.forward(self.model, feat).argmax(1)
            stats = torch.cat([dist2, pred.eq(y).sum().float().reshape(1)]).cpu()      # the iteration's one read-back
            state.update(pred=pred, dist=float(stats[0]) ** 0.5, correct=float(stats[1]), steps=t)
            if stop(state):
                break
        self.last_adv = feat[:, 3:6].contiguous()
        return state

    def batch_attack(self, features, labels):
        """-> (acc, original_accuracy, new_dists, mIoU, original_mIoU, rand_acc, rand_mIoU), NUattack.py:233."""
        lab = _labels(labels, np.int64)
        st = self._run(features, labels, lab, None, lambda s: s["correct"] / s["n"] < 1 / 13)
        rpred = self._noise_pred(st["ws"], st["feat"], st["xs"], [st["dist"]], st["n"])[0]
        return _untargeted_out(self.logger, st["pred"].cpu().numpy(), st["pred0"], rpred, lab, st["dist"])

    def _noise_pred(self, ws, feat, xs, dist, n):
        """Prediction [G, N] under random noise of the same l_2 size (NUattack.py:236-252): numpy's global generator, like the
        reference, once per cloud in cloud order - a seeded run consumes the stream as G consecutive batch_attack calls do;
        then one forward for the G noisy clouds."""
        G = len(dist)
        noise = np.empty((G, n, 3), np.float32)
        for g in range(G):
            z = np.random.uniform(0, 1, size=(n, 3))
            noise[g] = (z / np.linalg.norm(z) * dist[g]).astype(np.float32)
        rnd = feat.clone()
        rnd[:, 3:6] = torch.clamp(xs + torch.from_numpy(noise.reshape(G * n, 3)).cuda(), 0, 1)
        return ws.forward(self.model, rnd).argmax(1).cpu().numpy().reshape(G, n)

    # the accuracy exit as an integer ratio: mode 0 `correct / n < num / den`, mode 1 `hits / points > num / den`
    EXIT_MODE, EXIT_RATIO = 0, (1, 13)
    chunk = CHUNK           # steps per window (tests shorten it; at most CHUNK)
    window_hook = None      # tests, tools: called after every window's read-back with (first step, steps, tail, state, history rows)

    def _run_clouds(self, features, labels, ys_h, mask_h):
        """The lockstep loop: features [G, N, 6], labels / ys_h [G, N] (host), mask_h [G, N] bool or None.  -> the state,
        pred0 [G, N], per cloud the snapshot's pred [G, N], {n_correct, n_hits, dist2} [G, 3] and the exit steps [G]."""
        f = _features(features, clouds=True)
        G, n = int(f.shape[0]), int(f.shape[1])
        if tuple(ys_h.shape) != (G, n):
            raise ValueError("labels must be [G, N] = %s, got %s" % ((G, n), tuple(ys_h.shape)))
        if self.iteration < 1:
            raise ValueError("iteration must be positive")
        S, pred0 = self._start_clouds(f)
        S.labels.copy_(torch.from_numpy(np.ascontiguousarray(labels, np.int32).reshape(-1)))
        S.ys.copy_(torch.from_numpy(np.ascontiguousarray(ys_h, np.int32).reshape(-1)))
        if mask_h is not None:
            S.mask.copy_(torch.from_numpy(np.ascontiguousarray(mask_h, np.uint8).reshape(-1)))
            S.n_mask.copy_(torch.from_numpy(mask_h.reshape(G, n).sum(1).astype(np.int32)))
        for t in (S.dws, S.m, S.v, S.dist2, S.out_stats, S.out_adv, S.out_pred):
            t.zero_()
        win = _lib.RlaNuWindowArgs()
        win.model, win.ws = self.model.handle, S.ws.handle
        win.G, win.N, win.mode = G, n, self.EXIT_MODE
        win.num, win.den = int(self.EXIT_RATIO[0]), int(self.EXIT_RATIO[1])
        win.cs, win.lr = self.cs, self.lr
        _bind(win, S, "xs dws m v labels ys feat logits dlogits dfeat dist2 partials pred scratch hist out_adv out_pred out_stats "
                      "active exit_step=exit")
        win.mask = S.mask.data_ptr() if mask_h is not None else None
        win.n_mask = S.n_mask.data_ptr() if mask_h is not None else None

        def set_window(t0, n_run, tail):                 # tail, the cap: it also evaluates its last step, snapshotting the clouds still running
            win.n_steps, win.adam_t0, win.tail_eval = n_run, t0, 1 if tail else 0
            return n_run + (1 if tail else 0)

        # windows [1..W], [W+1..2W], ..; the last one is cut to the cap
        _, self.last_steps = _run_windows("psg_rla_nu_window", win, S, 1, self.iteration, self.chunk, set_window, self.window_hook)
        self.last_adv = S.out_adv.reshape(G, n, 3).clone()
        return S, pred0, S.out_pred.cpu().numpy().reshape(G, n), S.out_stats.cpu().numpy().astype(np.float64), G, n

    def batch_attack_clouds(self, features, labels):
        """G clouds in lockstep: features [G, N, 6], labels [G, N] -> a list of G tuples, each the reference's
        (acc, original_accuracy, new_dists, mIoU, original_mIoU, rand_acc, rand_mIoU) of that cloud (NUattack.py:233), the
        fields `batch_attack` returns.  Every cloud has its own early exit; one that exits stops moving."""
        lab = _labels(labels, np.int64)
        S, pred0, pred, stats, G, n = self._run_clouds(features, lab, lab, None)
        dist = np.sqrt(stats[:, 2])
        rpred = self._noise_pred(S.ws, S.feat, S.xs, dist, n)
        return [_untargeted_out(self.logger, pred[g], pred0[g], rpred[g], lab[g], float(dist[g])) for g in range(G)]


class tar_NUattack(NUattack):
    """tar_NUattack.py:12-244: the masked variant - only the points of class `ori` move (tar_NUattack.py:41), the hinge is
    taken against the target labels on those points (:105-110), the loop stops when more than 95 % of them are predicted as
    the target (:235)."""

    def __init__(self, model, batch_size=1, goal="t", distance_metric="l_2", confidence=0.0, learning_rate=0.01, field="color"):
        if check_field(field) != "color":
            raise NotImplementedError(_FIELD_ONLY % (field, "tar_NUattack"))
        _StepAttack.__init__(self, model, batch_size)
        if goal != "t" or distance_metric != "l_2":
            raise NotImplementedError("tar_NUattack: goal 't', l_2 (tester_S3DIS.py:44)")
        self.lr, self.cs, self.iteration = float(learning_rate), 1.0, 1000

    def batch_attack(self, features, labels, target=None, ori=2):
        """-> (target_points, sr, other_acc, original_other_accuracy, new_dists, other_mIoU, original_other_mIoU)."""
        lab = _labels(labels, np.int64)
        mask_h = _origin_points(lab, ori, "253-256")
        target_points = float(mask_h.sum())
        ys_target = np.where(mask_h, target, lab)
        mask_t = torch.from_numpy(mask_h).cuda()
        ys_t = torch.from_numpy(ys_target).cuda()

        def stop(s):
            s["sr"] = float((s["pred"][mask_t] == ys_t[mask_t]).sum()) / target_points
            return s["sr"] > 0.95
        st = self._run(features, labels, ys_target, mask_h, stop)
        return _targeted_out(self.logger, st["pred"].cpu().numpy(), st["pred0"], lab, ys_target, mask_h, st["dist"])

    EXIT_MODE, EXIT_RATIO = 1, (19, 20)

    def batch_attack_clouds(self, features, labels, target=None, ori=2):
        """G clouds in lockstep -> a list of G tuples (target_points, sr, other_acc, original_other_accuracy, new_dists,
        other_mIoU, original_other_mIoU), the fields `batch_attack` returns.  Raises ValueError, before any device work, when
        a cloud has no point of class `ori`."""
        lab = _labels(labels, np.int64)
        if lab.ndim != 2:
            raise ValueError("labels must be [G, N], got %s" % (lab.shape,))
        mask_h = _origin_points(lab, ori, "253-256")
        ys_target = np.where(mask_h, target, lab)
        S, pred0, pred, stats, G, n = self._run_clouds(features, lab, ys_target, mask_h)
        return [_targeted_out(self.logger, pred[g], pred0[g], lab[g], ys_target[g], mask_h[g], float(np.sqrt(stats[g, 2])))
                for g in range(G)]
