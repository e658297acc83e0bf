"""Numpy restatement of the lockstep BIM family of RandLA-Net on the coordinate field (psg_rla_bim_step_field_clouds,
psg_rla_tbim_retire_field_clouds, psg_rla_bim_field_window; randla/nb_field.py), built from the pieces that already state the
parts: rla_tbim_ref.latch / retire / bim_step (the latch with TBIM.batch_attack's ordering, the flags, the colour step) and
rla_coord_ref64.field_step (the field step of one cloud).  Per iteration: latch, leaving flag, field step on the active clouds,
under "both" the colour step, retire with positions.

`lockstep` takes switches that turn it into the mutants the host tests must catch; the defaults are the specification.  (The
order of the two steps under "both" is not among them: the field step reads and writes columns 0..2 and the colour step columns
3..5, each from its own gradient columns, and `delta` is written by a step before that step reads it - swapping them changes
nothing but the scratch `delta` is left with, so no result can tell the two orders apart.)"""
import numpy as np

import rla_coord_ref64 as C
import rla_tbim_ref as R

METRIC = {0: "l_inf", 1: "l_2"}


def field_step_clouds(feat, dfeat, dxyz, ori_xyz, running, eps, alpha, l2_metric, use_dxyz=True):
    """psg_rla_bim_step_field_clouds: rla_coord_ref64.field_step on every running cloud of feat [G, n, 6] in place, the gradient
    dfeat[:, 0:3] + dxyz as one float32 add."""
    for g in range(feat.shape[0]):
        if running is not None and not running[g]:
            continue
        grad = dfeat[g][:, 0:3].astype(np.float32) + dxyz[g].astype(np.float32) if use_dxyz else dfeat[g][:, 0:3].astype(np.float32)
        feat[g][:, 0:3] = C.field_step(feat[g][:, 0:3], grad, ori_xyz[g], eps, alpha, METRIC[l2_metric])


def retire(state, feat, final, snapshot_xyz="after"):
    """psg_rla_tbim_retire_field_clouds: rla_tbim_ref.retire (colours, flags) with the positions snapshot next to the colours."""
    go = [g for g in range(len(state["active"])) if state["active"][g] and (state["leaving"][g] or final)]
    R.retire(state, feat, final)
    if snapshot_xyz == "after":
        for g in go:
            state["out_adv_xyz"][g] = feat[g][:, 0:3]


def new_state(G, n):
    st = R.new_state(G, n)
    st["out_adv_xyz"] = np.zeros((G, n, 3), np.float32)
    return st


def lockstep(feat0, pred_fn, grad_fn, labels, hit_ys, mask, iteration, field="coord", num=9, den=10, eps=0.5, alpha=0.01, coord_eps=0.3,
             coord_alpha=0.02, l2_metric=0, chunk=10, snapshot_xyz="after", update_leaving=True, freeze_retired=True, use_dxyz=True):
    """The loop of TBIMField.batch_attack_clouds over scripted networks: pred_fn(it, feat) -> pred [G, n] stands for the pyramid,
    the forward and the arg-max, grad_fn(it, feat) -> (dfeat [G, n, 6], dxyz [G, n, 3]) for the hinge gradient and the full
    backward.  Windows of `chunk` iterations, cut at the cap; the loop stops after the window in which the last cloud left.
    -> (state, history rows [iterations run][G][3], feat, gradient steps per cloud)."""
    G, n = labels.shape
    feat, ori, ori_xyz = feat0.copy(), feat0[:, :, 3:6].copy(), feat0[:, :, 0:3].copy()
    n_mask = mask.reshape(G, n).sum(1).astype(np.int32)
    st, hist = new_state(G, n), []
    it0 = 0
    while it0 <= iteration:
        n_run = min(chunk, iteration - it0 + 1)
        for it in range(it0, it0 + n_run):
            final = 1 if it == iteration else 0
            row = np.zeros((G, 3), np.float32)
            R.latch(st, row, None, labels, hit_ys, mask, n_mask, num, den, it, final, feat=feat, pred=pred_fn(it, feat))
            if snapshot_xyz == "before":
                for g in range(G):
                    if st["active"][g] and (st["leaving"][g] or final):
                        st["out_adv_xyz"][g] = feat[g][:, 0:3]
            hist.append(row)
            running = st["active"].copy() if freeze_retired else None
            if not update_leaving:
                running &= 1 - st["leaving"]
            dfeat, dxyz = grad_fn(it, feat)
            field_step_clouds(feat, dfeat, dxyz, ori_xyz, running, coord_eps, coord_alpha, l2_metric, use_dxyz=use_dxyz)
            if field == "both":
                R.bim_step(feat, dfeat, ori, running, eps, alpha, l2_metric)
            retire(st, feat, final, snapshot_xyz=snapshot_xyz)
        it0 += n_run
        if (st["exit_step"] >= 0).all():
            break
    steps = np.where(st["exit_step"] >= 0, st["exit_step"], iteration) + 1
    return st, np.stack(hist), feat, steps


def host_loop(feat0_g, pred_fn_g, grad_fn_g, hit_ys_g, mask_g, iteration, field="coord", eps=0.5, alpha=0.01, coord_eps=0.3,
              coord_alpha=0.02, l2_metric=0):
    """TBIM.batch_attack's control flow on the coordinate field, one cloud, the same scripted networks: forward, read-back, field
    step (then the colour step under "both"), `if it > 0 and sr > 0.90: break`.  -> (pred of the last forward, positions and
    colours after the last update, gradient steps)."""
    feat = feat0_g.copy()
    ori, ori_xyz = feat0_g[:, 3:6].copy(), feat0_g[:, 0:3].copy()
    mk = mask_g.astype(bool)
    points = float(mk.sum())
    pred, steps = None, 0
    for it in range(iteration + 1):
        pred = np.asarray(pred_fn_g(it, feat), np.int32)
        sr = float(np.sum(pred[mk] == hit_ys_g[mk]) / points)
        dfeat, dxyz = grad_fn_g(it, feat)
        feat[:, 0:3] = C.field_step(feat[:, 0:3], dfeat[:, 0:3] + dxyz, ori_xyz, coord_eps, coord_alpha, METRIC[l2_metric])
        if field == "both":
            R.bim_step(feat[None], dfeat[None], ori[None], None, eps, alpha, l2_metric)
        steps = it + 1
        if it > 0 and sr > 0.90:
            break
    return pred, feat[:, 0:3].copy(), feat[:, 3:6].copy(), steps


def lockstep_bim(feat0, grad_fn, iteration, field="coord", eps=0.5, alpha=0.01, coord_eps=0.3, coord_alpha=0.02, l2_metric=0, chunk=10):
    """Mode 0 (BIMField.batch_attack_clouds): no latch, no exit; every cloud takes iterations 0 .. iteration, the window's last
    step under `final` snapshots all of them.  -> (out_adv_xyz, out_adv, active)"""
    G, n = feat0.shape[:2]
    feat, ori, ori_xyz = feat0.copy(), feat0[:, :, 3:6].copy(), feat0[:, :, 0:3].copy()
    st = new_state(G, n)
    it0 = 0
    while it0 <= iteration:
        n_run = min(chunk, iteration - it0 + 1)
        for it in range(it0, it0 + n_run):
            dfeat, dxyz = grad_fn(it, feat)
            field_step_clouds(feat, dfeat, dxyz, ori_xyz, st["active"], coord_eps, coord_alpha, l2_metric)
            if field == "both":
                R.bim_step(feat, dfeat, ori, st["active"], eps, alpha, l2_metric)
            if it == iteration:
                retire(st, feat, 1)
        it0 += n_run
    return st["out_adv_xyz"], st["out_adv"], st["active"]


def field_step_l2_f32(xyz_adv, g, ori, eps, alpha, shared_norms=False):
    """float32 emulation of the batched l_2 step, the kernels' stages over all clouds at once: xyz_adv, g, ori [G, n, 3] ->
    (positions [G, n, 3], norms [2][G]).  Each cloud is normalised and clipped with its own norms; shared_norms: with cloud 0's
    (the mutant)."""
    f32 = np.float32
    xyz_adv, g, ori = (np.asarray(a, f32) for a in (xyz_adv, g, ori))
    own = lambda a: (a.astype(np.float64) ** 2).sum((1, 2)).astype(f32)
    pick = lambda v: np.broadcast_to(v[:1], v.shape) if shared_norms else v
    gn2 = own(g)
    gn = np.maximum(f32(1e-12), np.sqrt(pick(gn2)))[:, None, None]
    delta = ((xyz_adv - ori) + f32(alpha) * (g / gn)).astype(f32)
    dn2 = own(delta)
    dn = np.sqrt(pick(dn2))
    with np.errstate(divide="ignore"):
        scale = np.where(dn > f32(eps), f32(eps) / dn, f32(1.0)).astype(f32)[:, None, None]
    return (ori + delta * scale).astype(f32), np.stack([gn2, dn2])
