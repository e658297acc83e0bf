"""Numpy restatements for RandLA-Net's NU attacks on the coordinate field (psg_rla_nu_coord_apply_clouds,
psg_rla_nu_coord_adam_clouds, psg_rla_nu_field_latch_clouds, psg_rla_nu_field_window): the positions and the Adam step on
`delta` in float64 with the counted bound of the float32 kernels, a float32 emulation of both kernels, the 4-column latch on
top of rla_nu_ref.latch, and the lockstep loop next to a plain per-cloud loop in the reference's order, both over scripted
networks.

`coord_adam64`, `coord_adam32` and `lockstep` take a `mutant` that turns them into the bugs the host tests must catch; the
default is the specification."""
import numpy as np

import rla_nu_ref as R

U, B1, B2, ADAM_EPS = R.U, R.B1, R.B2, R.ADAM_EPS

ADAM_MUTANTS = ("mask_ignored", "no_dist", "no_dxyz", "no_bias_correction", "no_guard")


# ---------------------------------------------------------------------------------------------------- apply
def apply64(ori, delta, mask=None):
    """xyz = ori + delta on the moving points, in float64 on float32 inputs -> (xyz, bound): one float32 addition, one rounding
    of its result; a point off the mask keeps ori exactly (bound 0)."""
    x, d = np.asarray(ori, np.float64), np.asarray(delta, np.float64)
    p = x + d
    b = U * np.abs(p)
    if mask is not None:
        on = np.asarray(mask, bool)[..., None]
        p, b = np.where(on, p, x), np.where(on, b, 0.0)
    return p, b


def apply32(ori, delta, mask=None):
    """the kernel's arithmetic in float32 -> (xyz float32, dist2 [...] float32: the double sum of the positions as written,
    rounded once)"""
    x = np.asarray(ori, np.float32)
    p = (x + np.asarray(delta, np.float32)).astype(np.float32)
    if mask is not None:
        p = np.where(np.asarray(mask, bool)[..., None], p, x)
    d = p.astype(np.float64) - x.astype(np.float64)
    return p, (d * d).sum((-2, -1)).astype(np.float32)


def dist2_64(xyz, ori):
    """sum (xyz as written - ori)^2 per cloud in float64 -> (value [...], bound): every difference of two floats is exact in
    double, every square rounds once (2^-53), the K = 3 n non-negative terms are added in double in a fixed order (at most
    (K - 1) 2^-53 of the sum, first order), the total is rounded to float once (2^-24); (K + 2) 2^-53 leaves the second-order
    terms room - the bound of tests/test_gpu_rla_nu_clouds.py for the colour sum."""
    d = np.asarray(xyz, np.float64) - np.asarray(ori, np.float64)
    ref = (d * d).sum((-2, -1))
    k = d.shape[-2] * 3
    return ref, ref * (2.0 ** -24 + (k + 2) * 2.0 ** -53)


# ---------------------------------------------------------------------------------------------------- Adam on delta
def coord_grad64(ori, xyz, dfeat3, dxyz, dist2, c, mask=None, mutant=None):
    """The gradient that enters Adam, float64 on float32 inputs -> (g, bound).  g = (dist > 0 ? (xyz - ori) / dist : 0) +
    c (dfeat3 + dxyz), zero off the mask.  Counted, u = 2^-24 of each float64 result: the inner sum 1, its product with c 1
    more; the distance term 3 (difference, root, quotient); their sum 1 (a fused multiply-add only removes one)."""
    x, p, a, b = (np.asarray(q, np.float64) for q in (ori, xyz, dfeat3, dxyz))
    dist = np.sqrt(np.asarray(dist2, np.float64))[..., None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        gd = (p - x) / dist if mutant == "no_guard" else np.where(dist > 0, (p - x) / np.where(dist > 0, dist, 1.0), 0.0)
    if mutant == "no_dist":
        gd = np.zeros_like(gd)
    ds = a if mutant == "no_dxyz" else a + b
    e_ds = U * np.abs(ds)
    cc = np.float64(np.float32(c))
    gs = cc * ds
    g = gd + gs
    e = 3 * U * np.abs(gd) + cc * e_ds + U * np.abs(gs) + U * np.abs(g)
    if mask is not None and mutant != "mask_ignored":
        on = np.asarray(mask, bool)[..., None]
        g, e = np.where(on, g, 0.0), np.where(on, e, 0.0)
    return g, e


def coord_adam64(ori, delta, m, v, xyz, dfeat3, dxyz, dist2, c, lr, t, mask=None, mutant=None):
    """psg_rla_nu_coord_adam_clouds on float32 inputs, every operation in float64: ori, delta, m, v, xyz (the positions the
    forward saw), dfeat3 (columns 0:3 of d score / d features), dxyz [..., n, 3], dist2 [...] (one per cloud), mask [..., n] or
    None.  -> ((delta', m', v'), (their bounds)); the moments and the step are rla_nu_ref.adam64's, operation for operation."""
    d0, m0, v0 = (np.asarray(q, np.float64) for q in (delta, m, v))
    g, e_g = coord_grad64(ori, xyz, dfeat3, dxyz, dist2, c, mask, mutant)
    b1, b2 = np.float64(B1), np.float64(B2)
    nb1, nb2 = np.float64(np.float32(1) - B1), np.float64(np.float32(1) - B2)
    m1 = b1 * m0 + nb1 * g
    e_m = U * np.abs(b1 * m0) + nb1 * e_g + U * np.abs(nb1 * g) + U * np.abs(m1)
    p = nb2 * g
    e_p = nb2 * e_g + U * np.abs(p)
    v1 = b2 * v0 + p * g
    e_v = U * np.abs(b2 * v0) + np.abs(p) * e_g + np.abs(g) * e_p + U * np.abs(p * g) + U * np.abs(v1)
    lr_t = np.float64(np.float32(lr) if mutant == "no_bias_correction" else R.adam_lr_t(lr, t))
    q = lr_t * m1
    e_q = lr_t * e_m + 2 * U * np.abs(q)                       # the product, and lr_t's own last bit (pow against **)
    r = np.sqrt(v1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e_r = np.where(r > 0, e_v / (2.0 * r), 0.0) + U * r
    den = r + np.float64(ADAM_EPS)
    e_den = e_r + U * den
    step = q / den
    e_step = e_q / den + np.abs(step) * e_den / den + U * np.abs(step)
    w1 = d0 - step
    return (w1, m1, v1), (e_step + U * np.abs(w1), e_m, e_v)


def coord_adam32(ori, delta, m, v, xyz, dfeat3, dxyz, dist2, c, lr, t, mask=None, mutant=None):
    """the kernel in float32 numpy, expression for expression (no fused multiply-adds) -> (delta', m', v') float32"""
    f = np.float32
    x, d0, m0, v0, p, a, b = (np.asarray(q, f) for q in (ori, delta, m, v, xyz, dfeat3, dxyz))
    dist = np.sqrt(np.asarray(dist2, f))[..., None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        gd = (p - x) / dist if mutant == "no_guard" else np.where(dist > 0, (p - x) / np.where(dist > 0, dist, f(1)), f(0))
    if mutant == "no_dist":
        gd = np.zeros_like(gd)
    ds = a if mutant == "no_dxyz" else a + b
    g = (gd + f(c) * ds).astype(f)
    if mask is not None and mutant != "mask_ignored":
        g = np.where(np.asarray(mask, bool)[..., None], g, f(0))
    m1 = (B1 * m0 + (f(1) - B1) * g).astype(f)
    v1 = (B2 * v0 + (f(1) - B2) * g * g).astype(f)
    lr_t = f(lr) if mutant == "no_bias_correction" else R.adam_lr_t(lr, t)
    return (d0 - lr_t * m1 / (np.sqrt(v1) + ADAM_EPS)).astype(f), m1, v1


# ---------------------------------------------------------------------------------------------------- the 4-column latch
def new_state(G, n):
    st = R.new_state(G, n)
    st["out_stats"] = np.zeros((G, 4), np.float32)
    st["out_adv_xyz"] = np.zeros((G, n, 3), np.float32)
    return st


def latch(state, hist_row, logits, labels, ys, mask, n_mask, feat, dist2_rgb, dist2_xyz, mode, num, den, step, can_exit, final, **kw):
    """psg_rla_nu_field_latch_clouds: rla_nu_ref.latch (counts, exit rules, the colour snapshot, pred) with the row
    {n_correct, n_hits, dist2_rgb or 0, dist2_xyz} [G, 4] and the position snapshot out_adv_xyz = feat[:, 0:3]."""
    G = labels.shape[0]
    d2 = np.zeros(G, np.float32) if dist2_rgb is None else np.asarray(dist2_rgb, np.float32)
    was = state["active"].copy()
    st3 = dict(state, out_stats=np.zeros((G, 3), np.float32))          # (shares every other array with `state`)
    row3 = np.zeros((G, 3), np.float32)
    R.latch(st3, row3, logits, labels, ys, mask, n_mask, feat, d2, mode, num, den, step, can_exit, final, **kw)
    for g in range(G):
        if not was[g]:
            continue
        row = np.array([row3[g, 0], row3[g, 1], d2[g], dist2_xyz[g]], np.float32)
        hist_row[g] = row
        if final or not state["active"][g]:                    # it left in this call, or the cap snapshots it
            state["out_stats"][g] = row
            state["out_adv_xyz"][g] = feat[g][:, 0:3]


# ---------------------------------------------------------------------------------------------------- control flow
LOCKSTEP_MUTANTS = ("eval_off_by_one", "frozen_still_steps", "no_tail")


def _one_hot(pred):
    z = np.zeros(pred.shape + (13,), np.float32)
    np.put_along_axis(z, np.asarray(pred, np.int64)[..., None], 1.0, -1)
    return z


def lockstep(feat0, pred_fn, grad_fn, labels, ys, mask, mode, num, den, cap, cs, lr, chunk=10, mutant=None):
    """The loop of the field classes over psg_rla_nu_field_window's step order, field "coord", on scripted networks:
    pred_fn(e, g, feat_g [n, 6]) -> pred [n] stands for the pyramid, the forward and the arg-max of evaluation index e of cloud
    g, grad_fn(e, g, feat_g) -> (dfeat [n, 6], dxyz [n, 3]) for the hinge gradient and the full backward at that state.
    Windows of `chunk` steps cut at the cap, the last one with the tail; the loop stops after the window in which the last
    cloud left.  -> (state, history rows [rows][G][4] with nan where a cloud was frozen, (delta, m, v), steps per cloud)."""
    G, n = labels.shape
    feat, ori = feat0.astype(np.float32).copy(), feat0[:, :, 0:3].astype(np.float32).copy()
    delta, m, v = (np.zeros((G, n, 3), np.float32) for _ in range(3))
    n_mask = None if mask is None else mask.reshape(G, n).sum(1).astype(np.int32)
    dist2 = np.zeros(G, np.float32)
    st, hist = new_state(G, n), []
    t0 = 1
    while t0 <= cap:
        n_run = min(chunk, cap - t0 + 1)
        tail = t0 + n_run - 1 == cap and mutant != "no_tail"
        for i in range(n_run + (1 if tail else 0)):
            t, last = t0 + i, i == n_run
            for g in np.flatnonzero(st["active"]):
                feat[g, :, 0:3], dist2[g] = apply32(ori[g], delta[g], None if mask is None else mask[g])
            e = t if mutant == "eval_off_by_one" else t - 1
            logits = np.stack([_one_hot(pred_fn(t - 1, g, feat[g])) for g in range(G)])
            row = np.full((G, 4), np.nan, np.float32)
            latch(st, row, logits, labels, ys, mask, n_mask, feat, None, dist2, mode, num, den, e, 1 if e >= 1 else 0, 1 if last else 0)
            hist.append(row)
            if last:
                break
            for g in range(G):
                if not st["active"][g] and mutant != "frozen_still_steps":
                    continue
                dfeat, dxyz = grad_fn(t - 1, g, feat[g])
                delta[g], m[g], v[g] = coord_adam32(ori[g], delta[g], m[g], v[g], feat[g][:, 0:3], dfeat[:, 0:3], dxyz, dist2[g], cs, lr, t,
                                                    None if mask is None else mask[g])
        t0 += n_run
        if (st["exit_step"] >= 0).all():
            break
    return st, np.stack(hist), (delta, m, v), np.where(st["exit_step"] >= 0, st["exit_step"], cap)


def plain_loop(g, feat0_g, pred_fn, grad_fn, labels_g, ys_g, mask_g, mode, cap, cs, lr):
    """One cloud in the reference's order (NUattack.py:189-213, the host loop of attack.NUattack._run): step, then evaluate
    the UPDATED variable, `correct / n < 1 / 13` or `hits / points > 0.95` in double, break.  -> dict(exit_step (-1: the cap),
    xyz, pred, rows {evaluation index: [n_correct, n_hits, 0, dist2]}, delta, m, v)."""
    n = labels_g.shape[0]
    feat, ori = feat0_g.astype(np.float32).copy(), feat0_g[:, 0:3].astype(np.float32).copy()
    delta, m, v = (np.zeros((n, 3), np.float32) for _ in range(3))
    rows, exit_step, pred = {}, -1, None
    for t in range(1, cap + 1):
        feat[:, 0:3], dist2 = apply32(ori, delta, mask_g)
        dfeat, dxyz = grad_fn(t - 1, g, feat)
        delta, m, v = coord_adam32(ori, delta, m, v, feat[:, 0:3], dfeat[:, 0:3], dxyz, dist2, cs, lr, t, mask_g)
        feat[:, 0:3], dist2 = apply32(ori, delta, mask_g)
        pred = np.asarray(pred_fn(t, g, feat), np.int32)
        n_correct = int((pred == labels_g).sum())
        n_hits = 0 if mask_g is None else int((mask_g.astype(bool) & (pred == ys_g)).sum())
        rows[t] = np.array([n_correct, n_hits, 0, dist2], np.float32)
        fire = R.fires_host(mode, n_correct, n) if mode == 0 else R.fires_host(mode, n_hits, int(mask_g.sum()))
        if fire:
            exit_step = t
            break
    return dict(exit_step=exit_step, xyz=feat[:, 0:3].copy(), pred=pred, rows=rows, delta=delta, m=m, v=v)
