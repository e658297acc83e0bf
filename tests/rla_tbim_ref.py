"""Numpy restatements for the lockstep RandLA-Net TBIM / tar_NBattack (psg_rla_tbim_latch_clouds, psg_rla_bim_step_clouds,
psg_rla_tbim_retire_clouds, psg_rla_tbim_window): the latch with TBIM.batch_attack's ordering (the exit is decided on the
forward BEFORE the iteration's update, the leaving cloud still takes that update, then its colours are snapshot and it is
retired), the integer exit test next to the host loop's double-precision one, the BIM update in float32, the lockstep loop
over scripted predictions and gradients, and TBIM.batch_attack's control flow without the device calls.

`latch`, `retire` and `lockstep` take switches that turn them into the mutants the host tests must catch; the defaults are the
specification."""
import numpy as np


def fires_int(num, den, hits, points):
    """The device's exit test: den * n_hits > num * n_mask, exact integers."""
    return den * np.asarray(hits, np.int64) > num * np.asarray(points, np.int64)


def fires_host(hits, points):
    """The host loop's test in double precision (randla/attack.py: `sr > 0.90` with sr = hits / points)."""
    return np.asarray(hits, np.float64) / np.asarray(points, np.float64) > 0.90


def first_max(logits):
    return np.asarray(logits).argmax(-1).astype(np.int32)


def new_state(G, n):
    return {"active": np.ones(G, np.uint8), "leaving": np.zeros(G, np.uint8), "exit_step": np.full(G, -1, np.int32),
            "out_adv": np.zeros((G, n, 3), np.float32), "out_pred": np.zeros((G, n), np.int32),
            "out_stats": np.zeros((G, 3), np.float32), "pred": np.zeros((G, n), np.int32)}


def latch(state, hist_row, logits, labels, hit_ys, mask, n_mask, num, den, it, final, feat=None, pred=None, strict=True, min_it=1,
          snapshot="after"):
    """One latch call on G clouds: logits [G, n, 13] (or pred [G, n] given), labels / hit_ys / mask [G, n].  Updates `state` and
    hist_row [G, 3] in place; an inactive cloud is not touched.  It neither clears `active` nor copies colours (the mutant
    snapshot='before' copies them here, from feat [G, n, 6])."""
    G = labels.shape[0]
    for g in range(G):
        if not state["active"][g]:
            continue
        p = first_max(logits[g]) if pred is None else np.asarray(pred[g], np.int32)
        n_correct = int((p == labels[g]).sum())
        n_hits = int((mask[g].astype(bool) & (p == hit_ys[g])).sum())
        fire = den * n_hits > num * int(n_mask[g]) if strict else den * n_hits >= num * int(n_mask[g])
        exits = bool(fire and it >= min_it)
        row = np.array([n_correct, n_hits, 0], np.float32)
        state["pred"][g] = p
        hist_row[g] = row
        if exits or final:
            state["out_pred"][g] = p
            state["out_stats"][g] = row
            if snapshot == "before":
                state["out_adv"][g] = feat[g][:, 3:6]
        if exits:
            state["exit_step"][g] = it
        state["leaving"][g] = 1 if exits else 0


def retire(state, feat, final, snapshot="after"):
    """After the update: the leaving clouds (final: every active one) get their colour snapshot and stop."""
    for g in range(len(state["active"])):
        if state["active"][g] and (state["leaving"][g] or final):
            if snapshot == "after":
                state["out_adv"][g] = feat[g][:, 3:6]
            state["active"][g] = 0
            state["leaving"][g] = 0


def bim_step(feat, dfeat, ori, running, eps, alpha, l2_metric):
    """psg_rla_bim_step's update (bim.py:84-98) of the running clouds of feat [G, n, 6] in place, float32 arithmetic with the
    two norms accumulated in double.  (The device's own yardstick is psg_rla_bim_step, bit for bit; this restates it.)"""
    f32 = np.float32
    for g in range(feat.shape[0]):
        if running is not None and not running[g]:
            continue
        adv, grad, x = feat[g][:, 3:6], dfeat[g][:, 3:6].astype(f32), ori[g].astype(f32)
        if not l2_metric:
            v = adv + f32(alpha) * np.sign(grad).astype(f32)
            v = np.minimum(np.maximum(v, x - f32(eps)), x + f32(eps))
        else:
            gn = np.maximum(f32(1e-12), np.sqrt(f32((grad.astype(np.float64) ** 2).sum())))
            delta = (adv - x + f32(alpha) * (grad / gn)).astype(f32)
            dn = np.sqrt(f32((delta.astype(np.float64) ** 2).sum()))
            scale = f32(eps) / dn if dn > f32(eps) else f32(1.0)
            v = x + delta * scale
        feat[g][:, 3:6] = np.minimum(np.maximum(v, f32(0.0)), f32(1.0)).astype(f32)


def lockstep(feat0, pred_fn, dfeat_fn, labels, hit_ys, mask, iteration, num=9, den=10, eps=0.5, alpha=0.01, l2_metric=0, chunk=10,
             strict=True, min_it=1, snapshot="after", update_leaving=True):
    """The loop of TBIM.batch_attack_clouds over scripted networks: pred_fn(it, feat) -> pred [G, n] stands for the forward and
    the arg-max, dfeat_fn(it, feat) -> [G, n, 6] for the hinge gradient and the backward.  Windows of `chunk` iterations, cut at
    the cap; the loop stops after the window in which the last cloud left.  -> (state, history rows [iterations run][G][3],
    feat, gradient steps per cloud)."""
    G, n = labels.shape
    feat, ori = feat0.copy(), feat0[:, :, 3:6].copy()
    n_mask = mask.reshape(G, n).sum(1).astype(np.int32)
    st, hist = new_state(G, n), []
    it0 = 0
    while it0 <= iteration:
        n_run = min(chunk, iteration - it0 + 1)
        for it in range(it0, it0 + n_run):
            final = 1 if it == iteration else 0
            row = np.zeros((G, 3), np.float32)
            latch(st, row, None, labels, hit_ys, mask, n_mask, num, den, it, final, feat=feat, pred=pred_fn(it, feat), strict=strict,
                  min_it=min_it, snapshot=snapshot)
            hist.append(row)
            running = st["active"].copy()
            if not update_leaving:
                running &= 1 - st["leaving"]
            bim_step(feat, dfeat_fn(it, feat), ori, running, eps, alpha, l2_metric)
            retire(st, feat, final, snapshot=snapshot)
        it0 += n_run
        if (st["exit_step"] >= 0).all():
            break
    steps = np.where(st["exit_step"] >= 0, st["exit_step"], iteration) + 1
    return st, np.stack(hist), feat, steps


def host_loop(feat0_g, pred_fn_g, dfeat_fn_g, hit_ys_g, mask_g, iteration, eps=0.5, alpha=0.01, l2_metric=0):
    """TBIM.batch_attack's control flow on one cloud with the same scripted networks (pred_fn_g(it, feat [n, 6]) -> [n]):
    forward, read-back, update, `if it > 0 and sr > 0.90: break`.  -> (pred of the last forward, colours after the last update,
    gradient steps)."""
    feat, ori = feat0_g.copy()[None], feat0_g[None, :, 3:6].copy()
    mk = mask_g.astype(bool)
    points = float(mk.sum())
    pred, steps = None, 0
    for it in range(iteration + 1):
        pred = np.asarray(pred_fn_g(it, feat[0]), np.int32)
        sr = float(np.sum(pred[mk] == hit_ys_g[mk]) / points)
        bim_step(feat, dfeat_fn_g(it, feat[0])[None], ori, None, eps, alpha, l2_metric)
        steps = it + 1
        if it > 0 and sr > 0.90:
            break
    return pred, feat[0][:, 3:6].copy(), steps


U = 2.0 ** -24


def bim_step64(feat, dfeat, ori, eps, alpha, norms=None):
    """bim_step's l_2 formula on float32 inputs, every operation in float64: feat, dfeat [G, n, 6], ori [G, n, 3].
    -> ((rgb [G, n, 3], norms [2][G], delta [G, n, 3]), (their bounds)).  norms: the squared norms to normalise with in place
    of the clouds' own (the mutants of the tests).  The bounds are per element and COUNTED: every float32 operation of the
    kernels adds one rounding, u = 2^-24 times the magnitude of its float64 result, to the error its operands bring (first
    order; a fused multiply-add only removes a rounding; sqrtf and the division are correctly rounded):
      |g|^2, |delta|^2   double sums (3 n terms: (3 n + 2) 2^-53, nothing next to u) rounded to float32 ONCE: 1; the second one
                         sums the float32 deltas as stored, so it brings their errors too: 2 sum |delta| e_delta
      gn = max(1e-12, sqrt |g|^2)   half the square's error plus 1; none where the floor holds
      delta = (adv - x) + alpha (g / gn)   the difference 1, the quotient 1 on top of gn's, the product 1, the sum 1
      scale = eps / sqrt |delta|^2 where clipped   the root as above, the quotient 1; none where scale = 1
      rgb = clip(x + delta scale, 0, 1)   the product 1, the sum 1; the clip is exact and moves no two values apart."""
    f, g, x = (np.asarray(q, np.float64) for q in (feat[:, :, 3:6], dfeat[:, :, 3:6], ori))
    eps, alpha, n3 = np.float64(np.float32(eps)), np.float64(np.float32(alpha)), f.shape[1] * 3
    dbl = (n3 + 2) * 2.0 ** -53
    gn2 = (g ** 2).sum((1, 2)) if norms is None else np.asarray(norms[0], np.float64)
    e_gn2 = (U + dbl) * gn2
    floor = np.sqrt(gn2) < np.float64(np.float32(1e-12))
    gn = np.where(floor, np.float64(np.float32(1e-12)), np.sqrt(gn2))
    with np.errstate(invalid="ignore", divide="ignore"):
        e_gn = np.where(floor, 0.0, e_gn2 / (2.0 * gn) + U * gn)
    gn, e_gn = gn[:, None, None], e_gn[:, None, None]
    a, q = f - x, g / gn
    e_q = np.abs(q) * e_gn / gn + U * np.abs(q)
    delta = a + alpha * q
    e_delta = U * np.abs(a) + alpha * e_q + U * np.abs(alpha * q) + U * np.abs(delta)
    own_dn2 = (delta ** 2).sum((1, 2))
    e_dn2 = 2.0 * (np.abs(delta) * e_delta).sum((1, 2)) + (U + dbl) * own_dn2
    dn2 = own_dn2 if norms is None else np.asarray(norms[1], np.float64)
    dn = np.sqrt(dn2)
    clipped = dn > eps
    with np.errstate(invalid="ignore", divide="ignore"):
        e_dn = np.where(dn > 0, e_dn2 / (2.0 * dn), 0.0) + U * dn
        scale = np.where(clipped, eps / dn, 1.0)
        e_scale = np.where(clipped, scale * e_dn / dn + U * scale, 0.0)
    scale, e_scale = scale[:, None, None], e_scale[:, None, None]
    out = x + delta * scale
    e_out = scale * e_delta + np.abs(delta) * e_scale + U * np.abs(delta * scale) + U * np.abs(out)
    return (np.clip(out, 0.0, 1.0), np.stack([gn2, own_dn2]), delta), (e_out, np.stack([e_gn2, e_dn2]), e_delta)
