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
