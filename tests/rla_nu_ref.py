"""Numpy restatements for the lockstep RandLA-Net NU attacks (psg_rla_nu_color_clouds / _adam_clouds / _latch_clouds):
the evaluation and exit latch the reference runs after every optimiser step (NUattack.py:190-213, tar_NUattack.py:235),
the integer exit tests next to the host's double-precision ones, and the colour arithmetic in float64.

`latch` takes switches that turn it into the mutants the host tests must catch; the defaults are the specification."""
import numpy as np

NU_BOUND = np.float32(1.0 - 1e-6)


def colors64(xs, dws, mask=None):
    """adv = (tanh(atanh(2 b x - b) + d_ws) + 1) / 2 in float64 on float32 inputs; masked-out points keep x exactly."""
    x, d, b = np.asarray(xs, np.float64), np.asarray(dws, np.float64), np.float64(NU_BOUND)
    adv = 0.5 * (np.tanh(np.arctanh(2.0 * b * x - b) + d) + 1.0)
    if mask is not None:
        adv = np.where(np.asarray(mask, bool)[..., None], adv, x)
    return adv


def fires_int(mode, num, den, count, total):
    """The device's exit test.  mode 0: den * n_correct < num * N; mode 1: den * n_hits > num * n_mask.  Exact integers."""
    count, total = np.asarray(count, np.int64), np.asarray(total, np.int64)
    return den * count < num * total if mode == 0 else den * count > num * total


def fires_host(mode, count, total):
    """The host loop's tests in double precision (randla/attack.py: `correct / n < 1 / 13`, `hits / points > 0.95`)."""
    ratio = np.asarray(count, np.float64) / np.asarray(total, np.float64)
    return ratio < 1 / 13 if mode == 0 else ratio > 0.95


def new_state(G, n):
    return {"active": np.ones(G, np.uint8), "exit_step": np.full(G, -1, np.int32), "out_adv": np.zeros((G, n, 3), np.float32),
            "out_pred": np.zeros((G, n), np.int32), "out_stats": np.zeros((G, 3), np.float32), "pred": np.zeros((G, n), np.int32)}


def latch(state, hist_row, logits, labels, ys, mask, n_mask, feat, dist2, mode, num, den, step, can_exit, final,
          argmax="first", strict=True, use_mask=True, min_step=1):
    """One latch call on G clouds: logits [G, n, 13], labels / ys [G, n], mask [G, n] or None, feat [G, n, 6], dist2 [G].
    Updates `state` (new_state) and hist_row [G, 3] in place; an inactive cloud is not touched."""
    G, n = labels.shape
    for g in range(G):
        if not state["active"][g]:
            continue
        z = logits[g]
        pred = z.argmax(1) if argmax == "first" else z.shape[1] - 1 - z[:, ::-1].argmax(1)
        n_correct = int((pred == labels[g]).sum())
        if mask is None:
            n_hits = 0
        else:
            on = mask[g].astype(bool) if use_mask else np.ones(n, bool)
            n_hits = int((on & (pred == ys[g])).sum())
        if mode == 0:
            fire = den * n_correct < num * n if strict else den * n_correct <= num * n
        else:
            fire = den * n_hits > num * int(n_mask[g]) if strict else den * n_hits >= num * int(n_mask[g])
        exits = bool(fire and can_exit and step >= min_step)
        row = np.array([n_correct, n_hits, dist2[g]], np.float32)
        state["pred"][g] = pred
        hist_row[g] = row
        if exits or final:
            state["out_adv"][g] = feat[g][:, 3:6]
            state["out_pred"][g] = pred
            state["out_stats"][g] = row
        if exits:
            state["exit_step"][g] = step
            state["active"][g] = 0
