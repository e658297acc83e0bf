"""Numpy restatements for the lockstep RandLA-Net NU attacks (psg_rla_nu_color_clouds / _adam_clouds / _latch_clouds):
the evaluation and exit latch the reference runs after every optimiser step (NUattack.py:190-213, tar_NUattack.py:235),
the integer exit tests next to the host's double-precision ones, the colour arithmetic in float64, and one Adam step in
float64 with the counted bound of the float32 kernel (adam64).

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


# ---- one Adam step in float64, with the float32 kernel's first-order error counted operation by operation
U = 2.0 ** -24
LIBM_ULPS = 5                    # atanhf, tanhf: the OpenCL full-profile limit the device's math library is built to (5 ulp; 1 ulp <= 2 u |result|)
B1, B2, ADAM_EPS = np.float32(0.9), np.float32(0.999), np.float32(1e-8)


def adam_lr_t(lr, t):
    """TF1 Adam's step size as the library forms it: in double from the float32 lr, rounded to float32 once"""
    return np.float32(np.float64(np.float32(lr)) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))


def adam64(xs, dws, m, v, adv, dscore, dist2, c, lr, t, mask=None, one_minus=None):
    """psg_rla_nu_adam_step / _clouds on float32 inputs, every operation in float64: xs, dws, m, v, adv (the colours the
    forward saw), dscore (d score / d colours) [..., n, 3], dist2 [...] (one per cloud), mask [..., n] or None.
    -> ((d_ws', m', v'), (their bounds)), the bounds per element and COUNTED: every float32 operation of the kernel adds one
    rounding, u = 2^-24 times the magnitude of its float64 result, to the error its operands bring (first order; a fused
    multiply-add only removes a rounding; sqrtf and the division are correctly rounded, atanhf and tanhf LIBM_ULPS ulp).
    The two gradient terms: gd = (adv - x) / dist carries 3 roundings (difference, root, quotient), gs = c dscore 1, their sum
    1 more of |gd + gs|; the chain factor (1 - th^2) / 2 carries what th = tanh(atanh(2 b x - b) + d_ws) brings plus 2.
    one_minus: (1 - beta1, 1 - beta2) as float32; the default is the kernel's (and TF1's), the float32 differences
    1 - 0.9f and 1 - 0.999f, which are exact - not float32(0.1) and float32(0.001), which oracle/randla_net.py takes."""
    x, d, m0, v0, a, s = (np.asarray(q, np.float64) for q in (xs, dws, m, v, adv, dscore))
    b, L = np.float64(NU_BOUND), LIBM_ULPS * 2 * U
    arg = 2.0 * b * x - b
    e = U * np.abs(2.0 * b * x) + U * np.abs(arg)
    at = np.arctanh(arg)
    e = e / (1.0 - arg * arg) + L * np.abs(at)
    w = at + d
    e = e + U * np.abs(w)
    th = np.tanh(w)
    e_th = (1.0 - th * th) * e + L * np.abs(th)
    chain = 0.5 * (1.0 - th * th)
    e_chain = 0.5 * (2.0 * np.abs(th) * e_th + U * th * th + U * (1.0 - th * th))
    dist = np.sqrt(np.asarray(dist2, np.float64))[..., None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        gd = np.where(dist > 0, (a - x) / dist, 0.0)
    gs = np.float64(np.float32(c)) * s
    e_sum = 3 * U * np.abs(gd) + U * np.abs(gs) + U * np.abs(gd + gs)
    g = (gd + gs) * chain
    e_g = np.abs(gd + gs) * e_chain + chain * e_sum + U * np.abs(g)
    if mask is not None:
        on = np.asarray(mask, bool)[..., None]
        g, e_g = np.where(on, g, 0.0), np.where(on, e_g, 0.0)
    b1, b2 = np.float64(B1), np.float64(B2)
    nb1, nb2 = (np.float64(q) for q in (one_minus or (np.float32(1) - B1, np.float32(1) - B2)))
    m1 = b1 * m0 + nb1 * g
    e_m = U * np.abs(b1 * m0) + nb1 * e_g + U * np.abs(nb1 * g) + U * np.abs(m1)
    p = nb2 * g
    e_p = nb2 * e_g + U * np.abs(p)
    v1 = b2 * v0 + p * g
    e_v = U * np.abs(b2 * v0) + np.abs(p) * e_g + np.abs(g) * e_p + U * np.abs(p * g) + U * np.abs(v1)
    lr_t = np.float64(adam_lr_t(lr, t))
    q = lr_t * m1
    e_q = lr_t * e_m + 2 * U * np.abs(q)                       # the product, and lr_t's own last bit (pow against **)
    r = np.sqrt(v1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e_r = np.where(r > 0, e_v / (2.0 * r), 0.0) + U * r
    den = r + np.float64(ADAM_EPS)
    e_den = e_r + U * den
    step = q / den
    e_step = e_q / den + np.abs(step) * e_den / den + U * np.abs(step)
    w1 = d - step
    return (w1, m1, v1), (e_step + U * np.abs(w1), e_m, e_v)
