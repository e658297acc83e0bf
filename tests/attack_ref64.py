"""Plain references for the attack arithmetic of csrc/psg_attack.hip, one function per entry point, with the bound of each.

TEST INFRASTRUCTURE ONLY: no GPU, no oracle import.  Every function restates its operation from the reference's formulas
(nontarget.py / target.py of the PointNet attacks, colper.py / tcolper.py of the ResGCN ones, torch.optim.Adam).

EXACT references (numpy float32, one IEEE operation per line, compared bit for bit): to_point_major, to_channel_major,
pgd_step(_field), the integer side of seg_stats, nu_step_latch, the value side of nu_restart_rooms.

FLOAT64 references (torch CPU float64, gradients by autograd through the restated loss): ce_logp_grad, inverse_tanh,
tanh_color, nu_f_loss_grad, gcn_f_loss_grad, nu_adam_step, the extra_l2 of nu_restart_rooms.  Each returns its values and,
per entry, a FIRST-ORDER error model of the float32 kernel: class V below carries (value, error) through the kernel's own
formula, every float32 operation adding u |result| (u = 2^-24) to the error its operands bring, a sum of n terms in ANY
order adding (n - 1) u sum|terms| (so the bound of an atomically accumulated sum does not depend on the order).  The error is
kept in five parts: plain arithmetic, and what enters at expf, logf, tanhf, sqrtf (each taken as u |result|, propagated
like everything else).  No ulp figure is documented for these four functions on the device, so each part is scaled by its
own constant = 4 x the largest |error| / (first-order bound) MEASURED on the MI355X over all cases of
tests/test_attack_kernels.py on the outputs named beside the constant; the margin covers other arguments.

  bound = plain + EXP_RATIO exp-part + LOG_RATIO log-part + TANH_RATIO tanh-part + SQRT_RATIO sqrt-part + 2^-149
(the last term: one subnormal, the format's resolution where a result underflows)."""
import numpy as np
import torch

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149
PLAIN, EXP, LOG, TANH, SQRT = range(5)
# measured on the MI355X: largest |error| / first-order bound (all five parts at factor 1) over every case of
# test_attack_kernels.py, which prints the figure of every output of every case:
#   expf   nu_f_loss_grad(_rooms): dlogp 0.4024 (257 rows, n_cls = 2), f sums 0.0612
#   logf   nu_inverse_tanh: w 0.6498 (2 x 4096 points)
#   tanhf  nu_tanh_color(_rooms): colours 0.9281 (45 x 4099 points)
#   sqrtf  nu_adam_step(_rooms): w 0.9955 (45 x 4099 points, step 2); m 0.9286 and v 0.9793 there
# outputs that mix two functions, under the same model: ce_logp_grad dlogp 0.6973 and cost 0.0251; the sums of
# gcn_f_loss_grad 0.0157, the L2 sums 0.1161, extra_l2 0.0002 (plain arithmetic only)
EXP_MEASURED = 0.4024
EXP_RATIO = 4 * EXP_MEASURED
LOG_MEASURED = 0.6498
LOG_RATIO = 4 * LOG_MEASURED
TANH_MEASURED = 0.9281
TANH_RATIO = 4 * TANH_MEASURED
SQRT_MEASURED = 0.9955
SQRT_RATIO = 4 * SQRT_MEASURED


def first_order(e):
    """the unscaled model: all five parts at factor 1 (what the measured ratios are taken against)"""
    return e.sum(0) + TINY


def bound(e):
    return e[PLAIN] + EXP_RATIO * e[EXP] + LOG_RATIO * e[LOG] + TANH_RATIO * e[TANH] + SQRT_RATIO * e[SQRT] + TINY


class V:
    """(value, error parts [5]) of a float32 evaluation, both float64; operands that are not V are exact"""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros((5,) + self.v.shape) if e is None else e

    @staticmethod
    def rounded(v, e, part=PLAIN):
        e = np.array(np.broadcast_to(e, (5,) + v.shape))
        with np.errstate(invalid="ignore"):
            e[part] += U * np.abs(v)
        return V(v, e)

    def __add__(self, o):
        if isinstance(o, V):
            return V.rounded(self.v + o.v, self.e + o.e)
        return V.rounded(self.v + o, self.e)

    def __sub__(self, o):
        if isinstance(o, V):
            return V.rounded(self.v - o.v, self.e + o.e)
        return V.rounded(self.v - o, self.e)

    def __rsub__(self, o):
        return V.rounded(o - self.v, self.e)

    def __mul__(self, o):
        with np.errstate(invalid="ignore"):
            if isinstance(o, V):
                return V.rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)
            return V.rounded(self.v * o, np.abs(o) * self.e)

    def __truediv__(self, o):
        with np.errstate(invalid="ignore", divide="ignore"):
            if isinstance(o, V):
                q = self.v / o.v
                return V.rounded(q, self.e / np.abs(o.v) + np.abs(q) / np.abs(o.v) * o.e)
            return V.rounded(self.v / o, self.e / np.abs(o))

    def exp(self):
        r = np.exp(self.v)
        return V.rounded(r, r * self.e, EXP)

    def log(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return V.rounded(np.log(self.v), self.e / np.abs(self.v), LOG)

    def tanh(self):
        r = np.tanh(self.v)
        with np.errstate(invalid="ignore"):
            return V.rounded(r, (1.0 - r * r) * self.e, TANH)

    def sqrt(self):
        r = np.sqrt(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            return V.rounded(r, np.where(r > 0, self.e / (2.0 * r), 0.0), SQRT)

    def sum(self, axis=None, keepdims=False):
        """n terms in any order: (n - 1) roundings, each of a partial sum no larger than sum|terms|"""
        n = self.v.size if axis is None else self.v.shape[axis]
        e = self.e.reshape(5, -1).sum(1) if axis is None else self.e.sum(axis + 1 if axis >= 0 else axis, keepdims=keepdims)
        e = np.array(e)
        e[PLAIN] += max(n - 1, 0) * U * np.abs(self.v).sum(axis=axis, keepdims=keepdims)
        return V(self.v.sum(axis=axis, keepdims=keepdims), e)

    def take(self, idx):
        """entry idx[r] of every row r of a [rows, C] value, as [rows, 1]"""
        r = np.arange(self.v.shape[0])
        return V(self.v[r, idx][:, None], self.e[:, r, idx][:, :, None])

    def where(self, cond, other):
        """cond ? self : the exact constant `other`"""
        return V(np.where(cond, self.v, other), np.where(cond, self.e, 0.0))


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64).copy())


# ================================================================================================ exact references
def to_point_major(src_cn):
    return np.ascontiguousarray(src_cn.transpose(0, 2, 1))


def to_channel_major(src_nc):
    return np.ascontiguousarray(src_nc.transpose(0, 2, 1))


def pgd_step_field(x, grad, ori, mask, c0, alpha, eps, direction, last, mutant=None):
    """x [B][N][9] after one sign step on channels c0:c0+3 (nontarget.py:37-39, target.py:41-43): points under `mask`
    ([N] or None) only; c0 = 3 projects onto the eps ball and then [0, 1], c0 = 0 onto the eps ball only; `last` returns
    the un-projected step.  alpha, eps, direction arrive as float32; the step is their float32 product."""
    x = x.copy()
    sel = slice(None) if mask is None else np.asarray(mask, bool)
    step = F(F(direction) * F(alpha))
    eps = F(eps)
    g = grad[:, sel, c0:c0 + 3]
    sg = np.where(g > 0, F(1), np.where(g < 0, F(-1), F(1) if mutant == "sign0" else F(0))).astype(F)
    move = (step * sg).astype(F)
    stepped = (x[:, sel, c0:c0 + 3] + move).astype(F)
    o = ori[:, sel]
    if mutant == "box_first":
        d = (np.minimum(np.maximum(stepped, F(0)), F(1)) - o).astype(F)
        proj = (o + np.minimum(np.maximum(d, -eps), eps)).astype(F)
    else:
        d = (stepped - o).astype(F)
        eta = np.minimum(np.maximum(d, -eps), eps)
        proj = (o + eta).astype(F)
        if c0 == 3 or mutant == "coord_box":
            proj = np.minimum(np.maximum(proj, F(0)), F(1))
    x[:, sel, c0:c0 + 3] = proj if (not last or mutant == "last_proj") else stepped
    return x


def pgd_step(x, grad, ori, mask, alpha, eps, direction, last, mutant=None):
    return pgd_step_field(x, grad, ori, mask, 3, alpha, eps, direction, last, mutant)


def seg_stats(logp, labels, n_cls):
    """pred = first arg-max; counters [3][n_cls] = seen, intersection, union (NB_nontarget_test_semseg.py:199-205)"""
    pred = logp.argmax(1).astype(np.int32)
    cnt = np.zeros((3, n_cls), np.int64)
    for c in range(n_cls):
        cnt[0, c] = (labels == c).sum()
        cnt[1, c] = ((pred == c) & (labels == c)).sum()
        cnt[2, c] = ((pred == c) | (labels == c)).sum()
    return cnt, pred


def latch_fire(n_correct, n_hits, n_mask, mode, dtype=np.float64):
    """the exit test (nontarget.py:87,95: the literal 4096 whatever N; target.py:105-121); 0 / 0 is NaN and never fires"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == 0:
            return dtype(n_correct) / dtype(4096) < dtype(1) / dtype(13)
        acc = dtype(n_hits) / dtype(n_mask)
        return acc > dtype(0.9) if mode == 2 else acc < dtype(1) / dtype(13)


def nu_step_latch(pred, labels, target, mask, n_mask, rows, mode, scal, x0, out, active, exit_step, step, mutant=None):
    """pred / labels [G*rows][N], mask [G][N] or None, scal [3][G], x0 [G*rows][N][9], out [G*rows][9][N].
    Returns (hist [5][G], scal, out, active, exit_step) after the call."""
    G = active.shape[0]
    N = pred.shape[1]
    out, active, exit_step = out.copy(), active.copy(), exit_step.copy()
    hist = np.zeros((5, G), F)
    for g in range(G):
        p, y = pred[g * rows:(g + 1) * rows], labels[g * rows:(g + 1) * rows]
        ok = p == y
        in_mask = np.ones(N, bool) if mask is None else mask[g] != 0
        hit = (p == target) if mode == 2 else ok
        n_correct = int(ok.sum())
        n_hits = int((hit if mode == 0 else hit & in_mask[None]).sum())
        hist[0, g], hist[1, g] = F(n_correct), F(n_hits)
        hist[2:, g] = scal[:, g]
        fire = bool(latch_fire(n_correct, n_hits, 0 if n_mask is None else int(n_mask[g]), mode))
        if fire and active[g] and (exit_step[g] < 0 or mutant == "refire"):
            out[g * rows:(g + 1) * rows] = x0[g * rows:(g + 1) * rows].transpose(0, 2, 1)
            exit_step[g] = step
            active[g] = 0
    return hist, np.zeros_like(scal), out, active, exit_step


def nu_restart_rooms(x0, x0_orig, mask, n_mask, flags, noise, noise_off, rows, mutant=None):
    """target.py:127-132 for the flagged groups: noise added to the masked colours by rank within the mask (ranks at or
    beyond n_mask[g] get none), then all nine channels clamped to [0, 1].  Returns (x0 exact float32, extra_l2 float64 [G],
    its error parts [5][G]); extra_l2 = sum((x0 - x0_orig)^2) over channels 0:3 and 6:9, NaN for unflagged groups."""
    x0 = x0.copy()
    G, N = mask.shape
    l2 = np.full(G, np.nan)
    e = np.zeros((5, G))
    for g in range(G):
        if not flags[g]:
            continue
        k = int(n_mask[g])
        on = mask[g] != 0
        rank = np.cumsum(on) - 1
        if mutant == "chunk_rank":
            rank = np.concatenate([np.cumsum(on[p:p + 256]) - 1 for p in range(0, N, 256)])
        pts = np.nonzero(on & (rank < k))[0]
        for row in range(rows):
            r = g * rows + row
            nz = noise[noise_off[g] + row * 3 * k: noise_off[g] + (row + 1) * 3 * k].reshape(3, k)
            x0[r, pts, 3:6] = (x0[r, pts, 3:6] + nz[:, rank[pts]].T).astype(F)
            if mutant == "clamp_colour_only":
                x0[r, :, 3:6] = np.minimum(np.maximum(x0[r, :, 3:6], F(0)), F(1))
            else:
                x0[r] = np.minimum(np.maximum(x0[r], F(0)), F(1))
        blk = slice(g * rows, (g + 1) * rows)
        d = V(x0[blk][:, :, [0, 1, 2, 6, 7, 8]]) - x0_orig[blk][:, :, [0, 1, 2, 6, 7, 8]].astype(np.float64)
        s = (d * d).sum()
        l2[g], e[:, g] = s.v, s.e
    return x0, l2, e


# ================================================================================================ float64 references
def ce_logp_grad(logp, labels, target, rows_active, scale, second=True):
    """d/dlogp of scale * sum_{r < rows_active} CE(logp_r, y_r), CE = log_softmax once more + NLL (nontarget.py:26,34,
    target.py:27,39).  Returns (dlogp [rows][C], cost, dlogp error parts, cost error parts)."""
    rows, C = logp.shape
    if rows_active == 0:
        return np.zeros((rows, C)), 0.0, np.zeros((5, rows, C)), np.zeros(5)
    y = np.full(rows, target, np.int64) if labels is None else labels.astype(np.int64)
    z = t64(logp).requires_grad_(True)
    lp2 = torch.log_softmax(z, 1) if second else z
    cost = -(lp2[:rows_active].gather(1, torch.from_numpy(y[:rows_active, None])).sum()) * float(scale)
    if rows_active:
        cost.backward()
    dl = np.zeros((rows, C)) if z.grad is None else z.grad.numpy()
    # the kernel's formula with its errors
    zz = V(logp[:rows_active])
    d = zz - logp[:rows_active].max(1, keepdims=True).astype(np.float64)
    lp = d - d.exp().sum(1, keepdims=True).log()
    onehot = np.arange(C)[None] == y[:rows_active, None]
    g = (lp.exp() - onehot.astype(np.float64)) * float(scale)
    e = np.zeros((5, rows, C))
    e[:, :rows_active] = g.e
    c = (lp.take(y[:rows_active]) * -float(scale)).sum()
    return dl, float(cost.detach()), e, c.e


def inverse_tanh(x0):
    """w = 0.5 log((1 + x) / (1 - x)), x = 2 c - 1, of the colours of x0 [B][N][9] (nontarget.py:110-116); (w, parts)"""
    c = x0[:, :, 3:6].astype(np.float64)
    x = t64(c) * 2 - 1
    with np.errstate(divide="ignore"):
        w = (0.5 * torch.log((1 + x) / (1 - x))).numpy()
        xv = V(c) * 2.0 - 1.0
        k = (((xv + 1.0) / (1.0 - xv)).log()) * 0.5
    return w, k.e


def tanh_color(w, mask, x0):
    """colour = 1/2 (tanh(w) + 1) into channels 3:6 of x0 (nontarget.py:107-108) under mask [N] (shared), [B][N] (per room)
    or None.  Returns (x0 float64 with untouched entries as given, parts (0 where untouched), written [B][N][9] bool)."""
    B, N, _ = x0.shape
    on = np.ones((B, N), bool) if mask is None else np.broadcast_to(np.asarray(mask, bool), (B, N))
    col = (0.5 * (torch.tanh(t64(w)) + 1)).numpy()
    k = (V(w).tanh() + 1.0) * 0.5
    out = x0.astype(np.float64)
    e = np.zeros((5,) + x0.shape)
    written = np.zeros(x0.shape, bool)
    written[:, :, 3:6] = on[:, :, None]
    out[:, :, 3:6] = np.where(on[:, :, None], col, out[:, :, 3:6])
    e[:, :, :, 3:6] = np.where(on[None, :, :, None], k.e, 0.0)
    return out, e, written


def softmax_f_decisions(logp, y, kappa, tsign, dtype):
    """the branch decisions of the f-loss evaluated in `dtype`: (arg-max, other class, pass)"""
    z = logp.astype(dtype)
    r = np.arange(len(z))
    p = np.exp(z - z.max(1, keepdims=True))
    p = p / p.sum(1, keepdims=True, dtype=dtype)
    others = p.copy()
    others[r, y] = -1
    oi = others.argmax(1)
    val = dtype(tsign) * (p[r, y] - p[r, oi])
    return z.argmax(1), oi, val >= -dtype(kappa), val


def nu_f_loss_grad(logp, labels, target, kappa, tsign, rows_per_sum=0, mutant=None):
    """f = clamp(tsign (p_y - max_{k != y} p_k), min = -kappa) on p = softmax(logp), summed (nontarget.py:119-128,
    target.py:148-168); rows_per_sum > 0: one sum per that many rows.  The maxima are taken as the reference takes them:
    torch.max over (1 - onehot) p and onehot p (first maximum; clamp passes the gradient at val >= -kappa).
    Returns (dlogp, f_sum [n_sums], pred, dlogp parts, f_sum parts)."""
    rows, C = logp.shape
    y = np.full(rows, target, np.int64) if labels is None else labels.astype(np.int64)
    z = t64(logp).requires_grad_(True)
    p = torch.softmax(z, 1)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(y), C).double()
    if mutant == "last_max":
        i, _ = torch.max(torch.flip((1 - onehot) * p, [1]), 1)
    else:
        i, _ = torch.max((1 - onehot) * p, 1)
    j, _ = torch.max(onehot * p, 1)
    val = float(tsign) * (j - i)
    if mutant == "gt":                     # clamp whose gradient passes only strictly above the threshold
        f = torch.where(val > -float(kappa), val, torch.full_like(val, -float(kappa)))
    else:
        f = torch.clamp(val, min=-float(kappa))
    f.sum().backward()
    n_sums = rows // rows_per_sum if rows_per_sum else 1
    fs = f.detach().numpy().reshape(n_sums, -1).sum(1)
    pred = logp.argmax(1).astype(np.int32)
    if mutant == "last_max":
        pred = (C - 1 - logp[:, ::-1].argmax(1)).astype(np.int32)
    # the kernel's formula with its errors, on the float64 decisions
    _, oi, passed, _ = softmax_f_decisions(logp, y, kappa, tsign, np.float64)
    d = V(logp) - logp.max(1, keepdims=True).astype(np.float64)
    ex = d.exp()
    pp = ex / ex.sum(1, keepdims=True)
    py, po = pp.take(y), pp.take(oi)
    v = (py - po) * float(tsign)
    fv = v.where(passed[:, None], -float(kappa))
    gy = np.where(passed, float(tsign), 0.0)[:, None]
    dot = py * gy + po * (-gy)
    cols = np.arange(C)[None]
    gc = np.where(cols == y[:, None], gy, np.where(cols == oi[:, None], -gy, 0.0))
    g = pp * (dot * -1.0 + gc)
    fe = np.stack([V(fv.v[s], fv.e[:, s]).sum().e for s in np.arange(rows).reshape(n_sums, -1)], 1)
    return z.grad.numpy(), fs, pred, g.e, fe


def gcn_f_decisions(z, y, mode, kappa, tsign, dtype):
    """(own > 0 [mode 0], pass) of the ResGCN f-loss evaluated in `dtype` on every row"""
    z = z.astype(dtype)
    r = np.arange(len(z))
    oth = z.copy()
    oth[r, y] = 0
    oth = np.maximum(oth.max(1), 0)
    own = z[r, y]
    live = own > 0
    if mode == 0:
        own = np.maximum(own, 0)
    val = dtype(tsign) * ((oth - own) if mode == 2 else (own - oth))
    return live, val >= -dtype(kappa), val


def gcn_f_loss_grad(z, labels, target, mask, mode, N, kappa, tsign, scale):
    """The f-losses of the ResGCN NU attacks on raw logits [rows][C], as the reference writes them (colper.py:108-113
    mode 0; tcolper.py:145-163 non_f mode 1, tar_f mode 2): one-hot products, torch.max over the class axis.  Modes 1, 2
    count batch row 0 (the first N rows) under mask [N] only.  Returns (scale d sum f / dz, sum f, pred, dz parts, f parts)."""
    rows, C = z.shape
    y = np.full(rows, target, np.int64) if (mode == 2 or labels is None) else labels.astype(np.int64)
    zt = t64(z).requires_grad_(True)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(y), C).double()
    oth, _ = torch.max((1 - onehot) * zt, 1)
    if mode == 0:
        own, _ = torch.max(onehot * zt, 1)
        counted = np.ones(rows, bool)
    else:
        own = zt.gather(1, torch.from_numpy(y[:, None]))[:, 0]
        counted = np.arange(rows) < N
        if mask is not None:
            counted[:N] &= np.asarray(mask, bool)
    val = float(tsign) * ((oth - own) if mode == 2 else (own - oth))
    f = torch.clamp(val, min=-float(kappa))[torch.from_numpy(counted)]
    (f.sum() * float(scale)).backward()
    vv = (V(oth.detach().numpy()) - own.detach().numpy()) if mode == 2 else (V(own.detach().numpy()) - oth.detach().numpy())
    fv = (vv * float(tsign)).where(val.detach().numpy() >= -float(kappa), -float(kappa))
    fe = V(np.where(counted, fv.v, 0.0), np.where(counted, fv.e, 0.0)).sum().e
    dz = zt.grad.numpy()
    e = np.zeros((5,) + dz.shape)
    e[PLAIN] = 2 * U * np.abs(dz)            # tsign * scale, and its negation or sum with an exact 0
    return dz, float(f.sum()), z.argmax(1).astype(np.int32), e, fe


def adam_update64(w, m, v, g, lr, beta1, beta2, eps, t, mutant=None):
    """torch.optim.Adam's single-tensor step in float64 (numpy): returns (w, m, v)"""
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * (g * g)
    tt = t - 1 if mutant == "bias_late" else t
    bc1, bc2 = 1 - beta1 ** tt, 1 - beta2 ** tt
    with np.errstate(invalid="ignore"):
        if mutant == "eps_inside":
            denom = np.sqrt(v / bc2 + eps)
        else:
            denom = np.sqrt(v) / np.sqrt(bc2) + eps
        return w + (-(lr / bc1)) * (m / denom), m, v


def nu_adam_step(w, m, v, mask, dx0, x0, ori, smooth_grad, c_smooth, c_l2, lr, beta1, beta2, eps, step, rooms=False,
                 room_active=None, mutant=None):
    """One optimiser step of NU_attack / tar_NU_attack on w [B][N][3] (nontarget.py:77-93): the gradient of
    sum(dx0 colour) + c_l2 sum((colour - ori)^2) + c_smooth sum(smooth_grad colour) w.r.t. w through colour =
    1/2 (tanh(w) + 1) by autograd (the colour's VALUE is the one stored in x0), then Adam.  mask [N] and smooth_grad [N][3]
    on batch row 0 (plain), or mask [B][N], smooth_grad [B][N][3] and one L2 sum per room (rooms; room_active [B] or None).
    Entries outside the mask and inactive rooms keep their values.  Returns (w, m, v, l2 [n_sums], parts of each)."""
    B, N, _ = w.shape
    on = np.ones((B, N), bool) if mask is None else np.broadcast_to(np.asarray(mask, bool), (B, N)).copy()
    if rooms and room_active is not None:
        on &= np.asarray(room_active, bool)[:, None]
    on3 = np.broadcast_to(on[:, :, None], w.shape)
    sg = np.zeros(w.shape)
    if smooth_grad is not None:
        if rooms:
            sg[:] = smooth_grad
        else:
            sg[0] = smooth_grad
    col_in = x0[:, :, 3:6].astype(np.float64)
    wt = t64(w).requires_grad_(True)
    th = torch.tanh(wt)
    col = 0.5 * (th + 1)
    col = t64(col_in) + (col - col.detach())           # the stored colour, with the derivative of tanh_space
    diff = col - t64(ori)
    loss = (t64(dx0[:, :, 3:6]) * col).sum() + float(c_l2) * (diff * diff).sum() + float(c_smooth) * (t64(sg) * col).sum()
    loss.backward()
    g = wt.grad.numpy()
    if mutant == "no_chain":
        with np.errstate(invalid="ignore", divide="ignore"):
            g = dx0[:, :, 3:6] + 2 * float(c_l2) * (col_in - ori) + float(c_smooth) * sg
    w2, m2, v2 = adam_update64(w.astype(np.float64), m.astype(np.float64), v.astype(np.float64), g, float(lr), float(beta1),
                               float(beta2), float(eps), step, mutant)
    w2, m2, v2 = (np.where(on3, a, b.astype(np.float64)) for a, b in ((w2, w), (m2, m), (v2, v)))
    d64 = np.where(on3, col_in - ori, 0.0)
    # the kernel's formula with its errors
    dv = V(col_in) - ori.astype(np.float64)
    sq = dv * dv
    gv = dv * (float(c_l2) * 2.0) + dx0[:, :, 3:6].astype(np.float64)
    if smooth_grad is not None:
        gv = gv + V(sg) * float(c_smooth)
    tv = V(w).tanh()
    gv = gv * 0.5 * (1.0 - tv * tv)
    mv = V(m) + (gv - V(m)) * (1 - float(beta1))
    vv = V(v) * float(beta2) + (gv * gv) * (1 - float(beta2))
    bc1, bc2 = 1 - float(beta1) ** step, 1 - float(beta2) ** step
    full = lambda c: V.rounded(np.full(w.shape, c), np.zeros((5,) + w.shape))     # noqa: E731  (a constant rounded to float32)
    denom = vv.sqrt() / full(np.sqrt(bc2)) + float(eps)
    wv = V(w) + (mv / denom) * full(-(float(lr) / bc1))
    keep = lambda k: np.where(on3[None], k.e, 0.0)                                # noqa: E731
    if rooms:
        l2 = d64.reshape(B, -1) ** 2
        l2e = np.stack([V(np.where(on3[b], sq.v[b], 0.0), np.where(on3[b][None], sq.e[:, b], 0.0)).sum().e for b in range(B)], 1)
        l2 = l2.sum(1)
    else:
        l2 = np.array([(d64 ** 2).sum()])
        l2e = V(np.where(on3, sq.v, 0.0), np.where(on3[None], sq.e, 0.0)).sum().e[:, None]
    return w2, m2, v2, l2, keep(wv), keep(mv), keep(vv), l2e
