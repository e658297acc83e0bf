"""Plain references for the whole-scene NU attack kernels of csrc/psg_scene_nu.hip.

TEST INFRASTRUCTURE ONLY: no GPU, no oracle import.  Three layers:
  EXACT (numpy float32 / Python integers, compared bit for bit): the two ordered list sums (scene_ref.grad_sum's walk), the
  set of points that move, the latch's counters and its integer decision.
  FLOAT32 RESTATEMENT (step32: one IEEE operation per line, numpy's tanh / sqrt standing in for the device's): the gradient
  assembly and torch's single-tensor Adam in nu_adam_step_kernel's expression order.
  FLOAT64 (step64, init64, colour64): attack_ref64.nu_adam_step / inverse_tanh / tanh_color at B = 1, N = n_scene, fed the
  float32 sums as dx0 and smooth_grad, with attack_ref64's first-order error model - what the kernels are held to.
stated_cost_step64 is the independent pin: float64 autograd of the cost AS THE ISSUE STATES IT, over the slots,
  sum_e <dx0[e] + cw sgrad[e], col[idx[e]]> + cw sum_p |col_p - c0_p|^2,   col = 1/2 (tanh w + 1),
followed by attack_ref64.adam_update64; it fixes "L2 once per point, the rest summed over slots"."""
import numpy as np
import torch

import attack_ref64
import scene_ref

F = np.float32
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8

SUM_MUTANTS = ("descending", "drop_last", "smooth_first_slot_only")
STEP_MUTANTS = ("l2_per_slot", "no_chain", "bias_late", "moves_unmasked")
MUTANTS = SUM_MUTANTS + STEP_MUTANTS + ("latch_float_division",)


def pad9(d3):
    """[rows][3] -> [rows][9] with the values in channels 3:6 (what scene_ref.grad_sum reads)"""
    out = np.zeros((d3.shape[0], 9), F)
    out[:, 3:6] = d3
    return out


def moves(occ_off, scene_mask, mutant=None):
    """the points that move: at least one slot, and under the mask"""
    mv = (occ_off[1:] - occ_off[:-1]) > 0
    if scene_mask is not None and mutant != "moves_unmasked":
        mv = mv & np.asarray(scene_mask, bool)
    return mv


def ordered_sums(dx0, sgrad, occ_off, occ_ent, scene_mask, mutant=None):
    """(Gf, Gs) [n_scene][3] float32: ((0 + d[e_0]) + d[e_1]) + ... over every moving point's slots in list order, d =
    dx0[e][3:6] and sgrad[e]; +0 for the other points"""
    mask = None if mutant == "moves_unmasked" else scene_mask
    order = mutant if mutant in ("descending", "drop_last") else None
    gf = scene_ref.grad_sum(dx0, occ_off, occ_ent, mask, order)
    if mutant == "smooth_first_slot_only":
        first = occ_ent[np.minimum(occ_off[:-1], occ_ent.size - 1)]
        gs = (np.zeros((occ_off.size - 1, 3), F) + sgrad[first]).astype(F)
        gs[~moves(occ_off, mask)] = F(0)
    else:
        gs = scene_ref.grad_sum(pad9(sgrad), occ_off, occ_ent, mask, order)
    return gf, gs


def adam_consts(lr, step):
    """(step_size, bc2_sqrt) as psg_nu_adam_step computes them: in double on the host from the float32 arguments"""
    bc1 = 1.0 - float(F(BETA1)) ** step
    bc2 = 1.0 - float(F(BETA2)) ** step
    return F(float(F(lr)) / bc1), F(np.sqrt(bc2))


def step32(w, m, v, c, c0, dx0, sgrad, occ_off, occ_ent, scene_mask, cw, lr, step):
    """One step in float32, one IEEE operation per line, nu_adam_step_kernel's expression order.  Returns (w, m, v, Gf, Gs)."""
    gf, gs = ordered_sums(dx0, sgrad, occ_off, occ_ent, scene_mask)
    mv = moves(occ_off, scene_mask)[:, None]
    cw, b1, b2, eps = F(cw), F(BETA1), F(BETA2), F(ADAM_EPS)
    step_size, bc2_sqrt = adam_consts(lr, step)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        diff = (c - c0).astype(F)
        l2w = (cw * F(2)).astype(F)
        l2g = (l2w * diff).astype(F)
        g = (gf + l2g).astype(F)
        sg = (cw * gs).astype(F)
        g = (g + sg).astype(F)
        th = np.tanh(w.astype(F)).astype(F)
        tt = (th * th).astype(F)
        one_tt = (F(1) - tt).astype(F)
        gh = (g * F(0.5)).astype(F)
        g = (gh * one_tt).astype(F)
        gm = (g - m).astype(F)
        ob1 = F(F(1) - b1)
        dm = (gm * ob1).astype(F)
        mm = (m + dm).astype(F)
        vb = (v * b2).astype(F)
        gg = (g * g).astype(F)
        ob2 = F(F(1) - b2)
        dv = (ob2 * gg).astype(F)
        vv = (vb + dv).astype(F)
        sq = np.sqrt(vv).astype(F)
        sqb = (sq / bc2_sqrt).astype(F)
        denom = (sqb + eps).astype(F)
        q = (mm / denom).astype(F)
        dw = (F(-step_size) * q).astype(F)
        ww = (w + dw).astype(F)
    return np.where(mv, ww, w), np.where(mv, mm, m), np.where(mv, vv, v), gf, gs


def step64(w, m, v, c, c0, dx0, sgrad, occ_off, occ_ent, scene_mask, cw, lr, step, mutant=None):
    """The float64 reference of psg_scene_nu_step FED THE FLOAT32 SUMS: attack_ref64.nu_adam_step at B = 1, N = n_scene.
    Returns (w, m, v [n_scene][3] float64, error parts of each [5][n_scene][3], Gf, Gs float32)."""
    assert mutant is None or mutant in SUM_MUTANTS + STEP_MUTANTS
    gf, gs = ordered_sums(dx0, sgrad, occ_off, occ_ent, scene_mask, mutant)
    mv = moves(occ_off, scene_mask, mutant)
    n = w.shape[0]
    lin = np.zeros((1, n, 9))
    lin[0, :, 3:6] = gf
    if mutant == "l2_per_slot":              # the L2 gradient once per SLOT: (length - 1) more copies of cw 2 (c - c0)
        length = (occ_off[1:] - occ_off[:-1]).astype(np.float64)[:, None]
        with np.errstate(invalid="ignore"):
            lin[0, :, 3:6] += (length - 1) * 2.0 * float(F(cw)) * (c.astype(np.float64) - c0.astype(np.float64))
    x0 = np.zeros((1, n, 9), F)
    x0[0, :, 3:6] = c
    inner = mutant if mutant in ("no_chain", "bias_late") else None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w2, m2, v2, _, we, me, ve, _ = attack_ref64.nu_adam_step(
            w[None], m[None], v[None], mv, lin, x0, c0[None], gs.astype(np.float64), float(F(cw)), float(F(cw)), float(F(lr)),
            float(F(BETA1)), float(F(BETA2)), float(F(ADAM_EPS)), step, mutant=inner)
    return w2[0], m2[0], v2[0], we[:, 0], me[:, 0], ve[:, 0], gf, gs


def stated_cost_step64(w, m, v, c0, dx0, sgrad, point_idx, scene_mask, cw, lr, step):
    """float64 autograd of the cost as the issue states it - the linear terms over the SLOTS, the L2 term over the POINTS -
    then torch's Adam in float64.  Points that do not move keep their values."""
    idx = torch.from_numpy(np.asarray(point_idx).reshape(-1).astype(np.int64))
    n = w.shape[0]
    mv = np.bincount(idx.numpy(), minlength=n) > 0
    if scene_mask is not None:
        mv &= np.asarray(scene_mask, bool)
    wt = attack_ref64.t64(w).requires_grad_(True)
    col = 0.5 * (torch.tanh(wt) + 1)
    on = torch.from_numpy(mv)[idx]                                     # slots of points that do not move give nothing
    lin = attack_ref64.t64(dx0[:, 3:6]) + float(F(cw)) * attack_ref64.t64(sgrad)
    cost = (lin[on] * col[idx[on]]).sum() + float(F(cw)) * ((col - attack_ref64.t64(c0)) ** 2)[torch.from_numpy(mv)].sum()
    cost.backward()
    g = wt.grad.numpy()
    w2, m2, v2 = attack_ref64.adam_update64(w.astype(np.float64), m.astype(np.float64), v.astype(np.float64), g, float(F(lr)),
                                            float(F(BETA1)), float(F(BETA2)), float(F(ADAM_EPS)), step)
    keep = mv[:, None]
    return np.where(keep, w2, w), np.where(keep, m2, m), np.where(keep, v2, v)


def init64(c0):
    """(w float64 [n_scene][3], error parts) of psg_scene_nu_init"""
    x0 = np.zeros((1, c0.shape[0], 9), F)
    x0[0, :, 3:6] = c0
    w, e = attack_ref64.inverse_tanh(x0)
    return w[0], e[:, 0]


def colour64(w, c, occ_off, scene_mask):
    """(c float64 [n_scene][3] after psg_scene_nu_colour, error parts (0 where untouched), written [n_scene] bool)"""
    mv = moves(occ_off, scene_mask)
    x0 = np.zeros((1, c.shape[0], 9), F)
    x0[0, :, 3:6] = c
    out, e, _ = attack_ref64.tanh_color(w[None], mv[None], x0)
    return out[0, :, 3:6], e[:, 0, :, 3:6], mv


def within(got, want, e):
    """[..] bool: |got - want| <= attack_ref64.bound(e), or the same value exactly (infinities), or NaN on both sides"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        return (got == want) | (np.abs(got - want) <= attack_ref64.bound(e)) | (np.isnan(got) & np.isnan(want))


def ratio(got, want, e):
    """largest |error| / first-order bound over the entries where both are finite"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / attack_ref64.first_order(e)
    ok = np.isfinite(r)
    return float(r[ok].max()) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------ the exit latch
def latch_counts(pred, labels, target, point_idx, scene_mask):
    """(n_hits, n_counted) as Python integers.  Non-targeted (scene_mask None): slots with pred == label, all slots.
    Targeted: slots of masked points with pred == target, slots of masked points."""
    pred = np.asarray(pred).reshape(-1)
    if scene_mask is None:
        return int((pred == np.asarray(labels).reshape(-1)).sum()), int(pred.size)
    on = np.asarray(scene_mask, bool)[np.asarray(point_idx).reshape(-1)]
    return int((on & (pred == target)).sum()), int(on.sum())


def latch_fire(n_hits, n_counted, num, den, targeted, mutant=None):
    """the decision, in integers (Python's are unbounded; the kernel's 64-bit products cannot overflow below 2^31 each)"""
    if mutant == "latch_float_division":
        with np.errstate(divide="ignore", invalid="ignore"):
            acc, bar = F(n_hits) / F(n_counted), F(num) / F(den)
        return bool(acc > bar) if targeted else bool(acc < bar)
    assert mutant is None
    return n_hits * den > num * n_counted if targeted else n_hits * den < num * n_counted


def latch_fire_quotients(n_hits, n_counted, num, den, targeted):
    """the same test written with double-precision quotients (0 / 0 never fires)"""
    if n_counted == 0:
        return False
    acc, bar = np.float64(n_hits) / np.float64(n_counted), np.float64(num) / np.float64(den)
    return bool(acc > bar) if targeted else bool(acc < bar)


# (n_hits, n_counted, num, den): the inputs the latch tests list beyond the exhaustive small ones - equality at counts that
# float32 cannot hold (above 2^24 a counter is rounded before the division), and the largest slot count the entry points take
LATCH_INPUTS = [
    (1290559, 16777267, 1, 13),                        # exactly 1 / 13: no exit; the float32 quotient lies below 1 / 13
    (16777251, 18641390, 9, 10),                       # exactly 9 / 10: no exit; the float32 quotient lies above 9 / 10
    (2 ** 24 + 1, 13 * (2 ** 24 + 1), 1, 13),
    (9 * (2 ** 24 + 1) + 1, 10 * (2 ** 24 + 1), 9, 10),
    (2 ** 24, 13 * 2 ** 24 + 1, 1, 13),
    (0, 5003, 0, 1), (5003, 5003, 0, 1), (0, 0, 9, 10), (0, 0, 1, 13),
    (238609294, 238609294, 9, 10), (18354560, 238609294, 1, 13),     # rows = INT_MAX / 9
]


def latch(pred, labels, target, point_idx, scene_mask, num, den, step, c, snap, exit_step, active):
    """(hist_row or None, snap, exit_step, active) after psg_scene_nu_latch; active == 0 leaves everything"""
    if not active:
        return None, snap, exit_step, active
    n_hits, n_counted = latch_counts(pred, labels, target, point_idx, scene_mask)
    if latch_fire(n_hits, n_counted, num, den, scene_mask is not None):
        return (n_hits, n_counted), c.copy(), step, 0
    return (n_hits, n_counted), snap, exit_step, active


def first_exit(history, num, den, targeted):
    """the step at which the integer rule first fires on recorded (n_hits, n_counted) rows, or -1"""
    for s, (h, n) in enumerate(np.asarray(history).tolist()):
        if latch_fire(int(h), int(n), num, den, targeted):
            return s
    return -1


# ------------------------------------------------------------------------------------------------ shared test inputs
CW, LR = 1e-4, 0.01                                       # the attack's defaults
STEP_CASES = [(1, False), (2, True), (1000, True)]        # (Adam step, warm state): the CPU mutants and the GPU kernels


def nu_step_case(seed, point_idx, n_scene, warm):
    """(w, m, v, c, c0, dx0 [rows][9], sgrad [rows][3], mask) for psg_scene_nu_step on scene_ref.step_case's gradients (exact
    zeros, a cancelling pair, a NaN, the order-sensitive triple 1, 1e8, -1e8 - in dx0 AND in sgrad), clean colours at 0, 1,
    1 / 255 and 254 / 255 (w = -inf, +inf and the two largest finite magnitudes a scene has).  warm: moments and a
    displaced w as after some steps; else the state before step 1 (w = inverse_tanh_space(c0), m = v = 0)."""
    rng = np.random.default_rng(seed)
    _, _, dx0, mask = scene_ref.step_case(seed, point_idx, n_scene)
    dx0 = (dx0 * F(0.01)).astype(F)                      # block gradients are small; the triple stays order-sensitive
    off, ent = scene_ref.occ_lists(point_idx, n_scene)
    t = ent[off[np.nonzero((off[1:] - off[:-1]) == 3)[0][0]]:][:3]
    dx0[t[0], 3:6], dx0[t[1], 3:6], dx0[t[2], 3:6] = F(1), F(1e8), F(-1e8)
    sgrad = rng.standard_normal((point_idx.size, 3)).astype(F)
    sgrad[t[0]], sgrad[t[1]], sgrad[t[2]] = F(1), F(1e8), F(-1e8)
    c0 = (np.floor(rng.random((n_scene, 3)) * 256.0) / 255.0).astype(F)
    c0[0::9], c0[1::9], c0[2::9], c0[3::9] = F(0), F(1), F(1 / 255.0), F(254 / 255.0)
    with np.errstate(divide="ignore"):
        x = (c0 * F(2) - F(1)).astype(F)
        w = (F(0.5) * np.log(((F(1) + x) / (F(1) - x)).astype(F)).astype(F)).astype(F)
    m, v = np.zeros((n_scene, 3), F), np.zeros((n_scene, 3), F)
    if warm:
        w = (w + rng.standard_normal((n_scene, 3)).astype(F) * F(0.05)).astype(F)
        m = (rng.standard_normal((n_scene, 3)) * 1e-3).astype(F)
        v = (rng.random((n_scene, 3)) * 1e-6).astype(F)
    mv = (off[1:] - off[:-1]) > 0
    with np.errstate(invalid="ignore"):
        c = np.where(mv[:, None], (F(0.5) * (np.tanh(w) + F(1)).astype(F)).astype(F), c0).astype(F)
    return w, m, v, c, c0, dx0, sgrad, mask


def latch_case(seed, point_idx, n_scene):
    """(pred, labels [rows] int32, target, mask [n_scene] bool, c [n_scene][3])"""
    rng = np.random.default_rng(seed)
    rows = point_idx.size
    labels = rng.integers(0, 13, rows).astype(np.int32)
    pred = np.where(rng.random(rows) < 0.4, labels, rng.integers(0, 13, rows)).astype(np.int32)
    mask = rng.random(n_scene) < 0.3
    mask[9] = True                                       # the point with 3000 slots counts
    return pred, labels, 4, mask, rng.random((n_scene, 3)).astype(F)
