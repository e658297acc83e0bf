"""Plain references for the coordinate field of the whole-scene NU attack (csrc/psg_scene_nu.hip: psg_scene_nu_field_step;
DESIGN.md section 5z).

TEST INFRASTRUCTURE ONLY: no GPU, no oracle import.  The layers of tests/scene_nu_ref.py:
  EXACT (numpy float32, compared bit for bit): the two ordered list sums - scene_nu_ref.ordered_sums on rows that carry
  channels 0:3 where it reads - and the set of points that move.
  FLOAT32 RESTATEMENT (step32: one IEEE operation per line, numpy's sqrt standing in for the device's): the gradient assembly
  of nu_coord_adam_kernel and torch's single-tensor Adam on the displacement itself (no tanh space).
  FLOAT64 (step64): nu_field_ref64.coord_adam_step at B = 1, N = n_scene, fed the float32 sums as dx0[0:3] and sgrad_xyz, with
  attack_ref64's first-order error model - what the kernel is held to, through scene_nu_ref.within: the expression
  tests/test_gpu_nu_field_kernels.py applies to psg_nu_coord_adam_step_rooms (equal, or |got - want| <= attack_ref64.bound),
  a NaN on both sides counting as equal because these inputs carry one.
stated_cost_step64 is the independent pin: float64 autograd of the cost as it is stated, over the slots,
  sum_e <dx0[e][0:3] + coord_c sgrad[e], delta[idx[e]]> + coord_c sum_p |delta_p|^2,
followed by attack_ref64.adam_update64; it fixes "L2 once per point, the rest summed over slots"."""
import numpy as np
import torch

import attack_ref64
import nu_field_ref64
import scene_nu_ref
import scene_ref
from scene_nu_ref import ADAM_EPS, BETA1, BETA2, adam_consts, moves, ratio, within  # noqa: F401

F = np.float32

SUM_MUTANTS = ("descending", "drop_last", "smooth_first_slot_only")
# l2_per_slot shows in warm cases only: before step 1 delta is zero and the L2 gradient with it, however often it is counted
STEP_MUTANTS = ("l2_per_slot", "tanh_chain", "smooth_unweighted", "bias_late", "moves_unmasked")

COORD_C, COORD_LR = 1e-4, 0.01                            # the attack's defaults (c and lr)
STEP_CASES = [(1, False), (2, True), (1000, True)]        # (Adam step, warm state): the CPU mutants and the GPU kernel


def pad9(d3):
    """[rows][3] -> [rows][9] with the values in channels 3:6, where scene_nu_ref.ordered_sums reads the block gradients"""
    return scene_nu_ref.pad9(np.ascontiguousarray(d3, F))


def ordered_sums(dx0, sgrad_xyz, occ_off, occ_ent, scene_mask, mutant=None):
    """(Gx, Gs) [n_scene][3] float32: ((0 + d[e_0]) + d[e_1]) + ... over every moving point's slots in list order, d =
    dx0[e][0:3] and sgrad_xyz[e]; +0 for the other points"""
    return scene_nu_ref.ordered_sums(pad9(dx0.reshape(-1, 9)[:, 0:3]), sgrad_xyz.reshape(-1, 3), occ_off, occ_ent, scene_mask, mutant)


def step32(delta, m, v, dx0, sgrad_xyz, occ_off, occ_ent, scene_mask, coord_c, coord_lr, step):
    """One step in float32, one IEEE operation per line, nu_coord_adam_kernel's expression order.  Returns (delta, m, v, Gx, Gs)."""
    gx, gs = ordered_sums(dx0, sgrad_xyz, occ_off, occ_ent, scene_mask)
    mv = moves(occ_off, scene_mask)[:, None]
    cc, b1, b2, eps = F(coord_c), F(BETA1), F(BETA2), F(ADAM_EPS)
    step_size, bc2_sqrt = adam_consts(coord_lr, step)
    d = delta.astype(F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        l2w = F(cc * F(2))
        l2g = (l2w * d).astype(F)
        g = (gx + l2g).astype(F)
        sg = (cc * gs).astype(F)
        g = (g + sg).astype(F)
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
        dd = (F(-step_size) * q).astype(F)
        new = (d + dd).astype(F)
    return np.where(mv, new, delta), np.where(mv, mm, m), np.where(mv, vv, v), gx, gs


def step64(delta, m, v, dx0, sgrad_xyz, occ_off, occ_ent, scene_mask, coord_c, coord_lr, step, mutant=None):
    """The float64 reference of psg_scene_nu_field_step FED THE FLOAT32 SUMS: nu_field_ref64.coord_adam_step at B = 1, N =
    n_scene.  Returns (delta, m, v [n_scene][3] float64, error parts of each [5][n_scene][3], Gx, Gs float32).  A mutant
    returns the values of a wrong step (the gradient written out, then attack_ref64.adam_update64) and None for the parts."""
    assert mutant is None or mutant in SUM_MUTANTS + STEP_MUTANTS
    gx, gs = ordered_sums(dx0, sgrad_xyz, occ_off, occ_ent, scene_mask, mutant)
    mv = moves(occ_off, scene_mask, mutant)
    n = delta.shape[0]
    cc, lr = float(F(coord_c)), float(F(coord_lr))
    b1, b2, eps = float(F(BETA1)), float(F(BETA2)), float(F(ADAM_EPS))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mutant is None:
            lin = np.zeros((1, n, 9), F)
            lin[0, :, 0:3] = gx
            d2, m2, v2, _, de, me, ve, _ = nu_field_ref64.coord_adam_step(delta[None], m[None], v[None], mv[None], lin, gs[None], cc, lr,
                                                                          b1, b2, eps, step)
            return d2[0], m2[0], v2[0], de[:, 0], me[:, 0], ve[:, 0], gx, gs
        d64, m64, v64 = delta.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
        counted = (occ_off[1:] - occ_off[:-1]).astype(np.float64)[:, None] if mutant == "l2_per_slot" else 1.0
        g = gx.astype(np.float64) + counted * 2.0 * cc * d64
        g = g + (1.0 if mutant == "smooth_unweighted" else cc) * gs.astype(np.float64)
        if mutant == "tanh_chain":               # the colour path's factor, which has no business on a displacement
            g = g * 0.5 * (1.0 - np.tanh(d64) ** 2)
        d2, m2, v2 = attack_ref64.adam_update64(d64, m64, v64, g, lr, b1, b2, eps, step, mutant if mutant == "bias_late" else None)
    keep = mv[:, None]
    return np.where(keep, d2, d64), np.where(keep, m2, m64), np.where(keep, v2, v64), None, None, None, gx, gs


def stated_cost_step64(delta, m, v, dx0, sgrad_xyz, point_idx, scene_mask, coord_c, coord_lr, step):
    """float64 autograd of the cost as it is stated - the linear terms over the SLOTS, the L2 term over the POINTS - then
    torch's Adam in float64.  Points that do not move keep their values."""
    idx = torch.from_numpy(np.asarray(point_idx).reshape(-1).astype(np.int64))
    n = delta.shape[0]
    mv = np.bincount(idx.numpy(), minlength=n) > 0
    if scene_mask is not None:
        mv &= np.asarray(scene_mask, bool)
    cc = float(F(coord_c))
    dt = attack_ref64.t64(delta).requires_grad_(True)
    on = torch.from_numpy(mv)[idx]                                     # slots of points that do not move give nothing
    lin = attack_ref64.t64(dx0.reshape(-1, 9)[:, 0:3]) + cc * attack_ref64.t64(sgrad_xyz.reshape(-1, 3))
    cost = (lin[on] * dt[idx[on]]).sum() + cc * (dt ** 2)[torch.from_numpy(mv)].sum()
    cost.backward()
    g = dt.grad.numpy()
    d2, m2, v2 = attack_ref64.adam_update64(delta.astype(np.float64), m.astype(np.float64), v.astype(np.float64), g,
                                            float(F(coord_lr)), float(F(BETA1)), float(F(BETA2)), float(F(ADAM_EPS)), step)
    keep = mv[:, None]
    return np.where(keep, d2, delta), np.where(keep, m2, m), np.where(keep, v2, v)


# ------------------------------------------------------------------------------------------------ shared test inputs
def field_step_case(seed, point_idx, n_scene, warm):
    """(delta, m, v, dx0 [rows][9], sgrad_xyz [rows][3], mask) for psg_scene_nu_field_step: scene_ref.step_case's gradients
    (exact zeros, a cancelling pair, a NaN, the order-sensitive triple 1, 1e8, -1e8) carried to channels 0:3 with other random
    numbers in 3:9; the triple and a NaN in sgrad_xyz as well.  warm: displacements between 1e-5 and 1e-2 m and moments as
    after some steps; else the state before step 1 (delta = m = v = 0)."""
    rng = np.random.default_rng(seed + 200)
    _, _, dx0_c, mask = scene_ref.step_case(seed, point_idx, n_scene)
    dx0 = rng.standard_normal(dx0_c.shape).astype(F)
    dx0[:, 0:3] = (dx0_c[:, 3:6] * F(0.01)).astype(F)      # block gradients are small; the triple below stays order-sensitive
    off, ent = scene_ref.occ_lists(point_idx, n_scene)
    length = off[1:] - off[:-1]
    t = ent[off[np.nonzero(length == 3)[0][0]]:][:3]
    dx0[t[0], 0:3], dx0[t[1], 0:3], dx0[t[2], 0:3] = F(1), F(1e8), F(-1e8)
    sgrad = rng.standard_normal((point_idx.size, 3)).astype(F)
    sgrad[t[0]], sgrad[t[1]], sgrad[t[2]] = F(1), F(1e8), F(-1e8)
    sgrad[ent[off[np.nonzero(length == 1)[0][3]]], 2] = F(np.nan)
    delta, m, v = np.zeros((n_scene, 3), F), np.zeros((n_scene, 3), F), np.zeros((n_scene, 3), F)
    if warm:
        delta = (rng.standard_normal((n_scene, 3)) * 10.0 ** rng.uniform(-5, -2, (n_scene, 3))).astype(F)
        m = (rng.standard_normal((n_scene, 3)) * 1e-3).astype(F)
        v = (rng.random((n_scene, 3)) * 1e-6).astype(F)
    return delta, m, v, dx0, sgrad, mask
