"""Float64 references and derived bounds for the coordinate-field NU kernels of csrc/psg_nu_field.cuh.

TEST INFRASTRUCTURE ONLY: no GPU.  Error models of the element-wise kernels are attack_ref64's (class V / bound).

Smooth term, derived (u = 2^-24): the kernel rounds each difference once (relative u, i.e. 2 u on its square), adds the three
squares with three roundings of partial sums no larger than the total (3 u) - at most 5 u on d^2, 2.5 u on d - and rounds the
square root once: |d_fp32 - d| <= 3.5 u d (1 + O(u)) <= D_ULPS u d with D_ULPS = 4.  A gradient term (a - r) / d has one
rounding in the difference, D_ULPS u in d and one in the division: (D_ULPS + 2) u |term|; nb terms added in fp32 add
(nb - 1) u sum|terms|.  Sums of n distances in any order: D_ULPS u sum d + (n - 1) u sum d.  The factor (1 + 2^-10) covers the
second-order terms, 2^-149 a result that underflows."""
import numpy as np
import torch

import attack_ref64 as A

F = np.float32
U = A.U
D_ULPS = 4.0
SLACK = 1.0 + 2.0 ** -10


# ------------------------------------------------------------------------------------------------ distances in fp32, two ways
def dist_direct_fp32(a, r):
    """[Na, Nr] fp32 distances the way smooth_knn_xyz_kernel evaluates them: rounded differences, squares added as
    fma(dz, dz, fma(dy, dy, dx * dx)) (each fma = the exact product-sum rounded once, computed in float64 here: a product of
    two fp32 numbers plus an fp32 number is exact in float64 up to one rounding far below fp32's), then sqrt."""
    a, r = a.astype(F), r.astype(F)
    d = (a[:, None, :] - r[None, :, :]).astype(F)
    s = (d[..., 0] * d[..., 0]).astype(F)
    s = (d[..., 1].astype(np.float64) * d[..., 1] + s).astype(F)
    s = (d[..., 2].astype(np.float64) * d[..., 2] + s).astype(F)
    return np.sqrt(s).astype(F)


def dist_expansion_fp32(a, r):
    """The colour kernel's distance (smooth_knn_kernel = torch.cdist's matmul expansion) restated in fp32 numpy:
    fma(-2 az, rz, fma(-2 ay, ry, -2 ax * rx)) + |a|^2 + |r|^2, clamped at 0, sqrt."""
    a, r = a.astype(F), r.astype(F)
    asq = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]).astype(F)
    rsq = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]).astype(F)
    m2 = (F(-2) * a).astype(F)
    s = (m2[:, None, 0] * r[None, :, 0]).astype(F)
    s = (m2[:, None, 1].astype(np.float64) * r[None, :, 1] + s).astype(F)
    s = (m2[:, None, 2].astype(np.float64) * r[None, :, 2] + s).astype(F)
    s = ((s + asq[:, None]).astype(F) + rsq[None, :]).astype(F)
    return np.sqrt(np.maximum(s, F(0))).astype(F)


def dist64(a, r):
    d = a.astype(np.float64)[:, None, :] - r.astype(np.float64)[None, :, :]
    return np.sqrt((d * d).sum(-1))


# ------------------------------------------------------------------------------------------------ Smooth_xyz
def smooth_xyz(adv, ref, nb, mutant=None):
    """One room: adv / ref [N][3] (fp32 values, float64 arithmetic).  Neighbours by (distance, index), lower index first
    (mutant "tie_high": higher index first).  Returns dict: idx [N][nb], d [N][nb], next_d [N] (rank nb + 1, inf if none),
    total, grad [N][3] with a neighbour at distance 0 adding exactly zero (mutant "zero_unit": it adds the unit vector
    (1, 0, 0)), abs_terms [N][3] = sum_j |(a - r_j) / d_j| per component."""
    d = dist64(adv, ref)
    N = d.shape[1]
    if mutant == "tie_high":
        order = (N - 1 - np.argsort(d[:, ::-1], axis=1, kind="stable"))
    else:
        order = np.argsort(d, axis=1, kind="stable")
    idx = order[:, :nb]
    dn = np.take_along_axis(d, idx, 1)
    next_d = np.take_along_axis(d, order[:, nb:nb + 1], 1)[:, 0] if N > nb else np.full(len(d), np.inf)
    g, absg = grad_on(adv, ref, idx, mutant)
    return dict(idx=idx.astype(np.int32), d=dn, next_d=next_d, total=float(dn.sum()), grad=g, abs_terms=absg)


def grad_on(adv, ref, idx, mutant=None):
    """(grad [N][3], sum of |terms| [N][3]) of sum_j |a - r_j| w.r.t. a over the given neighbour lists, float64."""
    diff = adv.astype(np.float64)[:, None, :] - ref.astype(np.float64)[idx]                    # [N][nb][3]
    dn = np.sqrt((diff * diff).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = np.where(dn[..., None] > 0, diff / dn[..., None], 0.0)
    if mutant == "zero_unit":
        terms = terms + (dn[..., None] == 0) * np.array([1.0, 0.0, 0.0])
    return terms.sum(1), np.abs(terms).sum(1)


def dist_bound(d):
    return D_ULPS * U * d * SLACK + A.TINY


def sum_bound(d_all):
    n = d_all.size
    return (D_ULPS + max(n - 1, 0)) * U * float(np.abs(d_all).sum()) * SLACK + A.TINY


def grad_bound(abs_terms, nb):
    return (D_ULPS + 2 + nb - 1) * U * abs_terms * SLACK + A.TINY


def near_tie(ref, nb):
    """[N] bool: float64 ranks nb and nb + 1 lie closer than twice the distance bound - the only queries whose neighbour set
    an fp32 evaluation within the bound may decide differently.  An EXACT tie is not one of them: equal float64 distances
    here come from duplicated points, whose fp32 distances are equal too, and the index decides."""
    gap = ref["next_d"] - ref["d"][:, -1]
    return (gap > 0) & (gap < 2 * dist_bound(ref["next_d"]))


def smooth_xyz_torch(adv, ref, nb):
    """The reference's Smooth (nontarget.py:131-135) in float64 by autograd: cdist without the matmul expansion, topk."""
    a = torch.from_numpy(adv.astype(np.float64)).requires_grad_(True)
    r = torch.from_numpy(ref.astype(np.float64))
    dist = torch.cdist(a[None], r[None], compute_mode="donot_use_mm_for_euclid_dist")[0]
    vals, idx = torch.topk(dist, nb, dim=1, largest=False)
    total = vals.sum()
    total.backward()
    return float(total.detach()), a.grad.numpy(), idx.numpy()


# ------------------------------------------------------------------------------------------------ apply and Adam
def coord_apply(x0, delta, ori_xyz, mask, active):
    """exact fp32: x0[b][i][0:3] = ori_xyz + delta on masked points of active rooms"""
    x0 = x0.copy()
    B, N, _ = x0.shape
    on = np.ones((B, N), bool) if mask is None else np.asarray(mask, bool).copy()
    if active is not None:
        on &= np.asarray(active, bool)[:, None]
    x0[:, :, 0:3] = np.where(on[:, :, None], (ori_xyz.astype(F) + delta.astype(F)).astype(F), x0[:, :, 0:3])
    return x0


def coord_adam_step(delta, m, v, mask, dx0, sgrad, coord_c, lr, beta1, beta2, eps, step, active=None, mutant=None):
    """One optimiser step on delta [B][N][3]: g = dx0[0:3] + 2 coord_c delta + coord_c sgrad (the gradient of
    sum(dx0 . delta) + coord_c sum(delta^2) + coord_c sum(sgrad . delta) by autograd), then torch.optim.Adam's single-tensor
    step (attack_ref64.adam_update64).  Returns (delta, m, v, l2 [B], parts of each) like attack_ref64.nu_adam_step; l2 is
    sum(delta^2) of the incoming delta per room, NaN-free zeros for inactive rooms.  Mutants: "no_l2_grad" drops 2 coord_c
    delta, "no_bias" runs Adam without bias correction."""
    B, N, _ = delta.shape
    on = np.ones((B, N), bool) if mask is None else np.asarray(mask, bool).copy()
    if active is not None:
        on &= np.asarray(active, bool)[:, None]
    on3 = np.broadcast_to(on[:, :, None], delta.shape)
    sg = np.zeros(delta.shape) if sgrad is None else sgrad.astype(np.float64)
    dt = A.t64(delta).requires_grad_(True)
    loss = (A.t64(dx0[:, :, 0:3]) * dt).sum() + float(coord_c) * (dt * dt).sum() + float(coord_c) * (A.t64(sg) * dt).sum()
    loss.backward()
    g = dt.grad.numpy()
    if mutant == "no_l2_grad":
        g = dx0[:, :, 0:3].astype(np.float64) + float(coord_c) * sg
    d64, m64, v64 = delta.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    if mutant == "no_bias":
        m2 = m64 + (g - m64) * (1 - float(beta1))
        v2 = v64 * float(beta2) + (1 - float(beta2)) * g * g
        d2 = d64 - float(lr) * m2 / (np.sqrt(v2) + float(eps))
    else:
        d2, m2, v2 = A.adam_update64(d64, m64, v64, g, float(lr), float(beta1), float(beta2), float(eps), step)
    d2, m2, v2 = (np.where(on3, a, b) for a, b in ((d2, d64), (m2, m64), (v2, v64)))
    # the kernel's formula with its errors
    V = A.V
    dv = V(delta)
    sq = dv * dv
    gv = dv * (float(coord_c) * 2.0) + dx0[:, :, 0:3].astype(np.float64)
    if sgrad is not None:
        gv = gv + V(sg) * float(coord_c)
    mv = V(m) + (gv - V(m)) * (1 - float(beta1))
    vv = V(v) * float(beta2) + (gv * gv) * (1 - float(beta2))
    bc1, bc2 = 1 - float(beta1) ** step, 1 - float(beta2) ** step
    full = lambda c: V.rounded(np.full(delta.shape, c), np.zeros((5,) + delta.shape))     # noqa: E731
    denom = vv.sqrt() / full(np.sqrt(bc2)) + float(eps)
    wv = dv + (mv / denom) * full(-(float(lr) / bc1))
    keep = lambda k: np.where(on3[None], k.e, 0.0)                                        # noqa: E731
    l2 = np.where(on3, d64 * d64, 0.0).reshape(B, -1).sum(1)
    l2e = np.stack([V(np.where(on3[b], sq.v[b], 0.0), np.where(on3[b][None], sq.e[:, b], 0.0)).sum().e for b in range(B)], 1)
    return d2, m2, v2, l2, keep(wv), keep(mv), keep(vv), l2e


# ------------------------------------------------------------------------------------------------ the shared cases
SMOOTH_SHAPES = ((1, 70, 5), (3, 257, 10), (2, 4096, 10), (1, 4096, 16))     # (B, N, nb)
SMOOTH_PERT = ((0.0,), (0.0, 1e-4, 1e-2), (1e-4, 1e-2), (1e-2,))            # metres, per room
TIE_SHARE_CAP = 1e-3
_CASES = {}


def smooth_cases():
    """make_rooms coordinates as the reference points, the same points plus a uniform perturbation of +-p per component as
    the adversarial ones (p = 0 exactly, 1e-4, 1e-2 m; the last case perturbs every second point only).  Room 0 of the third
    case holds 200 exactly duplicated points.  Built once, never modified; each case carries its float64 reference per
    room."""
    if "smooth" in _CASES:
        return _CASES["smooth"]
    from pointsecguard_amd.synthetic import make_rooms
    out = []
    for k, ((B, N, nb), perts) in enumerate(zip(SMOOTH_SHAPES, SMOOTH_PERT)):
        rng = np.random.default_rng([41, k])
        ref = np.ascontiguousarray(make_rooms(B, 50 + k, num_point=N)[:, :, 0:3])
        if k == 2:
            src = rng.permutation(N)[:200]
            ref[0, (src + 1) % N] = ref[0, src]
        adv = ref.copy()
        for b, p in enumerate(perts):
            if p:
                pert = ((rng.random((N, 3)) * 2 - 1) * p).astype(F)
                if k == 3:
                    pert[::2] = 0
                adv[b] = (ref[b] + pert).astype(F)
        refs = [smooth_xyz(adv[b], ref[b], nb) for b in range(B)]
        out.append(dict(B=B, N=N, nb=nb, perts=perts, ref=ref, adv=adv, refs=refs, name="smooth_xyz B=%d N=%d nb=%d" % (B, N, nb)))
    _CASES["smooth"] = out
    return out
