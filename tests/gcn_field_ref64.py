"""Float64 references and derived bounds for the ResGCN coordinate-field kernels: the Smooth term of this
network, smooth(adv, adv) on channels 0:3, and the coordinate Adam step with separate weights.

TEST INFRASTRUCTURE ONLY: no GPU.  The bounds are nu_field_ref64's (section 5l), derived and not measured: per distance
4 u d, per gradient term 6 u, a sum of t terms (t - 1) u of their absolute sum - here t is a point's own neighbour count plus
its in-degree, every pair term entering once with each sign."""
import numpy as np
import torch

import attack_ref64 as A
import nu_field_ref64 as R

F = np.float32
U = A.U


# ------------------------------------------------------------------------------------------------ smooth(adv, adv) on xyz
def sym_smooth(xyz, nb, mutant=None):
    """One room: xyz [N][3] (fp32 values, float64 arithmetic).  Every point takes its nb nearest points of the room, itself
    included, by (distance, index); the term u(i, j) = (a_i - a_j) / d goes with + to the query i and with - to the neighbour
    j, a pair at d == 0 adds exactly zero.  Returns nu_field_ref64.smooth_xyz's dict with the two-sided grad / abs_terms and
    indeg [N] (how many lists hold the point)."""
    ref = R.smooth_xyz(xyz, xyz, nb, mutant)
    idx = ref["idx"].astype(np.int64)
    x = xyz.astype(np.float64)
    diff = x[:, None, :] - x[idx]
    dn = np.sqrt((diff * diff).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = np.where(dn[..., None] > 0, diff / dn[..., None], 0.0)
    grad, absg = terms.sum(1), np.abs(terms).sum(1)
    np.subtract.at(grad, idx.reshape(-1), terms.reshape(-1, 3))
    np.add.at(absg, idx.reshape(-1), np.abs(terms).reshape(-1, 3))
    return dict(ref, grad=grad, abs_terms=absg, indeg=np.bincount(idx.reshape(-1), minlength=len(x)))


def sym_grad_bound(ref):
    """(6 + t - 1) u sum|terms| with t = own terms + in-degree"""
    t = ref["idx"].shape[1] + ref["indeg"]
    return (R.D_ULPS + 2 + t - 1)[:, None] * U * ref["abs_terms"] * R.SLACK + A.TINY


def grad_on_lists(xyz, idx):
    """(grad, sum|terms|, in-degree) of the two-sided Smooth on GIVEN neighbour lists idx [N][k], float64."""
    x = xyz.astype(np.float64)
    idx = idx.astype(np.int64)
    diff = x[:, None, :] - x[idx]
    dn = np.sqrt((diff * diff).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = np.where(dn[..., None] > 0, diff / dn[..., None], 0.0)
    grad, absg = terms.sum(1), np.abs(terms).sum(1)
    np.subtract.at(grad, idx.reshape(-1), terms.reshape(-1, 3))
    np.add.at(absg, idx.reshape(-1), np.abs(terms).reshape(-1, 3))
    indeg = np.bincount(idx.reshape(-1), minlength=len(x))
    t = idx.shape[1] + indeg
    return grad, (R.D_ULPS + 2 + t - 1)[:, None] * U * absg * R.SLACK + A.TINY, dn


def sym_smooth_torch(xyz, nb):
    """The reference's expression (colper.py:115-120: cdist, sort, first nb, sum) on xyz against itself, float64 autograd."""
    a = torch.from_numpy(xyz.astype(np.float64)).requires_grad_(True)
    dist = torch.cdist(a[None], a[None], compute_mode="donot_use_mm_for_euclid_dist")[0]
    vals = dist.sort(dim=1)[0][:, :nb]
    total = vals.sum()
    total.backward()
    return float(total.detach()), a.grad.numpy()


# ------------------------------------------------------------------------------------------------ the two passes in fp32 numpy
def d2_direct_fp32(xyz):
    """[N][N] fp32 d^2 = fma(dz, dz, fma(dy, dy, dx * dx)) on rounded differences, as both passes evaluate it"""
    a = xyz.astype(F)
    d = (a[:, None, :] - a[None, :, :]).astype(F)
    s = (d[..., 0] * d[..., 0]).astype(F)
    s = (d[..., 1].astype(np.float64) * d[..., 1] + s).astype(F)
    return (d[..., 2].astype(np.float64) * d[..., 2] + s).astype(F)


def pass1_lists(d32, nb):
    """pass 1's contract: every point's min(nb, N) neighbours in ascending (fp32 distance, index) order"""
    return np.argsort(d32, axis=1, kind="stable")[:, :nb].astype(np.int32)


def pass2_members(d32, lists, rule="d", d2=None):
    """Replay of smooth_xyz_sym_incoming_kernel's membership rule: member[k][i] <=> (d(k, i), i) <= (d(k, j*), j*) for k's last
    neighbour j* (the last one actually held).  rule "d2": the mutant that compares the squares; "no_index": the mutant
    without the index clause."""
    N = len(d32)
    last = lists[:, -1].astype(np.int64)
    val = d2 if rule == "d2" else d32
    key = val[np.arange(N), last][:, None]
    i = np.arange(N)[None, :]
    if rule == "no_index":
        return val <= key
    return (val < key) | ((val == key) & (i <= last[:, None]))


def members_of_lists(lists, N):
    out = np.zeros((len(lists), N), bool)
    out[np.arange(len(lists))[:, None], lists.astype(np.int64)] = True
    return out


# ------------------------------------------------------------------------------------------------ Adam with two weights
def coord_adam_step_w(delta, m, v, mask, dx0, sgrad, c_smooth, c_l2, lr, beta1, beta2, eps, step, active=None):
    """nu_field_ref64.coord_adam_step with g = dx0[0:3] + 2 c_l2 delta + c_smooth sgrad: the same float64 reference and the
    same error model (attack_ref64.V) of the kernel's formula.  Returns (delta, m, v, l2 [B], e_delta, e_m, e_v, e_l2)."""
    B, N, _ = delta.shape
    on = np.ones((B, N), bool) if mask is None else np.asarray(mask, bool).copy()
    if active is not None:
        on &= np.asarray(active, bool)[:, None]
    on3 = np.broadcast_to(on[:, :, None], delta.shape)
    sg = np.zeros(delta.shape) if sgrad is None else sgrad.astype(np.float64)
    dt = A.t64(delta).requires_grad_(True)
    loss = (A.t64(dx0[:, :, 0:3]) * dt).sum() + float(c_l2) * (dt * dt).sum() + float(c_smooth) * (A.t64(sg) * dt).sum()
    loss.backward()
    g = dt.grad.numpy()
    d64, m64, v64 = delta.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    d2, m2, v2 = A.adam_update64(d64, m64, v64, g, float(lr), float(beta1), float(beta2), float(eps), step)
    d2, m2, v2 = (np.where(on3, a, b) for a, b in ((d2, d64), (m2, m64), (v2, v64)))
    V = A.V
    dv = V(delta)
    sq = dv * dv
    gv = dv * (float(c_l2) * 2.0) + dx0[:, :, 0:3].astype(np.float64)
    if sgrad is not None:
        gv = gv + V(sg) * float(c_smooth)
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
SYM_N = (333, 1024, 2049, 4096)
SYM_SIGMA = (0.0, 1e-4, 1e-2)
SYM_NB = (5, 10, 16)
TIE_SHARE_CAP = R.TIE_SHARE_CAP
_CACHE = {}


def sym_points(n, sigma, room=0):
    """The first n points of make_rooms(2, 5)[room], channels 0:3, plus a normal perturbation of sigma metres (fp32)."""
    key = (n, sigma, room)
    if key not in _CACHE:
        from pointsecguard_amd.synthetic import make_rooms
        xyz = np.ascontiguousarray(make_rooms(2, 5)[room, :n, 0:3])
        if sigma:
            rng = np.random.default_rng([52, n, int(round(sigma * 1e6)), room])
            xyz = (xyz + (rng.standard_normal(xyz.shape) * sigma).astype(F)).astype(F)
        _CACHE[key] = xyz
    return _CACHE[key]


def dup_points(n, room=0):
    """The first n points of make_rooms_with_duplicates(2, 5)[room]: exact duplicates, decided by index."""
    from pointsecguard_amd.synthetic import make_rooms_with_duplicates
    return np.ascontiguousarray(make_rooms_with_duplicates(2, 5)[room, :n, 0:3])


def circle_points(n=48, r=0.37):
    """A centre and n points at (nearly) one distance from it: their fp32 d^2 differ in the last bits while many of the roots
    round to one d - where comparing d^2 and comparing d select different members."""
    th = np.arange(n) * (2 * np.pi / n) + 0.1
    pts = np.stack([r * np.cos(th), r * np.sin(th), np.zeros(n)], 1)
    return np.concatenate([np.zeros((1, 3)), pts]).astype(F)
