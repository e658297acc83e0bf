"""float64 stage reference for RandLA-Net's position-branch gradient (psg_rla_backward_full), with the bound of every stage.

TEST INFRASTRUCTURE ONLY; extends tests/randla_ref64.py (same method, same u = 2^-24, same `compare`).  The branch per
level: relpos [E, 10] = [dist, x_i - x_j, x_i, x_j] -> fxyz1 = lrelu(LFAmlp1 relpos) -> fxyz2 = lrelu(LFAmlp2 fxyz1); fxyz1 is
the second half of the concatenation of attentive pooling 1, fxyz2 that of pooling 2.  Stages, deepest level first, each fed
the snapshot's own inputs and decisions (sign bits of fxyz1 / fxyz2, the forward's stored rel and dist):

  att_pool_T_xyz   g_fxyz[e, c'] = a[e, h + c'] dagg[i, h + c'] + sum_c ds[e, c] W[c, h + c']: the softmax transpose of
                   randla_ref64.att_pool_T on the position half; bound: its ba / bds propagation, the dot product of length d
                   and one more addition ((d + 3) u on the magnitudes), scaled by SOFTMAX_T_RATIO as it stands (the same
                   arithmetic: expf, the 16-term sums, the products).
  G2               lrelu_T(g_fxyz2, bits of fxyz2);   G1 = lrelu_T(g_fxyz1 + conv_T(G2, LFAmlp2), bits of fxyz1): an accumulator
                   with two contributors (randla_ref64.acc);   g_rp = conv_T(G1, LFAmlp1): dot-product bounds.
  relpos_T         g_rel = g_rp[1:4] + g_rp[0] * (rel / dist): one rounding for the division and one for the product
                   (2 u |g_rp[0] rel / dist|), one for the sum; side_i = g_rel + g_rp[4:7], side_j = g_rp[7:10] - g_rel: one more
                   rounding each.  dist == 0 adds EXACTLY zero from the distance column (self edges: rel is identically zero,
                   so zero is the derivative; distinct coincident points: the stated convention).
  point_sum        a point's 16 own edges, its in-edges, and for a sampled row the next level's complete gradient: t terms
                   in any order, (t + 1) u on the absolute sum.

No new device-function constant: the division is IEEE (the unit is built with -ffp-contract=off) and sqrtf / expf do not
occur outside the attention weights, which SOFTMAX_T_RATIO covers.  Largest error / bound measured on the MI355X
(tests/test_gpu_rla_coord.py prints every stage's figure; 8192, 8704 and 2 x 8192 points, split path): G2 0.46 (level 0,
2 x 8192), G1 0.33 (level 0, 8192), g_rp 0.36 (level 0, 8704), side_i 0.99 (level 0, 2 x 8192), side_j 0.99 (level 2, 8704),
gxyz 0.24 (level 0, 8704).  side_i / side_j come that close because their bound is exactly the two or three roundings the
kernel performs; the float32 numpy emulation of the CPU tests reaches 0.97 / 0.99.
"""
import numpy as np

import randla_ref64 as R

U, RK = R.U, R.RK


def att_pool_T_xyz(f, fxyz, neigh, Wb, dagg, dt=np.float64, direct=True):
    """transpose of att_pool w.r.t. the position half fxyz -> (g_fxyz [n * 16, h], bound); direct=False (negative tests)
    drops the direct term a * dagg"""
    W = Wb[0]
    n, h = f.shape
    d = 2 * h
    cat, a, ba = R._attention(f, fxyz, neigh, W, dt)
    dagg = np.asarray(dagg).astype(dt)[:, None, :]
    g = cat * dagg
    dot = (a * g).sum(1, keepdims=True)
    ds = a * (g - dot)
    ddir = a[:, :, h:] * dagg[:, :, h:]
    a64, g64 = a.astype(np.float64), np.abs(g.astype(np.float64))
    bdot = (ba * g64 + a64 * U * g64).sum(1, keepdims=True) + (RK + 2) * U * (a64 * g64).sum(1, keepdims=True)
    gd = np.abs((g - dot).astype(np.float64))
    bds = ba * gd + a64 * (U * g64 + bdot + U * gd) + U * np.abs(ds)
    bddir = ba[:, :, h:] * np.abs(dagg[:, :, h:].astype(np.float64)) + U * np.abs(ddir)
    W2 = W[:, h:]
    out = ds @ W2.astype(dt)
    mag = np.abs(ds.astype(np.float64)) @ np.abs(W2)
    b = bds @ np.abs(W2)
    if direct:
        out = ddir + out
        mag = mag + np.abs(ddir.astype(np.float64))
        b = b + bddir
    return out.reshape(-1, h), R.SOFTMAX_T_RATIO * (b + (d + 3) * U * mag + U * np.abs(out)).reshape(-1, h)


def relpos_fwd(rel, dt=np.float64):
    """the distance column from the difference columns (the forward stage whose transpose relpos_T is)"""
    rel = np.asarray(rel).astype(dt)
    return np.sqrt((rel * rel).sum(-1))


def relpos_T(relpos, g_rp, dt=np.float64, dist_col=True, flip_j=False):
    """per edge e = (i, k), j = neigh[e]: -> (side_i [E, 4], bound, side_j [E, 4], bound), column 3 zero.  rel and dist are the
    forward's own stored values.  dist_col=False / flip_j=True: negative tests."""
    rp, g = np.asarray(relpos).astype(dt), np.asarray(g_rp).astype(dt)
    dist, rel = rp[:, 0:1], rp[:, 1:4]
    zero = dist == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = np.where(zero, dt(0), rel / np.where(zero, dt(1), dist))
    t = g[:, 0:1] * unit if dist_col else np.zeros_like(unit)
    g_rel = g[:, 1:4] + t                                       # (dist == 0: t is +-0, so g_rel is g_rp[1:4] itself)
    # (first order; the factor 1 + 4 u covers the products of two roundings, which the three lines below leave out)
    b_rel = (1 + 4 * U) * (2 * U * np.abs(t.astype(np.float64)) + U * np.abs(g_rel.astype(np.float64)))
    side_i = g_rel + g[:, 4:7]
    side_j = (g[:, 7:10] + g_rel) if flip_j else (g[:, 7:10] - g_rel)
    pad = lambda v: np.concatenate([v, np.zeros((len(v), 1), v.dtype)], 1)          # noqa: E731
    bi = b_rel + (1 + 4 * U) * U * np.abs(side_i.astype(np.float64))
    bj = b_rel + (1 + 4 * U) * U * np.abs(side_j.astype(np.float64))
    return pad(side_i), pad(bi), pad(side_j), pad(bj)


def point_sum(side_i, side_j, neigh, g_next, pool, dt=np.float64, in_edges=True, chain=True):
    """gxyz [n, 3] of one level: own edges + in-edges + (sampled rows) the next level's gradient -> (value, bound)"""
    n = len(neigh)
    own = np.asarray(side_i)[:, :3].astype(dt).reshape(n, RK, 3)
    out = own.sum(1)
    mag = np.abs(own.astype(np.float64)).sum(1)
    terms = np.full((n, 1), float(RK))
    if in_edges:
        idx = neigh.reshape(-1)
        sj = np.asarray(side_j)[:, :3].astype(dt)
        np.add.at(out, idx, sj)
        np.add.at(mag, idx, np.abs(sj.astype(np.float64)))
        terms = terms + np.bincount(idx, minlength=n).astype(np.float64)[:, None]
    if chain and g_next is not None:
        gn = np.asarray(g_next).astype(dt)
        out[pool] += gn
        mag[pool] += np.abs(gn.astype(np.float64))
        terms[pool] += 1.0
    return out, (terms + 1) * U * mag


def fxyz_bits(fwd, i):
    """the sign bits of fxyz1 / fxyz2 of a forward snapshot: its taps, or (an emulation keeps none) the outputs' own signs -
    leaky ReLU keeps the sign of its argument"""
    out = []
    for k, m in (("fxyz1", "m_fxyz1"), ("fxyz2", "m_fxyz2")):
        out.append(np.asarray(fwd[(m, i)]) if (m, i) in fwd else np.asarray(fwd[(k, i)]) > 0)
    return out


def check_fxyz_masks(P, fwd, rep):
    """the sign words the full workspace keeps for the branch's two layers, as randla_ref64.compare_mask checks the others"""
    for i in range(5):
        E = "Encoder_layer_%d" % i
        _, _, z, bz = R.conv(np.asarray(fwd[("relpos", i)]), P[E + "LFAmlp1"], act=True)
        R.compare_mask(rep, ("m_fxyz1", i), fwd[("m_fxyz1", i)], z, bz)
        _, _, z, bz = R.conv(np.asarray(fwd[("fxyz1", i)]), P[E + "LFAmlp2"], act=True)
        R.compare_mask(rep, ("m_fxyz2", i), fwd[("m_fxyz2", i)], z, bz)


MUTANTS = ("no_in_edges", "no_dist", "flip_j", "no_chain", "swap_masks", "no_direct")


def walk_xyz(P, fwd, bwd, geo, taps=None, dt=np.float64, mutant=None):
    """the position-branch stages behind randla_ref64.walk_backward, in the order of psg_rla_backward_full: fwd = the forward
    snapshot, bwd = the gradient snapshot (g_agg2, g_agg1 per level) -> (taps, Report); 30 stages and ("dxyz", 0) = gxyz of
    level 0.  mutant (negative tests): one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    w = R._Walk(taps, dt)
    F = lambda k, i: np.asarray(fwd[(k, i)])                   # noqa: E731
    B = lambda k, i: np.asarray(bwd[(k, i)])                   # noqa: E731
    g_next = None
    for i in range(4, -1, -1):
        E = "Encoder_layer_%d" % i
        nb = geo["neigh"][i]
        bits1, bits2 = fxyz_bits(fwd, i)
        if mutant == "swap_masks":
            bits1, bits2 = bits2, bits1
        direct = mutant != "no_direct"
        v, b = att_pool_T_xyz(F("fagg1", i), F("fxyz2", i), nb, P[E + "LFAatt_pooling_2fc"], B("g_agg2", i), dt, direct)
        G2 = w.out(("G2", i), *R.lrelu_T(v, b, bits2, dt))
        part = att_pool_T_xyz(F("fpc", i), F("fxyz1", i), nb, P[E + "LFAatt_pooling_1fc"], B("g_agg1", i), dt, direct)
        v, b = R.acc([part, R.conv_T(G2, P[E + "LFAmlp2"], dt=dt)])
        G1 = w.out(("G1", i), *R.lrelu_T(v, b, bits1, dt))
        g_rp = w.out(("g_rp", i), *R.conv_T(G1, P[E + "LFAmlp1"], dt=dt))
        si, bi, sj, bj = relpos_T(F("relpos", i), g_rp, dt, dist_col=mutant != "no_dist", flip_j=mutant == "flip_j")
        si = w.out(("side_i", i), si, bi)
        sj = w.out(("side_j", i), sj, bj)
        g_next = w.out(("gxyz", i), *point_sum(si, sj, nb, g_next, geo["pool"][i], dt, in_edges=mutant != "no_in_edges",
                                                  chain=mutant != "no_chain"))
    if taps is None:
        w.t[("dxyz", 0)] = g_next
    else:
        R.compare(w.rep, ("dxyz", 0), taps[("dxyz", 0)], np.asarray(taps[("gxyz", 0)]), None)
    return w.t, w.rep


def sign_bars(ours, ref):
    """(share of entries whose sign agrees, largest |ref| among the disagreeing entries / max |ref|)"""
    agree = np.sign(ours) == np.sign(ref)
    flip = float(np.abs(ref[~agree]).max() / np.abs(ref).max()) if not agree.all() else 0.0
    return float(agree.mean()), flip


# ---------------------------------------------------------------------------------------------------- the field step
def field_step(xyz_adv, g, ori, eps, alpha, metric):
    """psg_rla_bim_step_field in numpy float32, expression for expression (bim.py:84-96 on the coordinate columns, no box):
    l_inf bit for bit; l_2 with the two norms accumulated in float64 like the kernel's -> the new positions [n, 3] float32"""
    xyz_adv, g, ori = (np.asarray(a, np.float32) for a in (xyz_adv, g, ori))
    eps, alpha = np.float32(eps), np.float32(alpha)
    if metric == "l_inf":
        v = xyz_adv + alpha * np.sign(g).astype(np.float32)
        return np.minimum(np.maximum(v, ori - eps), ori + eps)
    gn = np.maximum(np.float32(1e-12), np.sqrt(np.float32((g.astype(np.float64) ** 2).sum())))
    delta = (xyz_adv - ori) + alpha * (g / gn)
    dn = np.sqrt(np.float32((delta.astype(np.float64) ** 2).sum()))
    scale = eps / dn if dn > eps else np.float32(1.0)
    return ori + delta * np.float32(scale)


def field_step_l2_bound(xyz_adv, g, ori, eps, alpha):
    """float64 value of the l_2 step and, per entry, how far the float32 kernel may lie from it: the norms are float64 sums
    rounded once and rooted (2 u relative each, any summation order of 3 n doubles being far below that), the unit vector a
    division and a product, delta two additions, the rescale a division and a product, the result one addition."""
    a, g64, o = (np.asarray(v, np.float64) for v in (xyz_adv, g, ori))
    gn = max(1e-12, np.sqrt((g64 ** 2).sum()))
    step = alpha * g64 / gn
    delta = a - o + step
    bdelta = U * np.abs(a - o) + 5 * U * np.abs(step) + U * np.abs(delta)
    dn = np.sqrt((delta ** 2).sum())
    # |d dn| <= |bdelta|_2 (the norm is 1-Lipschitz) + 2 u dn
    bdn = np.sqrt((bdelta ** 2).sum()) + 2 * U * dn
    scale = eps / dn if dn > eps else 1.0
    bscale = (scale * bdn / dn + 2 * U * scale) if dn > eps else (eps * bdn / dn if dn + bdn > eps else 0.0)
    moved = delta * scale
    out = o + moved
    return out, bdelta * scale + np.abs(delta) * bscale + U * np.abs(moved) + U * np.abs(out)
