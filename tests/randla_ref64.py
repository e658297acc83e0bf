"""float64 stage reference for the RandLA-Net kernels (csrc/psg_randla_net.hip), with the error bound of every stage.

TEST INFRASTRUCTURE ONLY.  One function per stage of oracle/randla_net.py (conv, relative position encoding, attentive
pooling, random-sample max-pool, nearest up-sample + concat) and one per transpose; every function takes the stage's
inputs as arrays - the tests pass in what the GPU produced - and returns (value, bound): the stage in float64 and, per
entry, how far a float32 evaluation of the same stage may lie from it.

Bounds (u = 2^-24, the unit round-off of float32; all evaluated in float64):
  linear stages - a dot product of length K in ANY summation order with fp32 accumulation, so one formula serves every
      GEMM tile shape and every gather: |got - ref| <= (K + 2) u (|x| |w|^T + |b| + |pre-add|) + u |ref|; an accumulator
      with several contributors adds their bounds, plus u sum|v| for each further addition.
  leaky ReLU - 1-Lipschitz, so the pre-activation's bound carries over (whichever side of 0 either value lies on), plus
      one rounding u |out| of the product with the slope; the reference multiplies by float32(0.2) like the kernels.
  max-pool, up-sample + concat, the difference columns of relpos - exact (bit-equal).
  relpos distance - sqrtf of a 3-term sum of squares of the GPU's own differences: first order, every square passes through at
      most three roundings (halved by the root: 1.5 u) and the root is taken as one ulp (2 u): 4 u |dist| rounded up; no ulp figure is
      documented for sqrtf, so that first-order bound is scaled by DIST_RATIO = 4 x the measured ratio (below).
  softmax stages (attentive pooling and its transpose) - first-order propagation of (a) the score's dot-product bound,
      (b) the rounding of s - max, u |s - max|, (c) expf taken as one ulp, 2 u, each acting as a perturbation ds of the
      score: |da_k| <= a_k (ds_k + sum_j a_j ds_j) + 18 u a_k (16-term sum, reciprocal, product), then the weighted sum /
      the products of the transpose as linear stages on top.  No ulp figure is documented for expf, so that first-order
      bound is scaled by SOFTMAX_RATIO (poolings) / SOFTMAX_T_RATIO (transposes) = 4 x the measured ratio (below).
The transposes take the decisions (arg byte, mask bit) as inputs, so a last-bit flip cannot move an entry.

`walk` composes the stages into the whole network twice over: with taps=None it EMULATES the network in a given dtype
(float64: tied to RandLAOracle(float64) by the self-checks; float32: a stand-in for the GPU in the CPU tests); with
taps = a snapshot of the workspace it CHECKS every stage, feeding each one the snapshot's own inputs and comparing the
snapshot's output under the stage's bound.
"""
import numpy as np

U = 2.0 ** -24
SLOPE = float(np.float32(0.2))
RK = 16
D_OUT = (16, 64, 128, 256, 512)
RATIO = (4, 4, 4, 4, 2)
# Device math functions (expf in the attentive poolings, sqrtf in relpos: the HIP documentation installed with the compiler
# states no ulp figure for either), handled as the method prescribes: the largest per-entry |error| / first-order bound
# MEASURED on the MI355X on the stages' own inputs, and the constant = 4 x that, the margin for clouds that reach other
# arguments.  Measured with tests/test_randla_stages.py (which prints every stage's figure) over its three shapes on the
# default path and the 8704-point cloud under each of the four PSG_RLA_* switches, 5 levels each:
#   agg1 / agg2 (forward poolings)      0.120 (8192 points, default path; 0.092 .. 0.109 elsewhere)
#   d_fagg1 / d_fpc (their transposes)  0.044 (8704 points, PSG_RLA_NO_DIRECT; 0.035 .. 0.041 elsewhere)
#   relpos distance, of 4 u |dist|      0.558 (2 x 8192 points, level 0; 0.484 at 8192 and 8704 points, every path)
# (the float32 numpy emulation of the CPU tests reaches 0.10, 0.04 and 0.48)
SOFTMAX_MEASURED = 0.120
SOFTMAX_RATIO = 4 * SOFTMAX_MEASURED
SOFTMAX_T_MEASURED = 0.044
SOFTMAX_T_RATIO = 4 * SOFTMAX_T_MEASURED
DIST_MEASURED = 0.558
DIST_RATIO = 4 * DIST_MEASURED
MASK_CAP = 1e-4                      # share of a stage's entries whose sign bit may differ INSIDE the pre-activation's bound


# ---------------------------------------------------------------------------------------------------- parameters
def fold(params, name, rounded=True):
    """make_layer's fold of BatchNorm into (W [cout, cin], b [cout] or None) in float64; rounded=True: the float32
    values the kernels multiply by (held in float64), rounded=False: the exact fold (ties this file to the oracle)."""
    w = np.asarray(params[name + ".weight"], np.float64)
    bias = params.get(name + ".bias")
    bn = name + ".bn.gamma" in params
    s, sh = np.ones(w.shape[0]), np.zeros(w.shape[0])
    if bn:
        g, be, mu, var = (np.asarray(params[name + ".bn." + k], np.float64) for k in ("gamma", "beta", "mean", "var"))
        s = g / np.sqrt(var + 1e-6)
        sh = be - mu * s
    W = w * s[:, None]
    b = (0.0 if bias is None else np.asarray(bias, np.float64)) * s + sh if (bn or bias is not None) else None
    if rounded:
        W = W.astype(np.float32).astype(np.float64)
        b = None if b is None else b.astype(np.float32).astype(np.float64)
    return W, b


def layer_names():
    names = ["fc0"]
    for i in range(5):
        p = "Encoder_layer_%d" % i
        names += [p + s for s in ("mlp1", "LFAmlp1", "LFAatt_pooling_1fc", "LFAatt_pooling_1mlp", "LFAmlp2", "LFAatt_pooling_2fc",
                                  "LFAatt_pooling_2mlp", "mlp2", "shortcut")]
    return names + ["decoder_0"] + ["Decoder_layer_%d" % j for j in range(5)] + ["fc1", "fc2", "fc"]


def fold_all(params, rounded=True):
    return {n: fold(params, n, rounded) for n in layer_names()}


def geometry(xyz, neigh, up, batch=1):
    """xyz [N, 3] of level 0, neigh[i] [n_i, 16] and up[i] [n_i] as ROW NUMBERS of the cloud-major buffers (what the
    workspace holds) -> dict with the per-level points and the level row of every sampled row."""
    geo = {"neigh": [np.asarray(a, np.int64) for a in neigh], "up": [np.asarray(a, np.int64).reshape(-1) for a in up], "xyz": [], "pool": []}
    cur = np.asarray(xyz, np.float32)
    for i in range(5):
        n = cur.shape[0]
        nc = n // batch
        rows = (np.arange(batch)[:, None] * nc + np.arange(nc // RATIO[i])[None, :]).reshape(-1)
        geo["xyz"].append(cur)
        geo["pool"].append(rows)
        cur = cur[rows]
    return geo


# ---------------------------------------------------------------------------------------------------- stages
def lrelu(z, bz, dt):
    out = np.where(z > 0, z, dt(SLOPE) * z)
    return out, bz + U * np.abs(out)


def conv(x, Wb, pre=None, act=False, dt=np.float64):
    """rows . W^T + b (+ pre-add) [-> leaky ReLU]: -> (out, bound of out, pre-activation z, bound of z)."""
    W, b = Wb
    x = np.asarray(x).astype(dt)
    z = x @ W.astype(dt).T
    mag = np.abs(x.astype(np.float64)) @ np.abs(W).T
    if b is not None:
        z = z + b.astype(dt)
        mag = mag + np.abs(b)
    if pre is not None:
        z = z + np.asarray(pre).astype(dt)
        mag = mag + np.abs(np.asarray(pre, np.float64))
    bz = (W.shape[1] + 2) * U * mag + U * np.abs(z)
    if not act:
        return z, bz, z, bz
    out, bo = lrelu(z, bz, dt)
    return out, bo, z, bz


def conv_T(dz, Wb, bdz=None, cols=None, dt=np.float64):
    """dz . W (columns `cols` of the input side), the transpose of conv: -> (din, bound); bdz = bound of dz when dz is
    itself a computed intermediate that no tap shows."""
    W = Wb[0] if cols is None else Wb[0][:, cols]
    dz = np.asarray(dz).astype(dt)
    v = dz @ W.astype(dt)
    a = np.abs(dz.astype(np.float64))
    b = (W.shape[0] + 2) * U * (a @ np.abs(W)) + U * np.abs(v)
    if bdz is not None:
        b = b + bdz @ np.abs(W)
    return v, b


def lrelu_T(v, b, bits, dt=np.float64):
    """gradient through leaky ReLU with the sign bits as an input"""
    out = np.where(bits, v, dt(SLOPE) * v)
    return out, np.where(bits, b, SLOPE * b + U * np.abs(out))


def acc(parts):
    """an accumulator with several contributors [(value, bound)], added in the order given"""
    v, b, mag = parts[0][0], parts[0][1], np.abs(parts[0][0]).astype(np.float64)
    for pv, pb in parts[1:]:
        v = v + pv
        b = b + pb
        mag = mag + np.abs(pv)
    return v, b + (len(parts) - 1) * U * mag


def relpos(xyz, neigh, dt=np.float64):
    """[dist, xyz_i - xyz_j, xyz_i, xyz_j] per edge, [n * 16, 10], in dt arithmetic (float32: the difference columns are
    what the kernel stores, bit for bit)"""
    xyz = np.asarray(xyz, np.float32).astype(dt)
    nb = xyz[neigh]                                            # [n, 16, 3]
    tile = np.broadcast_to(xyz[:, None, :], nb.shape)
    rel = tile - nb
    d = np.sqrt((rel * rel).sum(-1, keepdims=True))
    return np.concatenate([d, rel, tile, nb], -1).reshape(-1, 10)


def relpos_dist(rel):
    """distance column from the difference columns [E, 3] -> (dist, bound)"""
    d = np.sqrt((np.asarray(rel, np.float64) ** 2).sum(-1))
    return d, DIST_RATIO * 4 * U * d


def _attention(f, fxyz, neigh, W, dt):
    n, h = f.shape
    cat = np.concatenate([np.asarray(f).astype(dt)[neigh], np.asarray(fxyz).astype(dt).reshape(n, RK, h)], -1)      # [n, 16, d]
    s = cat @ W.astype(dt).T
    m = s.max(1, keepdims=True)
    e = np.exp(s - m)
    a = e / e.sum(1, keepdims=True)
    # first-order bound of a: perturbations of the score (dot product of length d - the split path's T[neigh] + S2 has
    # (h + 3) u of the same magnitude, which is smaller -, the rounding of s - max, expf as one ulp)
    ac = np.abs(cat.astype(np.float64))
    ds = (W.shape[1] + 2) * U * (ac @ np.abs(W).T) + U * np.abs(s) + U * np.abs(s - m) + 2 * U
    a64 = a.astype(np.float64)
    ba = a64 * (ds + (a64 * ds).sum(1, keepdims=True)) + 18 * U * a64
    return cat, a, ba


def att_pool(f, fxyz, neigh, Wb, dt=np.float64, perturb_slot=None):
    """gather [f[neigh], f_xyz], scores (no bias), softmax over the 16 neighbours, weighted sum -> (agg [n, d], bound)."""
    cat, a, ba = _attention(f, fxyz, neigh, Wb[0], dt)
    if perturb_slot is not None:                                # (negative tests: one neighbour slot's weight off by a factor)
        a = a.copy()
        a[:, perturb_slot[0], :] *= dt(1.0 + perturb_slot[1])
    agg = (cat * a).sum(1)
    ac = np.abs(cat.astype(np.float64))
    b = (ac * ba).sum(1) + (RK + 2) * U * (ac * a).sum(1) + U * np.abs(agg)
    return agg, SOFTMAX_RATIO * b


def seg_sum(vals, bvals, idx, n, extra_terms=0, dt=np.float64):
    """out[j] = sum over the entries e with idx[e] == j of vals[e] (the inverse-list gathers / the float-atomic scatters)"""
    out = np.zeros((n,) + vals.shape[1:], dt)
    np.add.at(out, idx, vals.astype(dt))
    mag = np.zeros((n,) + vals.shape[1:])
    np.add.at(mag, idx, np.abs(vals.astype(np.float64)))
    b = np.zeros_like(mag)
    if bvals is not None:
        np.add.at(b, idx, bvals)
    cnt = np.bincount(idx, minlength=n).astype(np.float64).reshape((n,) + (1,) * (vals.ndim - 1))
    return out, b + (cnt + 1 + extra_terms) * U * mag + U * np.abs(out)


def att_pool_T(f, fxyz, neigh, Wb, dagg, dt=np.float64):
    """transpose of att_pool w.r.t. f: through the softmax (ds = a (g - sum a g), g = cat dagg), the direct term a dagg, the
    score layer's feature half and the gather over the in-edges -> (df [n, h], bound), before the activation's derivative."""
    W = Wb[0]
    n, h = f.shape
    d = 2 * h
    cat, a, ba = _attention(f, fxyz, neigh, W, dt)
    dagg = np.asarray(dagg).astype(dt)[:, None, :]
    g = cat * dagg
    dot = (a * g).sum(1, keepdims=True)
    ds = a * (g - dot)
    ddir = a[:, :, :h] * dagg[:, :, :h]
    a64, g64 = a.astype(np.float64), np.abs(g.astype(np.float64))
    bdot = (ba * g64 + a64 * U * g64).sum(1, keepdims=True) + (RK + 2) * U * (a64 * g64).sum(1, keepdims=True)
    gd = np.abs((g - dot).astype(np.float64))
    bds = ba * gd + a64 * (U * g64 + bdot + U * gd) + U * np.abs(ds)
    bddir = ba[:, :, :h] * np.abs(dagg[:, :, :h].astype(np.float64)) + U * np.abs(ddir)
    W1 = W[:, :h]
    edge = ddir + ds @ W1.astype(dt)                            # [n, 16, h]
    edge_mag = np.abs(ddir.astype(np.float64)) + np.abs(ds.astype(np.float64)) @ np.abs(W1)
    bedge = bddir + bds @ np.abs(W1)
    # every product passes through at most d + 1 additions on its edge and cnt on its row, in whichever order the path takes
    # them (per-edge GEMM then gather, or gather then GEMM on points): (d + cnt + 4) u on the magnitudes
    idx = neigh.reshape(-1)
    out = np.zeros((n, h), dt)
    np.add.at(out, idx, edge.reshape(-1, h))
    mag, b = np.zeros((n, h)), np.zeros((n, h))
    np.add.at(mag, idx, edge_mag.reshape(-1, h))
    np.add.at(b, idx, bedge.reshape(-1, h))
    cnt = np.bincount(idx, minlength=n).astype(np.float64)[:, None]
    return out, SOFTMAX_T_RATIO * (b + (d + cnt + 4) * U * mag + U * np.abs(out))


def max_pool(enc, nbp):
    """max over the 16 gathered rows of every sampled row, arg = lowest k that attains it (exact)"""
    g = enc[nbp]                                                # [n_sub, 16, C]
    return g.max(1), g.argmax(1).astype(np.uint8)


def max_pool_T(d_samp, arg, nbp, n, dt=np.float64):
    """row nbp[r, arg[r, c]] collects d_samp[r, c] -> (d_enc part [n, C], bound)"""
    r, C = d_samp.shape
    rows = np.take_along_axis(nbp, arg.astype(np.int64), 1)     # [n_sub, C]
    cols = np.broadcast_to(np.arange(C)[None, :], rows.shape)
    out, mag, cnt = np.zeros((n, C), dt), np.zeros((n, C)), np.zeros((n, C))
    np.add.at(out, (rows, cols), np.asarray(d_samp).astype(dt))
    np.add.at(mag, (rows, cols), np.abs(np.asarray(d_samp, np.float64)))
    np.add.at(cnt, (rows, cols), 1.0)
    return out, (cnt + 1) * U * mag


def upsample_cat(skip, coarse, up):
    return np.concatenate([skip, coarse[up]], 1)


def colper_dlogits(z, y):
    """gradient of sum_n max(0, max_k((1 - onehot) z)_k - z_y) w.r.t. z (the masked entry of the true class is 0 and takes
    part in the max)"""
    n = z.shape[0]
    ar = np.arange(n)
    masked = np.array(z, np.float64)
    masked[ar, y] = 0.0
    oi = masked.argmax(1)
    on = masked[ar, oi] - z[ar, y] > 0
    dz = np.zeros(z.shape, np.float64)
    dz[ar[on], y[on]] = -1.0
    hit = on & (oi != y)
    dz[ar[hit], oi[hit]] = 1.0
    return dz


def unpack_bits(words, M):
    """[rows, ceil(M / 32)] sign-bit words -> [rows, M] bool"""
    w = np.asarray(words).astype(np.uint32).reshape(len(words), -1)
    c = np.arange(M)
    return ((w[:, c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)


# ---------------------------------------------------------------------------------------------------- comparison
class Report:
    def __init__(self):
        self.fail, self.ratio, self.flips, self.stages = [], {}, {}, []

    def note(self, msg):
        self.fail.append(msg)

    def softmax_ratio(self):
        """largest error / first-order bound over the softmax stages (the figures SOFTMAX_MEASURED / SOFTMAX_T_MEASURED record)"""
        r = [SOFTMAX_RATIO * v for k, v in self.ratio.items() if k[0] in ("agg1", "agg2")]
        r += [SOFTMAX_T_RATIO * v for k, v in self.ratio.items() if k[0] in ("d_fagg1", "d_fpc")]
        return max(r) if r else 0.0

    def dist_ratio(self):
        """largest error / (4 u |dist|) over the relpos distances (the figure DIST_MEASURED records)"""
        r = [DIST_RATIO * v for k, v in self.ratio.items() if k[0] == "relpos[0]"]
        return max(r) if r else 0.0


def compare(rep, key, got, ref, bound):
    """every entry of got within bound of ref; bound None: bit-equal.  Records the largest error / bound of the stage."""
    rep.stages.append(key)
    got = np.asarray(got)
    if got.shape != ref.shape:
        rep.note("%s: shape %s, expected %s" % (key, got.shape, ref.shape))
        return
    if bound is None:
        bad = got != ref                                        # bit-equal: +0.0 and -0.0 differ
        if got.dtype.kind == "f" and ref.dtype == got.dtype:
            bad = got.view("u%d" % got.itemsize) != ref.view("u%d" % ref.itemsize)
        if bad.any():
            i = np.argwhere(bad)[0]
            rep.note("%s: %d entries not bit-equal, first at %s: got %r, want %r" % (key, bad.sum(), tuple(i), got[tuple(i)], ref[tuple(i)]))
        return
    err = np.abs(got.astype(np.float64) - ref)
    if not np.isfinite(got).all():
        rep.note("%s: non-finite entries" % (key,))
        return
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    rep.ratio[key] = float(ratio.max()) if ratio.size else 0.0
    bad = err > bound
    if bad.any():
        i = tuple(np.argwhere(ratio == ratio.max())[0])
        rows = np.unique(np.argwhere(bad)[:, 0])
        rep.note("%s: %d of %d entries beyond the bound (rows %s..%s, %d rows); worst at %s: got %.9g, want %.9g, err %.3g, bound %.3g"
                 % (key, bad.sum(), bad.size, rows[0], rows[-1], len(rows), i, got[i], ref[i], err[i], bound[i]))


def compare_mask(rep, key, bits, z, bz):
    """bit == (z > 0) wherever |z| > bz; inside the bound either value passes, but at most MASK_CAP of the entries differ"""
    want = z > 0
    diff = np.asarray(bits) != want
    outside = diff & (np.abs(z) > bz)
    rep.flips[key] = (int(diff.sum()), int(diff.size))
    if outside.any():
        i = tuple(np.argwhere(outside)[0])
        rep.note("%s: %d sign bits differ outside the bound, first at %s: z = %.6g, bound %.3g" % (key, outside.sum(), i, z[i], bz[i]))
    elif diff.sum() > MASK_CAP * diff.size:
        rep.note("%s: %d of %d sign bits differ inside the bound (cap %g)" % (key, diff.sum(), diff.size, MASK_CAP))


# ---------------------------------------------------------------------------------------------------- the network
class _Walk:
    """emulate (taps None): outputs are kept and fed on; check: outputs are compared, the snapshot's values are fed on"""

    def __init__(self, taps, dt):
        self.taps, self.dt, self.t, self.rep = taps, dt, {}, Report()

    def out(self, key, value, bound):
        if self.taps is None:
            self.t[key] = value
            return value
        compare(self.rep, key, self.taps[key], value, bound)
        return np.asarray(self.taps[key]).astype(np.float64)

    def bits(self, key, z, bz):
        if self.taps is None:
            self.t[key] = z > 0
            return self.t[key]
        compare_mask(self.rep, key, self.taps[key], z, bz)
        return np.asarray(self.taps[key])

    def act_conv(self, key, mkey, x, Wb, pre=None):
        out, bo, z, bz = conv(x, Wb, pre=pre, act=True, dt=self.dt)
        if mkey is not None:
            self.bits(mkey, z, bz)
        return self.out(key, out, bo)


def walk_forward(P, feats, geo, taps=None, dt=np.float64, hook=None):
    """the forward stages in the order of psg_rla_forward -> (taps, Report).  hook (negative tests): {stage key: kwargs}."""
    w = _Walk(taps, dt)
    hook = hook or {}
    fin = w.act_conv(("f0", 0), ("m_f0", 0), feats, P["fc0"])
    enc0 = samp = None
    samps = []
    for i in range(5):
        E = "Encoder_layer_%d" % i
        nb, pool = geo["neigh"][i], geo["pool"][i]
        fpc = w.act_conv(("fpc", i), ("m_fpc", i), fin, P[E + "mlp1"])
        rp = relpos(geo["xyz"][i], nb, dt)
        if taps is not None:
            got = np.asarray(taps[("relpos", i)])
            compare(w.rep, ("relpos[1:]", i), got[:, 1:], relpos(geo["xyz"][i], nb, np.float32)[:, 1:], None)
            dist, bd = relpos_dist(got[:, 1:4])
            compare(w.rep, ("relpos[0]", i), got[:, 0], dist, bd)
            rp = got.astype(np.float64)
        else:
            w.t[("relpos", i)] = rp
        fxyz1 = w.act_conv(("fxyz1", i), None, rp, P[E + "LFAmlp1"])
        fxyz2 = w.act_conv(("fxyz2", i), None, fxyz1, P[E + "LFAmlp2"])
        agg1 = w.out(("agg1", i), *att_pool(fpc, fxyz1, nb, P[E + "LFAatt_pooling_1fc"], dt, **hook.get(("agg1", i), {})))
        fagg1 = w.act_conv(("fagg1", i), ("m_fagg1", i), agg1, P[E + "LFAatt_pooling_1mlp"])
        agg2 = w.out(("agg2", i), *att_pool(fagg1, fxyz2, nb, P[E + "LFAatt_pooling_2fc"], dt, **hook.get(("agg2", i), {})))
        fagg2 = w.act_conv(("fagg2", i), ("m_fagg2", i), agg2, P[E + "LFAatt_pooling_2mlp"])
        sc, bsc, _, _ = conv(fin, P[E + "shortcut"], dt=dt)
        sc = w.out(("sc", i), sc, bsc)
        enc = w.act_conv(("enc", i), ("m_enc", i), fagg2, P[E + "mlp2"], pre=sc)
        if taps is not None:                                    # max is exact: on the snapshot's own enc, in its own dtype
            s, a = max_pool(np.asarray(taps[("enc", i)]), nb[pool])
            compare(w.rep, ("samp", i), taps[("samp", i)], s, None)
            compare(w.rep, ("arg", i), taps[("arg", i)], a, None)
            samp = np.asarray(taps[("samp", i)]).astype(np.float64)
        else:
            samp, w.t[("arg", i)] = max_pool(enc, nb[pool])
            w.t[("samp", i)] = samp
        if i == 0:
            enc0 = enc
        samps.append(samp)
        fin = samp
    feat = w.act_conv(("dec0", 0), ("m_dec0", 0), samp, P["decoder_0"])
    for j in range(5):
        lvl = 4 - j
        skip = enc0 if j == 4 else samps[3 - j]
        if taps is not None:
            skip_t = taps[("enc", 0)] if j == 4 else taps[("samp", 3 - j)]
            coarse_t = taps[("dec0", 0)] if j == 0 else taps[("dec_out", j - 1)]
            compare(w.rep, ("dec_cat", j), taps[("dec_cat", j)], upsample_cat(np.asarray(skip_t), np.asarray(coarse_t), geo["up"][lvl]), None)
            cat = np.asarray(taps[("dec_cat", j)]).astype(np.float64)
        else:
            cat = w.t[("dec_cat", j)] = upsample_cat(skip, feat, geo["up"][lvl])
        feat = w.act_conv(("dec_out", j), ("m_dec", j), cat, P["Decoder_layer_%d" % j])
    f1 = w.act_conv(("fc1o", 0), ("m_fc1", 0), feat, P["fc1"])
    f2 = w.act_conv(("fc2o", 0), ("m_fc2", 0), f1, P["fc2"])
    lo, blo, _, _ = conv(f2, P["fc"], dt=dt)
    w.out(("logits", 0), lo, blo)
    return w.t, w.rep


def walk_backward(P, fwd, dlogits, geo, taps=None, dt=np.float64, hook=None):
    """the gradient buffers in the order of psg_rla_backward, each the sum of its contributors in the order the host code
    lists them; fwd = the forward snapshot (values, arg bytes, sign bits as [rows, M] bool) -> (taps, Report).
    hook (negative tests): {gradient key: the mask key to apply INSTEAD of the right one}."""
    w = _Walk(taps, dt)
    hook = hook or {}
    F = lambda k, i=0: np.asarray(fwd[(k, i)])                 # noqa: E731

    def masked(key, mkey, v, b):
        mkey = hook.get(key, mkey)
        return w.out(key, *lrelu_T(v, b, F(*mkey), dt))

    d_fc2o = masked(("d_fc2o", 0), ("m_fc2", 0), *conv_T(dlogits, P["fc"], dt=dt))
    d_fc1o = masked(("d_fc1o", 0), ("m_fc1", 0), *conv_T(d_fc2o, P["fc2"], dt=dt))
    d_dec = {4: masked(("d_dec_out", 4), ("m_dec", 4), *conv_T(d_fc1o, P["fc1"], dt=dt))}
    skip_part = {}                                              # decoder's contribution to d_samp[i] / d_enc[0]: (value, bound)
    d_dec0 = None
    for j in range(4, -1, -1):
        lvl = 4 - j
        Wb = P["Decoder_layer_%d" % j]
        cs = Wb[0].shape[0]
        dcat, bdcat = conv_T(d_dec[j], Wb, dt=dt)               # (lives in scratch: no tap; its bound goes to both consumers)
        if dt != np.float64:
            dcat = dcat.astype(dt)
        skip_part[lvl - 1] = (dcat[:, :cs], bdcat[:, :cs])      # key -1: d_enc of level 0
        n_sub = len(geo["pool"][lvl])
        v, b = seg_sum(dcat[:, cs:], bdcat[:, cs:], geo["up"][lvl], n_sub, dt=dt)
        if j == 0:
            d_dec0 = masked(("d_dec0", 0), ("m_dec0", 0), v, b)
        else:
            d_dec[j - 1] = masked(("d_dec_out", j - 1), ("m_dec", j - 1), v, b)
    # d_samp[i] = decoder skip part + next level's shortcut^T + next level's mlp1^T (level 4: decoder_0^T alone); the encoder
    # runs deepest level first, so level i + 1's d_enc and d_fpc exist when d_samp[i] is closed
    d_enc, d_fpc = {}, {}
    out = {}
    for i in range(4, -1, -1):
        E = "Encoder_layer_%d" % i
        nb, pool = geo["neigh"][i], geo["pool"][i]
        n, d = len(nb), D_OUT[i]
        if i == 4:
            d_samp = w.out(("d_samp", 4), *conv_T(d_dec0, P["decoder_0"], dt=dt))
        else:
            N1 = "Encoder_layer_%d" % (i + 1)
            d_samp = w.out(("d_samp", i), *acc([skip_part[i], conv_T(d_enc[i + 1], P[N1 + "shortcut"], dt=dt),
                                                conv_T(d_fpc[i + 1], P[N1 + "mlp1"], dt=dt)]))
        parts = [max_pool_T(d_samp, F("arg", i), nb[pool], n, dt)]
        if i == 0:
            parts.insert(0, skip_part[-1])
        v, b = acc(parts)
        d_enc[i] = masked(("d_enc", i), ("m_enc", i), v, b)
        g_fagg2 = masked(("g_fagg2", i), ("m_fagg2", i), *conv_T(d_enc[i], P[E + "mlp2"], dt=dt))
        g_agg2 = w.out(("g_agg2", i), *conv_T(g_fagg2, P[E + "LFAatt_pooling_2mlp"], dt=dt))
        d_fagg1 = masked(("d_fagg1", i), ("m_fagg1", i), *att_pool_T(F("fagg1", i), F("fxyz2", i), nb, P[E + "LFAatt_pooling_2fc"], g_agg2, dt))
        g_agg1 = w.out(("g_agg1", i), *conv_T(d_fagg1, P[E + "LFAatt_pooling_1mlp"], dt=dt))
        d_fpc[i] = masked(("d_fpc", i), ("m_fpc", i), *att_pool_T(F("fpc", i), F("fxyz1", i), nb, P[E + "LFAatt_pooling_1fc"], g_agg1, dt))
    v, b = acc([conv_T(d_enc[0], P["Encoder_layer_0shortcut"], dt=dt), conv_T(d_fpc[0], P["Encoder_layer_0mlp1"], dt=dt)])
    d_f0 = masked(("d_f0", 0), ("m_f0", 0), v, b)
    w.out(("dfeatures", 0), *conv_T(d_f0, P["fc0"], dt=dt))
    return w.t, w.rep


def check_inverse(rep, key, keys, n_targets, off, ent):
    """the inverse list (off [n_targets + 1], ent [len(keys)]) is the exact transpose of `keys`, ascending within a row"""
    keys = np.asarray(keys).reshape(-1)
    want_ent = np.argsort(keys, kind="stable")
    want_off = np.searchsorted(keys[want_ent], np.arange(n_targets + 1), side="left")
    compare(rep, (key + "_ent", 0), np.asarray(ent).reshape(-1), want_ent.astype(np.int32), None)
    compare(rep, (key + "_off", 0), np.asarray(off).reshape(-1), want_off.astype(np.int32), None)
