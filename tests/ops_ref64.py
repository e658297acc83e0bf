"""float64 statements of the per-operator entry points of include/psg.h ("Per-operator entry points": csrc/psg_ops.hip and
the end of csrc/psg_resgcn.hip), the worst-case float32 bounds they are tested with, the seeded inputs of every case and
the checks themselves (tests/test_ops_kernels.py runs them on the kernels' outputs and, without a GPU, on deliberately wrong
variants of the references).

Two classes of input.

EXACT: small integers and dyadic fractions, so that every product and every partial sum is a float32 number whatever the
order of the sum and whether or not a multiply-add is fused; the float64 result, rounded to float32 (which changes nothing),
is then what ANY correct float32 evaluation gives, and the kernels must produce its bytes.  assert_exact() checks the
precondition on the float64 side.

REAL: standard normal operands (weights scaled by 0.2).  u = 2^-24 is the unit roundoff of float32.  The bounds, none of
which rests on a measured constant:

  dot product of length K plus bias, any order, fused or not
      B = (K + 2) u (sum_k |x_k w_k| + |b|).
      The computed value is sum_k x_k w_k (1 + d_k) + b (1 + d_b) with |1 + d| <= (1 + u)^(K + 1): every term passes through
      at most one rounding of its product and at most K additions (K - 1 among the products, one with the bias; a fused
      multiply-add only removes roundings).  (1 + u)^(K + 1) - 1 <= (K + 2) u for (K + 1) u < 2 / (K + 2), i.e. every K here.
  ReLU and affine after it, y = s relu(z) + t
      |s| B + 2 u (|s relu(z)| + |t|): relu is exact and 1-Lipschitz, so its argument's error B is scaled by |s|; the
      product and the sum round once each (u |s relu z| and u |s relu z + t|), second-order terms are covered by the
      factor 2 on |t| and by the slack of B.
  atomic or gathered sum of n terms, each term rounded at most once before it is added
      (n + 1) u sum |terms|: one rounding of the term and at most n - 1 additions give (1 + u)^n - 1 <= (n + 1) u.

A pre-activation with |z64| <= B is UNDECIDED: float32 may see either sign.  Either bit is accepted there, and the output
must agree with the bit the kernel itself wrote: clear -> exactly shift[c] (0 without an affine), set -> within the bound.
Everywhere else the bit is the float64 one, a clear bit's output is exactly shift[c], and a case may have at most
UNDECIDED_CAP undecided entries."""
import functools

import numpy as np

U = 2.0 ** -24
F = np.float32
D = np.float64
UNDECIDED_CAP = 1e-3
KNB = 16                                     # neighbours of the ResGCN graph operators


def seeded(*ints):
    return np.random.default_rng(list(ints))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, ref.dtype, ref.shape)
    if got.size == 0:
        return
    bad = np.nonzero((bits(got).reshape(got.shape + (-1,)) != bits(ref).reshape(ref.shape + (-1,))).any(-1).reshape(-1))[0]
    assert bad.size == 0, "%s: %d elements differ, first at flat index %d" % (what, bad.size, bad[0])


def assert_exact(grid, *abs_sums):
    """The EXACT precondition: every listed array holds, entry by entry, the sum of the MAGNITUDES of the terms of one sum
    (so it bounds every partial sum in every order); all terms are multiples of `grid` (a power of two).  Then every partial
    sum is a multiple of grid below 2^24 grid, i.e. a float32 number, and no rounding ever happens."""
    for s in abs_sums:
        s = np.asarray(s, D)
        assert np.all(s / grid == np.round(s / grid)), "a magnitude sum is off the grid 2^%d" % int(np.log2(grid))
        assert s.size == 0 or float(s.max()) < 2.0 ** 24 * grid, "a partial sum may reach 2^24 ulps of the grid: %g" % float(s.max())


def pos0(a):
    """-0 -> +0 (a sum that starts from +0 never ends at -0 in round-to-nearest)"""
    return np.asarray(a, D) + 0.0


def ratio_line(name, ratio, undecided=0):
    print("RATIO %-46s %.4f undecided %d" % (name, ratio, undecided))


def check_bound(name, got, ref, bound):
    """every entry within its bound of the float64 value; prints the largest error / bound"""
    got = np.asarray(got, D)
    err = np.abs(got - ref)
    ok = err <= bound                                    # NaN (a canary that was never overwritten) fails
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    ratio_line(name, float(np.nanmax(r)) if r.size else 0.0)
    assert ok.all(), "%s: %d of %d entries outside the bound (worst error / bound %.3g)" % (
        name, int((~ok).sum()), ok.size, float(np.nanmax(np.where(ok, 0.0, r))) if np.isfinite(r[~ok]).any() else float("inf"))


# ================================================================================================ ReLU bit tables
def words(M):
    return (M + 31) // 32


def pack_bits(bit, stride=None):
    """[rows][M] bool -> the flat uint32 table with rows of `stride` words (default ceil(M / 32), the contract); bits at
    channels >= M of the last word are 0.  A smaller stride models a kernel that packs rows of M / 32 words: later rows
    overwrite the tail of earlier ones."""
    rows, M = bit.shape
    nw = words(M)
    pad = np.zeros((rows, nw * 32), bool)
    pad[:, :M] = bit
    w = (pad.reshape(rows, nw, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    if stride is None or stride == nw:
        return w
    flat = np.zeros(rows * nw, np.uint32)
    for r in range(rows):
        flat[r * stride:r * stride + nw] = w[r]
    return flat.reshape(rows, nw)


def unpack_bits(table, M, stride=None):
    """the flat table read with rows of `stride` words -> [rows][M] bool"""
    rows = table.shape[0]
    nw = words(M)
    flat = np.ascontiguousarray(table).reshape(-1).astype(np.uint32)
    if stride is None:
        stride = nw
    idx = (np.arange(rows)[:, None] * stride + np.arange(nw)[None, :])
    w = flat[idx]
    return (((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)).reshape(rows, nw * 32)[:, :M]


def random_bits(rng, rows, M):
    return rng.random((rows, M)) < 0.6


# ================================================================================================ 1. the shared layer
SMALL_SHAPES = ((1, 1, 1), (63, 12, 32), (130, 259, 70), (200, 37, 70), (512, 96, 192), (512, 96, 256))
LARGE_SHAPES = ((2048, 64, 1024), (2051, 64, 1029), (2048, 37, 1024))
GEMM_SHAPES = SMALL_SHAPES + LARGE_SHAPES
# (name, bias, relu, affine, mask_out); a linear layer has no ReLU bits, so it takes no mask_out
VARIANTS = (("lin", False, False, False, False), ("lin+b", True, False, False, False), ("relu", True, True, False, False),
            ("relu+m", True, True, False, True), ("aff", True, True, True, False), ("aff+m", True, True, True, True))
STRIDES = ((0, 0), (1, 0), (4, 0), (0, 3), (1, 3), (4, 3))          # (ld_in - K, ld_out - M)
EXACT_SCALES = np.array([0.5, 1.0, 2.0, -1.0])


def draw_layer(rng, rows, K, M, exact):
    """operands of one layer.  EXACT: a fifth of the channels have a zero weight row and bias, a tenth of the rows are zero
    (their pre-activation is the bias, 0 for a fifth of the channels): about a fifth of the pre-activations are exactly 0."""
    if exact:
        x = rng.integers(-4, 5, (rows, K)).astype(F)
        w = rng.integers(-2, 3, (M, K)).astype(F)
        b = rng.integers(-3, 4, M).astype(F)
        dead = rng.random(M) < 0.2
        w[dead] = 0
        b[dead] = 0
        x[rng.random(rows) < 0.1] = 0
        sc = EXACT_SCALES[rng.integers(0, 4, M)].astype(F)
        sh = (rng.integers(-16, 17, M) / 8.0).astype(F)
    else:
        x = rng.standard_normal((rows, K)).astype(F)
        w = (rng.standard_normal((M, K)) * 0.2).astype(F)
        b = rng.standard_normal(M).astype(F)
        sc = (rng.uniform(0.5, 1.5, M) * np.where(rng.random(M) < 0.25, -1, 1)).astype(F)
        sh = rng.standard_normal(M).astype(F)
    return x, w, b, sc, sh


@functools.lru_cache(maxsize=2)
def gemm_case(shape, exact):
    rows, K, M = shape
    x, w, b, sc, sh = draw_layer(seeded(101, rows, K, M, int(exact)), rows, K, M, exact)
    x64, w64 = x.astype(D), w.astype(D)
    c = dict(shape=shape, exact=exact, x=x, w=w, b=b, sc=sc, sh=sh, dot=x64 @ w64.T, absdot=np.abs(x64) @ np.abs(w64).T,
             name="%dx%dx%d %s" % (rows, K, M, "exact" if exact else "real"))
    if exact:
        assert_exact(2.0 ** -3, (c["absdot"] + np.abs(b.astype(D))) * 2 + 2)       # |scale| <= 2, |shift| <= 2, grid 2^-3
    return c


def layer_ref(c, variant, mutant=None):
    """out = [relu](x . w^T + bias) [* scale + shift] in float64, the ReLU bits, the bound of every entry and the undecided set.
    mutant: one of the wrong kernels of the teeth tests."""
    _, bias, relu, affine, _ = variant
    rows, K, M = c["shape"]
    dot, absdot = c["dot"], c["absdot"]
    b = c["b"].astype(D) if bias else np.zeros(M)
    if mutant == "drop_k":                                  # the last k never enters
        dot = dot - c["x"][:, K - 1:].astype(D) @ c["w"][:, K - 1:].astype(D).T
    if mutant == "nbr_bias":
        b = np.roll(b, 1)
    z = pos0(dot + b)
    B = (K + 2) * U * (absdot + np.abs(b))
    r = dict(z=z, B=B, relu=relu, M=M)
    if not relu:
        r.update(y=z, bound=B, bit=None, und=np.zeros_like(z, bool), clear=np.zeros(M, F))
    else:
        bit = z >= 0 if mutant == "ge" else z > 0
        s, t = (c["sc"].astype(D), c["sh"].astype(D)) if affine else (np.ones(M), np.zeros(M))
        if mutant == "affine_first":
            y = np.maximum(z * s + t, 0)
        else:
            y = np.where(bit, z, 0.0) * s + t
        r.update(y=y, bit=bit, und=np.abs(z) <= B, clear=(c["sh"] if affine else np.zeros(M, F)),
                 bound=(np.abs(s) * B + 2 * U * (np.abs(s * np.maximum(z, 0)) + np.abs(t))) if affine else B)
    if mutant == "reorder":                                 # tiles handed out in another order: 64-row blocks change places
        perm = np.roll(np.arange(rows), -64)
        r["y"] = r["y"][perm]
        if relu:
            r["bit"] = r["bit"][perm]
    return r


def layer_out(r, exact, stride=None):
    """what a kernel that computes r would store: float32 rows and the packed bits"""
    return r["y"].astype(F), (pack_bits(r["bit"], stride) if r["relu"] else None)


def check_layer(name, r, got, got_mask, exact):
    """the whole forward check (see the module docstring).  got [rows][M] float32; got_mask [rows][ceil(M/32)] uint32 or
    None.  Returns the number of undecided entries."""
    M = r["M"]
    if exact:
        assert_bits(got, r["y"].astype(F), name + " out")
        if got_mask is not None:
            assert_bits(got_mask, pack_bits(r["bit"]), name + " ReLU bits")
        return 0
    err = np.abs(got.astype(D) - r["y"])
    inb = err <= r["bound"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / r["bound"])
    if not r["relu"]:
        ratio_line(name, float(ratio.max()))
        assert inb.all(), "%s: %d entries outside the bound, worst %.3g" % (name, int((~inb).sum()), float(ratio.max()))
        return 0
    und = r["und"]
    is_clear = bits(got).reshape(got.shape + (4,)) == bits(np.broadcast_to(r["clear"], got.shape)).reshape(got.shape + (4,))
    is_clear = is_clear.all(-1)
    if got_mask is not None:
        table = np.ascontiguousarray(got_mask).astype(np.uint32)
        if M % 32:
            assert not (table[:, -1] >> np.uint32(M % 32)).any(), name + ": bits at channels >= M of the last word are not zero"
        kbit = unpack_bits(table, M)
        assert (kbit == r["bit"])[~und].all(), "%s: %d decided ReLU bits differ" % (name, int((kbit != r["bit"])[~und].sum()))
        ok = np.where(kbit, inb, is_clear)                   # the output agrees with the bit the kernel wrote
        ok &= und | np.where(r["bit"], inb, is_clear)
    else:
        ok = np.where(und, inb | is_clear, np.where(r["bit"], inb, is_clear))
    ratio_line(name, float(np.where(is_clear & ~r["bit"], 0.0, ratio).max()), int(und.sum()))
    assert ok.all(), "%s: %d entries fail (outside the bound, or not exactly shift under a clear bit)" % (name, int((~ok).sum()))
    return int(und.sum())


# ---- backward: din = (dout . w) * bits of the layer below;  wT [K][M]
@functools.lru_cache(maxsize=2)
def bwd_case(shape, exact):
    rows, K, M = shape
    rng = seeded(102, rows, K, M, int(exact))
    if exact:
        g = rng.integers(-4, 5, (rows, M)).astype(F)
        wT = rng.integers(-2, 3, (K, M)).astype(F)
        g[rng.random(rows) < 0.1] = 0
    else:
        g = rng.standard_normal((rows, M)).astype(F)
        wT = (rng.standard_normal((K, M)) * 0.2).astype(F)
    c = dict(shape=shape, exact=exact, g=g, wT=wT, below=random_bits(rng, rows, K), dot=pos0(g.astype(D) @ wT.astype(D).T),
             absdot=np.abs(g.astype(D)) @ np.abs(wT.astype(D)).T, name="bwd %dx%dx%d %s" % (rows, K, M, "exact" if exact else "real"))
    if exact:
        assert_exact(1.0, c["absdot"])
    return c


def bwd_ref(c, with_mask, mutant=None):
    rows, K, M = c["shape"]
    dot = c["dot"]
    if mutant == "drop_k":
        dot = pos0(dot - c["g"][:, M - 1:].astype(D) @ c["wT"][:, M - 1:].astype(D).T)
    bit = np.ones((rows, K), bool)
    if with_mask:
        bit = unpack_bits(pack_bits(c["below"]), K, K // 32 if mutant == "mask_stride" else None)
    return dict(y=np.where(bit, dot, 0.0), bit=bit, bound=(M + 2) * U * c["absdot"])


def check_bwd(name, r, got, exact):
    if exact:
        assert_bits(got, r["y"].astype(F), name)
        return
    assert_bits(got[~r["bit"]], np.zeros(int((~r["bit"]).sum()), F), name + ": entries under a clear bit")
    check_bound(name, got, r["y"], r["bound"])


# ---- backward through a layer's own ReLU: one float32 product, so float32(float64 product) is THE result on all inputs
RELU_BITS_M = (1, 31, 32, 33, 70)


def relu_bits_case(M, exact):
    rows = 130
    rng = seeded(103, M, int(exact))
    g = rng.integers(-4, 5, (rows, M)).astype(F) if exact else rng.standard_normal((rows, M)).astype(F)
    g[::7, ::3] = F(-0.0)
    sc = EXACT_SCALES[rng.integers(0, 4, M)].astype(F) if exact else rng.standard_normal(M).astype(F)
    return dict(M=M, rows=rows, g=g, sc=sc, bit=random_bits(rng, rows, M), name="relu_bits M=%d %s" % (M, "exact" if exact else "real"))


def relu_bits_ref(c, with_scale, mutant=None):
    bit = unpack_bits(pack_bits(c["bit"]), c["M"], c["M"] // 32 if mutant == "mask_stride" else None)
    v = (c["g"].astype(D) * c["sc"].astype(D)).astype(F) if with_scale else c["g"]
    return np.where(bit, v, F(0.0)).astype(F)


# ================================================================================================ 3. the SA stack
SA_CASES = (((5,), 3, 1, 1), ((5,), 12, 16, 7), ((32, 32, 64), 12, 16, 130), ((32, 32, 64), 3, 255, 7), ((33, 70, 40), 3, 255, 1),
            ((33, 70, 40), 12, 1, 130), ((33, 70, 40), 12, 16, 7))       # (widths, cin, K, n_groups)


@functools.lru_cache(maxsize=None)
def sa_case(i, exact):
    widths, cin, K, G = SA_CASES[i]
    rng = seeded(104, i, int(exact))
    rows = G * K
    if exact:
        x = rng.integers(-4, 5, (rows, cin)).astype(F)
        dout = rng.integers(-4, 5, (G, widths[-1])).astype(F)
    else:
        x = rng.standard_normal((rows, cin)).astype(F)
        dout = rng.standard_normal((G, widths[-1])).astype(F)
    ws, bs, c_in = [], [], cin
    for wd in widths:
        if exact:                                            # ternary and sparse: three layers stay small integers
            ws.append((rng.integers(-1, 2, (wd, c_in)) * (rng.random((wd, c_in)) < 0.5)).astype(F))
            bs.append(-rng.integers(0, 2, wd).astype(F) + F(0.0))     # biases <= 0: a zero row stays zero through every layer
        else:
            ws.append((rng.standard_normal((wd, c_in)) * 0.2).astype(F))
            bs.append(rng.standard_normal(wd).astype(F))
        c_in = wd
    zero_g, same_g = (0, 1) if G > 1 else ((0, None) if i % 2 == 0 else (None, 0))
    if zero_g is not None and exact:
        x[zero_g * K:(zero_g + 1) * K] = 0                   # every last-layer output 0: arg = 0, zero gradient
    if same_g is not None:
        x[same_g * K:(same_g + 1) * K] = x[same_g * K]       # K identical rows: arg = 0
    return dict(widths=widths, cin=cin, K=K, G=G, rows=rows, x=x, w=ws, b=bs, dout=dout, exact=exact, zero_g=zero_g if exact else None,
                same_g=same_g, name="sa %s cin=%d K=%d G=%d %s" % (list(widths), cin, K, G, "exact" if exact else "real"))


def first_argmax(v, axis, last=False):
    """torch.max's choice: the first index that attains the maximum (last=True: the wrong one)"""
    if last:
        n = v.shape[axis]
        return n - 1 - np.argmax(np.flip(v, axis), axis)
    return np.argmax(v, axis)


def sa_ref(c, mutant=None):
    """float64 stack: per layer relu(h . w^T + b) and its bits, the max over the K samples with the first arg-max, and the input
    gradient of dout.  Also the magnitude sums assert_exact needs."""
    h = c["x"].astype(D)
    habs = np.abs(h)
    masks, mags = [], []
    for w, b in zip(c["w"], c["b"]):
        z = pos0(h @ w.astype(D).T + b.astype(D))
        mags.append(habs @ np.abs(w.astype(D)).T + np.abs(b.astype(D)))
        bit = z >= 0 if mutant == "ge" else z > 0
        masks.append(bit)
        h = np.where(z > 0, z, 0.0)
        habs = mags[-1]
    C = h.shape[1]
    hk = h.reshape(c["G"], c["K"], C)
    arg = first_argmax(hk, 1, last=mutant == "last_max")
    out = np.take_along_axis(hk, arg[:, None, :], 1)[:, 0, :]
    g = np.zeros_like(hk)
    np.put_along_axis(g, arg[:, None, :], c["dout"].astype(D)[:, None, :], 1)
    g = g.reshape(c["rows"], C) * masks[-1]
    gabs = np.abs(g)
    for l in range(len(c["w"]) - 1, -1, -1):
        g = pos0(g @ c["w"][l].astype(D))
        gabs = gabs @ np.abs(c["w"][l].astype(D))
        mags.append(gabs)
        if l:
            g = np.where(masks[l - 1], g, 0.0)
    return dict(out=out, arg=arg.astype(np.uint8), masks=masks, drows=g, last=h, mags=mags)


# ================================================================================================ 4. grouping
def group_cases():
    out, i = [], 0
    for B in (1, 2):
        for N in (5, 300):
            for S in (1, 17):
                for K in (1, 16):
                    for Dn in (0, 6, 9):
                        for ff in (0, 1):
                            out.append((i, B, N, S, K, Dn, ff))
                            i += 1
    return out


@functools.lru_cache(maxsize=None)
def group_case(key, exact):
    i, B, N, S, K, Dn, ff = key
    rng = seeded(105, i, int(exact))
    if exact:                                                # coordinates on the 2^-6 grid, integer features and gradients
        xyz = (rng.integers(-64, 65, (B, N, 3)) / 64.0).astype(F)
        feat = rng.integers(-4, 5, (B, N, Dn)).astype(F)
        drows = rng.integers(-4, 5, (B * S * K, Dn + 3)).astype(F)
    else:
        xyz = rng.standard_normal((B, N, 3)).astype(F)
        feat = rng.standard_normal((B, N, Dn)).astype(F)
        drows = rng.standard_normal((B * S * K, Dn + 3)).astype(F)
    drows[3::5] = F(0.0)                                     # gradients that contain +0 and -0
    drows[4::5, ::2] = F(-0.0)
    mode = ("random", "hub", "padded")[i % 3]
    gidx = rng.integers(0, N, (B, S, K)).astype(np.int32)
    if mode == "hub":                                        # every index of every group is the same point
        gidx[:] = N // 2
    elif mode == "padded":                                   # ball query's padding: the first hit repeated
        n_hit = rng.integers(1, K + 1, (B, S, 1))
        gidx = np.where(np.arange(K)[None, None, :] < n_hit, gidx, gidx[:, :, :1]).astype(np.int32)
    new_xyz = np.take_along_axis(xyz, gidx[:, :, 0:1].repeat(3, 2).astype(np.int64), 1)    # [B][S][3]: a sampled point each
    return dict(B=B, N=N, S=S, K=K, D=Dn, ff=ff, xyz=xyz, feat=feat, new_xyz=np.ascontiguousarray(new_xyz), gidx=gidx, drows=drows,
                exact=exact, mode=mode, name="group B=%d N=%d S=%d K=%d D=%d ff=%d %s %s" % (B, N, S, K, Dn, ff, mode, "exact" if exact else "real"))


def group_rows_ref(c, mutant=None):
    """rows[(b, s, k)] = [xyz[g] - new_xyz[s], feat[g]] (feat_first: [feat, rel]).  One float32 subtraction or a copy: the
    float64 difference rounded to float32 is the float32 difference (the exact difference is rounded once either way)."""
    B, S, K = c["gidx"].shape
    bi = np.arange(B)[:, None, None]
    rel = (c["xyz"].astype(D)[bi, c["gidx"]] - c["new_xyz"].astype(D)[:, :, None, :]).astype(F)
    f = c["feat"][bi, c["gidx"]]
    ff = c["ff"] ^ (mutant == "feat_first")
    return np.concatenate([f, rel] if ff else [rel, f], -1).reshape(B * S * K, c["D"] + 3)


def group_rows_bwd_ref(c, mutant=None):
    """dfeat[b][g] += the feature columns of drows; returns the float64 sums, the bound and the untouched points"""
    B, N, Dn = c["B"], c["N"], c["D"]
    ff = c["ff"] ^ (mutant == "feat_first")
    g = c["drows"].astype(D).reshape(B, -1, Dn + 3)
    g = g[:, :, :Dn] if ff else g[:, :, 3:]
    flat = (np.arange(B)[:, None] * N + c["gidx"].reshape(B, -1)).reshape(-1)
    s, a, n = np.zeros((B * N, Dn)), np.zeros((B * N, Dn)), np.zeros((B * N, Dn))
    if mutant == "assign":
        s[flat] = g.reshape(-1, Dn)
    else:
        np.add.at(s, flat, g.reshape(-1, Dn))
    np.add.at(a, flat, np.abs(g.reshape(-1, Dn)))
    np.add.at(n, flat, 1.0)
    touched = np.zeros(B * N, bool)
    touched[flat] = True
    return dict(y=pos0(s).reshape(B, N, Dn), mag=a.reshape(B, N, Dn), bound=((n + 1) * U * a).reshape(B, N, Dn), untouched=~touched.reshape(B, N))


# ================================================================================================ 5. 3-NN interpolation
EXACT_W3 = np.array([[0.25, 0.5, 0.25], [1, 0, 0], [0.5, 0.5, 0]], F)


def interp_cases():
    out, i = [], 0
    for N in (1, 301):
        for S in (1, 2, 64):
            for D1 in (0, 5):
                for D2 in (1, 70):
                    out.append((i, 2, N, S, D1, D2))
                    i += 1
    return out


@functools.lru_cache(maxsize=None)
def interp_case(key, exact):
    i, B, N, S, D1, D2 = key
    rng = seeded(106, i, int(exact))
    pad = 2                                                  # dout rows are wider than D1 + D2
    if exact:
        f2 = rng.integers(-4, 5, (B, S, D2)).astype(F)
        f1 = rng.integers(-4, 5, (B, N, D1)).astype(F)
        w = EXACT_W3[rng.integers(0, 3, (B, N))]
        dout = rng.integers(-4, 5, (B, N, D1 + D2 + pad)).astype(F)
    else:
        f2 = rng.standard_normal((B, S, D2)).astype(F)
        f1 = rng.standard_normal((B, N, D1)).astype(F)
        w = rng.random((B, N, 3)) + 0.05
        w = (w / w.sum(-1, keepdims=True)).astype(F)
        dout = rng.standard_normal((B, N, D1 + D2 + pad)).astype(F)
    dout[:, 1::4, ::3] = F(0.0)
    idx = rng.integers(0, S, (B, N, 3)).astype(np.int32)     # S = 1: all three indices equal
    if i % 2:
        idx[:, :, 0] = S - 1                                 # a hub: every point names the last coarse point
    return dict(B=B, N=N, S=S, D1=D1, D2=D2, ld=D1 + D2 + pad, f1=f1, f2=f2, w=np.ascontiguousarray(w), idx=idx, dout=dout, exact=exact,
                name="interp N=%d S=%d D1=%d D2=%d %s" % (N, S, D1, D2, "exact" if exact else "real"))


def interp_fwd_ref(c, dtype=D):
    """[feat1, sum_j w_j feat2[idx_j]] with the order ((w0 f0 + w1 f1) + w2 f2); dtype float32 is the restatement with
    separate roundings that the kernel promises, float64 the reference.  Also sum |terms| for the bound (4 u: n = 3)."""
    bi = np.arange(c["B"])[:, None, None]
    f = c["f2"].astype(dtype)[bi, c["idx"]]                  # [B][N][3][D2]
    t = c["w"].astype(dtype)[..., None] * f
    y = (t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]
    out = np.concatenate([c["f1"].astype(dtype), y], -1)
    mag = np.concatenate([np.abs(c["f1"].astype(D)), np.abs(c["w"].astype(D)[..., None] * c["f2"].astype(D)[bi, c["idx"]]).sum(2)], -1)
    bound = np.concatenate([np.zeros(c["f1"].shape), 4 * U * mag[..., c["D1"]:]], -1)
    return out, bound, mag


def interp_bwd_ref(c, mutant=None):
    B, N, S, D1, D2 = c["B"], c["N"], c["S"], c["D1"], c["D2"]
    col0 = 0 if mutant == "col0" else D1
    g = c["dout"].astype(D)[:, :, col0:col0 + D2]
    t = (c["w"].astype(D)[..., None] * g[:, :, None, :]).reshape(-1, D2)          # [B*N*3][D2]
    flat = (np.arange(B)[:, None, None] * S + c["idx"]).reshape(-1)
    s, a, n = np.zeros((B * S, D2)), np.zeros((B * S, D2)), np.zeros((B * S, D2))
    if mutant == "assign":
        s[flat] = t
    else:
        np.add.at(s, flat, t)
    np.add.at(a, flat, np.abs(t))
    np.add.at(n, flat, 1.0)
    return dict(y=pos0(s).reshape(B, S, D2), mag=a.reshape(B, S, D2), bound=((n + 1) * U * a).reshape(B, S, D2))


# ================================================================================================ 6. graph operators
GRAPH_ROOMS = ((1, 16), (3, 100), (2, 257))


def draw_nbr(rng, rooms, N):
    """room-local neighbour tables with the vertex itself, duplicates and a hub"""
    nbr = rng.integers(0, N, (rooms * N, KNB)).astype(np.int32)
    v = np.arange(rooms * N) % N
    nbr[::3, 0] = v[::3]                                     # the vertex itself (what a kNN graph puts first)
    nbr[1::4, 7] = nbr[1::4, 2]                              # a duplicate
    nbr[:, 5] = 0                                            # a hub: everybody names vertex 0 of the room
    return nbr


def mr_cases():
    return [(i * 3 + j, rooms, N, C) for i, (rooms, N) in enumerate(GRAPH_ROOMS) for j, C in enumerate((9, 64, 67))]


@functools.lru_cache(maxsize=None)
def mr_case(key, exact):
    i, rooms, N, C = key
    rng = seeded(107, i, int(exact))
    R = rooms * N
    draw = (lambda *s: rng.integers(-4, 5, s).astype(F)) if exact else (lambda *s: rng.standard_normal(s).astype(F))
    return dict(rooms=rooms, N=N, R=R, C=C, x=draw(R, C), nbr=draw_nbr(rng, rooms, N), dcat=draw(R, 2 * C),
                arg=rng.integers(0, KNB, (R, C)).astype(np.uint8), exact=exact, name="mr %dx%d C=%d %s" % (rooms, N, C, "exact" if exact else "real"))


def global_nbr(c):
    return (np.arange(c["R"]) // c["N"] * c["N"])[:, None] + c["nbr"]


def mr_fwd_ref(c, mutant=None):
    """cat = [x_i, max_k (x_j - x_i)] and the first arg-max: float32(float64 difference) is the float32 difference"""
    x = c["x"].astype(D)
    rel = (x[global_nbr(c)] - x[:, None, :]).astype(F)       # [R][16][C]
    arg = first_argmax(rel, 1, last=mutant == "last_max")
    return np.concatenate([c["x"], np.take_along_axis(rel, arg[:, None, :], 1)[:, 0]], -1), arg.astype(np.uint8)


def mr_bwd_ref(c, mutant=None):
    """dx[i] = dcat_x[i] - dcat_m[i], then dx[nbr(i, arg)] += dcat_m[i]"""
    R, C = c["R"], c["C"]
    gx, gm = c["dcat"].astype(D)[:, :C], c["dcat"].astype(D)[:, C:]
    s = gx.copy() if mutant == "no_self" else gx - gm
    a = np.abs(gx) + np.abs(gm)
    n = np.full((R, C), 2.0)
    tgt = np.take_along_axis(global_nbr(c), c["arg"].astype(np.int64), 1)          # [R][C]
    cols = np.broadcast_to(np.arange(C), (R, C))
    if mutant == "assign":
        s[tgt, cols] = gm
    else:
        np.add.at(s, (tgt, cols), gm)
    np.add.at(a, (tgt, cols), np.abs(gm))
    np.add.at(n, (tgt, cols), 1.0)
    return dict(y=s, mag=a, bound=(n + 1) * U * a)


def edge_cases():
    return [(i * 2 + j, rooms, N, C) for i, (rooms, N) in enumerate(GRAPH_ROOMS) for j, C in enumerate((9, 64))]


@functools.lru_cache(maxsize=None)
def edge_case(key, exact):
    i, rooms, N, C = key
    rng = seeded(108, i, int(exact))
    R = rooms * N
    nbr = draw_nbr(rng, rooms, N)
    if exact:
        x = rng.integers(-4, 5, (R, C)).astype(F)
        wcat = rng.integers(-2, 3, (128, C)).astype(F)
        b = -rng.integers(0, 4, 64).astype(F) + F(0.0)       # <= 0, a quarter exactly 0
        sc = EXACT_SCALES[rng.integers(0, 4, 64)].astype(F)  # a negative scale among them
        sc[0] = -1.0
        sh = (rng.integers(-16, 17, 64) / 8.0).astype(F)
        dead = N - 1                                         # a vertex whose sixteen edges are all inactive: x = 0, only
        x[dead] = 0                                          # itself as neighbour, so z = b <= 0 on every edge
        nbr[dead] = dead
    else:
        x = rng.standard_normal((R, C)).astype(F)
        wcat = (rng.standard_normal((128, C)) * 0.2).astype(F)
        b = rng.standard_normal(64).astype(F)
        sc = (rng.uniform(0.5, 1.5, 64) * np.where(rng.random(64) < 0.25, -1, 1)).astype(F)
        sh = rng.standard_normal(64).astype(F)
        dead = None
    bcat = np.concatenate([b, np.zeros(64, F)])
    return dict(rooms=rooms, N=N, R=R, C=C, x=x, nbr=nbr, wcat=wcat, bcat=bcat, sc=sc, sh=sh, dead=dead, exact=exact,
                name="edge %dx%d C=%d %s" % (rooms, N, C, "exact" if exact else "real"))


def edge_fwd_ref(c, mutant=None):
    """y_i = max_k (scale relu(P_i + Q_j) + shift), [P | Q] = x . wcat^T + bcat; arg = first maximum, bit 7 = that edge was
    active.  Bounds: Bz = B_P + B_Q + u |z| for the sum of the two products (plus second order: factor 1 + u), then the ReLU /
    affine bound per edge; |max_k a_k - max_k b_k| <= max_k |a_k - b_k|."""
    C = c["C"]
    x, w, b = c["x"].astype(D), c["wcat"].astype(D), c["bcat"].astype(D)
    pq = pos0(x @ w.T + b)
    mag = np.abs(x) @ np.abs(w).T + np.abs(b)
    Bpq = (C + 2) * U * mag
    gn = global_nbr(c)
    z = pq[:, None, :64] + pq[gn][:, :, 64:]                 # [R][16][64]
    Bz = (Bpq[:, None, :64] + Bpq[gn][:, :, 64:]) * (1 + U) + U * np.abs(z)
    s, t = c["sc"].astype(D), c["sh"].astype(D)
    act = z >= 0 if mutant == "ge" else z > 0
    yk = np.maximum(z * s + t, 0) if mutant == "affine_first" else np.where(z > 0, z, 0.0) * s + t
    bk = np.abs(s) * Bz + 2 * U * (np.abs(s * np.maximum(z, 0)) + np.abs(t))
    k = first_argmax(yk, 1, last=mutant == "last_max")
    y = np.take_along_axis(yk, k[:, None, :], 1)[:, 0]
    a = np.take_along_axis(act, k[:, None, :], 1)[:, 0]
    return dict(pq=pq, Bpq=Bpq, mag=mag, z=z, Bz=Bz, yk=yk, bk=bk, y=y, bound=bk.max(1), arg=(k | np.where(a, 0x80, 0)).astype(np.uint8))


def check_edge(name, c, r, got_y, got_arg):
    if c["exact"]:
        assert_bits(got_y, r["y"].astype(F), name + " out")
        assert_bits(got_arg, r["arg"], name + " arg")
        if c["dead"] is not None:
            assert not got_arg[c["dead"]].any() and (got_y[c["dead"]] == c["sh"]).all(), name + ": the vertex without an active edge"
        return
    check_bound(name, got_y, r["y"], r["bound"])
    k = (got_arg & 0x7F).astype(np.int64)
    assert (k < KNB).all(), name + ": arg out of range"
    mine = np.take_along_axis(r["yk"], k[:, None, :], 1)[:, 0]
    slack = np.take_along_axis(r["bk"], k[:, None, :], 1)[:, 0] + np.take_along_axis(r["bk"], (r["arg"] & 0x7F).astype(np.int64)[:, None, :], 1)[:, 0]
    assert ((k == (r["arg"] & 0x7F)) | (np.abs(mine - r["y"]) <= slack)).all(), name + ": arg names an edge that is not a maximum within the bound"
    zk = np.take_along_axis(r["z"], k[:, None, :], 1)[:, 0]
    decided = np.abs(zk) > np.take_along_axis(r["Bz"], k[:, None, :], 1)[:, 0]
    assert (((got_arg & 0x80) != 0) == (zk > 0))[decided].all(), name + ": active bit of the winning edge"


# ================================================================================================ 7. pairwise distance
def pd_cases():
    return [(i * 3 + j, 2, N, C) for i, N in enumerate((64, 100, 257)) for j, C in enumerate((9, 64, 67))]


@functools.lru_cache(maxsize=None)
def pd_case(key, exact):
    i, B, N, C = key
    rng = seeded(109, i, int(exact))
    x = rng.integers(-4, 5, (B, N, C)).astype(F) if exact else rng.standard_normal((B, N, C)).astype(F)
    return dict(B=B, N=N, C=C, x=x, exact=exact, name="pd N=%d C=%d %s" % (N, C, "exact" if exact else "real"))


def pd_ref(c, mutant=None):
    """(|x_i|^2 - 2 x_i . x_j) + |x_j|^2.  Bound (C + 4) u (|x_i|^2 + 2 sum |x_ik x_jk| + |x_j|^2): each of the three parts is a
    sum of C products (at most C + 1 roundings per term, as in B above), the product with -2 is exact, two more additions."""
    x = c["x"].astype(D)
    sq = (x * x).sum(-1)
    dot = x @ x.transpose(0, 2, 1)
    y = (sq[:, :, None] - 2 * dot) + (0.0 if mutant == "no_norm" else sq[:, None, :])
    mag = sq[:, :, None] + 2 * (np.abs(x) @ np.abs(x).transpose(0, 2, 1)) + sq[:, None, :]
    return pos0(y), (c["C"] + 4) * U * mag, mag
