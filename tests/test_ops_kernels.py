"""The per-operator entry points of include/psg.h (csrc/psg_ops.hip, the end of csrc/psg_resgcn.hip), each called alone against
tests/ops_ref64.py at ragged shapes: the shared layer psg_pw_mlp_fwd / _bwd through every reachable path of gemm_rows_kernel
(64 x 64 and 128 x 128 workgroup tiles, interior and general, re-ordered and not, every epilogue, padded strides),
psg_apply_relu_bits, the SA stack, grouping, 3-NN interpolation, the MRConv gather, EdgeConv's forward and pairwise_distance.

Every case runs on EXACT inputs (bytes of the float64 result) and on REAL inputs (derived worst-case bounds, none measured; the
module docstring of ops_ref64 derives them).  Outputs are pre-filled with NaN / 0xFF canaries, padding columns of the inputs
hold NaN, every GPU case runs twice and must repeat bit for bit except where float atomics accumulate REAL sums.  All operands
come straight from fresh allocations: base pointers are 16-byte aligned (misaligned operands are not part of this file).

The CPU part pins every reference to torch float64 autograd of its own formula, asserts the EXACT precondition and the cap on
undecided ReLU decisions for every case, and shows that each listed wrong variant of a kernel fails the very check the GPU
tests run, on the very inputs they use."""
import ctypes

import numpy as np
import pytest
import torch

import ops_ref64 as R
from ops_ref64 import D, F, assert_bits, check_bound

EXACT_REAL = (True, False)
CLS = lambda e: "exact" if e else "real"         # noqa: E731
shape_id = lambda s: "x".join(map(str, s))       # noqa: E731


def t64(a):
    return torch.from_numpy(np.asarray(a, D))


def close64(a, b, what):
    a, b = np.asarray(a, D), np.asarray(b, D)
    assert np.abs(a - b).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(b).max(initial=0.0)), what


# ================================================================================================ CPU: the references are right
def test_layer_references_match_torch_float64_autograd():
    for shape in ((63, 12, 32), (130, 259, 70)):
        c = R.gemm_case(shape, False)
        x = t64(c["x"]).requires_grad_(True)
        z = x @ t64(c["w"]).T + t64(c["b"])                                   # conv
        y = torch.relu(z) * t64(c["sc"]) + t64(c["sh"])                       # ReLU, then the BatchNorm affine
        r = R.layer_ref(c, R.VARIANTS[5])
        close64(r["y"], y.detach().numpy(), "layer forward")
        assert np.array_equal(r["bit"], (z > 0).numpy())
        close64(R.layer_ref(c, R.VARIANTS[1])["y"], z.detach().numpy(), "linear layer")
        b = R.bwd_case(shape, False)                                          # din = d/dh of sum(g * (h . W^T)), W = wT^T
        h = torch.zeros(shape[0], shape[1], dtype=torch.float64, requires_grad=True)
        ((h @ t64(b["wT"])) * t64(b["g"])).sum().backward()
        rb = R.bwd_ref(b, True)
        close64(rb["y"], h.grad.numpy() * b["below"], "layer backward")


def test_sa_reference_matches_torch_float64_autograd():
    for i in range(len(R.SA_CASES)):
        c = R.sa_case(i, False)
        x = t64(c["x"]).requires_grad_(True)
        h = x
        for w, b in zip(c["w"], c["b"]):
            h = torch.relu(h @ t64(w).T + t64(b))                             # conv, then ReLU
        out, arg = h.reshape(c["G"], c["K"], -1).max(1)                       # max over the K samples
        (out * t64(c["dout"])).sum().backward()
        r = R.sa_ref(c)
        close64(r["out"], out.detach().numpy(), c["name"])
        # a group of K identical rows: which of the equal samples torch.max names is not pinned (it differs between CPUs), so
        # that group is compared through the sum of its rows' gradients and its arg is left out
        keep = np.ones(c["G"], bool)
        if c["same_g"] is not None:
            keep[c["same_g"]] = False
        gr, gt = r["drows"].reshape(c["G"], c["K"], -1), x.grad.numpy().reshape(c["G"], c["K"], -1)
        close64(gr[keep], gt[keep], c["name"] + " gradient")
        close64(gr.sum(1), gt.sum(1), c["name"] + " gradient summed over a group")
        lone = (r["last"].reshape(c["G"], c["K"], -1) == r["out"][:, None, :]).sum(1) == 1      # (all samples 0 after the ReLU: a tie)
        assert lone[keep].any() and np.array_equal(r["arg"][lone], arg.numpy().astype(np.uint8)[lone])
        first = np.take_along_axis(r["last"].reshape(c["G"], c["K"], -1), r["arg"][None].astype(np.int64).transpose(1, 0, 2), 1)[:, 0]
        assert np.array_equal(first, r["out"])


def test_group_reference_matches_torch_float64_autograd():
    for key in R.group_cases()[::5]:
        c = R.group_case(key, False)
        B, N, S, K, Dn = c["B"], c["N"], c["S"], c["K"], c["D"]
        feat = t64(c["feat"]).requires_grad_(True)
        bi = torch.arange(B)[:, None, None]
        gi = torch.from_numpy(c["gidx"].astype(np.int64))
        rel = t64(c["xyz"])[bi, gi] - t64(c["new_xyz"])[:, :, None, :]        # index_points, centred
        rows = torch.cat([feat[bi, gi], rel] if c["ff"] else [rel, feat[bi, gi]], -1).reshape(B * S * K, Dn + 3)
        assert_bits(R.group_rows_ref(c), rows.detach().numpy().astype(F), c["name"])
        if Dn:
            (rows * t64(c["drows"])).sum().backward()
            close64(R.group_rows_bwd_ref(c)["y"], feat.grad.numpy(), c["name"] + " gradient")


def test_interp_reference_matches_torch_float64_autograd():
    for key in R.interp_cases():
        c = R.interp_case(key, False)
        f2 = t64(c["f2"]).requires_grad_(True)
        bi = torch.arange(c["B"])[:, None, None]
        y = (f2[bi, torch.from_numpy(c["idx"].astype(np.int64))] * t64(c["w"])[..., None]).sum(2)      # the interpolation sum
        out = torch.cat([t64(c["f1"]), y], -1)
        ref, bound, _ = R.interp_fwd_ref(c)
        close64(ref, out.detach().numpy(), c["name"])
        cot = t64(c["dout"])[:, :, :c["D1"] + c["D2"]]
        (out * cot).sum().backward()
        close64(R.interp_bwd_ref(c)["y"], f2.grad.numpy(), c["name"] + " gradient")
        # the float32 restatement with separate roundings lies inside the float64 bound
        assert (np.abs(R.interp_fwd_ref(c, F)[0].astype(D) - ref) <= bound).all(), c["name"]


def test_graph_references_match_torch_float64_autograd():
    for key in R.mr_cases():
        c = R.mr_case(key, False)
        x = t64(c["x"]).requires_grad_(True)
        gn = torch.from_numpy(R.global_nbr(c))
        m, arg = (x[gn] - x[:, None, :]).max(1)
        cat = torch.cat([x, m], -1)                                           # cat[x_i, max_k (x_j - x_i)]
        got, garg = R.mr_fwd_ref(c)
        close64(got, cat.detach().numpy().astype(F), c["name"])
        rel = (x[gn] - x[:, None, :]).detach().numpy()
        lone = (rel == rel.max(1, keepdims=True)).sum(1) == 1                 # a neighbour named twice ties with itself:
        assert lone.any() and np.array_equal(garg[lone], arg.numpy().astype(np.uint8)[lone])      # torch's choice there is not pinned
        assert np.array_equal(np.take_along_axis(rel, garg[:, None, :].astype(np.int64), 1)[:, 0], rel.max(1))
        (cat * t64(c["dcat"])).sum().backward()                               # (either choice names the same vertex: same gradient)
        close64(R.mr_bwd_ref(dict(c, arg=garg))["y"], x.grad.numpy(), c["name"] + " gradient")
    for key in R.edge_cases():
        c = R.edge_case(key, False)
        x, gn = t64(c["x"]), torch.from_numpy(R.global_nbr(c))
        w2 = t64(c["wcat"][64:])
        w1 = t64(c["wcat"][:64]) + w2                                         # wcat = [W1 - W2 ; W2]
        xi = x[:, None, :].expand(-1, R.KNB, -1)
        z = torch.cat([xi, x[gn] - xi], -1) @ torch.cat([w1, w2], 1).T + t64(c["bcat"][:64])
        y = (torch.relu(z) * t64(c["sc"]) + t64(c["sh"])).max(1)[0]           # max_k BasicConv([x_i, x_j - x_i])
        r = R.edge_fwd_ref(c)
        close64(r["y"], y.numpy(), c["name"])
        assert (np.abs(r["z"]) <= r["Bz"]).mean() <= R.UNDECIDED_CAP, c["name"]
    for key in R.pd_cases():
        c = R.pd_case(key, False)
        x = t64(c["x"])
        sq = (x * x).sum(-1, keepdim=True)
        close64(R.pd_ref(c)[0], (sq + -2 * (x @ x.transpose(2, 1)) + sq.transpose(2, 1)).numpy(), c["name"])      # the expansion


# ================================================================================================ CPU: preconditions
def test_exact_inputs_are_exact():
    """assert_exact for every EXACT case (gemm_case / bwd_case assert it when they are built)"""
    for shape in R.GEMM_SHAPES:
        R.gemm_case(shape, True)
        R.bwd_case(shape, True)
    for i in range(len(R.SA_CASES)):
        R.assert_exact(1.0, *R.sa_ref(R.sa_case(i, True))["mags"])
    for key in R.group_cases():
        c = R.group_case(key, True)
        R.assert_exact(2.0 ** -6, np.abs(c["xyz"]).max() + np.abs(c["new_xyz"]))
        if c["D"]:
            R.assert_exact(1.0, R.group_rows_bwd_ref(c)["mag"])
    for key in R.interp_cases():
        c = R.interp_case(key, True)
        R.assert_exact(0.25, R.interp_fwd_ref(c)[2], R.interp_bwd_ref(c)["mag"])
    for key in R.mr_cases():
        R.assert_exact(1.0, R.mr_bwd_ref(R.mr_case(key, True))["mag"])
    for key in R.edge_cases():
        r = R.edge_fwd_ref(R.edge_case(key, True))
        R.assert_exact(2.0 ** -3, (r["mag"][:, :64].max() + r["mag"][:, 64:].max()) * 2 + 2)
    for key in R.pd_cases():
        R.assert_exact(1.0, R.pd_ref(R.pd_case(key, True))[2])


def test_exact_inputs_hit_zero_preactivations_and_ties():
    zero = [float((R.layer_ref(R.gemm_case(s, True), R.VARIANTS[2])["z"] == 0).mean()) for s in R.SMALL_SHAPES[1:]]
    assert min(zero) > 0.1 and max(zero) < 0.4, zero                         # "about a fifth"
    for i in range(len(R.SA_CASES)):
        c = R.sa_case(i, True)
        r = R.sa_ref(c)
        if c["zero_g"] is not None:
            assert not r["out"][c["zero_g"]].any() and not r["arg"][c["zero_g"]].any()
            assert not r["drows"][c["zero_g"] * c["K"]:(c["zero_g"] + 1) * c["K"]].any()
        if c["same_g"] is not None:
            assert not r["arg"][c["same_g"]].any()
    assert any(R.group_rows_bwd_ref(R.group_case(k, True))["untouched"].any() for k in R.group_cases() if k[5])


@pytest.mark.parametrize("shape", R.GEMM_SHAPES, ids=shape_id)
def test_undecided_relu_decisions_stay_under_the_cap(shape):
    c = R.gemm_case(shape, False)
    for v in R.VARIANTS[2:]:
        und = R.layer_ref(c, v)["und"]
        print("UNDECIDED %s %s %d of %d" % (c["name"], v[0], int(und.sum()), und.size))
        assert und.mean() <= R.UNDECIDED_CAP, (c["name"], v[0], und.mean())


# ================================================================================================ CPU: teeth
def fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def layer_fails(c, v, mutant):
    M = c["shape"][2]
    rm = R.layer_ref(c, v, mutant)
    got, gm = R.layer_out(rm, c["exact"], M // 32 if mutant == "mask_stride" else None)
    return fails(R.check_layer, c["name"], R.layer_ref(c, v), got, gm if v[4] else None, c["exact"])


TEETH_SHAPES = R.SMALL_SHAPES + ((2051, 64, 1029),)


@pytest.mark.parametrize("mutant", ["drop_k", "nbr_bias", "ge", "affine_first", "mask_stride", "reorder"])
def test_wrong_layer_fails_the_forward_check(mutant, capsys):
    hit = 0
    for exact in EXACT_REAL:
        for shape in TEETH_SHAPES:
            rows, K, M = shape
            c = R.gemm_case(shape, exact)
            for v in R.VARIANTS:
                applies = {"drop_k": rows > 1, "nbr_bias": v[1] and M > 1, "ge": exact and v[4] and rows > 1, "affine_first": v[3] and rows > 1,
                           "mask_stride": v[4] and M % 32 != 0 and rows > 1, "reorder": rows > 64}[mutant]
                r = R.layer_ref(c, v)
                o, m = R.layer_out(r, exact)
                assert not fails(R.check_layer, c["name"], r, o, m if v[4] else None, exact)       # the reference itself passes
                if applies:
                    assert layer_fails(c, v, mutant), (mutant, c["name"], v[0])
                    hit += 1
    assert hit


@pytest.mark.parametrize("mutant", ["drop_k", "mask_stride"])
def test_wrong_layer_fails_the_backward_check(mutant):
    for exact in EXACT_REAL:
        for shape in TEETH_SHAPES:
            rows, K, M = shape
            if rows == 1 or (mutant == "mask_stride" and K % 32 == 0):
                continue
            c = R.bwd_case(shape, exact)
            assert fails(R.check_bwd, c["name"], R.bwd_ref(c, True), R.bwd_ref(c, True, mutant)["y"].astype(F), exact), (mutant, c["name"])
    for M in R.RELU_BITS_M:
        for exact in EXACT_REAL:
            c = R.relu_bits_case(M, exact)
            assert (M % 32 == 0) or (bits_differ(R.relu_bits_ref(c, True, "mask_stride"), R.relu_bits_ref(c, True)))


def bits_differ(a, b):
    return bool((R.bits(a) != R.bits(b)).any())


def check_sum(name, r, got, exact):
    """an accumulated or gathered sum: the bytes of the float64 result on EXACT inputs, the (n + 1) u bound on REAL ones"""
    if exact:
        assert_bits(got, r["y"].astype(F), name)
    else:
        check_bound(name, got, r["y"], r["bound"])


@pytest.mark.parametrize("mutant", ["ge", "last_max"])
def test_wrong_sa_stack_breaks_byte_equality(mutant):
    hit = 0
    for i in range(len(R.SA_CASES)):
        c = R.sa_case(i, True)
        r, m = R.sa_ref(c), R.sa_ref(c, mutant)
        if mutant == "ge":
            hit += any((a != b).any() for a, b in zip(r["masks"], m["masks"]))
        elif c["K"] > 1:
            assert (r["arg"] != m["arg"]).any(), c["name"]
            hit += 1
    assert hit >= 3


@pytest.mark.parametrize("mutant", ["feat_first", "assign"])
def test_wrong_grouping_fails(mutant):
    for exact in EXACT_REAL:
        for key in R.group_cases():
            c = R.group_case(key, exact)
            if not c["D"]:
                continue
            r = R.group_rows_bwd_ref(c)
            if mutant == "feat_first":
                assert bits_differ(R.group_rows_ref(c, mutant), R.group_rows_ref(c)), c["name"]
                assert fails(check_sum, c["name"], r, R.group_rows_bwd_ref(c, mutant)["y"].astype(F), exact), c["name"]
            elif c["mode"] == "hub" and c["S"] * c["K"] > 1:
                assert fails(check_sum, c["name"], r, R.group_rows_bwd_ref(c, mutant)["y"].astype(F), exact), c["name"]


@pytest.mark.parametrize("mutant", ["col0", "assign"])
def test_wrong_interpolation_transpose_fails(mutant):
    for exact in EXACT_REAL:
        for key in R.interp_cases():
            c = R.interp_case(key, exact)
            if (mutant == "col0" and not c["D1"]) or (mutant == "assign" and c["N"] == 1):
                continue
            assert fails(check_sum, c["name"], R.interp_bwd_ref(c), R.interp_bwd_ref(c, mutant)["y"].astype(F), exact), (mutant, c["name"])


@pytest.mark.parametrize("mutant", ["last_max", "no_self", "assign"])
def test_wrong_mrconv_fails(mutant):
    for exact in EXACT_REAL:
        for key in R.mr_cases():
            c = R.mr_case(key, exact)
            if mutant == "last_max":
                if exact:                                                     # integer features: ties in every case
                    assert (R.mr_fwd_ref(c, mutant)[1] != R.mr_fwd_ref(c)[1]).any(), c["name"]
            else:
                assert fails(check_sum, c["name"], R.mr_bwd_ref(c), R.mr_bwd_ref(c, mutant)["y"].astype(F), exact), (mutant, c["name"])


@pytest.mark.parametrize("mutant", ["ge", "last_max", "affine_first"])
def test_wrong_edgeconv_fails(mutant):
    for exact in EXACT_REAL:
        for key in R.edge_cases():
            c = R.edge_case(key, exact)
            r, m = R.edge_fwd_ref(c), R.edge_fwd_ref(c, mutant)
            assert not fails(R.check_edge, c["name"], c, r, r["y"].astype(F), r["arg"])
            if exact or mutant == "affine_first":
                assert fails(R.check_edge, c["name"], c, r, m["y"].astype(F), m["arg"]), (mutant, c["name"])


def check_pd(name, c, got):
    ref, bound, _ = R.pd_ref(c)
    if c["exact"]:
        assert_bits(got, ref.astype(F), name)
        assert_bits(got, np.ascontiguousarray(got.transpose(0, 2, 1)), name + ": symmetry")
        assert_bits(np.einsum("bii->bi", got), np.zeros((c["B"], c["N"]), F), name + ": diagonal")
    else:
        check_bound(name, got, ref, bound)


def test_distance_without_a_norm_fails():
    for exact in EXACT_REAL:
        for key in R.pd_cases():
            c = R.pd_case(key, exact)
            assert not fails(check_pd, c["name"], c, R.pd_ref(c)[0].astype(F))
            assert fails(check_pd, c["name"], c, R.pd_ref(c, "no_norm")[0].astype(F)), c["name"]


# ================================================================================================ host refusals (no launch)
def test_host_refusals():
    """each is PSG_ERR_ARG (rc = -1) from the argument checks: nothing is launched, the pointers are never followed"""
    from pointsecguard_amd import _lib
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    arr = (ctypes.c_void_p * 9)(*([ctypes.addressof(buf)] * 9))
    widths = (ctypes.c_int * 9)(*([5] * 9))

    def refused(name, *args):
        with pytest.raises(_lib.PsgError, match=r"rc=-1"):
            _lib.call(name, *args)

    refused("psg_pw_mlp_fwd", p, 4, 4, 4, p, p, 0, 4, p, 4, None, p, p, None)                  # a scale without the ReLU
    refused("psg_global_max", p, 1, 4, 96, p, p, p, None)                                      # C no multiple of 64
    for G, K, n in ((4, 256, 1), (4, 16, 9), (4, 0, 1), (1 << 24, 255, 1), (0, 16, 1)):
        refused("psg_sa_mlp_max_fwd", p, G, K, 3, n, widths, arr, arr, p, p, arr, p, p, None)
        refused("psg_sa_mlp_max_bwd", p, p, G, K, 3, n, widths, arr, arr, p, p, p, None)


# ================================================================================================ GPU
gpu = pytest.mark.gpu


def lib():
    from pointsecguard_amd import _lib, runtime
    return _lib, runtime.ptr, runtime.stream


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def nanf(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def padded(a, pad):
    """rows of a with `pad` more columns that hold NaN: the kernels must not read them"""
    t = nanf(a.shape[0], a.shape[1] + pad)
    t[:, :a.shape[1]] = dev(a)
    return t


def is_canary(a):
    return bool(np.isnan(a).all())


def twice(run, skip=()):
    """two runs of one case from fresh buffers (the second with the other mask canary): bit-equal except the atomically
    accumulated REAL sums named in `skip`"""
    a, b = run(0), run(1)
    for k in a:
        if k not in skip and a[k] is not None:
            assert_bits(a[k], b[k], "second run, " + k)
    return a


def run_layer(c, v, stride, second):
    _lib, P, st = lib()
    _, bias, relu, affine, with_mask = v
    rows, K, M = c["shape"]
    xin, out = padded(c["x"], stride[0]), nanf(rows, M + stride[1])
    w, b, sc, sh = dev(c["w"]), dev(c["b"]), dev(c["sc"]), dev(c["sh"])
    mk = torch.full((rows, R.words(M)), 0 if second else -1, dtype=torch.int32, device="cuda") if with_mask else None
    _lib.call("psg_pw_mlp_fwd", P(xin), K + stride[0], rows, K, P(w), P(b) if bias else None, int(relu), M, P(out), M + stride[1], P(mk),
              P(sc) if affine else None, P(sh) if affine else None, st())
    o = host(out)
    assert stride[1] == 0 or is_canary(o[:, M:]), c["name"] + ": columns >= M of a padded row were written"
    return dict(out=np.ascontiguousarray(o[:, :M]), mask=host(mk).view(np.uint32) if with_mask else None)


def layer_test(shape, exact, combos):
    c = R.gemm_case(shape, exact)
    for v, stride in combos:
        got = twice(lambda second: run_layer(c, v, stride, second))
        R.check_layer("%s %s ld+%d/+%d" % (c["name"], v[0], stride[0], stride[1]), R.layer_ref(c, v), got["out"], got["mask"], exact)


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
@pytest.mark.parametrize("shape", R.SMALL_SHAPES, ids=shape_id)
def test_pw_mlp_fwd_small_tiles(shape, exact):
    """64 x 64 tiles, one per wave: every epilogue under every stride pair"""
    layer_test(shape, exact, [(v, s) for v in R.VARIANTS for s in R.STRIDES])


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
@pytest.mark.parametrize("shape", R.LARGE_SHAPES, ids=shape_id)
def test_pw_mlp_fwd_large_tiles(shape, exact):
    """128 x 128 tiles (>= 128 of them): every epilogue and every stride pair once, rotated against each other so that the
    masked epilogues meet both the float4 path (strides that are multiples of 4) and the general one"""
    k = R.LARGE_SHAPES.index(shape)
    layer_test(shape, exact, [(v, R.STRIDES[(i + k) % 6]) for i, v in enumerate(R.VARIANTS)] +
               [(R.VARIANTS[5], R.STRIDES[0]), (R.VARIANTS[5], R.STRIDES[2]), (R.VARIANTS[3], R.STRIDES[5])])


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
@pytest.mark.parametrize("shape", R.GEMM_SHAPES, ids=shape_id)
def test_pw_mlp_bwd(shape, exact):
    """the transposed shapes: the product runs over M, the mask rows of the layer below have ceil(K / 32) words"""
    _lib, P, st = lib()
    rows, K, M = shape
    c = R.bwd_case(shape, exact)
    table = R.pack_bits(c["below"]).view(np.int32)
    for with_mask in (True, False):
        for pi, po in ((0, 0), (1, 3), (4, 0), (0, 4)):
            def run(second):
                g, out = padded(c["g"], pi), nanf(rows, K + po)
                wT, mk = dev(c["wT"]), dev(table)
                _lib.call("psg_pw_mlp_bwd", P(g), M + pi, rows, M, P(wT), P(mk) if with_mask else None, K, P(out), K + po, st())
                o = host(out)
                assert po == 0 or is_canary(o[:, K:]), c["name"] + ": columns >= K of a padded row were written"
                return dict(din=np.ascontiguousarray(o[:, :K]))
            R.check_bwd("%s mask=%d ld+%d/+%d" % (c["name"], with_mask, pi, po), R.bwd_ref(c, with_mask), twice(run)["din"], exact)


@gpu
def test_apply_relu_bits():
    _lib, P, st = lib()
    for M in R.RELU_BITS_M:
        for exact in EXACT_REAL:
            c = R.relu_bits_case(M, exact)
            for with_scale in (True, False):
                for pad in (0, 3):
                    def run(second):
                        g = nanf(c["rows"], M + pad)
                        g[:, :M] = dev(c["g"])
                        tb, sc = dev(R.pack_bits(c["bit"]).view(np.int32)), dev(c["sc"])
                        _lib.call("psg_apply_relu_bits", P(g), M + pad, P(tb), P(sc) if with_scale else None, c["rows"], M, st())
                        o = host(g)
                        assert pad == 0 or is_canary(o[:, M:]), c["name"]
                        return dict(g=np.ascontiguousarray(o[:, :M]))
                    assert_bits(twice(run)["g"], R.relu_bits_ref(c, with_scale), "%s scale=%d ld+%d" % (c["name"], with_scale, pad))


def ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
@pytest.mark.parametrize("i", range(len(R.SA_CASES)))
def test_sa_mlp_max(i, exact):
    """the stack against float64 (EXACT) and, on all inputs, against the same layers run one at a time through
    psg_pw_mlp_fwd / _bwd with a numpy max between them: the ping-pong, scratch and mask plumbing"""
    _lib, P, st = lib()
    c = R.sa_case(i, exact)
    n, rows, K, G, widths = len(c["widths"]), c["rows"], c["K"], c["G"], c["widths"]
    wmax, clast = max(widths), widths[-1]
    cw = (ctypes.c_int * n)(*widths)
    w, b, wT = [dev(a) for a in c["w"]], [dev(a) for a in c["b"]], [dev(a.T) for a in c["w"]]

    def run(second, with_masks=True):
        x, dout = dev(c["x"]), dev(c["dout"])
        sa, sb = nanf(rows, wmax), nanf(rows, wmax)
        masks = [torch.full((rows, R.words(wd)), 0 if second else -1, dtype=torch.int32, device="cuda") for wd in widths]
        out, arg = nanf(G, clast), torch.full((G, clast), 0xFF, dtype=torch.uint8, device="cuda")
        _lib.call("psg_sa_mlp_max_fwd", P(x), G, K, c["cin"], n, cw, ptr_array(w), ptr_array(b), P(sa), P(sb),
                  ptr_array(masks) if with_masks else None, P(out), P(arg), st())
        last = host(sb if (n - 1) & 1 else sa).reshape(-1)[:rows * clast].reshape(rows, clast).copy()
        res = dict(out=host(out), arg=host(arg), last=last)
        if with_masks:
            res.update({"mask%d" % l: host(m).view(np.uint32) for l, m in enumerate(masks)})
            drows = nanf(rows, c["cin"])
            _lib.call("psg_sa_mlp_max_bwd", P(dout), P(arg), G, K, c["cin"], n, cw, ptr_array(wT), ptr_array(masks), P(sa), P(sb), P(drows), st())
            res["drows"] = host(drows)
        return res
    got = twice(run)
    bare = run(0, with_masks=False)                                           # masks = NULL is accepted in the forward
    assert_bits(bare["out"], got["out"], c["name"] + ": out without masks")
    assert_bits(bare["arg"], got["arg"], c["name"] + ": arg without masks")
    # arg names the first sample that attains the maximum of the kernel's own last-layer output
    lk = got["last"].reshape(G, K, clast)
    assert_bits(got["arg"], np.argmax(lk, 1).astype(np.uint8), c["name"] + ": arg")
    assert_bits(got["out"], lk.max(1), c["name"] + ": out")
    if c["same_g"] is not None:
        assert not got["arg"][c["same_g"]].any(), c["name"] + ": K identical rows"
    # the same layers one at a time
    h, ld = dev(c["x"]), c["cin"]
    for l, wd in enumerate(widths):
        o, mk = nanf(rows, wd), torch.full((rows, R.words(wd)), -1, dtype=torch.int32, device="cuda")
        _lib.call("psg_pw_mlp_fwd", P(h), ld, rows, ld, P(w[l]), P(b[l]), 1, wd, P(o), wd, P(mk), None, None, st())
        assert_bits(got["mask%d" % l], host(mk).view(np.uint32), c["name"] + ": mask of layer %d" % l)
        h, ld = o, wd
    assert_bits(got["last"], host(h), c["name"] + ": last layer")
    last_bit = R.unpack_bits(got["mask%d" % (n - 1)], clast).reshape(G, K, clast)
    g0 = np.where((np.arange(K)[None, :, None] == got["arg"][:, None, :]) & last_bit, c["dout"][:, None, :], F(0.0)).astype(F)
    g = dev(g0.reshape(rows, clast))
    for l in range(n - 1, -1, -1):
        c_in = widths[l - 1] if l else c["cin"]
        o = nanf(rows, c_in)
        _lib.call("psg_pw_mlp_bwd", P(g), widths[l], rows, widths[l], P(wT[l]), P(dev(got["mask%d" % (l - 1)].view(np.int32))) if l else None,
                  c_in, P(o), c_in, st())
        g = o
    assert_bits(got["drows"], host(g), c["name"] + ": drows")
    if exact:
        r = R.sa_ref(c)
        assert_bits(got["out"], r["out"].astype(F), c["name"] + ": out against float64")
        assert_bits(got["arg"], r["arg"], c["name"] + ": arg against float64")
        for l in range(n):
            assert_bits(got["mask%d" % l], R.pack_bits(r["masks"][l]), c["name"] + ": mask %d against float64" % l)
        assert_bits(got["drows"], r["drows"].astype(F), c["name"] + ": drows against float64")
        if c["zero_g"] is not None:
            z = c["zero_g"]
            assert not got["out"][z].any() and not got["arg"][z].any() and not R.bits(got["drows"][z * K:(z + 1) * K]).any(), c["name"]


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
def test_group_rows(exact):
    _lib, P, st = lib()
    for key in R.group_cases():
        c = R.group_case(key, exact)
        B, N, S, K, Dn, ff = c["B"], c["N"], c["S"], c["K"], c["D"], c["ff"]

        def run(second):
            xyz, feat, nx, gi, dr = dev(c["xyz"]), dev(c["feat"]) if Dn else None, dev(c["new_xyz"]), dev(c["gidx"]), dev(c["drows"])
            rows = nanf(B * S * K, Dn + 3)
            _lib.call("psg_group_rows", P(xyz), P(feat), P(nx), P(gi), B, N, S, K, Dn, ff, P(rows), st())
            res = dict(rows=host(rows))
            if Dn:
                df = nanf(B, N, Dn)                                           # a missing zero-fill shows
                _lib.call("psg_group_rows_bwd", P(dr), P(gi), B, N, S, K, Dn, ff, P(df), st())
                res["dfeat"] = host(df)
            return res
        got = twice(run, skip=() if exact else ("dfeat",))
        assert_bits(got["rows"], R.group_rows_ref(c), c["name"])               # one subtraction or one copy: bytes on all inputs
        if Dn:
            r = R.group_rows_bwd_ref(c)
            check_sum(c["name"] + " bwd", r, got["dfeat"], exact)
            assert not R.bits(got["dfeat"][r["untouched"]]).any(), c["name"] + ": a point no group names is not +0"


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
def test_three_interp(exact):
    _lib, P, st = lib()
    for key in R.interp_cases():
        c = R.interp_case(key, exact)
        B, N, S, D1, D2 = c["B"], c["N"], c["S"], c["D1"], c["D2"]

        def run(second):
            f2, f1, idx, w, dout = dev(c["f2"]), dev(c["f1"]) if D1 else None, dev(c["idx"]), dev(c["w"]), dev(c["dout"])
            out, d2 = nanf(B, N, D1 + D2), nanf(B, S, D2)
            _lib.call("psg_three_interp_fwd", P(f2), P(idx), P(w), P(f1), B, N, S, D1, D2, P(out), st())
            _lib.call("psg_three_interp_bwd", P(dout), c["ld"], D1, P(idx), P(w), B, N, S, D2, P(d2), st())
            return dict(out=host(out), dfeat2=host(d2))
        got = twice(run, skip=() if exact else ("dfeat2",))
        ref, bound, _ = R.interp_fwd_ref(c)
        assert_bits(got["out"], R.interp_fwd_ref(c, F)[0], c["name"] + ": the float32 order ((w0 f0 + w1 f1) + w2 f2)")
        check_bound(c["name"] + " fwd", got["out"], ref, bound)
        check_sum(c["name"] + " bwd", R.interp_bwd_ref(c), got["dfeat2"], exact)


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
def test_mrconv_gather(exact):
    _lib, P, st = lib()
    for key in R.mr_cases():
        c = R.mr_case(key, exact)
        Rr, N, C, pad = c["R"], c["N"], c["C"], 3

        def run(second):
            x, nbr, dcat, arg_in = padded(c["x"], pad), dev(c["nbr"]), dev(c["dcat"]), dev(c["arg"])
            cat, arg = nanf(Rr, 2 * C), torch.full((Rr, C), 0xFF, dtype=torch.uint8, device="cuda")
            dx = nanf(Rr, C + pad)                                            # the contract is "fully written"
            _lib.call("psg_mrconv_gather_fwd", P(x), C + pad, Rr, N, C, P(nbr), P(cat), P(arg), st())
            _lib.call("psg_mrconv_gather_bwd", P(dcat), Rr, N, C, P(nbr), P(arg_in), P(dx), C + pad, st())
            o = host(dx)
            assert is_canary(o[:, C:]), c["name"] + ": columns >= C of dx were written"
            return dict(cat=host(cat), arg=host(arg), dx=np.ascontiguousarray(o[:, :C]))
        got = twice(run, skip=() if exact else ("dx",))
        cat, arg = R.mr_fwd_ref(c)
        assert_bits(got["cat"], cat, c["name"] + " cat")
        assert_bits(got["arg"], arg, c["name"] + " arg")
        check_sum(c["name"] + " bwd", R.mr_bwd_ref(c), got["dx"], exact)


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
def test_edgeconv_fwd(exact):
    _lib, P, st = lib()
    for key in R.edge_cases():
        c = R.edge_case(key, exact)
        Rr, N, C = c["R"], c["N"], c["C"]

        def run(second):
            x, nbr = padded(c["x"], 3), dev(c["nbr"])
            wcat, bcat, sc, sh = dev(c["wcat"]), dev(c["bcat"]), dev(c["sc"]), dev(c["sh"])
            pq, out, arg = nanf(Rr, 128), nanf(Rr, 68), torch.full((Rr, 64), 0x7F, dtype=torch.uint8, device="cuda")
            _lib.call("psg_edgeconv_fwd", P(x), C + 3, Rr, N, C, P(nbr), P(wcat), P(bcat), P(sc), P(sh), P(pq), P(out), 68, P(arg), st())
            o = host(out)
            assert is_canary(o[:, 64:]), c["name"] + ": columns >= 64 of out were written"
            return dict(pq=host(pq), out=np.ascontiguousarray(o[:, :64]), arg=host(arg))
        got = twice(run)
        r = R.edge_fwd_ref(c)
        if exact:
            assert_bits(got["pq"], r["pq"].astype(F), c["name"] + " [P | Q]")
        else:
            check_bound(c["name"] + " [P | Q]", got["pq"], r["pq"], r["Bpq"])
        R.check_edge(c["name"], c, r, got["out"], got["arg"])


@gpu
@pytest.mark.parametrize("exact", EXACT_REAL, ids=CLS)
def test_pairwise_distance(exact):
    _lib, P, st = lib()
    for key in R.pd_cases():
        c = R.pd_case(key, exact)
        B, N, C = c["B"], c["N"], c["C"]

        def run(second):
            x, sq, out = dev(c["x"]), nanf(B * N), nanf(B, N, N)
            _lib.call("psg_gcn_pairwise_distance", P(x), B, N, C, P(sq), P(out), st())
            return dict(out=host(out))
        check_pd(c["name"], c, twice(run)["out"])
