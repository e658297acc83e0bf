"""RandLA-Net, stage by stage: every kernel of csrc/psg_randla_net.hip against the float64 statement of ITS OWN operation
(tests/randla_ref64.py) on ITS OWN inputs, read through the workspace tap psg_rla_debug_ptr.  Because every stage is fed
what the GPU produced, and the transposes take the GPU's decisions (arg bytes, sign bits) as inputs, a last-bit flip
cannot move an entry downstream, and every bound below is asserted on EVERY entry - no share of entries, no slack factor.
What this pins: each kernel computes the operation oracle/randla_net.py states.  The network as a whole stays PARITY
UNPINNED against the TensorFlow-1 reference, which cannot run here (tests/test_randla_net.py keeps the end-to-end bars).

u = 2^-24.  "linear(K)": |got - ref64| <= (K + 2) u (|x| |w|^T + |b| + |pre-add|) + u |ref64|, any summation order;
"+ lrelu": the same bound (leaky ReLU is 1-Lipschitz) + u |out| for the product with the slope; "exact": bit-equal;
"softmax": the first-order bound of randla_ref64._attention (expf taken as one ulp) scaled by 4 x the largest error / bound
MEASURED on the MI355X over this file's shapes and the four switches - no ulp figure is documented for the device's expf and
sqrtf: 0.120 for the poolings (SOFTMAX_RATIO 0.48), 0.044 for their transposes (SOFTMAX_T_RATIO 0.176); "dist": 4 u |dist|
(three roundings under the root, the root taken as one ulp) scaled likewise, measured 0.558 (DIST_RATIO 2.232).  The figures, where
each was reached and the margin stand beside the constants in randla_ref64.py.  d = 16, 64, 128, 256, 512 and h = d / 2 by level; d_in = 8, 32, 128, 256, 512.

  forward stage                      K            bound
  fc0 -> f0, m_f0                    6            linear + lrelu
  mlp1 -> fpc, m_fpc                 d_in         linear + lrelu
  relpos                             -            columns 1..9 exact; column 0 (distance) dist
  LFAmlp1 -> fxyz1, LFAmlp2 -> fxyz2 10, h        linear + lrelu
  att_pooling_1 -> agg1, _2 -> agg2  d (scores), 16 (sum)   softmax
  att1_mlp -> fagg1, att2_mlp -> fagg2   d        linear + lrelu
  shortcut -> sc                     d_in         linear
  mlp2 + sc -> enc, m_enc            d            linear (pre-add) + lrelu
  max-pool -> samp, arg              -            exact; arg = lowest k
  decoder_0 -> dec0                  1024         linear + lrelu
  up-sample + concat -> dec_cat[j]   -            exact
  Decoder_layer_j -> dec_out[j]      1536, 768, 384, 160, 64    linear + lrelu
  fc1, fc2, fc                       32, 64, 32   linear + lrelu, linear + lrelu, linear
  sign bits: bit == (ref64 pre-activation > 0) wherever |pre-activation| > its bound; inside the bound at most 1e-4 of the
  stage's entries may differ.  The float32 emulation of the network (randla_ref64.walk_forward, dtype float32) against the
  float64 stages differs inside the bound on 0 of 2 818 048 sign bits at 8192 points and on 0 of 2 994 176 at 8704 (seen on the CPU,
  test_float32_emulation_passes_every_stage), and RandLAOracle(float32), an independent float32 evaluation, on 0 of 8 847 360
  and 0 of 9 400 320 (test_float32_oracle_sign_bits_stay_under_the_cap), so the cap leaves the margin the issue reckons with.

  gradient buffer                    contributors, in host order                                              bound
  d_fc2o, d_fc1o, d_dec_out[4]       fc^T (K 13), fc2^T (32), fc1^T (64), then the sign bits                  linear + slope
  d_dec_out[j-1], d_dec0             Decoder_layer_j^T (K = its cout; lives in scratch) summed over up == t   linear + sum(cnt)
  d_samp[i]                          decoder skip part + shortcut^T(d_enc[i+1]) + mlp1^T(d_fpc[i+1])         3 linear, accumulated
  d_samp[4]                          decoder_0^T (1024)                                                       linear
  d_enc[i]                           [level 0: decoder skip part +] max-pool^T(d_samp[i], arg), then m_enc    sum(cnt) + slope
  g_fagg2, g_agg2, g_agg1            mlp2^T (2d) then m_fagg2; att2_mlp^T (d); att1_mlp^T (h)                 linear
  d_fagg1, d_fpc                     attentive pooling^T: softmax, direct term, score layer's feature half,
                                     sum over in-edges (d + cnt + 4 roundings per product), then the mask     softmax
  d_f0                               shortcut^T(d_enc[0]) + mlp1^T(d_fpc[0]), then m_f0                      2 linear + slope
  dfeatures                          fc0^T (8)                                                                linear
  inverse lists: exactly argsort(kind="stable") of neigh / up / the sampled edges.

The per-edge attention buffers (a1, cat1, a2, cat2) hold T and S2 on the split path, scores and the concatenation on the
unfused one and nothing on the fused one: they are not tapped; every path is checked through agg1 / agg2 / d_fagg1 / d_fpc,
whose meaning does not depend on the path.  tests/test_gpu_alt_paths.py runs this file under the four RandLA switches."""
import numpy as np
import pytest

from oracle import randla, randla_net
from pointsecguard_amd.synthetic import randla_params
import randla_ref64 as R

SHAPES = {"n8192": (8192, 1), "n8704": (8704, 1), "b2x8192": (8192, 2)}


def make_cloud(n, batch, seed):
    """random clouds as in test_randla_net.py; the second cloud of a batch carries 256 duplicated points (same position, same
    colour) in its first 512 rows, which survive to level 2: their enc rows are equal, so the max-pool meets exact ties"""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((batch, n, 3), dtype=np.float32) * np.array([4, 3, 3], np.float32)).astype(np.float32)
    rgb = rng.random((batch, n, 3), dtype=np.float32)
    if batch > 1:
        xyz[1, 256:512] = xyz[1, :256]
        rgb[1, 256:512] = rgb[1, :256]
    labels = rng.integers(0, 13, batch * n)
    return xyz.reshape(-1, 3), rgb.reshape(-1, 3), labels


# ------------------------------------------------------------------------------------------------ CPU: the reference itself
def knn_tree(support, query, k):
    """oracle.randla.knn_brute's result on clouds without equidistant neighbours (random float32 points), from a k-d tree:
    the brute-force distance matrix of an 8704-point cloud takes 10 s"""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return randla.knn_brute(support, query, k)
    return np.stack([cKDTree(s.astype(np.float64)).query(q.astype(np.float64), k)[1].reshape(len(q), k) for s, q in zip(support, query)]).astype(np.int32)


@pytest.fixture(scope="module")
def cpu_case():
    """pyramids of one 8192- and one 8704-point cloud and the float32 emulation of the whole network on each"""
    out = {}
    P = R.fold_all(randla_params(3))
    for n in (8192, 8704):
        xyz, rgb, labels = make_cloud(n, 1, 12)
        pts, neigh, pools, ups = randla.pyramid(xyz[None], knn=knn_tree)
        geo = R.geometry(xyz, [a[0] for a in neigh], [u[0][:, 0] for u in ups])
        feats = np.concatenate([xyz, rgb], 1)
        fwd, _ = R.walk_forward(P, feats, geo, dt=np.float32)
        dl = R.colper_dlogits(fwd[("logits", 0)], labels)
        bwd, _ = R.walk_backward(P, fwd, dl, geo, dt=np.float32)
        out[n] = dict(xyz=xyz, rgb=rgb, labels=labels, geo=geo, feats=feats, fwd=fwd, bwd=bwd, dl=dl,
                      pyr=([p[0] for p in pts], [a[0] for a in neigh], [p[0] for p in pools], [u[0] for u in ups]))
    return P, out


def test_float64_stages_compose_to_the_oracle(cpu_case, monkeypatch):
    """the stage functions, composed in float64 with the exact (unrounded) fold and the oracle's slope (0.2, not the kernels'
    float32(0.2)), ARE RandLAOracle(float64): logits and colour gradient to 1e-12 of their maximum"""
    import torch
    monkeypatch.setattr(R, "SLOPE", 0.2)
    _, cases = cpu_case
    c = cases[8192]
    params = randla_params(3)
    P = R.fold_all(params, rounded=False)
    fwd, _ = R.walk_forward(P, c["feats"], c["geo"])
    o64 = randla_net.RandLAOracle(params, dtype=torch.float64)
    _, logits, g = randla_net.loss_and_grad(o64, c["xyz"], c["rgb"], c["labels"], c["pyr"])
    assert np.abs(fwd[("logits", 0)] - logits).max() <= 1e-12 * np.abs(logits).max()
    bwd, _ = R.walk_backward(P, fwd, R.colper_dlogits(fwd[("logits", 0)], c["labels"]), c["geo"])
    assert np.abs(bwd[("dfeatures", 0)][:, 3:] - g).max() <= 1e-12 * np.abs(g).max()


def test_transposes_are_adjoint():
    """<J v, u> = <v, J^T u> to 1e-12 for every transpose, on random vectors"""
    import torch
    rng = np.random.default_rng(5)
    n, h, n_sub = 60, 8, 15
    d = 2 * h
    nb = rng.integers(0, n, (n, 16))
    rel = lambda a, b: abs(a - b) <= 1e-12 * max(abs(a), abs(b))          # noqa: E731
    W = (rng.standard_normal((d, d)), None)
    # conv
    x, u = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    assert rel((R.conv(x, (W[0], None))[0] * u).sum(), (x * R.conv_T(u, W)[0]).sum())
    # attentive pooling: J v from torch's forward-mode derivative of the oracle's own statement
    f, fxyz, v, u = rng.standard_normal((n, h)), rng.standard_normal((n * 16, h)), rng.standard_normal((n, h)), rng.standard_normal((n, d))
    tn, tW, tx = torch.from_numpy(nb), torch.from_numpy(W[0]), torch.from_numpy(fxyz).reshape(n, 16, h)

    def pool(ft):
        cat = torch.cat([ft[tn], tx], -1)
        return (cat * torch.softmax(cat @ tW.T, 1)).sum(1)
    out, jv = torch.autograd.functional.jvp(pool, torch.from_numpy(f), torch.from_numpy(v))
    assert np.abs(out.numpy() - R.att_pool(f, fxyz, nb, W)[0]).max() <= 1e-12
    assert rel(float((jv.numpy() * u).sum()), float((v * R.att_pool_T(f, fxyz, nb, W, u)[0]).sum()))
    # max-pool with the decision as an input; up-sample + concat
    enc, us = rng.standard_normal((n, d)), rng.standard_normal((n_sub, d))
    nbp = nb[:n_sub]
    _, arg = R.max_pool(enc, nbp)
    jv = np.take_along_axis(enc[nbp], arg[:, None, :].astype(np.int64), 1)[:, 0]
    assert rel((jv * us).sum(), (enc * R.max_pool_T(us, arg, nbp, n)[0]).sum())
    up = rng.integers(0, n_sub, n)
    skip, coarse, uc = rng.standard_normal((n, 4)), rng.standard_normal((n_sub, 6)), rng.standard_normal((n, 10))
    lhs = (R.upsample_cat(skip, coarse, up) * uc).sum()
    assert rel(lhs, (skip * uc[:, :4]).sum() + (coarse * R.seg_sum(uc[:, 4:], None, up, n_sub)[0]).sum())
    bits = rng.random((n, d)) > 0.5
    assert rel((np.where(bits, x, R.SLOPE * x) * u).sum(), (x * R.lrelu_T(u, 0 * u, bits)[0]).sum())


@pytest.mark.parametrize("n", [8192, 8704])
def test_float32_emulation_passes_every_stage(cpu_case, n):
    """a float32 evaluation of the network (numpy, BLAS summation order) stays inside every derived bound on every entry,
    and its sign bits never differ from the float64 ones inside the bound on more than the cap (counts in the docstring)"""
    P, cases = cpu_case
    c = cases[n]
    _, rep = R.walk_forward(P, c["feats"], c["geo"], taps=c["fwd"])
    assert not rep.fail, rep.fail
    flips = sum(a for a, _ in rep.flips.values())
    print("sign bits inside the bound: %d of %d" % (flips, sum(b for _, b in rep.flips.values())))
    print("softmax stages: largest error / first-order bound %.3f" % rep.softmax_ratio())
    _, repb = R.walk_backward(P, c["fwd"], c["dl"], c["geo"], taps=c["bwd"])
    assert not repb.fail, repb.fail
    assert len(rep.stages) == 80 and len(rep.flips) == 29 and len(repb.stages) == 45


@pytest.mark.parametrize("n", [8192, 8704])
def test_float32_oracle_sign_bits_stay_under_the_cap(cpu_case, n):
    """the cap on sign bits that differ inside the bound, confirmed with an independent float32 evaluation: every
    activated layer of RandLAOracle(float32) (torch, BatchNorm applied unfolded) on the oracle's own float32 inputs against
    the float64 stage: ALL differing bits, inside the bound or not, stay under the cap at every stage (seen: 0 of 8 847 360
    bits at 8192 points, 0 of 9 400 320 at 8704, the per-edge layers included)"""
    import torch
    P, cases = cpu_case
    c = cases[n]
    o32 = randla_net.RandLAOracle(randla_params(3), dtype=torch.float32)
    calls, conv32 = [], o32.conv

    def spy(x, name, act=True):
        y = conv32(x, name, act)
        calls.append((name, x.detach().reshape(-1, x.shape[-1]).numpy(), y.detach().reshape(-1, y.shape[-1]).numpy(), act))
        return y
    o32.conv = spy
    randla_net.loss_and_grad(o32, c["xyz"], c["rgb"], c["labels"], c["pyr"])
    rep, pending = R.Report(), None
    for name, x, y, act in calls:
        if act:
            _, _, z, bz = R.conv(x, P[name], act=True)
            R.compare_mask(rep, name, y > 0, z, bz)
        elif name.endswith("mlp2"):
            pending = (name, x, y)
        elif name.endswith("shortcut"):                         # enc = leaky_relu(mlp2 + shortcut)
            _, _, z, bz = R.conv(pending[1], P[pending[0]], pre=y, act=True)
            R.compare_mask(rep, pending[0], pending[2] + y > 0, z, bz)
    assert len(rep.flips) == 39                                 # the 29 sign-bit words and the 10 per-edge layers, which keep none
    print("float32 oracle: sign bits that differ: %d of %d" % (sum(a for a, _ in rep.flips.values()), sum(b for _, b in rep.flips.values())))
    for k, (a, b) in rep.flips.items():
        assert a <= R.MASK_CAP * b, (k, a, b)


def failing(rep):
    return sorted({m.split(":")[0] for m in rep.fail})


def test_check_has_teeth(cpu_case):
    """the comparison fails, at the stage that is wrong and nowhere else, when a snapshot is wrong in one of the ways the
    end-to-end bars let through"""
    P, cases = cpu_case
    c = cases[8704]
    # one neighbour slot's attention weight off by 1 % (slot 11 of level 1's second pooling)
    wrong, _ = R.walk_forward(P, c["feats"], c["geo"], dt=np.float32, hook={("agg2", 1): {"perturb_slot": (11, 0.01)}})
    # (the whole wrong network's snapshot, as a GPU with that bug would show it: every later stage is consistent with it)
    _, rep = R.walk_forward(P, c["feats"], c["geo"], taps=wrong)
    assert failing(rep) == ["('agg2', 1)"], rep.fail
    # the last row of the 17-row stage (decoder_0 at 8704 points) not written
    snap = dict(c["fwd"])
    assert snap[("dec0", 0)].shape[0] == 17
    snap[("dec0", 0)] = snap[("dec0", 0)].copy()
    snap[("dec0", 0)][16] = 0.0
    _, rep = R.walk_forward(P, c["feats"], c["geo"], taps=snap)
    assert "('dec0', 0)" in failing(rep) and all("rows 16..16" in m for m in rep.fail if m.startswith("('dec0', 0)")), rep.fail
    # a mask from the neighbouring buffer: forward (m_fagg1 holds m_fpc's bits) and backward (d_fpc closed with m_fagg1)
    snap = dict(c["fwd"])
    snap[("m_fagg1", 2)] = snap[("m_fpc", 2)]
    _, rep = R.walk_forward(P, c["feats"], c["geo"], taps=snap)
    assert failing(rep) == ["('m_fagg1', 2)"], rep.fail
    wrong, _ = R.walk_backward(P, c["fwd"], c["dl"], c["geo"], dt=np.float32, hook={("d_fpc", 2): ("m_fagg1", 2)})
    _, rep = R.walk_backward(P, c["fwd"], c["dl"], c["geo"], taps=wrong)
    assert failing(rep) == ["('d_fpc', 2)"], rep.fail


def test_debug_tap_refuses_a_null_workspace():
    from pointsecguard_amd import _lib
    lib = _lib.load()
    assert not lib.psg_rla_debug_ptr(None, 0, 0, None, None)
    assert b"psg_rla_debug_ptr" in lib.psg_last_error()


# ------------------------------------------------------------------------------------------------ GPU
FWD_NET = ["f0", "dec0", "fc1o", "fc2o", "logits"]
FWD_DEC = ["dec_cat", "dec_out"]
FWD_LEVEL = ["fpc", "agg1", "fagg1", "agg2", "fagg2", "sc", "enc", "samp", "arg", "relpos", "fxyz1", "fxyz2"]
BWD_NET = ["d_fc2o", "d_fc1o", "d_dec0", "d_f0"]
BWD_LEVEL = ["d_samp", "d_enc", "d_fagg1", "d_fpc", "g_fagg2", "g_agg2", "g_agg1"]


def snapshot(ws, net, dec, level, masks):
    import torch
    t = {}
    for k in net:
        t[(k, 0)] = ws.debug(k)
    for k in dec:
        for j in range(5):
            t[(k, j)] = ws.debug(k, j)
    for k in level:
        for i in range(5):
            t[(k, i)] = ws.debug(k, i)
    for k, lv, M in masks:
        t[(k, lv)] = ws.debug(k, lv)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    for k, lv, M in masks:
        out[(k, lv)] = R.unpack_bits(out[(k, lv)].view(np.uint32), M)
    return out


def mask_list():
    m = [("m_f0", 0, 8), ("m_dec0", 0, 1024), ("m_fc1", 0, 64), ("m_fc2", 0, 32)]
    m += [("m_dec", j, c) for j, c in enumerate((512, 256, 128, 32, 32))]
    for i, d in enumerate(R.D_OUT):
        m += [("m_fpc", i, d // 2), ("m_fagg1", i, d // 2), ("m_fagg2", i, d), ("m_enc", i, 2 * d)]
    return m


@pytest.fixture(scope="module")
def runs():
    """shape name -> its run (made once per module, on first use)"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = gpu_run(name)
        return cache[name]
    return get


def gpu_run(name):
    """one forward and one backward on the GPU, every tap copied back (the forward state BEFORE the backward recycles
    it), every stage checked once; the tests below read the reports"""
    import torch
    from pointsecguard_amd.randla import network
    n, batch = SHAPES[name]
    xyz, rgb, labels = make_cloud(n, batch, 12)
    params = randla_params(3)
    P = R.fold_all(params)
    model, ws = network.RandLAModel(params), network.RandLAWorkspace(n, batch=batch)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    ws.set_cloud(dev(xyz))
    geo = R.geometry(xyz, [ws.index(0, l).cpu().numpy() for l in range(5)], [ws.index(1, l).cpu().numpy() for l in range(5)], batch)
    feats = np.concatenate([xyz, rgb], 1)
    logits = ws.forward(model, dev(feats))
    fwd = snapshot(ws, FWD_NET, FWD_DEC, FWD_LEVEL, mask_list())
    assert np.array_equal(fwd[("logits", 0)], logits.cpu().numpy())
    _, dl = network.colper_grad(logits, dev(labels.astype(np.int32)))
    dfeat = ws.backward(model, dl)
    bwd = snapshot(ws, BWD_NET, ["d_dec_out"], BWD_LEVEL, [])
    bwd[("dfeatures", 0)] = dfeat.cpu().numpy()
    dl = dl.cpu().numpy()
    assert np.array_equal(dl, R.colper_dlogits(fwd[("logits", 0)], labels).astype(np.float32))
    _, rep_f = R.walk_forward(P, feats, geo, taps=fwd)
    _, rep_b = R.walk_backward(P, fwd, dl, geo, taps=bwd)
    for rep in (rep_f, rep_b):
        for k in sorted(rep.ratio, key=str):
            print("%-20s error / bound %.3f" % (k, rep.ratio[k]))
    print("softmax stages: largest error / first-order bound %.3f (forward) %.3f (backward)" % (rep_f.softmax_ratio(), rep_b.softmax_ratio()))
    print("relpos distance: largest error / (4 u |dist|) %.3f" % rep_f.dist_ratio())
    print("sign bits inside the bound: %d" % sum(a for a, _ in rep_f.flips.values()))
    return dict(name=name, ws=ws, model=model, geo=geo, fwd=fwd, bwd=bwd, rep_f=rep_f, rep_b=rep_b, batch=batch, n=n)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_forward_stages(runs, shape):
    """every forward stage of the docstring's table, on every entry, and every sign bit"""
    run = runs(shape)
    rep = run["rep_f"]
    assert not rep.fail, "\n".join(rep.fail)
    assert len(rep.stages) == 80 and len(rep.flips) == 29


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_backward_stages(runs, shape):
    """every gradient buffer of the docstring's table, on every entry"""
    run = runs(shape)
    rep = run["rep_b"]
    assert not rep.fail, "\n".join(rep.fail)
    assert len(rep.stages) == 45


@pytest.mark.gpu
def test_gpu_max_pool_ties_and_clouds(runs):
    """the batch's second cloud has duplicated points: exact ties occur in the max-pool and arg is the lowest k (checked entry
    by entry in the forward stages; here: that the case really occurred), and its rows index its own cloud"""
    run = runs("b2x8192")
    n, geo, fwd = run["n"], run["geo"], run["fwd"]
    ties = 0
    for i in range(3):
        g = fwd[("enc", i)][geo["neigh"][i][geo["pool"][i]]]
        ties += int(((g == g.max(1, keepdims=True)).sum(1) > 1).sum())
        lo = len(geo["neigh"][i]) // 2
        assert geo["neigh"][i][lo:].min() >= lo and geo["neigh"][i][:lo].max() < lo
        assert geo["up"][i][lo:].min() >= len(geo["pool"][i]) // 2
    assert ties > 0
    assert not [m for m in run["rep_f"].fail if m.startswith(("('samp'", "('arg'"))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_inverse_lists(runs, shape):
    """inv / invu / invp are the exact transposes of neigh, up and the sampled edges, ascending within each row"""
    run = runs(shape)
    ws, geo = run["ws"], run["geo"]
    rep = R.Report()
    for i in range(5):
        nb, n_sub = geo["neigh"][i], len(geo["pool"][i])
        get = lambda k: ws.debug(k, i).cpu().numpy()           # noqa: E731
        R.check_inverse(rep, "inv%d" % i, nb, len(nb), get("inv_off"), get("inv_ent"))
        R.check_inverse(rep, "invu%d" % i, geo["up"][i], n_sub, get("invu_off"), get("invu_ent"))
        R.check_inverse(rep, "invp%d" % i, nb[geo["pool"][i]], len(nb), get("invp_off"), get("invp_ent"))
    assert not rep.fail, "\n".join(rep.fail)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_debug_tap_refuses_unknown_buffers(runs, shape):
    run = runs(shape)
    from pointsecguard_amd import _lib
    ws = run["ws"]
    lib = _lib.load()
    for what, level in ((99, 0), (7, 0), (10, 5), (10, -1), (0, 1), (42, 5)):
        assert not lib.psg_rla_debug_ptr(ws.handle, what, level, None, None)
        assert b"psg_rla_debug_ptr" in lib.psg_last_error()
    assert tuple(ws.debug("dec_cat", 0).shape) == (run["n"] * run["batch"] // 256, 1536)
