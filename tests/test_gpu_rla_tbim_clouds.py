"""GPU tests of the lockstep RandLA-Net TBIM / tar_NBattack (psg_rla_bim_step_clouds, psg_rla_tbim_latch_clouds,
psg_rla_tbim_retire_clouds, psg_rla_tbim_window, TBIM.batch_attack_clouds).

The step kernels, which need no workspace, run alone at G = 3 with N in {1, 63, 832, 1000} (less than a wave, ragged tails, more
than one workgroup); everything that needs the network at G = 3 with N = 8192 or 8704 = 17 * 512, the smallest shapes a
workspace accepts.  No run exceeds 20 iterations."""
import ctypes

import numpy as np
import pytest

import rla_tbim_ref as R
from pointsecguard_amd.synthetic import randla_params

pytestmark = pytest.mark.gpu
G = 3
SMALL = [1, 63, 832, 1000]
PARTS = 32


def dev(a, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dt is not None:
        t = t.to(dt)
    return t.cuda().contiguous()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def P(t):
    from pointsecguard_amd import runtime
    return runtime.ptr(t)


KEEP = []


@pytest.fixture(autouse=True)
def _drop_uploads():
    yield
    KEEP.clear()


def D(a):
    """Upload and pass by pointer; the tensor is kept until the test ends (a temporary's block would be handed to the next
    upload before the kernel has read it)."""
    t = dev(a)
    KEEP.append(t)
    return P(t)


def call(name, *args):
    from pointsecguard_amd import _lib, runtime
    _lib.call(name, *args, runtime.stream())


# ---------------------------------------------------------------------------------------------- 1. the update
EPS, ALPHA = 0.05, 0.01


def step_case(n):
    """Cloud 0: at the clean colours, a random gradient (l_2: |delta| = alpha < eps, scale 1).  Cloud 1: an all-zero gradient
    (the 1e-12 floor) half an eps away (scale 1).  Cloud 2: two eps away (clipped)."""
    rng = np.random.default_rng(n)
    ori = (0.2 + 0.5 * rng.random((G, n, 3))).astype(np.float32)
    feat = rng.random((G, n, 6)).astype(np.float32)
    feat[:, :, 3:6] = ori
    feat[1, :, 3:6] += np.float32(0.5 * EPS / np.sqrt(3 * n))
    feat[2, :, 3:6] += np.float32(2.0 * EPS / np.sqrt(3 * n))
    dfeat = rng.standard_normal((G, n, 6)).astype(np.float32)
    dfeat[1] = 0.0
    return feat, dfeat, ori


def step_one_cloud(feat, dfeat, ori, n, l2):
    """psg_rla_bim_step on every cloud alone -> (feat, norms [2][G], delta) per cloud"""
    out = []
    for g in range(G):
        f, norms, delta = dev(feat[g]), dev(np.full(2, -5.0, np.float32)), dev(np.full((n, 3), -5.0, np.float32))
        call("psg_rla_bim_step", P(f), D(dfeat[g]), D(ori[g]), n, EPS, ALPHA, l2, P(norms), P(delta))
        out.append((host(f), host(norms), host(delta)))
    return out


def step_clouds(feat, dfeat, ori, running, n, l2):
    f, norms, delta = dev(feat), dev(np.full((2, G), -5.0, np.float32)), dev(np.full((G, n, 3), -5.0, np.float32))
    call("psg_rla_bim_step_clouds", P(f), D(dfeat), D(ori), None if running is None else D(running), G, n, EPS, ALPHA, l2, P(norms),
         P(delta))
    return host(f), host(norms), host(delta)


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("n", SMALL)
def test_step_clouds_equals_the_one_cloud_step(n, l2):
    """psg_rla_bim_step_clouds against psg_rla_bim_step cloud by cloud (bit for bit), and for l_2 both against the float64
    formula.  That bound is per element and counted, one rounding u = 2^-24 of the float64 result per float32 operation
    (rla_tbim_ref.bim_step64 carries them along): the norms 1 each (double sums rounded once; |delta|^2 also what the deltas
    bring), gn 1.5 of its own, delta 4 (difference, quotient, product, sum) + gn's, scale 1.5 + 1 where clipped, the colour 2
    (product, sum) + delta's + scale's."""
    feat, dfeat, ori = step_case(n)
    want = step_one_cloud(feat, dfeat, ori, n, l2)
    got_f, got_norms, got_delta = step_clouds(feat, dfeat, ori, None, n, l2)
    for g in range(G):
        assert same(got_f[g], want[g][0]), g
        assert same(got_f[g][:, :3], feat[g][:, :3])                  # xyz is not touched
        if l2:
            assert same(got_norms[:, g], want[g][1]) and same(got_delta[g], want[g][2]), g
    assert not same(got_f, feat)
    if l2:
        # the regimes the case was made for, from the device's own norms
        gn, dn = np.sqrt(got_norms[0].astype(np.float64)), np.sqrt(got_norms[1].astype(np.float64))
        print("n", n, "|g|", gn, "|delta| / eps", dn / EPS)
        assert gn[1] == 0.0 and gn[0] > 0.0 and dn[0] < EPS and dn[1] < EPS and dn[2] > EPS
        d64 = np.sqrt(((got_f[2][:, 3:6].astype(np.float64) - ori[2]) ** 2).sum())
        assert abs(d64 - EPS) <= 1e-5 * EPS + 3 * n * 2.0 ** -24          # clipped onto the eps sphere (float32 colours)
        # both entry points launch one kernel set now, so the yardstick is the float64 step with its counted bound
        # (rla_tbim_ref.bim_step64); the mutant - cloud g normalised by cloud (g + 1) % G's norms - must leave it somewhere
        ref, bound = R.bim_step64(feat, dfeat, ori, EPS, ALPHA)
        one = [np.stack([w[k] for w in want]) for k in range(3)]
        for tag, (f, norms, delta) in (("clouds", (got_f, got_norms, got_delta)), ("one cloud", (one[0], one[1].T, one[2]))):
            for name, got, k in (("feat", f[:, :, 3:6], 0), ("norms", norms, 1), ("delta", delta, 2)):
                err = np.abs(got.astype(np.float64) - ref[k])
                print("n", n, tag, name, "largest error / bound", float((err / np.maximum(bound[k], 1e-300)).max()))
                assert (err <= bound[k]).all(), (tag, name)
            mutant = R.bim_step64(feat, dfeat, ori, EPS, ALPHA, norms=np.roll(ref[1], -1, axis=1))[0][0]
            assert (np.abs(mutant - f[:, :, 3:6]) > bound[0]).any(), tag
    else:
        assert linf_matches_numpy(got_f, feat, dfeat, ori)
    # two runs: the same bits
    again = step_clouds(feat, dfeat, ori, None, n, l2)
    assert same(again[0], got_f) and same(again[1], got_norms) and same(again[2], got_delta)
    # cloud 1 not running, NaN in its gradient: none of its bytes is written; clouds 0 and 2: the same bits as before
    poisoned = dfeat.copy()
    poisoned[1] = np.nan
    f_c, norms_c, delta_c = step_clouds(feat, poisoned, ori, np.array([1, 0, 1], np.uint8), n, l2)
    assert same(f_c[1], feat[1]) and same(f_c[[0, 2]], got_f[[0, 2]])
    if l2:
        assert (norms_c[:, 1] == -5.0).all() and (delta_c[1] == -5.0).all()
        assert same(norms_c[:, [0, 2]], got_norms[:, [0, 2]]) and same(delta_c[[0, 2]], got_delta[[0, 2]])
    else:
        assert (norms_c == -5.0).all() and (delta_c == -5.0).all()     # l_inf uses neither


def linf_matches_numpy(got_f, feat, dfeat, ori):
    """l_inf in float32 numpy: clip(adv + alpha sign(g), x - eps, x + eps), then [0, 1] - every operation is one rounding
    (alpha * sign is exact, so a fused multiply-add gives the same bits)."""
    f32 = np.float32
    v = feat[:, :, 3:6] + f32(ALPHA) * np.sign(dfeat[:, :, 3:6]).astype(f32)
    v = np.minimum(np.maximum(v, ori - f32(EPS)), ori + f32(EPS))
    return same(got_f[:, :, 3:6], np.minimum(np.maximum(v, f32(0)), f32(1)).astype(f32))


# ---------------------------------------------------------------------------------------------- 2. latch and retire
class DevLatch:
    def __init__(self, n):
        import torch
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
        self.n = n
        self.pred, self.out_pred = z(G, n, dt=torch.int32), z(G, n, dt=torch.int32)
        self.out_adv, self.out_stats = z(G, n, 3), z(G, 3)
        self.active = torch.ones(G, dtype=torch.uint8, device="cuda")
        self.leaving = z(G, dt=torch.uint8)
        self.exit = torch.full((G,), -1, dtype=torch.int32, device="cuda")
        self.scratch = z(G, 2 * PARTS + 1, dt=torch.int32)

    def latch(self, hist_row, logits, labels, hit_ys, mask, n_mask, num, den, it, final):
        row = dev(hist_row)
        call("psg_rla_tbim_latch_clouds", D(logits), D(labels), D(hit_ys), D(mask), D(n_mask), G, self.n, num, den, it, final, P(row),
             P(self.pred), P(self.out_pred), P(self.out_stats), P(self.active), P(self.leaving), P(self.exit), P(self.scratch))
        hist_row[...] = host(row)

    def retire(self, feat, final):
        call("psg_rla_tbim_retire_clouds", D(feat), G, self.n, final, P(self.out_adv), P(self.active), P(self.leaving))

    def state(self):
        return {"active": host(self.active), "leaving": host(self.leaving), "exit_step": host(self.exit), "out_adv": host(self.out_adv),
                "out_pred": host(self.out_pred), "out_stats": host(self.out_stats), "pred": host(self.pred)}


def assert_state_equal(d, ref, tag):
    got = d.state()
    for k, v in ref.items():
        assert same(got[k], v), (tag, k)


@pytest.mark.parametrize("n", SMALL)
def test_latch_and_retire_vs_numpy_with_ties_and_freeze(n):
    """Logits from {0, 1, 2}: ties everywhere, the first maximum counts.  Iteration 0 with a threshold everything passes (never
    exits), two exit rounds with a threshold that some clouds pass, then poisoned inputs with final = 1: retired clouds keep
    their bytes, the others are snapshot without an exit step unless the test fires."""
    rng = np.random.default_rng(n)
    labels = rng.integers(0, 13, (G, n)).astype(np.int32)
    mask = (rng.random((G, n)) < 0.5).astype(np.uint8)
    mask[:, 0] = 1
    hit_ys = np.where(mask.astype(bool), 1, labels).astype(np.int32)
    n_mask = mask.sum(1).astype(np.int32)
    d, ref = DevLatch(n), R.new_state(G, n)
    # first maximum == class 1 with probability (1 / 3)(2 / 3) = 2 / 9: over the rounds some clouds fire and some do not
    for i, (it, num, den, final, poison) in enumerate([(0, 0, 1, 0, 0), (1, 2, 9, 0, 0), (2, 2, 9, 0, 0), (3, 1, 1, 1, 1)]):
        logits = rng.integers(0, 3, (G, n, 13)).astype(np.float32) + (100.0 * poison)
        if i == 0:
            logits[:, :, 1] = 5.0                    # every masked point hits: only `it >= 1` keeps the clouds in
        feat = rng.random((G, n, 6), dtype=np.float32) + poison
        row_d, row_r = np.full((G, 3), -1.0, np.float32), np.full((G, 3), -1.0, np.float32)
        d.latch(row_d, logits, labels, hit_ys, mask, n_mask, num, den, it, final)
        R.latch(ref, row_r, logits, labels, hit_ys, mask, n_mask, num, den, it, final)
        assert same(row_d, row_r), i
        assert_state_equal(d, ref, (i, "latch"))
        if i == 0:
            assert (row_r[:, 1] == n_mask).all() and (ref["exit_step"] == -1).all() and not ref["leaving"].any()
        d.retire(feat, final)
        R.retire(ref, feat, final)
        assert_state_equal(d, ref, (i, "retire"))
    print("n", n, "exit steps", ref["exit_step"])
    assert not ref["active"].any()


def test_latch_on_the_threshold():
    """40 masked points: 35, 36 and 37 hits are one below, ON and one above 9/10."""
    n = 832
    labels = np.tile((np.arange(n) % 13).astype(np.int32), (G, 1))
    mask = np.zeros((G, n), np.uint8)
    mask[:, ::21][:, :40] = 1
    assert (mask.sum(1) == 40).all()
    hit_ys = np.where(mask.astype(bool), (labels + 5) % 13, labels).astype(np.int32)
    pred = labels.copy()
    for g, k in enumerate((35, 36, 37)):
        idx = np.flatnonzero(mask[g])[:k]
        pred[g, idx] = hit_ys[g, idx]
    logits = np.zeros((G, n, 13), np.float32)
    np.put_along_axis(logits, pred[..., None].astype(np.int64), 1.0, -1)
    n_mask = mask.sum(1).astype(np.int32)
    feat = np.random.default_rng(1).random((G, n, 6), dtype=np.float32)
    for it, want in ((0, [-1, -1, -1]), (1, [-1, -1, 1])):
        d, ref = DevLatch(n), R.new_state(G, n)
        row_d, row_r = np.zeros((G, 3), np.float32), np.zeros((G, 3), np.float32)
        d.latch(row_d, logits, labels, hit_ys, mask, n_mask, 9, 10, it, 0)
        R.latch(ref, row_r, logits, labels, hit_ys, mask, n_mask, 9, 10, it, 0)
        assert same(row_d, row_r) and row_d[:, 1].tolist() == [35, 36, 37] and row_d[:, 2].tolist() == [0, 0, 0]
        assert_state_equal(d, ref, it)
        assert ref["exit_step"].tolist() == want and ref["active"].tolist() == [1, 1, 1]      # the latch does not retire
        d.retire(feat, 0)
        R.retire(ref, feat, 0)
        assert_state_equal(d, ref, (it, "retire"))
        assert ref["active"].tolist() == [1, 1, 0 if it else 1]


# ---------------------------------------------------------------------------------------------- network fixtures
def make_clouds(n, seed):
    """G clouds on one set of coordinates with their own colours and labels."""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((n, 3), dtype=np.float32) * np.array([4, 3, 3], np.float32)).astype(np.float32)
    rgb = rng.random((G, n, 3), dtype=np.float32)
    labels = rng.integers(0, 13, (G, n))
    return xyz, rgb, labels


@pytest.fixture(scope="module")
def model():
    from pointsecguard_amd.randla import network
    return network.RandLAModel(randla_params(3))


@pytest.fixture(scope="module")
def ws8704():
    from pointsecguard_amd.randla import network
    return network.RandLAWorkspace(8704, batch=G)


@pytest.fixture(scope="module")
def ws8192():
    from pointsecguard_amd.randla import network
    return network.RandLAWorkspace(8192, batch=G)


class Bufs:
    """The buffers of psg_rla_tbim_window_args for G clouds of n points."""

    def __init__(self, n, xyz, rgb, labels, goal, ori=3, target=9, eps=EPS, alpha=ALPHA):
        import torch
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
        self.n, self.eps, self.alpha = n, eps, alpha
        mask = labels == ori
        hit = np.where(mask, target, labels)
        self.sign = -1.0 if goal == "t" else 1.0
        self.feat0 = dev(np.concatenate([np.broadcast_to(xyz, (G, n, 3)), rgb], -1).reshape(G * n, 6))
        self.ori = dev(rgb.reshape(G * n, 3))
        self.labels, self.hit_ys = dev(labels.reshape(-1).astype(np.int32)), dev(hit.reshape(-1).astype(np.int32))
        self.loss_ys = dev((hit if goal == "t" else labels).reshape(-1).astype(np.int32))
        self.mask = dev(mask.reshape(-1).astype(np.uint8))
        self.n_mask = dev(mask.reshape(G, n).sum(1).astype(np.int32))
        self.feat, self.dfeat = z(G * n, 6), z(G * n, 6)
        self.logits, self.dlogits = z(G * n, 13), z(G * n, 13)
        self.norms, self.delta = z(2, G), z(G * n, 3)
        self.pred, self.out_pred = z(G * n, dt=torch.int32), z(G * n, dt=torch.int32)
        self.scratch = z(G, 2 * PARTS + 1, dt=torch.int32)
        self.hist = z(16, G, 3)
        self.out_adv, self.out_stats = z(G * n, 3), z(G, 3)
        self.active, self.leaving, self.exit = z(G, dt=torch.uint8), z(G, dt=torch.uint8), z(G, dt=torch.int32)
        self.reset()

    RESULT = ("feat", "hist", "out_adv", "out_pred", "out_stats", "active", "leaving", "exit", "pred", "norms", "delta")

    def reset(self):
        self.feat.copy_(self.feat0)
        for t in (self.hist, self.out_adv, self.out_pred, self.out_stats, self.pred, self.norms, self.delta, self.leaving):
            t.zero_()
        self.active.fill_(1)
        self.exit.fill_(-1)

    def result(self):
        return {k: host(getattr(self, k)).copy() for k in self.RESULT}

    def args(self, model, ws, num, den, l2, it0, n_steps, final, over=()):
        from pointsecguard_amd import _lib
        a = _lib.RlaTbimWindowArgs()
        a.model, a.ws = model.handle, ws.handle
        a.n_steps, a.G, a.N, a.it0, a.num, a.den, a.final, a.l2_metric = n_steps, G, self.n, it0, num, den, final, l2
        a.eps, a.alpha, a.sign = self.eps, self.alpha, self.sign
        for k in ("ori", "mask", "n_mask", "labels", "hit_ys", "loss_ys", "feat", "logits", "dlogits", "dfeat", "norms", "delta", "pred",
                  "scratch", "hist", "out_adv", "out_pred", "out_stats", "active", "leaving"):
            setattr(a, k, getattr(self, k).data_ptr())
        a.exit_step = self.exit.data_ptr()
        for k, v in dict(over).items():
            setattr(a, k, v)
        return a

    def hand(self, model, ws, num, den, l2, it0, n_steps, final):
        """The window's sequence through the step entry points, with a read-back between them."""
        import torch
        for i in range(n_steps):
            fin = 1 if final and i == n_steps - 1 else 0
            call("psg_rla_forward", model.handle, ws.handle, P(self.feat), P(self.logits))
            call("psg_rla_tbim_latch_clouds", P(self.logits), P(self.labels), P(self.hit_ys), P(self.mask), P(self.n_mask), G, self.n, num,
                 den, it0 + i, fin, P(self.hist[i]), P(self.pred), P(self.out_pred), P(self.out_stats), P(self.active), P(self.leaving),
                 P(self.exit), P(self.scratch))
            host(self.exit)
            call("psg_rla_colper_grad_masked", P(self.logits), P(self.loss_ys), P(self.mask), self.sign, G * self.n, P(self.dlogits), None)
            call("psg_rla_backward", model.handle, ws.handle, P(self.dlogits), P(self.dfeat))
            torch.cuda.synchronize()
            call("psg_rla_bim_step_clouds", P(self.feat), P(self.dfeat), P(self.ori), P(self.active), G, self.n, self.eps, self.alpha, l2,
                 P(self.norms), P(self.delta))
            float(self.feat[0, 3])
            call("psg_rla_tbim_retire_clouds", P(self.feat), G, self.n, fin, P(self.out_adv), P(self.active), P(self.leaving))
            host(self.active)


def set_cloud(ws, model, b):
    """Geometry of the batch and the first forward of (cloud, model), which computes the xyz branch outside any capture."""
    ws.set_cloud(b.feat0[:, 0:3].contiguous())
    return ws.forward(model, b.feat0)


# ---------------------------------------------------------------------------------------------- 3. windows == steps
def clean_pred(model, feats):
    """The clean prediction [G, n] of G clouds, on a workspace of its own."""
    from pointsecguard_amd.randla import network
    n = feats.shape[1]
    ws = network.RandLAWorkspace(n, batch=G)
    f = dev(feats.reshape(-1, 6).astype(np.float32))
    ws.set_cloud(f[:, 0:3].contiguous())
    return host(ws.forward(model, f).argmax(1)).reshape(G, n).astype(np.int64)


def window_case(model, n, goal):
    """-> xyz, rgb, labels, ori, target, l2, eps, alpha, (num, den).
    't': labels = the clean prediction, origin = the class predicted most, target = the next, l_2 with steps large enough that
    the hits rise by tens of points per iteration, at a rate that depends on the cloud's colours.
    'ut': random labels (the hinge against the true labels is then on at the origin points), target = the class predicted most,
    l_inf.  The thresholds were read off recorded hit counts so that clouds leave inside the windows (asserted below; the kernels
    are bit-reproducible, so it holds in every run)."""
    if goal == "t":
        feats, rgb, labels, ori, target = predicted_setup(model, n, 44)
        return feats[0, :, :3], rgb, labels, ori, target, 1, 2.0, 0.4, WINDOW_THRESHOLD["t"]
    xyz, rgb, labels = make_clouds(n, 21)
    pred0 = clean_pred(model, np.concatenate([np.broadcast_to(xyz, (G, n, 3)), rgb], -1))
    target = int(np.bincount(pred0.reshape(-1), minlength=13).argmax())
    ori = 3 if target != 3 else 4
    return xyz, rgb, labels, ori, target, 0, EPS, ALPHA, WINDOW_THRESHOLD["ut"]


# recorded: 't' hits 0, 23, 39, 55, .. / 0, 11, 19, 24, 29, 34, 40 / 0, 11, 24, 41 of 6790 / 7829 / 6751 origin points (leave at
# 2, 6, 3); 'ut' hits 519, 522, .. / 464, .. 482 at most / 465, 470, 471, 478 of 677 / 629 / 612 (leave at 1, never, 3)
WINDOW_THRESHOLD = {"t": (1, 200), "ut": (77, 100)}


@pytest.mark.parametrize("n,goal", [(8704, "t"), (8192, "ut")])
def test_windows_equal_hand_driven_steps(model, ws8704, ws8192, n, goal):
    """A 1-step window, a 10-step window and a cut 3-step final window, each from the same start, against the same sequence
    through the step entry points on the same workspace: colours, history rows, snapshots, flags and exit steps bit-equal -
    without a graph handle, and with one (the iteration index then comes from the device row) eagerly, captured and replayed."""
    import torch
    from pointsecguard_amd import _lib, runtime
    ws = ws8704 if n == 8704 else ws8192
    xyz, rgb, labels, ori, target, l2, eps, alpha, (num, den) = window_case(model, n, goal)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = Bufs(n, xyz, rgb, labels, goal, ori, target, eps, alpha)
        set_cloud(ws, model, b)
        for it0, n_steps, final in ((0, 1, 0), (0, 10, 0), (10, 3, 1)):
            b.reset()
            b.hand(model, ws, num, den, l2, it0, n_steps, final)
            want = b.result()
            graph = ctypes.c_void_p()
            _lib.call("psg_nu_graph_create", ctypes.byref(graph))
            try:
                for rnd, gh in enumerate((None, graph, graph, graph, graph)):
                    b.reset()
                    a = b.args(model, ws, num, den, l2, it0, n_steps, final)
                    _lib.call("psg_rla_tbim_window", ctypes.byref(a), gh, runtime.stream())
                    got = b.result()
                    for k in Bufs.RESULT:
                        assert same(got[k], want[k]), (it0, n_steps, final, rnd, k)
                side.synchronize()
                stats = _lib.capture_stats(graph)
                print("goal", goal, "window", (it0, n_steps, final), "graph", stats, "exit", want["exit"], "n_mask", host(b.n_mask),
                      "hits per step", want["hist"][:n_steps, :, 1].T.tolist())
                assert stats["captures_tried"] == 1 and stats["captures_failed"] == 0 and stats["replays"] >= 2, stats
                assert not same(want["feat"], host(b.feat0))
                if n_steps == 10:                        # the premise: clouds leave inside the window, not all at one step
                    assert len(set(want["exit"].tolist())) >= 2 and (want["exit"] >= 1).any(), want["exit"]
                    assert same(want["active"], (want["exit"] < 0).astype(np.uint8))
                if final:
                    assert not want["active"].any() and want["out_adv"].any()
            finally:
                side.synchronize()
                _lib.call("psg_nu_graph_destroy", graph)


def test_window_refusals(model, ws8704, ws8192):
    """Every refusal is an error with a message, nothing is enqueued, and the stream still serves a good window afterwards."""
    import torch
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.randla import network
    n = 8704
    xyz, rgb, labels = make_clouds(n, 21)
    b = Bufs(n, xyz, rgb, labels, "t")
    set_cloud(ws8704, model, b)
    fresh = network.RandLAWorkspace(n, batch=G)           # no cloud set
    before = b.result()
    cases = [({"n_steps": 0}, ws8704, -1), ({"n_steps": 17}, ws8704, -1), ({"den": 0}, ws8704, -1), ({"den": -3}, ws8704, -1),
             ({"mask": None}, ws8704, -1), ({"n_mask": None}, ws8704, -1), ({}, ws8192, -1), ({"G": 2}, ws8704, -1),
             ({}, fresh, -3)]
    for over, ws, rc_want in cases:
        a = b.args(model, ws, 9, 10, 1, 0, 1, 0, over)
        rc = _lib.load().psg_rla_tbim_window(ctypes.byref(a), None, runtime.stream())
        msg = _lib.load().psg_last_error().decode()
        assert rc == rc_want and "psg_rla_tbim_window" in msg, (over, rc, msg)
        with pytest.raises(_lib.PsgError):
            _lib.call("psg_rla_tbim_window", ctypes.byref(a), None, runtime.stream())
    torch.cuda.synchronize()
    after = b.result()
    for k in Bufs.RESULT:
        assert same(before[k], after[k]), k
    a = b.args(model, ws8704, 9, 10, 1, 0, 1, 0)
    _lib.call("psg_rla_tbim_window", ctypes.byref(a), None, runtime.stream())
    torch.cuda.synchronize()
    assert not same(b.result()["feat"], before["feat"])


# ---------------------------------------------------------------------------------------------- 4. independence
def leaving_labels(pred0_g, ori, target):
    """Labels under which a cloud leaves at iteration 1: its origin points are those already predicted as the target plus a
    twentieth as many that are not (sr starts above 20 / 21 and the hinge has points to push, so the colours do move); every
    other point carries a label that is neither the prediction nor the origin class."""
    lab = (pred0_g + 1) % 13
    lab[lab == ori] = (ori + 2) % 13
    idx = np.flatnonzero(pred0_g == target)
    assert idx.size >= 20
    lab[idx] = ori
    lab[np.flatnonzero(pred0_g != target)[:idx.size // 20]] = ori
    return lab


def test_clouds_are_independent(model, ws8192):
    """Cloud 2 replaced by colours and labels that leave at iteration 1: the complete trajectories and results of clouds 0 and
    1 stay bit-identical."""
    from pointsecguard_amd import _lib, runtime
    n, steps = 8192, 5
    xyz, rgb, labels = make_clouds(n, 33)
    runs = []
    for replaced in (False, True):
        rgb_r, labels_r = rgb.copy(), labels.copy()
        target = 9
        if replaced:
            rgb_r[2] = np.random.default_rng(77).random((n, 3), dtype=np.float32)
            b = Bufs(n, xyz, rgb_r, labels_r, "t")
            pred0 = host(set_cloud(ws8192, model, b).argmax(1)).reshape(G, n)
            target = int(np.bincount(pred0[2], minlength=13).argmax())      # a class cloud 2 is predicted as
            labels_r[2] = leaving_labels(pred0[2], 3, target)
        b = Bufs(n, xyz, rgb_r, labels_r, "t", ori=3, target=9, eps=2.0, alpha=0.4)
        if replaced:                                      # (cloud 2 alone aims at its own target class)
            hit = host(b.hit_ys).reshape(G, n)
            hit[2] = np.where(labels_r[2] == 3, target, labels_r[2])
            b.hit_ys.copy_(dev(hit.reshape(-1)))
            b.loss_ys.copy_(b.hit_ys)
        set_cloud(ws8192, model, b)
        traj = []
        for it in range(steps):
            a = b.args(model, ws8192, 1, 2, 1, it, 1, 1 if it == steps - 1 else 0)
            _lib.call("psg_rla_tbim_window", ctypes.byref(a), None, runtime.stream())
            traj.append(b.result())
        runs.append(traj)
    assert runs[1][-1]["exit"][2] == 1
    keep = np.r_[0:2 * n]
    assert not same(runs[0][0]["feat"][keep], runs[0][-1]["feat"][keep])       # (clouds 0 and 1 do move)
    for t, (ra, rb) in enumerate(zip(*runs)):
        for k in ("feat", "out_adv", "out_pred", "pred", "delta"):
            assert same(ra[k][keep], rb[k][keep]), (t, k)
        for k in ("out_stats", "active", "leaving", "exit"):
            assert same(ra[k][:2], rb[k][:2]), (t, k)
        assert same(ra["hist"][:, :2], rb["hist"][:, :2]) and same(ra["norms"][:, :2], rb["norms"][:, :2]), t
    # the retired cloud stopped moving after iteration 1
    assert same(runs[1][1]["feat"][2 * n:], runs[1][-1]["feat"][2 * n:])


# ---------------------------------------------------------------------------------------------- 5. exits at different steps
def first_exit(num, den, counts, totals, cap):
    """Per cloud the first iteration 1..cap whose recorded hits pass the integer test, or -1."""
    out = []
    for g in range(counts.shape[1]):
        hit = [e for e in range(1, cap + 1) if R.fires_int(num, den, int(counts[e, g]), int(totals[g]))]
        out.append(hit[0] if hit else -1)
    return out


def predicted_setup(model, n, seed):
    """Clouds whose labels are the clean prediction; origin = the class every cloud is predicted as most, target = the next."""
    from pointsecguard_amd.randla import attack
    xyz, rgb, _ = make_clouds(n, seed)
    rgb[1] = 0.25 * rgb[1]                               # full range, dim, nearly grey: the hits rise at different rates
    rgb[2] = 0.45 + 0.1 * rgb[2]
    feats = np.concatenate([np.broadcast_to(xyz, (G, n, 3)), rgb], -1)
    S0 = attack._CloudsState(n, G)
    S0.ws.set_cloud(dev(feats.reshape(-1, 6)[:, :3]))
    labels = host(S0.ws.forward(model, dev(feats.reshape(-1, 6))).argmax(1)).reshape(G, n).astype(np.int64)
    del S0
    order = np.argsort(-np.array([min((labels[g] == c).sum() for g in range(G)) for c in range(13)]), kind="stable")
    ori, target = int(order[0]), int(order[1])
    assert all((labels[g] == ori).sum() > 0 for g in range(G))
    return feats, rgb, labels, ori, target


def test_exits_at_different_steps(model):
    """One run with exits disabled records every iteration (1-step windows): the history row, the prediction and the colours
    AFTER the iteration's update.  A threshold picked from the recorded hits makes the clouds leave at different iterations;
    the rerun in 10-step windows gives each cloud the recorded colours after the update of its exit iteration and the
    prediction before that update."""
    from pointsecguard_amd.randla import attack
    n, cap = 8192, 12
    feats, rgb, labels, ori, target = predicted_setup(model, n, 44)
    cls = attack.tar_NBattack(model, goal="t", distance_metric="l_2")
    cls.config(magnitude=2.0, alpha=0.4, iteration=cap)
    rec = {}

    def hook(it0, n_run, final, S, rows):
        assert n_run == 1
        rec[(it0, "row")] = rows[0].copy()
        rec[(it0, "adv")] = host(S.feat[:, 3:6]).reshape(G, n, 3).copy()
        rec[(it0, "pred")] = host(S.pred).reshape(G, n).copy()

    cls.EXIT_RATIO, cls.chunk, cls.window_hook = (1, 1), 1, hook          # n_hits > n_mask never holds
    cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
    assert (cls.last_steps == cap + 1).all() and len(rec) == 3 * (cap + 1)
    assert same(host(cls.last_adv), rec[(cap, "adv")])
    counts = np.stack([rec[(e, "row")][:, 1] for e in range(cap + 1)]).astype(np.int64)        # [cap + 1][G]
    totals = (labels == ori).sum(1)
    print("hits per iteration", counts.T.tolist(), "totals", totals.tolist())
    choice = None
    for e in range(1, cap + 1):                          # candidate thresholds: the recorded ratios themselves
        for g in range(G):
            num, den = int(counts[e, g]), int(totals[g])
            ex = first_exit(num, den, counts, totals, cap)
            if len(set(x for x in ex if x >= 0)) >= 2:
                choice = (num, den, ex)
                break
        if choice:
            break
    assert choice is not None, "premise: two distinct exit iterations"
    num, den, ex = choice
    print("threshold", num, "/", den, "exit iterations", ex)
    cls.EXIT_RATIO, cls.chunk, cls.window_hook = (num, den), attack.CHUNK, None
    outs = cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
    assert cls.last_steps.tolist() == [x + 1 if x >= 0 else cap + 1 for x in ex]
    S = cls._clouds[(n, G)]
    assert host(S.exit).tolist() == ex and not host(S.active).any()
    adv = host(cls.last_adv)
    for g in range(G):
        e = ex[g] if ex[g] >= 0 else cap
        assert same(adv[g], rec[(e, "adv")][g]), g
        assert same(host(S.out_pred).reshape(G, n)[g], rec[(e, "pred")][g]), g
        assert same(host(S.out_stats)[g], rec[(e, "row")][g]), g
        if e >= 1:
            assert not same(adv[g], rec[(e - 1, "adv")][g]), g           # the exiting iteration's update was applied
    assert len(outs) == G and all(np.isfinite(o).all() for o in outs)


# ---------------------------------------------------------------------------------------------- 6. the class
def mean_iou(pred, true):
    iou = []
    for c in sorted(set(pred.tolist()) | set(true.tolist())):        # (the reference's arithmetic: the union as a float32)
        inter = np.sum((pred == c) & (true == c))
        iou.append(inter / np.float32(np.sum(true == c) + np.sum(pred == c) - inter))
    return float(np.mean(iou))


@pytest.mark.parametrize("metric", ["l_2", "l_inf"])
@pytest.mark.parametrize("goal", ["t", "ut"])
def test_one_cloud_equals_batch_attack(model, goal, metric):
    """`batch_attack_clouds` on [1, N, 6] against `batch_attack` on the same cloud: last_adv and every tuple field, once with
    labels under which the loop leaves at iteration 1 and once with labels under which it runs to the cap."""
    from pointsecguard_amd.randla import attack, network
    n, cap, ori = 8192, 3, 3
    xyz, rgb, labels = make_clouds(n, 61)
    feats = np.concatenate([xyz, rgb[0]], -1)
    ws = network.RandLAWorkspace(n)
    ws.set_cloud(dev(xyz))
    pred0 = host(ws.forward(model, dev(feats)).argmax(1))
    del ws
    counts = np.bincount(pred0, minlength=13)
    target = int(counts.argmax())                        # "leaves": a class the cloud is predicted as
    rare = int(np.argsort(counts + (np.arange(13) == ori) * n, kind="stable")[0])      # "cap": the rarest class that is not ori
    one = attack.tar_NBattack(model, goal=goal, distance_metric=metric)
    lock = attack.tar_NBattack(model, goal=goal, distance_metric=metric)
    for cls in (one, lock):
        cls.config(magnitude=EPS if metric == "l_inf" else 1.0, alpha=ALPHA if metric == "l_inf" else 0.2, iteration=cap)
    for name, lab, want_steps in (("leaves", leaving_labels(pred0, ori, target), 2), ("cap", labels[0], cap + 1)):
        tgt = target if name == "leaves" else rare
        want = one.batch_attack(feats, lab, target=tgt, ori=ori)
        got = lock.batch_attack_clouds(feats[None], lab[None], target=tgt, ori=ori)
        print(goal, metric, name, "steps", lock.last_steps, "tuple", got[0])
        assert len(got) == 1 and got[0] == want, (name, got[0], want)
        assert got[0][4] > 0.0, name                      # the colours moved
        assert lock.last_adv.shape == (1, n, 3) and same(host(lock.last_adv)[0], host(one.last_adv)), name
        if goal == "t" or name == "cap":
            # (goal 'ut' ascends the hinge against the TRUE labels: the hits may fall below 9/10 only later or never)
            assert lock.last_steps.tolist() == [want_steps], name


def test_clouds_class_fields_and_refusals(model):
    import torch
    from pointsecguard_amd import _lib
    from pointsecguard_amd.randla import attack
    n, ori, target, cap = 8192, 3, 9, 19          # 20 iterations: a full window, and a full window that is the last
    xyz, rgb, labels = make_clouds(n, 56)
    feats = np.concatenate([np.broadcast_to(xyz, (G, n, 3)), rgb], -1)
    cls = attack.TBIM(model, goal="t", distance_metric="l_2")
    # refusals, before any device work: no state is built
    with pytest.raises(ValueError, match="config"):
        cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
    cls.config(magnitude=1.0, alpha=0.2, iteration=0)
    with pytest.raises(ValueError, match="iteration"):
        cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
    cls.config(iteration=cap)
    bad = labels.copy()
    bad[1][bad[1] == ori] = 0
    with pytest.raises(ValueError, match=r"cloud\(s\) 1"):
        cls.batch_attack_clouds(feats, bad, target=target, ori=ori)
    with pytest.raises(ValueError, match="features"):
        cls.batch_attack_clouds(feats[0], labels[0], target=target, ori=ori)
    with pytest.raises(ValueError, match="features"):
        cls.batch_attack_clouds(feats[:, :, :5], labels, target=target, ori=ori)
    with pytest.raises(ValueError, match="labels"):
        cls.batch_attack_clouds(feats, labels[:, :-1], target=target, ori=ori)
    with pytest.raises(ValueError, match="labels"):
        cls.batch_attack_clouds(feats, labels[:2], target=target, ori=ori)
    assert cls._clouds == {} and cls.last_adv is None

    class Log:
        lines = []

        def info(self, s):
            self.lines.append(s)

    cls.config(logger=Log())
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        results = []
        for _ in range(3):                               # the same shape three times: the full window eager, captured, replayed
            outs = cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
            results.append((outs, host(cls.last_adv).copy(), cls.last_steps.copy()))
        side.synchronize()
        S = cls._clouds[(n, G)]
        pred = host(S.out_pred).reshape(G, n)
        pred0 = host(S.ws.forward(model, dev(feats.reshape(-1, 6).astype(np.float32))).argmax(1)).reshape(G, n)
    outs, adv, steps = results[0]
    for o2, adv2, steps2 in results[1:]:
        assert o2 == outs and same(adv2, adv) and np.array_equal(steps2, steps)
    for handle in (S.graph, S.graph_tail):
        stats = _lib.capture_stats(handle)
        print("class graph", stats, "steps", steps, "tuples", outs)
        assert stats["captures_tried"] == 1 and stats["captures_failed"] == 0 and stats["replays"] >= 1, stats
    assert len(outs) == G and len(Log.lines) == 3 * G and Log.lines[0].startswith("points=")
    assert adv.shape == (G, n, 3) and adv.min() >= 0.0 and adv.max() <= 1.0 and steps.shape == (G,)
    for g in range(G):
        mk = labels[g] == ori
        tp = float(mk.sum())
        hit = np.where(mk, target, labels[g])
        # new_dists: the float32 norm of 3 n float32 differences against the same sum in double - each difference is one
        # rounding (2^-24 relative), the float32 reduction at most 3 n 2^-24 relative in the worst order
        dist = float(np.sqrt(((adv[g].astype(np.float64) - rgb[g]) ** 2).sum()))
        want = (tp, (pred[g][mk] == hit[mk]).sum() / tp, (pred[g][~mk] == hit[~mk]).sum() / (n - tp),
                (pred0[g][~mk] == labels[g][~mk]).sum() / (n - tp), dist, mean_iou(pred[g][~mk], labels[g][~mk]),
                mean_iou(pred0[g][~mk], labels[g][~mk]))
        assert len(outs[g]) == 7
        for k in (0, 1, 2, 3, 5, 6):
            assert outs[g][k] == want[k], (g, k)
        assert abs(outs[g][4] - dist) <= dist * (3 * n + 2) * 2.0 ** -24, g
        assert outs[g][4] > 0.0
