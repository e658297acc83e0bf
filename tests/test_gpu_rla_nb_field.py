"""GPU tests of the lockstep BIM family of RandLA-Net on the coordinate field:
psg_rla_bim_step_field_clouds, psg_rla_tbim_retire_field_clouds, psg_rla_bim_field_window, randla.nb_field's four classes.

The step and retire kernels, which need no workspace, run alone at G = 3 with N in {1, 63, 832, 1000} (less than a wave, ragged
tails, more than one workgroup); everything that needs the network at G = 3 with N = 8192 or 8704 = 17 * 512, the smallest
shapes a workspace accepts, cloud 1 carrying 256 duplicated points.  No run exceeds 13 iterations."""
import ctypes

import numpy as np
import pytest

import rla_coord_ref64 as C
import rla_nb_field_ref as F
from pointsecguard_amd.synthetic import randla_params
from test_gpu_rla_tbim_clouds import D, KEEP, P, _drop_uploads, call, dev, first_exit, host, leaving_labels, mean_iou, same  # noqa: F401

pytestmark = pytest.mark.gpu
G = 3
SMALL = [1, 63, 832, 1000]
PARTS = 32
PSG_ERR_ARG = -1                     # include/psg.h
COORD, BOTH = 1, 2                   # PSG_NU_FIELD_COORD / PSG_NU_FIELD_BOTH
EPS, ALPHA = 0.05, 0.01


# ---------------------------------------------------------------------------------------------- 1. the field step
def step_case(n):
    """Cloud 0: at the clean positions, random gradients (l_2: |delta| = alpha < eps, scale 1).  Cloud 1: all-zero gradients (the
    1e-12 floor) half an eps away (scale 1).  Cloud 2: two eps away (clipped)."""
    rng = np.random.default_rng(n)
    ori = (rng.random((G, n, 3)) * np.array([4, 3, 3])).astype(np.float32)
    feat = rng.random((G, n, 6)).astype(np.float32)
    feat[:, :, 0:3] = ori
    feat[1, :, 0:3] += np.float32(0.5 * EPS / np.sqrt(3 * n))
    feat[2, :, 0:3] += np.float32(2.0 * EPS / np.sqrt(3 * n))
    dfeat = rng.standard_normal((G, n, 6)).astype(np.float32)
    dxyz = rng.standard_normal((G, n, 3)).astype(np.float32)
    dfeat[1], dxyz[1] = 0.0, 0.0
    return feat, dfeat, dxyz, ori


def step_one_cloud(feat, dfeat, dxyz, ori, n, l2):
    """psg_rla_bim_step_field on every cloud alone -> (feat, norms [2], delta) per cloud"""
    out = []
    for g in range(G):
        f, norms, delta = dev(feat[g]), dev(np.full(2, -5.0, np.float32)), dev(np.full((n, 3), -5.0, np.float32))
        call("psg_rla_bim_step_field", P(f), D(dfeat[g]), D(dxyz[g]), D(ori[g]), n, EPS, ALPHA, l2, P(norms), P(delta))
        out.append((host(f), host(norms), host(delta)))
    return out


def step_clouds(feat, dfeat, dxyz, ori, running, n, l2, with_xyz=True):
    f, norms, delta = dev(feat), dev(np.full((2, G), -5.0, np.float32)), dev(np.full((G, n, 3), -5.0, np.float32))
    xyz = dev(np.full((G, n, 3), -5.0, np.float32))
    call("psg_rla_bim_step_field_clouds", P(f), D(dfeat), D(dxyz), D(ori), None if running is None else D(running), G, n, EPS, ALPHA, l2,
         P(norms), P(delta), P(xyz) if with_xyz else None)
    return host(f), host(norms), host(delta), host(xyz)


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("n", SMALL)
def test_step_clouds_equals_the_one_cloud_step(n, l2):
    """psg_rla_bim_step_field_clouds against psg_rla_bim_step_field cloud by cloud, bit for bit (one kernel set serves both, so
    the float32 numpy step - l_inf bit for bit - and, for l_2, rla_coord_ref64.field_step_l2_bound are the outside yardsticks)."""
    feat, dfeat, dxyz, ori = step_case(n)
    want = step_one_cloud(feat, dfeat, dxyz, ori, n, l2)
    got_f, got_norms, got_delta, got_xyz = step_clouds(feat, dfeat, dxyz, ori, None, n, l2)
    for g in range(G):
        assert same(got_f[g], want[g][0]), g
        assert same(got_f[g][:, 3:], feat[g][:, 3:])                   # the colours are not touched
        if l2:
            assert same(got_norms[:, g], want[g][1]) and same(got_delta[g], want[g][2]), g
    assert same(got_xyz, got_f[:, :, 0:3]) and not same(got_f, feat)
    grad = dfeat[:, :, 0:3] + dxyz
    if l2:
        gn, dn = np.sqrt(got_norms[0].astype(np.float64)), np.sqrt(got_norms[1].astype(np.float64))
        print("n", n, "|g|", gn, "|delta| / eps", dn / EPS)
        assert gn[1] == 0.0 and gn[0] > 0.0 and dn[0] < EPS and dn[1] < EPS and dn[2] > EPS
        for g in range(G):
            ref, bound = C.field_step_l2_bound(feat[g][:, 0:3], grad[g], ori[g], np.float64(np.float32(EPS)), np.float64(np.float32(ALPHA)))
            err = np.abs(got_f[g][:, 0:3].astype(np.float64) - ref)
            print("n", n, "cloud", g, "largest error / bound", float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), g
        # cloud g normalised with cloud 0's norms leaves that bound somewhere
        mutant, _ = F.field_step_l2_f32(feat[:, :, 0:3], grad, ori, EPS, ALPHA, shared_norms=True)
        ref2, bound2 = C.field_step_l2_bound(feat[2][:, 0:3], grad[2], ori[2], np.float64(np.float32(EPS)), np.float64(np.float32(ALPHA)))
        assert (np.abs(mutant[2].astype(np.float64) - ref2) > bound2).any()
    else:
        for g in range(G):
            assert same(got_f[g][:, 0:3], C.field_step(feat[g][:, 0:3], grad[g], ori[g], EPS, ALPHA, "l_inf")), g
    # two runs: the same bits; without xyz_out: the same feat, and nothing else differs
    again = step_clouds(feat, dfeat, dxyz, ori, None, n, l2)
    assert all(same(a, b) for a, b in zip(again, (got_f, got_norms, got_delta, got_xyz)))
    no_xyz = step_clouds(feat, dfeat, dxyz, ori, None, n, l2, with_xyz=False)
    assert same(no_xyz[0], got_f) and same(no_xyz[1], got_norms) and same(no_xyz[2], got_delta) and (no_xyz[3] == -5.0).all()
    # cloud 1 not running, NaN in its gradients: none of its bytes is written; clouds 0 and 2: the same bits as before
    pf, px = dfeat.copy(), dxyz.copy()
    pf[1], px[1] = np.nan, np.nan
    f_c, norms_c, delta_c, xyz_c = step_clouds(feat, pf, px, ori, np.array([1, 0, 1], np.uint8), n, l2)
    assert same(f_c[1], feat[1]) and (xyz_c[1] == -5.0).all()
    assert same(f_c[[0, 2]], got_f[[0, 2]]) and same(xyz_c[[0, 2]], got_xyz[[0, 2]])
    if l2:
        assert (norms_c[:, 1] == -5.0).all() and (delta_c[1] == -5.0).all()
        assert same(norms_c[:, [0, 2]], got_norms[:, [0, 2]]) and same(delta_c[[0, 2]], got_delta[[0, 2]])
    else:
        assert (norms_c == -5.0).all() and (delta_c == -5.0).all()     # l_inf uses neither


def test_step_clouds_refusals():
    from pointsecguard_amd import _lib, runtime
    lib = _lib.load()
    n = 63
    feat, dfeat, dxyz, ori = step_case(n)
    f, df, dx, o = dev(feat), dev(dfeat), dev(dxyz), dev(ori)
    norms, delta = dev(np.zeros((2, G), np.float32)), dev(np.zeros((G, n, 3), np.float32))

    def rc(*p, g=G, nn=n, l2=1):
        ptrs = [None if t is None else P(t) for t in p]
        return lib.psg_rla_bim_step_field_clouds(*ptrs[:4], None, g, nn, EPS, ALPHA, l2, *ptrs[4:], None, runtime.stream())

    for bad in ((None, df, dx, o, norms, delta), (f, None, dx, o, norms, delta), (f, df, None, o, norms, delta), (f, df, dx, None, norms, delta),
                (f, df, dx, o, None, delta), (f, df, dx, o, norms, None)):
        assert rc(*bad) == PSG_ERR_ARG and b"psg_rla_bim_step_field_clouds" in lib.psg_last_error()
    assert rc(f, df, dx, o, norms, delta, g=0) == PSG_ERR_ARG and rc(f, df, dx, o, norms, delta, nn=0) == PSG_ERR_ARG
    assert rc(f, df, dx, o, norms, delta, g=70000) == PSG_ERR_ARG
    assert same(host(f), feat)
    assert rc(f, df, dx, o, None, None, l2=0) == 0                       # l_inf needs neither


# ---------------------------------------------------------------------------------------------- 2. retire
@pytest.mark.parametrize("n", SMALL)
def test_retire_snapshots_both_halves(n):
    """Leaving, staying and frozen clouds, then `final`: both snapshots exact, the flags exact; a frozen cloud keeps its bytes
    under poisoned features."""
    import torch
    rng = np.random.default_rng(n)
    st = F.new_state(G, n)
    out_adv, out_xyz = (torch.zeros(G, n, 3, device="cuda") for _ in range(2))
    active, leaving = dev(np.array([1, 1, 0], np.uint8)), dev(np.array([1, 0, 1], np.uint8))    # leaving, staying, frozen (flag set)
    st["active"][:], st["leaving"][:] = [1, 1, 0], [1, 0, 1]
    for rnd, final in enumerate((0, 0, 1, 1)):
        feat = rng.random((G, n, 6), dtype=np.float32) + rnd
        if rnd:
            feat[0] = np.nan                                 # cloud 0 retired in round 0
        call("psg_rla_tbim_retire_field_clouds", D(feat), G, n, final, P(out_adv), P(out_xyz), P(active), P(leaving))
        F.retire(st, feat, final)
        assert same(host(out_adv), st["out_adv"]) and same(host(out_xyz), st["out_adv_xyz"]), rnd
        assert same(host(active), st["active"]) and same(host(leaving), st["leaving"]), rnd
        if rnd == 0:
            assert st["active"].tolist() == [0, 1, 0] and st["leaving"].tolist() == [0, 0, 1]       # a frozen cloud's flag is left alone
            assert same(st["out_adv_xyz"][0], feat[0][:, 0:3]) and same(st["out_adv"][0], feat[0][:, 3:6])
            assert not st["out_adv_xyz"][1].any() and not st["out_adv_xyz"][2].any()
        if rnd == 1:
            assert st["active"].tolist() == [0, 1, 0]
    assert not st["active"].any() and np.isfinite(st["out_adv"]).all() and st["out_adv_xyz"][1].any() and not st["out_adv_xyz"][2].any()


# ---------------------------------------------------------------------------------------------- network fixtures
def make_clouds(n, seed):
    """G clouds with their own positions, colours and labels; cloud 1 carries 256 duplicated points (position and colour)"""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((G, n, 3), dtype=np.float32) * np.array([4, 3, 3], np.float32)).astype(np.float32)
    rgb = rng.random((G, n, 3), dtype=np.float32)
    xyz[1, 256:512], rgb[1, 256:512] = xyz[1, :256], rgb[1, :256]
    labels = rng.integers(0, 13, (G, n))
    return xyz, rgb, labels


@pytest.fixture(scope="module")
def model():
    from pointsecguard_amd.randla import network
    return network.RandLAModel(randla_params(3))


@pytest.fixture(scope="module")
def ws8704():
    from pointsecguard_amd.randla import network
    return network.RandLAWorkspace(8704, batch=G, full=True)


@pytest.fixture(scope="module")
def ws8192():
    from pointsecguard_amd.randla import network
    return network.RandLAWorkspace(8192, batch=G, full=True)


def clean_pred(model, ws, feats):
    n = feats.shape[1]
    f = dev(feats.reshape(-1, 6).astype(np.float32))
    ws.set_cloud(f[:, 0:3].contiguous())
    return host(ws.forward(model, f).argmax(1)).reshape(G, n).astype(np.int64)


class Bufs:
    """The buffers of psg_rla_bim_field_window_args for G clouds of n points."""

    def __init__(self, n, xyz, rgb, labels, goal, field, ori=3, target=9, eps=EPS, alpha=ALPHA, coord_eps=EPS, coord_alpha=ALPHA, hit=None):
        import torch
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")          # noqa: E731
        self.n, self.field, self.eps, self.alpha, self.coord_eps, self.coord_alpha = n, field, eps, alpha, coord_eps, coord_alpha
        mask = labels == ori
        hit = np.where(mask, target, labels) if hit is None else hit
        self.sign = -1.0 if goal == "t" else 1.0
        self.feat0 = dev(np.concatenate([xyz, rgb], -1).reshape(G * n, 6))
        self.ori, self.ori_xyz = dev(rgb.reshape(G * n, 3)), dev(xyz.reshape(G * n, 3))
        self.labels, self.hit_ys = dev(labels.reshape(-1).astype(np.int32)), dev(hit.reshape(-1).astype(np.int32))
        self.loss_ys = dev((hit if goal == "t" else labels).reshape(-1).astype(np.int32))
        self.mask = dev(mask.reshape(-1).astype(np.uint8))
        self.n_mask = dev(mask.reshape(G, n).sum(1).astype(np.int32))
        self.feat, self.dfeat = z(G * n, 6), z(G * n, 6)
        self.xyz, self.dxyz = z(G * n, 3), z(G * n, 3)
        self.logits, self.dlogits = z(G * n, 13), z(G * n, 13)
        self.norms, self.norms_xyz, self.delta = z(2, G), z(2, G), z(G * n, 3)
        self.pred, self.out_pred = z(G * n, dt=torch.int32), z(G * n, dt=torch.int32)
        self.scratch = z(G, 2 * PARTS + 1, dt=torch.int32)
        self.hist = z(16, G, 3)
        self.out_adv, self.out_adv_xyz, self.out_stats = z(G * n, 3), z(G * n, 3), z(G, 3)
        self.active, self.leaving, self.exit = z(G, dt=torch.uint8), z(G, dt=torch.uint8), z(G, dt=torch.int32)
        self.reset()

    RESULT = ("feat", "xyz", "hist", "out_adv", "out_adv_xyz", "out_pred", "out_stats", "active", "leaving", "exit", "pred", "norms",
              "norms_xyz", "delta")

    def reset(self):
        self.feat.copy_(self.feat0)
        self.xyz.copy_(self.ori_xyz)
        for t in (self.hist, self.out_adv, self.out_adv_xyz, self.out_pred, self.out_stats, self.pred, self.norms, self.norms_xyz, self.delta,
                  self.leaving):
            t.zero_()
        self.active.fill_(1)
        self.exit.fill_(-1)

    def result(self):
        return {k: host(getattr(self, k)).copy() for k in self.RESULT}

    def args(self, model, ws, mode, num, den, l2, it0, n_steps, final, over=()):
        from pointsecguard_amd import _lib
        a = _lib.RlaBimFieldWindowArgs()
        a.model, a.ws = model.handle, ws.handle
        a.n_steps, a.G, a.N, a.it0, a.num, a.den, a.final, a.l2_metric = n_steps, G, self.n, it0, num, den, final, l2
        a.mode, a.field = mode, self.field
        a.eps, a.alpha, a.sign, a.coord_eps, a.coord_alpha = self.eps, self.alpha, self.sign, self.coord_eps, self.coord_alpha
        for k in ("labels", "feat", "logits", "dlogits", "dfeat", "norms_xyz", "delta", "pred", "scratch", "out_adv", "out_adv_xyz", "out_pred",
                  "out_stats", "active", "ori_xyz", "xyz", "dxyz"):
            setattr(a, k, getattr(self, k).data_ptr())
        if self.field == BOTH:
            a.ori, a.norms = self.ori.data_ptr(), self.norms.data_ptr()
        if mode:
            for k in ("mask", "n_mask", "hit_ys", "loss_ys", "hist", "leaving"):
                setattr(a, k, getattr(self, k).data_ptr())
            a.exit_step = self.exit.data_ptr()
        for k, v in dict(over).items():
            setattr(a, k, v)
        return a

    def window(self, model, ws, *rest):
        from pointsecguard_amd import _lib, runtime
        a = self.args(model, ws, *rest)
        _lib.call("psg_rla_bim_field_window", ctypes.byref(a), runtime.stream())

    def hand(self, model, ws, mode, num, den, l2, it0, n_steps, final):
        """The window's sequence through psg_rla_set_cloud and the step entry points, with a read-back between them."""
        import torch
        for i in range(n_steps):
            fin = 1 if final and i == n_steps - 1 else 0
            call("psg_rla_set_cloud", ws.handle, P(self.xyz))
            call("psg_rla_forward", model.handle, ws.handle, P(self.feat), P(self.logits))
            if mode:
                call("psg_rla_tbim_latch_clouds", P(self.logits), P(self.labels), P(self.hit_ys), P(self.mask), P(self.n_mask), G, self.n, num,
                     den, it0 + i, fin, P(self.hist[i]), P(self.pred), P(self.out_pred), P(self.out_stats), P(self.active), P(self.leaving),
                     P(self.exit), P(self.scratch))
                host(self.exit)
                call("psg_rla_colper_grad_masked", P(self.logits), P(self.loss_ys), P(self.mask), self.sign, G * self.n, P(self.dlogits), None)
            else:
                call("psg_rla_colper_grad_masked", P(self.logits), P(self.labels), None, 1.0, G * self.n, P(self.dlogits), None)
            call("psg_rla_backward_full", model.handle, ws.handle, P(self.dlogits), P(self.dfeat), P(self.dxyz))
            torch.cuda.synchronize()
            call("psg_rla_bim_step_field_clouds", P(self.feat), P(self.dfeat), P(self.dxyz), P(self.ori_xyz), P(self.active), G, self.n,
                 self.coord_eps, self.coord_alpha, l2, P(self.norms_xyz), P(self.delta), P(self.xyz))
            if self.field == BOTH:
                call("psg_rla_bim_step_clouds", P(self.feat), P(self.dfeat), P(self.ori), P(self.active), G, self.n, self.eps, self.alpha, l2,
                     P(self.norms), P(self.delta))
            float(self.feat[0, 0])
            if mode:
                call("psg_rla_tbim_retire_field_clouds", P(self.feat), G, self.n, fin, P(self.out_adv), P(self.out_adv_xyz), P(self.active),
                     P(self.leaving))
            elif fin:                                        # mode 0 has no leaving flags: a zeroed array stands for none
                call("psg_rla_tbim_retire_field_clouds", P(self.feat), G, self.n, 1, P(self.out_adv), P(self.out_adv_xyz), P(self.active),
                     P(self.leaving))
            host(self.active)


def in_l2_ball(d, eps, n):
    """|d|_2 per cloud of positions written in float32 below 8 m: the clipped delta has norm eps up to a few roundings (1e-6
    relative is generous), and every one of the 3 n coordinates is ori + delta * scale rounded once, at most 2^-22 off"""
    return (np.sqrt((d.reshape(d.shape[0], -1) ** 2).sum(1)) <= eps * (1 + 1e-6) + np.sqrt(3 * n) * 2.0 ** -22).all()


def knn_rows(xyz_dev, n):
    """psg_knn_points of every cloud on its own positions, as row numbers of the cloud-major buffers"""
    import torch
    from pointsecguard_amd import _lib, runtime
    out = torch.empty(G * n, 16, dtype=torch.int32, device="cuda")
    _lib.call("psg_knn_points", runtime.context(xyz_dev.device), P(xyz_dev), P(xyz_dev), G, n, n, 16, P(out), runtime.stream())
    return host(out).reshape(G, n, 16) + (np.arange(G) * n)[:, None, None]


def predicted_setup(model, ws, n, seed):
    """Clouds whose labels are the clean prediction (full range, dim, nearly grey colours: the hits rise at different rates);
    origin = the class every cloud is predicted as most, target = the next."""
    xyz, rgb, _ = make_clouds(n, seed)
    rgb[1] = 0.25 * rgb[1]
    rgb[2] = 0.45 + 0.1 * rgb[2]
    labels = clean_pred(model, ws, np.concatenate([xyz, rgb], -1))
    order = np.argsort(-np.array([min((labels[g] == c).sum() for g in range(G)) for c in range(13)]), kind="stable")
    ori, target = int(order[0]), int(order[1])
    assert all((labels[g] == ori).sum() > 0 for g in range(G))
    return xyz, rgb, labels, ori, target


# the two cases of the window tests: (goal, l2, mode-1 threshold, colour eps / alpha, coordinate eps / alpha)
T_L2 = ("t", 1, 2.0, 0.4, 4.0, 0.8)
UT_LINF = ("ut", 0, EPS, ALPHA, 0.05, 0.01)


def window_case(model, ws, n, goal):
    if goal == "t":
        xyz, rgb, labels, ori, target = predicted_setup(model, ws, n, 44)
        return xyz, rgb, labels, ori, target, T_L2
    xyz, rgb, labels = make_clouds(n, 21)
    pred0 = clean_pred(model, ws, np.concatenate([xyz, rgb], -1))
    target = int(np.bincount(pred0.reshape(-1), minlength=13).argmax())
    return xyz, rgb, labels, 3 if target != 3 else 4, target, UT_LINF


# ---------------------------------------------------------------------------------------------- 3. windows == steps
# recorded ("coord"): 't' hits 0, 13, 32, 47, 60, 62, 65, 91 / 0, 5, 12, 13, 28, .. 61 / 0, 33, 40, 41, 68 of 6839 / 7894 / 6795 origin
# points (leave at 7, never, 4); 'ut' hits 498, 499 / 502, 507 / 528, 527 of 630 / 646 / 675 (cloud 0 leaves at 1)
WINDOW_THRESHOLD = {"t": (1, 100), "ut": (79, 100)}


@pytest.mark.parametrize("field", [COORD, BOTH])
@pytest.mark.parametrize("n,goal", [(8704, "t"), (8192, "ut")])
def test_windows_equal_hand_driven_steps(model, ws8704, ws8192, n, goal, field):
    """Mode 1: a 1-step window, a 10-step window and a cut 3-step final window, each from the same start, against the same
    sequence through psg_rla_set_cloud and the step entry points on the same workspace: positions, colours, history rows,
    snapshots, flags, exit steps, norms and delta bit-equal, and a second window run bit-equal to the first.  After the 10-step
    window the workspace's level-0 neighbour table is psg_knn_points of the positions the window left; under "coord" the colours
    keep their bytes."""
    ws = ws8704 if n == 8704 else ws8192
    xyz, rgb, labels, ori, target, (_, l2, eps, alpha, ceps, calpha) = window_case(model, ws, n, goal)
    b = Bufs(n, xyz, rgb, labels, goal, field, ori, target, eps, alpha, ceps, calpha)
    num, den = WINDOW_THRESHOLD[goal]
    for it0, n_steps, final in ((0, 1, 0), (0, 10, 0), (10, 3, 1)):
        b.reset()
        b.hand(model, ws, 1, num, den, l2, it0, n_steps, final)
        want = b.result()
        for rnd in range(2):
            b.reset()
            b.window(model, ws, 1, num, den, l2, it0, n_steps, final)
            got = b.result()
            for k in Bufs.RESULT:
                assert same(got[k], want[k]), (it0, n_steps, final, rnd, k)
        print("goal", goal, "field", field, "window", (it0, n_steps, final), "exit", want["exit"], "n_mask", host(b.n_mask),
              "hits per step", want["hist"][:n_steps, :, 1].T.tolist())
        assert same(got["feat"][:, 0:3], got["xyz"]) and not same(got["xyz"], host(b.ori_xyz))
        if field == COORD:
            assert same(got["feat"][:, 3:6], host(b.feat0)[:, 3:6]) and not got["norms"].any()
        else:
            assert not same(got["feat"][:, 3:6], host(b.feat0)[:, 3:6])
        if n_steps == 10:
            # the pyramid of an iteration is built on the positions the update before it left: one more step, and the level-0
            # table is psg_knn_points of the positions the 10-step window left
            left = b.xyz.clone()
            b.window(model, ws, 1, num, den, l2, 10, 1, 0)
            table = host(ws.index(0, 0)).reshape(G, n, 16)
            assert np.array_equal(table, knn_rows(left, n)) and not np.array_equal(table, knn_rows(b.ori_xyz, n))
            assert same(want["active"], (want["exit"] < 0).astype(np.uint8))
            # the premise: clouds leave inside the window, not all at one step
            assert len(set(want["exit"].tolist())) >= 2 and (want["exit"] >= 1).any(), want["exit"]
        if final:
            assert not got["active"].any() and got["out_adv_xyz"].any()
            live = want["exit"] < 0                           # the cap's snapshot: the features the window left
            rows = np.repeat(live, n)
            assert same(got["out_adv_xyz"][rows], got["feat"][rows, 0:3]) and same(got["out_adv"][rows], got["feat"][rows, 3:6])


@pytest.mark.parametrize("field", [COORD, BOTH])
@pytest.mark.parametrize("l2", [0, 1])
def test_mode_0_window_equals_hand_steps(model, ws8192, field, l2):
    """BIM, iteration = 4: windows of 3 + 2 steps, the last one final, against 5 hand steps; nothing of mode 1's is bound."""
    n = 8192
    xyz, rgb, labels = make_clouds(n, 21)
    ceps, calpha = (4.0, 0.8) if l2 else (0.05, 0.01)
    eps, alpha = (2.0, 0.4) if l2 else (EPS, ALPHA)
    b = Bufs(n, xyz, rgb, labels, "ut", field, eps=eps, alpha=alpha, coord_eps=ceps, coord_alpha=calpha)
    b.hand(model, ws8192, 0, 0, 1, l2, 0, 5, 1)
    want = b.result()
    b.reset()
    b.window(model, ws8192, 0, 0, 1, l2, 0, 3, 0)
    mid = b.result()
    assert mid["active"].all() and not mid["out_adv_xyz"].any() and not same(mid["xyz"], host(b.ori_xyz))
    b.window(model, ws8192, 0, 0, 1, l2, 3, 2, 1)
    got = b.result()
    for k in Bufs.RESULT:
        assert same(got[k], want[k]), k
    assert not got["active"].any() and same(got["out_adv_xyz"], got["xyz"]) and same(got["out_adv"], got["feat"][:, 3:6])
    assert (got["exit"] == -1).all() and not got["hist"].any() and not got["out_pred"].any()
    d = got["xyz"].astype(np.float64) - xyz.reshape(-1, 3)
    if l2:
        assert in_l2_ball(d.reshape(G, n, 3), ceps, n)
    else:
        # the clip bounds are fl(x - eps), fl(x + eps): one rounding of a number below 8 off the exact ball
        assert np.abs(d).max() <= np.float64(np.float32(ceps)) + 2.0 ** -22
    assert same(got["feat"][:, 3:6], host(b.feat0)[:, 3:6]) == (field == COORD)


def test_window_refusals(model, ws8704, ws8192):
    """Every refusal is PSG_ERR_ARG with a message, nothing is enqueued - the buffers keep their bytes - and the stream still
    serves a good window afterwards."""
    import torch
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.randla import network
    n = 8704
    xyz, rgb, labels = make_clouds(n, 21)
    b = Bufs(n, xyz, rgb, labels, "t", BOTH)
    plain = network.RandLAWorkspace(n, batch=G)
    lib = _lib.load()
    before = b.result()
    cases = [("psg_rla_ws_create_full", plain, 1, 1, {}), ("the workspace is for", ws8192, 1, 1, {}), ("the workspace is for", ws8704, 1, 1, {"G": 2}),
             ("field", ws8704, 1, 1, {"field": 0}), ("field", ws8704, 1, 1, {"field": 3}), ("mode", ws8704, 1, 1, {"mode": 2}),
             ("n_steps", ws8704, 1, 1, {"n_steps": 0}), ("it0", ws8704, 1, 1, {"it0": -1}), ("threshold", ws8704, 1, 1, {"den": 0}),
             ("threshold", ws8704, 0, 1, {"den": -3})]
    cases += [("mode 1 needs", ws8704, 1, 1, {k: None}) for k in ("mask", "n_mask", "hit_ys", "loss_ys", "hist", "leaving", "exit_step")]
    cases += [("l_2 metric needs", ws8704, m, 1, {k: None}) for k in ("norms_xyz", "delta", "norms") for m in (0, 1)]
    cases += [("field both needs ori", ws8704, 1, 0, {"ori": None})]
    cases += [("null argument", ws8704, m, 0, {k: None}) for m in (0, 1) for k in
              ("model", "ws", "ori_xyz", "xyz", "dxyz", "out_adv_xyz", "out_adv", "labels", "feat", "logits", "dlogits", "dfeat", "pred", "scratch",
               "out_pred", "out_stats", "active")]
    for text, ws, mode, l2, over in cases:
        a = b.args(model, ws, mode, 9, 10, l2, 0, 1, 0, over)
        rc = lib.psg_rla_bim_field_window(ctypes.byref(a), runtime.stream())
        msg = lib.psg_last_error()
        assert rc == PSG_ERR_ARG and b"psg_rla_bim_field_window" in msg and text.encode() in msg, (text, over, rc, msg)
    assert lib.psg_rla_bim_field_window(None, runtime.stream()) == PSG_ERR_ARG
    torch.cuda.synchronize()
    after = b.result()
    for k in Bufs.RESULT:
        assert same(before[k], after[k]), k
    # what each mode and field may leave out
    for mode, field, l2 in ((0, COORD, 0), (1, COORD, 0), (0, BOTH, 1)):
        b.field = field
        b.reset()
        b.window(model, ws8704, mode, 9, 10, l2, 0, 1, 0)
        torch.cuda.synchronize()
        assert not same(b.result()["xyz"], before["xyz"])


# ---------------------------------------------------------------------------------------------- 4. independence
def test_clouds_are_independent(model, ws8192):
    """Cloud 2 replaced by positions, colours and labels that leave at iteration 1: the complete trajectories and results of
    clouds 0 and 1 stay bit-identical, and the retired cloud stops moving."""
    n, steps = 8192, 5
    xyz, rgb, labels = make_clouds(n, 33)
    runs = []
    for replaced in (False, True):
        xyz_r, rgb_r, labels_r, hit = xyz.copy(), rgb.copy(), labels.copy(), None
        if replaced:
            rng = np.random.default_rng(77)
            rgb_r[2] = rng.random((n, 3), dtype=np.float32)
            xyz_r[2] = (rng.random((n, 3), dtype=np.float32) * np.array([4, 3, 3], np.float32)).astype(np.float32)
            pred0 = clean_pred(model, ws8192, np.concatenate([xyz_r, rgb_r], -1))
            target = int(np.bincount(pred0[2], minlength=13).argmax())      # a class cloud 2 is predicted as
            labels_r[2] = leaving_labels(pred0[2], 3, target)
            hit = np.where(labels_r == 3, 9, labels_r)
            hit[2] = np.where(labels_r[2] == 3, target, labels_r[2])        # (cloud 2 alone aims at its own target class)
        b = Bufs(n, xyz_r, rgb_r, labels_r, "t", BOTH, ori=3, target=9, eps=2.0, alpha=0.4, coord_eps=4.0, coord_alpha=0.8, hit=hit)
        traj = []
        for it in range(steps):
            b.window(model, ws8192, 1, 1, 2, 1, it, 1, 1 if it == steps - 1 else 0)
            traj.append(b.result())
        runs.append(traj)
    assert runs[1][-1]["exit"][2] == 1 and (runs[0][-1]["exit"][:2] == -1).all()
    keep = np.r_[0:2 * n]
    assert not same(runs[0][0]["xyz"][keep], runs[0][-1]["xyz"][keep])       # (clouds 0 and 1 do move)
    for t, (ra, rb) in enumerate(zip(*runs)):
        for k in ("feat", "xyz", "out_adv", "out_adv_xyz", "out_pred", "pred"):
            assert same(ra[k][keep], rb[k][keep]), (t, k)
        for k in ("out_stats", "active", "leaving", "exit"):
            assert same(ra[k][:2], rb[k][:2]), (t, k)
        for k in ("hist", "norms", "norms_xyz"):
            assert same(ra[k][:, :2], rb[k][:, :2]), (t, k)
    assert same(runs[1][1]["feat"][2 * n:], runs[1][-1]["feat"][2 * n:]) and same(runs[1][1]["xyz"][2 * n:], runs[1][-1]["xyz"][2 * n:])
    assert not same(runs[1][0]["xyz"][2 * n:], runs[1][1]["xyz"][2 * n:])    # the exiting iteration's update was applied


# ---------------------------------------------------------------------------------------------- 5. exits at different steps
CAP = 12


@pytest.mark.parametrize("field", ["coord", "both"])
def test_exits_at_different_steps(model, ws8192, field):
    """One run with exits disabled records every iteration (1-step windows): the history row, the prediction, and positions and
    colours AFTER the iteration's update.  A threshold picked from the recorded hits makes clouds leave at different iterations
    and one reach the cap (the premise, asserted); the rerun in 10-step windows gives each cloud the recorded state after the
    update of its exit iteration and the prediction before that update."""
    from pointsecguard_amd.randla import attack, nb_field
    n = 8192
    xyz, rgb, labels, ori, target = predicted_setup(model, ws8192, n, 44)
    feats = np.concatenate([xyz, rgb], -1)
    cls = nb_field.tar_NBattackField(model, goal="t", distance_metric="l_2", field=field)
    cls.config(magnitude=2.0, alpha=0.4, iteration=CAP, coord_magnitude=4.0, coord_alpha=0.8)
    rec = {}

    def hook(it0, n_run, final, S, rows):
        assert n_run == 1
        rec[(it0, "row")] = rows[0].copy()
        rec[(it0, "feat")] = host(S.feat).reshape(G, n, 6).copy()
        rec[(it0, "pred")] = host(S.pred).reshape(G, n).copy()

    cls.EXIT_RATIO, cls.chunk, cls.window_hook = (1, 1), 1, hook          # n_hits > n_mask never holds
    cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
    assert (cls.last_steps == CAP + 1).all() and len(rec) == 3 * (CAP + 1)
    assert same(host(cls.last_adv_xyz), rec[(CAP, "feat")][:, :, 0:3]) and same(host(cls.last_adv), rec[(CAP, "feat")][:, :, 3:6])
    counts = np.stack([rec[(e, "row")][:, 1] for e in range(CAP + 1)]).astype(np.int64)        # [CAP + 1][G]
    totals = (labels == ori).sum(1)
    print("field", field, "hits per iteration", counts.T.tolist(), "totals", totals.tolist())
    choice = None
    for e in range(1, CAP + 1):                          # candidate thresholds: the recorded ratios themselves
        for g in range(G):
            num, den = int(counts[e, g]), int(totals[g])
            ex = first_exit(num, den, counts, totals, CAP)
            if len(set(x for x in ex if x >= 0)) >= 2 and -1 in ex:
                choice = (num, den, ex)
                break
        if choice:
            break
    assert choice is not None, "premise: two distinct exit iterations and one cloud at the cap"
    num, den, ex = choice
    print("threshold", num, "/", den, "exit iterations", ex)
    cls.EXIT_RATIO, cls.chunk, cls.window_hook = (num, den), attack.CHUNK, None
    outs = cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
    assert cls.last_steps.tolist() == [x + 1 if x >= 0 else CAP + 1 for x in ex]
    S = cls._field_clouds[(n, G)]
    assert host(S.exit).tolist() == ex and not host(S.active).any()
    adv_xyz, adv = host(cls.last_adv_xyz), host(cls.last_adv)
    for g in range(G):
        e = ex[g] if ex[g] >= 0 else CAP
        assert same(adv_xyz[g], rec[(e, "feat")][g][:, 0:3]) and same(adv[g], rec[(e, "feat")][g][:, 3:6]), g
        assert same(host(S.out_pred).reshape(G, n)[g], rec[(e, "pred")][g]), g
        assert same(host(S.out_stats)[g], rec[(e, "row")][g]), g
        assert not same(adv_xyz[g], rec[(e - 1, "feat")][g][:, 0:3]), g        # the exiting iteration's update was applied
    assert len(outs) == G and all(np.isfinite(o).all() for o in outs)


# ---------------------------------------------------------------------------------------------- 6. the classes
N_CLS = 8192


def one_cloud(seed):
    xyz, rgb, labels = make_clouds(N_CLS, seed)
    return np.concatenate([xyz, rgb], -1), labels


def settings(metric):
    return dict(magnitude=EPS if metric == "l_inf" else 1.0, alpha=ALPHA if metric == "l_inf" else 0.2,
                coord_magnitude=0.05 if metric == "l_inf" else 2.0, coord_alpha=0.01 if metric == "l_inf" else 0.4)


@pytest.mark.parametrize("metric", ["l_2", "l_inf"])
@pytest.mark.parametrize("field", ["coord", "both"])
def test_targeted_one_cloud_equals_batch_attack(model, field, metric):
    """`tar_NBattackField.batch_attack_clouds` on [1, N, 6] against the parent's `batch_attack` on the same cloud: last_adv_xyz,
    last_adv, last_dist_xyz and every tuple field, once with labels under which the loop leaves at iteration 1 and once with labels
    under which it runs to the cap."""
    from pointsecguard_amd.randla import attack, nb_field, network
    n, cap, ori = N_CLS, 3, 3
    feats, labels = one_cloud(61)
    ws = network.RandLAWorkspace(n)
    ws.set_cloud(dev(feats[0][:, 0:3]))
    pred0 = host(ws.forward(model, dev(feats[0])).argmax(1))
    del ws
    counts = np.bincount(pred0, minlength=13)
    target = int(counts.argmax())                        # "leaves": a class the cloud is predicted as
    rare = int(np.argsort(counts + (np.arange(13) == ori) * n, kind="stable")[0])      # "cap": the rarest class that is not ori
    one = attack.tar_NBattack(model, goal="t", distance_metric=metric, field=field)
    lock = nb_field.tar_NBattackField(model, goal="t", distance_metric=metric, field=field)
    for cls in (one, lock):
        cls.config(iteration=cap, **settings(metric))
    for name, lab, want_steps in (("leaves", leaving_labels(pred0, ori, target), 2), ("cap", labels[0], cap + 1)):
        tgt = target if name == "leaves" else rare
        want = one.batch_attack(feats[0], lab, target=tgt, ori=ori)
        got = lock.batch_attack_clouds(feats[:1], lab[None], target=tgt, ori=ori)
        print(field, metric, name, "steps", lock.last_steps, "tuple", got[0], "dist_xyz", lock.last_dist_xyz)
        assert len(got) == 1 and got[0] == want, (name, got[0], want)
        assert lock.last_adv_xyz.shape == (1, n, 3) and same(host(lock.last_adv_xyz)[0], host(one.last_adv_xyz)), name
        assert same(host(lock.last_adv)[0], host(one.last_adv)), name
        assert lock.last_dist_xyz.shape == (1,) and float(lock.last_dist_xyz[0]) == float(one.last_dist_xyz) > 0.0, name
        assert (got[0][4] > 0.0) == (field == "both"), name
        assert lock.last_steps.tolist() == [want_steps], name


@pytest.mark.parametrize("metric", ["l_2", "l_inf"])
@pytest.mark.parametrize("field", ["coord", "both"])
def test_untargeted_one_cloud_equals_batch_attack_and_slot_0(model, field, metric):
    """`NBattackField.batch_attack_clouds` on [1, N, 6] equals `NBattack(field=...).batch_attack` bit for bit; slot 0 of a G = 2
    call equals the G = 1 call; the positions stay in the eps ball; the workspace is left on the moved positions."""
    from pointsecguard_amd.randla import attack, nb_field
    n, cap = N_CLS, 3
    feats, labels = one_cloud(62)
    one = attack.NBattack(model, distance_metric=metric, field=field)
    lock = nb_field.NBattackField(model, distance_metric=metric, field=field)
    for cls in (one, lock):
        cls.config(iteration=cap, **settings(metric))
    lock.chunk = 3                                           # 4 updates: a window of 3 and a final window of 1
    want = host(one.batch_attack(feats[0], labels[0]))
    got = host(lock.batch_attack_clouds(feats[:1], labels[:1]))
    assert got.shape == (1, n, 3) and same(got[0], want)
    assert same(host(lock.last_adv_xyz)[0], host(one.last_adv_xyz)) and float(lock.last_dist_xyz[0]) == float(one.last_dist_xyz) > 0.0
    assert same(got[0], feats[0][:, 3:6]) == (field == "coord")
    xyz1, dist1 = host(lock.last_adv_xyz).copy(), lock.last_dist_xyz.copy()
    got2 = host(lock.batch_attack_clouds(feats[:2], labels[:2]))
    assert got2.shape == (2, n, 3) and same(got2[0], got[0]) and same(host(lock.last_adv_xyz)[0], xyz1[0])
    assert lock.last_dist_xyz.shape == (2,) and lock.last_dist_xyz[0] == dist1[0]
    assert not same(host(lock.last_adv_xyz)[1], xyz1[0])
    d = host(lock.last_adv_xyz).astype(np.float64) - feats[:2, :, 0:3]
    ceps = settings(metric)["coord_magnitude"]
    if metric == "l_2":
        assert in_l2_ball(d, ceps, n)
    else:
        assert np.abs(d).max() <= np.float64(np.float32(ceps)) + 2.0 ** -22
    S = lock._field_clouds[(n, 2)]
    table = host(S.ws.index(0, 0)).reshape(2, n, 16)
    import torch
    out = torch.empty(2 * n, 16, dtype=torch.int32, device="cuda")
    from pointsecguard_amd import _lib, runtime
    xyz_dev = lock.last_adv_xyz.reshape(2 * n, 3).contiguous()
    _lib.call("psg_knn_points", runtime.context(xyz_dev.device), P(xyz_dev), P(xyz_dev), 2, n, n, 16, P(out), runtime.stream())
    assert np.array_equal(table, host(out).reshape(2, n, 16) + (np.arange(2) * n)[:, None, None])


def test_clouds_class_fields_and_refusals(model):
    """G = 3: the tuples against a recomputation from the snapshots, the eps ball, `field="color"` the parents' bytes, and every
    refusal of the classes before any device work."""
    from pointsecguard_amd.randla import attack, nb_field
    n, ori, target, cap = N_CLS, 3, 9, 11          # 12 iterations: a full window and a cut final one
    xyz, rgb, labels = make_clouds(n, 56)
    feats = np.concatenate([xyz, rgb], -1)
    cls = nb_field.TBIMField(model, goal="t", distance_metric="l_2", field="both")
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
    with pytest.raises(ValueError, match="target"):
        cls.batch_attack_clouds(feats, labels, ori=ori)
    with pytest.raises(ValueError, match="features"):
        cls.batch_attack_clouds(feats[0], labels[0], target=target, ori=ori)
    with pytest.raises(ValueError, match="features"):
        cls.batch_attack_clouds(feats[:, :, :5], labels, target=target, ori=ori)
    with pytest.raises(ValueError, match="labels"):
        cls.batch_attack_clouds(feats, labels[:, :-1], target=target, ori=ori)
    with pytest.raises(ValueError, match="labels"):
        cls.batch_attack_clouds(feats, labels[:2], target=target, ori=ori)
    bim = nb_field.BIMField(model, field="coord")
    with pytest.raises(ValueError, match="config"):
        bim.batch_attack_clouds(feats, labels)
    bim.config(magnitude=EPS, alpha=ALPHA, iteration=0)
    with pytest.raises(ValueError, match="iteration"):
        bim.batch_attack_clouds(feats, labels)
    bim.config(iteration=2)
    with pytest.raises(ValueError, match="features"):
        bim.batch_attack_clouds(feats[0], labels[0])
    with pytest.raises(ValueError, match="labels"):
        bim.batch_attack_clouds(feats, labels[:2])
    assert "_field_clouds" not in cls.__dict__ and "_field_clouds" not in bim.__dict__ and cls.last_adv is None
    with pytest.raises(NotImplementedError):
        nb_field.NBattackField(model, batch_size=2, field="coord")
    with pytest.raises(NotImplementedError):
        nb_field.tar_NBattackField(model, batch_size=2)

    class Log:
        lines = []

        def info(self, s):
            self.lines.append(s)

    cls.config(logger=Log())
    outs = cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
    adv, adv_xyz, steps = host(cls.last_adv), host(cls.last_adv_xyz), cls.last_steps.copy()
    outs2 = cls.batch_attack_clouds(feats, labels, target=target, ori=ori)
    assert outs2 == outs and same(host(cls.last_adv_xyz), adv_xyz) and same(host(cls.last_adv), adv)
    S = cls._field_clouds[(n, G)]
    pred = host(S.out_pred).reshape(G, n)
    from pointsecguard_amd.randla import network
    pred0 = clean_pred(model, network.RandLAWorkspace(n, batch=G, full=True), feats)
    print("steps", steps, "tuples", outs, "dist_xyz", cls.last_dist_xyz)
    assert len(outs) == G and len(Log.lines) == 2 * G and Log.lines[0].startswith("points=")
    assert adv.shape == (G, n, 3) and adv.min() >= 0.0 and adv.max() <= 1.0 and steps.shape == (G,) and cls.last_dist_xyz.shape == (G,)
    for g in range(G):
        mk = labels[g] == ori
        tp = float(mk.sum())
        hit = np.where(mk, target, labels[g])
        dist = float(np.sqrt(((adv[g].astype(np.float64) - rgb[g]) ** 2).sum()))
        dist_xyz = float(np.sqrt(((adv_xyz[g].astype(np.float64) - xyz[g]) ** 2).sum()))
        want = (tp, (pred[g][mk] == hit[mk]).sum() / tp, (pred[g][~mk] == hit[~mk]).sum() / (n - tp),
                (pred0[g][~mk] == labels[g][~mk]).sum() / (n - tp), dist, mean_iou(pred[g][~mk], labels[g][~mk]),
                mean_iou(pred0[g][~mk], labels[g][~mk]))
        assert len(outs[g]) == 7
        for k in (0, 1, 2, 3, 5, 6):
            assert outs[g][k] == want[k], (g, k)
        # float32 norms of 3 n float32 differences against the same sums in double (tests/test_gpu_rla_tbim_clouds.py)
        assert abs(outs[g][4] - dist) <= dist * (3 * n + 2) * 2.0 ** -24 and outs[g][4] > 0.0, g
        assert abs(cls.last_dist_xyz[g] - dist_xyz) <= dist_xyz * (3 * n + 2) * 2.0 ** -24 and dist_xyz > 0.0, g
        # coord_magnitude follows magnitude when unset
        assert in_l2_ball(adv_xyz[g][None].astype(np.float64) - xyz[g], 1.0, n) and in_l2_ball(adv[g][None].astype(np.float64) - rgb[g], 1.0, n)
    # field = "color": the parents' code and bytes
    par = attack.tar_NBattack(model, goal="t", distance_metric="l_2")
    sub = nb_field.tar_NBattackField(model, goal="t", distance_metric="l_2", field="color")
    for c in (par, sub):
        c.config(magnitude=1.0, alpha=0.2, iteration=2)
    assert sub.batch_attack_clouds(feats, labels, target=target, ori=ori) == par.batch_attack_clouds(feats, labels, target=target, ori=ori)
    assert same(host(sub.last_adv), host(par.last_adv)) and sub.last_adv_xyz is None
    parb = attack.BIM(model, batch_size=G, distance_metric="l_2")
    subb = nb_field.BIMField(model, distance_metric="l_2", field="color")
    for c in (parb, subb):
        c.config(magnitude=1.0, alpha=0.2, iteration=2)
    got = host(subb.batch_attack_clouds(feats, labels))
    assert got.shape == (G, n, 3) and same(got, host(parb.batch_attack(feats, labels)))
    par1 = attack.BIM(model, distance_metric="l_2")
    par1.config(magnitude=1.0, alpha=0.2, iteration=2)
    assert same(host(subb.batch_attack_clouds(feats[:1], labels[:1]))[0], host(par1.batch_attack(feats[0], labels[0])))
