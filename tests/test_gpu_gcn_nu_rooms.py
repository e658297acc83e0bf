"""The lockstep ResGCN NU attacks (NU_attack.forward_rooms / tar_NU_attack.forward_rooms, psg_gcn_nu_window) on the 5-block
fixture network and 1024-point rooms: windows against the same entry points driven step by step, lockstep against rooms
alone, the reference's recorded states through one-step windows, tar_NU control flow and the generators' positions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NB, N = 5, 1024
F = np.float32
U = 2.0 ** -24


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dt is not None:
        t = t.to(dt)
    return t.cuda().contiguous()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def host(t):
    return t.detach().cpu().numpy()


def _new_net(sd):
    from types import SimpleNamespace
    from pointsecguard_amd.resgcn.sem_seg_dense.architecture import DenseDeepGCN
    opt = SimpleNamespace(n_filters=64, k=16, act="relu", norm="batch", bias=True, epsilon=0.0, stochastic=True,
                          conv="edge", n_blocks=NB, block="res", in_channels=9, dropout=0.0, n_classes=13)
    net = DenseDeepGCN(opt)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda().eval()


@pytest.fixture(scope="module")
def net(gcn_weights_sd):
    return _new_net(gcn_weights_sd)


@pytest.fixture(scope="module")
def rooms3(net, golden_gcn_nu, golden_gcn_tarnu, golden_gcn_room):
    """three fixture rooms [3, 9, N, 1], their labels, the clean predictions (computed once, shared)"""
    r = np.stack([golden_gcn_nu["rooms"][0], golden_gcn_tarnu["rooms"][0], golden_gcn_room["room"]])
    labels = np.stack([golden_gcn_nu["labels"][0], golden_gcn_tarnu["labels"][0], golden_gcn_room["labels"]]).astype(np.int64)
    x = dev(r.transpose(0, 2, 1)[:, :, :, None])
    with torch.no_grad():
        pred = torch.cat([net(x[i:i + 1]) for i in range(3)]).argmax(dim=1)          # [3, 13, N] -> [3, N]
    return x, labels, host(pred).astype(np.int64)


def _attacks():
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks import torchattacks
    return torchattacks


def _state_of(net, R, nb):
    return next(s for k, s in net._psg_gcn_nu_states.items() if k[1] == R and k[3] == nb)


# ============================================================================ windows against hand-driven steps
def _init(S, x, labels, mk):
    from pointsecguard_amd import _lib, runtime
    R = x.shape[0]
    S.labels.copy_(dev(labels, torch.int32))
    if mk is not None:
        S.mask.copy_(dev(mk.astype(np.uint8)))
        S.n_mask.copy_(dev(mk.sum(1).astype(np.int32)))
    _lib.call("psg_to_point_major", runtime.ptr(x[:, :, :, 0].contiguous()), R, 9, N, runtime.ptr(S.x0), runtime.stream())
    S.ori.copy_(S.x0[:, :, 3:6])
    _lib.call("psg_nu_inverse_tanh", runtime.ptr(S.x0), R, N, runtime.ptr(S.w), runtime.stream())
    S.m.zero_(); S.v.zero_(); S.scal.zero_(); S.active.fill_(1); S.exit.fill_(-1); S.out.zero_()
    S.pred.fill_(-1); S.nn_state.fill_(-1)


def _hand_step(S, model, ws, step, R, nb, mode, target, kappa, c_f, c_l2, lr, hist_row, masked):
    """one optimiser step through the per-operation entry points, in the window's order"""
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.attacks.torchattacks.attacks.nu import ADAM_EPS, BETA1, BETA2, ctypes_off
    P, st = runtime.ptr, runtime.stream
    mk = P(S.mask) if masked else None
    _lib.call("psg_nu_tanh_color_rooms", P(S.w), mk, R, N, P(S.x0), st())
    ws.forward(model, S.x0, S.logits)
    _lib.call("psg_gcn_f_loss_grad_rooms", P(S.logits), P(S.labels), target, mk, mode, R, N, 13, kappa, 1.0, c_f, P(S.dlogits),
              P(S.scal[0]), P(S.pred), st())
    ws.backward(model, S.dlogits, S.dx0)
    _lib.call("psg_smooth_knn_sym_rooms", ctypes_off(S.x0, 3), 9, N * 9, R, N, nb, P(S.scal[1]), P(S.sgrad), P(S.active),
              P(S.nn_state), st())
    _lib.call("psg_nu_adam_step_rooms", P(S.w), P(S.m), P(S.v), mk, P(S.dx0), P(S.x0), P(S.ori), P(S.sgrad), 1e-4, c_l2, lr, BETA1,
              BETA2, ADAM_EPS, step + 1, R, N, P(S.active), P(S.scal[2]), st())
    _lib.call("psg_nu_step_latch", P(S.pred), P(S.labels), target, mk if mode else None, P(S.n_mask) if mode else None, R, 1, N, mode,
              P(S.scal), P(hist_row), P(S.x0), P(S.out), P(S.active), P(S.exit), step, st())


@pytest.mark.parametrize("variant", ["nu", "tarnu"])
def test_windows_equal_hand_driven_steps(net, rooms3, variant):
    """31 steps at R = 2: the windows [0], [1..10] (eager), [11..20] (captured), [21..30] (replayed) against the same entry
    points called step by step from here; state and integer history bit for bit, the float sums to the rounding of their
    atomic additions (f: 4 workgroup partials, Smooth: 16 wave partials, L2: 12 partials per room)."""
    from pointsecguard_amd import _lib
    from pointsecguard_amd.attacks.torchattacks.attacks.nu import ADAM_EPS, BETA1, BETA2
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu as gnu
    x, labels, _ = rooms3
    R, steps, lr, kappa = 2, 31, 0.05, 0.0
    x, labels = x[:R].contiguous(), labels[:R]
    if variant == "nu":
        nb, mode, target, c_f, c_l2, mk = 10, 0, 0, 0.1, 1.0, None
    else:
        nb, mode, target, c_f, c_l2 = 5, 2, 6, 1.0, 0.5
        mk = np.zeros((R, N), bool)
        mk[0, ::3] = True
        mk[1, 1::2] = True
    model, ws = net._packed(), net._workspace(R, N)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        A, B = gnu._GcnNuState(x.device, R, N, nb), gnu._GcnNuState(x.device, R, N, nb)
        hist_a = torch.zeros(steps, 5, R, device="cuda")
        _init(A, x, labels, mk)
        zmax = 0.0
        for s in range(steps):
            _hand_step(A, model, ws, s, R, nb, mode, target, kappa, c_f, c_l2, lr, hist_a[s], mk is not None)
            zmax = max(zmax, float(A.logits.abs().max()))
        _init(B, x, labels, mk)
        hist_b = torch.zeros(steps, 5, R, device="cuda")
        win = _lib.GcnNuWindowArgs(
            model=model.handle.value, ws=ws.handle.value, G=R, N=N, mode=mode, use_target=int(mode == 2), target=target, neighbour=nb,
            kappa=kappa, tsign=1.0, c_f=c_f, c_smooth=1e-4, c_l2=c_l2, lr=lr, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, w=B.w.data_ptr(),
            m=B.m.data_ptr(), v=B.v.data_ptr(), mask=B.mask.data_ptr() if mk is not None else None, n_mask=B.n_mask.data_ptr(),
            x0=B.x0.data_ptr(), ori=B.ori.data_ptr(), labels=B.labels.data_ptr(), logits=B.logits.data_ptr(),
            dlogits=B.dlogits.data_ptr(), dx0=B.dx0.data_ptr(), sgrad=B.sgrad.data_ptr(), pred=B.pred.data_ptr(),
            scal=B.scal.data_ptr(), nn_state=B.nn_state.data_ptr(), hist=B.hist.data_ptr(), out=B.out.data_ptr(),
            active=B.active.data_ptr(), exit_step=B.exit.data_ptr())
        for s0, n in ((0, 1), (1, 10), (11, 10), (21, 10)):
            win.step0, win.n_steps, win.adam_t0 = s0, n, s0
            ws.nu_window(win, B.graph if n == 10 else None)
            hist_b[s0:s0 + n].copy_(B.hist[:n])
    side.synchronize()
    stats = _lib.capture_stats(B.graph)
    print(variant, "graph", stats, "exit steps", host(A.exit), host(B.exit))
    assert stats["replays"] >= 1 and stats["captures_failed"] == 0 and stats["captures_tried"] == 1, stats
    for name in ("w", "m", "v", "x0", "pred", "out", "exit", "active", "nn_state", "sgrad", "dx0"):
        assert np.array_equal(bits(host(getattr(A, name))), bits(host(getattr(B, name)))), name
    ha, hb = host(hist_a).astype(np.float64), host(hist_b).astype(np.float64)
    assert np.array_equal(ha[:, :2], hb[:, :2])
    assert (ha[:, 0] > 0).any()
    # a sum of p partials in any order: (p - 1) u sum|partials|; |f| <= 2 max|logit| per point, Smooth and L2 terms are >= 0
    assert (np.abs(ha[:, 2] - hb[:, 2]) <= 2 * 3 * U * N * 2 * zmax).all()
    assert (np.abs(ha[:, 3] - hb[:, 3]) <= 2 * 15 * U * np.abs(ha[:, 3])).all()
    assert (np.abs(ha[:, 4] - hb[:, 4]) <= 2 * 11 * U * np.abs(ha[:, 4])).all()


def test_window_refusals(net):
    from pointsecguard_amd import _lib
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu as gnu
    model, ws = net._packed(), net._workspace(2, N)
    S = gnu._GcnNuState(torch.device("cuda"), 2, N, 5)
    p = S.w.data_ptr()
    base = dict(model=model.handle.value, ws=ws.handle.value, G=2, N=N, mode=0, neighbour=5, n_steps=1, w=p, m=p, v=p, x0=p, ori=p, labels=p,
                logits=p, dlogits=p, dx0=p, sgrad=p, pred=p, scal=p, nn_state=p, hist=p, out=p, active=p, exit_step=p)
    for change in (dict(G=1), dict(N=512), dict(mode=1), dict(mode=3), dict(neighbour=17), dict(n_steps=0), dict(w=None),
                   dict(mode=2, use_target=1, target=13, mask=p, n_mask=p)):
        with pytest.raises(_lib.PsgError):
            ws.nu_window(_lib.GcnNuWindowArgs(**dict(base, **change)))


# ================================================================================= lockstep against rooms alone
def test_lockstep_equals_rooms_alone_with_an_exit_at_step_0(net, rooms3):
    """NU_attack, R = 3: room 1's labels are (clean prediction + 1) % 13, so none of its points is correct and it leaves at step
    0 (n_correct / 4096 < 1 / 13) with its step-0 image while the others run on; every room equals forward_rooms on it alone."""
    ta = _attacks()
    x, labels, pred = rooms3
    labels = labels.copy()
    labels[1] = (pred[1] + 1) % 13
    y = torch.from_numpy(labels).cuda()
    kw = dict(c=0.1, kappa=0, steps=12, lr=0.1)
    adv, n = ta.NU_attack(net, **kw).forward_rooms(x, y)
    print("steps run", n)
    assert n[1] == 1 and n[0] > 1
    # the step-0 image: colours through tanh(atanh(.)) once, everything else the input, and nothing later touched it
    alone = {}
    for r in range(3):
        a, k = ta.NU_attack(net, **kw).forward_rooms(x[r:r + 1], y[r:r + 1])
        alone[r] = host(a)[0]
        assert k[0] == n[r], (r, k, n)
        assert np.array_equal(bits(host(adv)[r]), bits(alone[r])), r
    a1, k1 = ta.NU_attack(net, **dict(kw, steps=1)).forward_rooms(x[1:2], y[1:2])
    assert np.array_equal(bits(host(a1)[0]), bits(host(adv)[1]))
    geo = [0, 1, 2, 6, 7, 8]
    assert np.array_equal(bits(host(adv)[:, geo]), bits(host(x)[:, geo]))


# ========================================================================================= reference fixtures
def _expand(a, mask):
    out = np.zeros((1, 3, N), F)
    if mask is None:
        out[0] = a
    else:
        out[0][:, mask] = a
    return np.ascontiguousarray(out.transpose(0, 2, 1))


@pytest.mark.parametrize("name,nb,tv,steps", [("nu", 10, False, (0, 1, 2)), ("tarnu", 5, True, (0, 20, 22))])
def test_one_step_windows_on_the_recorded_states(net, golden_gcn_nu, golden_gcn_tarnu, name, nb, tv, steps):
    """the bars of test_gpu_resgcn.py::test_gcn_nu_steps_with_reference_graphs, through psg_gcn_nu_window (n_steps = 1, R = 1)
    under the reference's graphs"""
    from pointsecguard_amd import _lib
    from pointsecguard_amd.attacks.torchattacks.attacks.nu import ADAM_EPS, BETA1, BETA2
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu as gnu
    g = golden_gcn_tarnu if tv else golden_gcn_nu
    mask = g["mask"] if tv else None
    model, ws = net._packed(), net._workspace(1, N)
    S = gnu._GcnNuState(torch.device("cuda"), 1, N, nb)
    c = float(g["c"])
    c_f, c_l2 = (c, 1.0) if not tv else (1.0, c)
    x = dev(g["rooms"].transpose(0, 2, 1)[:, :, :, None])
    for t in steps:
        _init(S, x, g["labels"].astype(np.int64), mask[None] if tv else None)
        S.w.copy_(dev(_expand(g["s%d_w_before" % t][0], mask)))
        if t:
            S.m.copy_(dev(_expand(g["s%d_m" % (t - 1)][0], mask)))
            S.v.copy_(dev(_expand(g["s%d_v" % (t - 1)][0], mask)))
        m0 = S.m.clone()
        ws.set_graphs(dev(g["graphs_s%d" % t].astype(np.int32)[:, None]))
        try:
            win = _lib.GcnNuWindowArgs(
                model=model.handle.value, ws=ws.handle.value, step0=t, n_steps=1, G=1, N=N, mode=2 if tv else 0, use_target=int(tv),
                target=int(g["target"]) if tv else 0, neighbour=nb, adam_t0=int(g["s%d_t" % t]) - 1, kappa=float(g["kappa"]), tsign=1.0,
                c_f=c_f, c_smooth=1e-4, c_l2=c_l2, lr=float(g["s%d_lr" % t]), beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, w=S.w.data_ptr(),
                m=S.m.data_ptr(), v=S.v.data_ptr(), mask=S.mask.data_ptr() if tv else None, n_mask=S.n_mask.data_ptr(),
                x0=S.x0.data_ptr(), ori=S.ori.data_ptr(), labels=S.labels.data_ptr(), logits=S.logits.data_ptr(),
                dlogits=S.dlogits.data_ptr(), dx0=S.dx0.data_ptr(), sgrad=S.sgrad.data_ptr(), pred=S.pred.data_ptr(),
                scal=S.scal.data_ptr(), nn_state=S.nn_state.data_ptr(), hist=S.hist.data_ptr(), out=S.out.data_ptr(),
                active=S.active.data_ptr(), exit_step=S.exit.data_ptr())
            ws.nu_window(win)
            torch.cuda.synchronize()
        finally:
            ws.set_graphs(None)
        h = host(S.hist[0]).astype(np.float64)[:, 0]
        cost = c_f * h[2] + 1e-4 * h[3] + c_l2 * h[4]
        sel = slice(None) if mask is None else mask
        grad = host((S.m - m0) / (1.0 - BETA1) + m0).transpose(0, 2, 1)[0][:, sel]
        w_after = host(S.w).transpose(0, 2, 1)[0][:, sel]
        ref = g["s%d_grad" % t][0]
        print(name, t, "cost", cost, g["costs"][t])
        assert abs(cost - g["costs"][t]) <= 1e-4 * abs(g["costs"][t]) + 1e-2, (t, cost, g["costs"][t])
        assert (np.abs(grad - ref) <= 1e-2 * np.abs(ref).max()).mean() >= 0.99, t
        assert (np.abs(w_after - g["s%d_w_after" % t][0]) <= 1e-4).mean() >= 0.99, t


def test_free_running_costs_follow_the_fixtures(net, golden_gcn_nu, golden_gcn_tarnu):
    """what test_gpu_resgcn.py::test_gcn_nu_attack_api asks of the one-room loop, of forward_rooms at R = 1"""
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu as gnu
    ta = _attacks()
    g = golden_gcn_nu
    x, y = dev(g["rooms"].transpose(0, 2, 1)[:, :, :, None]), dev(g["labels"].astype(np.int64))
    atk = ta.NU_attack(net, c=float(g["c"]), kappa=0, steps=int(g["steps"]), lr=float(g["lr"]))
    costs = []
    adv, n = gnu.gcn_nu_attack_rooms(atk, x, y, neighbour=10, trace=lambda **kw: costs.append(float(kw["cost"][0])))
    assert adv.shape == x.shape and n[0] == int(g["n_steps_run"]) and len(costs) == n[0]
    assert np.allclose(costs[:3], g["costs"][:3], rtol=2e-2), (costs[:3], g["costs"][:3])
    assert torch.equal(adv[:, :3], x[:, :3]) and torch.equal(adv[:, 6:], x[:, 6:])
    gt = golden_gcn_tarnu
    xt, yt = dev(gt["rooms"].transpose(0, 2, 1)[:, :, :, None]), dev(gt["labels"].astype(np.int64))
    tatk = ta.tar_NU_attack(net, c=1.0, kappa=0, steps=5, lr=0.1, target=int(gt["target"]), mask=None)
    tcosts = []
    tadv, _ = gnu.gcn_nu_attack_rooms(tatk, xt, yt, masks=gt["mask"][None], target=int(gt["target"]), neighbour=5, targeted_variant=True,
                                      trace=lambda **kw: tcosts.append(float(kw["cost"][0])))
    assert np.allclose(tcosts[:3], gt["costs"][:3], rtol=2e-2), (tcosts[:3], gt["costs"][:3])
    moved = host((tadv[:, 3:6, :, 0] != xt[:, 3:6, :, 0]).any(dim=1)[0])
    assert not moved[~gt["mask"]].any()


# =========================================================================================== tar_NU control flow
def _tar_masks(labels, pred):
    """the untargeted goal on the mask (tcolper.py:121-123): a mask over points the clean network gets right starts at
    accuracy 1 and runs on"""
    return np.stack([(labels[r] == pred[r]) & (np.arange(N) % 2 == 0) for r in range(len(labels))])


def test_tar_nu_past_the_halving(net, rooms3):
    """past step 50 the lr is halved and the moments are zeroed (tcolper.py:125-127): the first step of the new optimiser leaves
    m = (1 - beta1) g and v = (1 - beta2) g^2, i.e. v = 0.1 m^2 element by element; atk.lr is restored on return"""
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu as gnu
    ta = _attacks()
    x, labels, pred = rooms3
    mk = _tar_masks(labels, pred)[:1]
    assert mk.sum() > 50
    atk = ta.tar_NU_attack(net, c=1.0, kappa=1000.0, steps=52, lr=0.002, target=None, mask=None)
    seen = {}

    def rec(step, row, extra, who):
        if row is not None and step in (50, 51):
            S = _state_of(net, 1, 5)
            seen[step] = (host(S.m).astype(np.float64), host(S.v).astype(np.float64))

    adv, n = gnu.gcn_nu_attack_rooms(atk, x[:1], torch.from_numpy(labels[:1]).cuda(), masks=mk, target=None, neighbour=5,
                                     targeted_variant=True, trace=lambda **kw: seen.setdefault(("lr", kw["step"]), atk.lr), record=rec)
    print("steps", n)
    assert n[0] == 52 and atk.lr == 0.002                          # ran past the halving; restored on return
    assert seen[("lr", 50)] == 0.002 and seen[("lr", 51)] == 0.001
    m50, v50 = seen[50]
    m51, v51 = seen[51]
    assert np.abs(m51).max() > 0
    assert np.allclose(v51, 0.1 * m51 ** 2, rtol=1e-4, atol=0)     # (1 - 0.999f) / (1 - 0.9f)^2 = 0.1000046
    assert not np.allclose(v50, 0.1 * m50 ** 2, rtol=1e-2, atol=0)


def test_tar_nu_restart_lockstep_equals_alone_and_rng_parity(net, rooms3):
    """A restart run.  Started from the PointNet test's settings (c = 0, kappa = 1, lr = 3) and adjusted: the learning rate is
    NEGATIVE, which turns Adam's descent into ascent - the cost rises from step to step, so the restart test of
    tcolper.py:129 (`cost >= prev_cost[step - 10]`) fires after step 20 by construction and the accuracy exit cannot (the
    margin grows).  Room 0 runs under a mask over points the clean network gets right; room 1 under a mask over points it
    gets wrong, so it leaves at step 0 and the lockstep call makes ONE draw from the device generator, the draw of the call
    on room 0 alone from the same seed.  Asserted: a restart happened, only the flagged room was touched by it, the
    restarting room's lockstep image equals its alone-run image, and at R = 1 both generators end where `forward` ends."""
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu as gnu
    ta = _attacks()
    x, labels, pred = rooms3
    mk = _tar_masks(labels, pred)[:2]
    mk[1] = (labels[1] != pred[1])
    assert mk[1].sum() > 0 and mk[0].sum() > 50
    y = torch.from_numpy(labels).cuda()
    kw = dict(c=0.0, kappa=1, steps=23, lr=-0.05, target=None)
    events, before = [], {}

    def rec(step, row, extra, who):
        if row is None:
            events.append((step, who.tolist()))
            before[step] = host(_state_of(net, len(who), 5).x0).copy()

    torch.cuda.manual_seed(21)
    atk = ta.tar_NU_attack(net, mask=None, **kw)
    pair, k2 = gnu.gcn_nu_attack_rooms(atk, x[:2].contiguous(), y[:2], masks=mk, target=None, neighbour=5, targeted_variant=True,
                                       record=rec)
    print("restart events", events, "steps", k2)
    assert events == [(20, [True, False])] and k2.tolist() == [23, 1] and atk.lr == -0.05
    S2 = _state_of(net, 2, 5)
    assert np.array_equal(bits(host(S2.x0)[1]), bits(before[20][1]))                 # the room that is not flagged: untouched
    torch.cuda.manual_seed(21)
    n_events = len(events)
    solo, k1 = gnu.gcn_nu_attack_rooms(ta.tar_NU_attack(net, mask=None, **kw), x[:1], y[:1], masks=mk[:1], target=None, neighbour=5,
                                       targeted_variant=True, record=rec)
    assert k1[0] == 23 and events[n_events:] == [(20, [True])]
    assert np.array_equal(bits(host(solo)[0]), bits(host(pair)[0]))
    other, ko = ta.tar_NU_attack(net, mask=None, **kw).forward_rooms(x[1:2], y[1:2], mk[1:2])
    assert ko[0] == 1 and np.array_equal(bits(host(other)[0]), bits(host(pair)[1]))

    def run(rooms_form):                                           # generators: forward_rooms at R = 1 against forward
        torch.manual_seed(5)
        torch.cuda.manual_seed(21)
        a = ta.tar_NU_attack(net, mask=mk[0], **kw)
        out = a.forward_rooms(x[:1], y[:1], mk[:1])[0] if rooms_form else a.forward(x[:1], y[:1])
        return host(out), torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    a, cpu_a, dev_a = run(True)
    b, cpu_b, dev_b = run(False)
    assert torch.equal(cpu_a, cpu_b) and torch.equal(dev_a, dev_b)
    torch.manual_seed(5)
    assert not torch.equal(cpu_a, torch.get_rng_state())           # (the stochastic graphs did draw)
    assert a.shape == b.shape


def test_nu_rng_parity_with_forward(net, rooms3):
    """NU_attack at R = 1: the unused noise draws of colper.py:93-94 and the stochastic-graph draws, with an exit inside a
    window (speculative steps give their draws back)"""
    ta = _attacks()
    x, labels, pred = rooms3
    y = torch.from_numpy(labels).cuda()
    kw = dict(c=5.0, kappa=0, steps=14, lr=0.5)

    def run(rooms_form):
        torch.manual_seed(9); torch.cuda.manual_seed(9)
        atk = ta.NU_attack(net, **kw)
        if rooms_form:
            out, k = atk.forward_rooms(x[:1], y[:1])
        else:
            n = []
            from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks.nu import gcn_nu_attack
            out, k = gcn_nu_attack(atk, x[:1], y[:1], neighbour=10, trace=lambda **kw_: n.append(1)), [None]
            k = [len(n)]
        return host(out), int(k[0]), torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    a, ka, cpu_a, dev_a = run(True)
    b, kb, cpu_b, dev_b = run(False)
    print("NU steps", ka, kb)
    assert ka == kb
    assert torch.equal(cpu_a, cpu_b) and torch.equal(dev_a, dev_b)
