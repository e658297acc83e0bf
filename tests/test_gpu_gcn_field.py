"""GPU tests of the ResGCN coordinate-field attacks (field="coord" | "both") on the 5-block fixture network
and its 1024-point rooms: the fused NB loop and the NU windows against the same entry points driven step by step from here
(state bit for bit), the head graph following the moved points, the coordinate gradient against the reference's own autograd
(golden_gcn_room["dx"]) and the CPU oracle, the control flow of the rooms form, and the Python surface."""
import numpy as np
import pytest
import torch

from test_gpu_gcn_nu_rooms import N, NB, U, _new_net, _tar_masks, bits, dev, host

pytestmark = pytest.mark.gpu
F = np.float32
FIELDS = {"coord": 1, "both": 2}
# coordinates of the fixture rooms lie below 4 m: an fp32 addition there rounds by at most half an ulp of 4, 2^-23; the step
# (add), the difference to the clean point and the projection (add) are three of them, the float32 value of alpha a fourth
ROUND4 = 4 * 2.0 ** -23


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
        pred = torch.cat([net(x[i:i + 1]) for i in range(3)]).argmax(dim=1)
    return x, labels, host(pred).astype(np.int64)


def _attacks():
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks import torchattacks
    return torchattacks


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ==================================================================================================== the fused NB loop
def _hand_nb(model, ws, images, labels, field, eps, alpha, ceps, calpha, iters, keep_xyz=None):
    """psg_gcn_nb_attack_field's launches one at a time through the single entry points"""
    from pointsecguard_amd import _lib, runtime
    P, st = runtime.ptr, runtime.stream
    B = images.shape[0]
    x0 = torch.empty(B, N, 9, device="cuda")
    _lib.call("psg_to_point_major", P(images), B, 9, N, P(x0), st())
    ori, ori_xyz = x0[:, :, 3:6].contiguous(), x0[:, :, 0:3].contiguous()
    dl = torch.empty(B, N, 13, device="cuda")
    for t in range(iters):
        if keep_xyz is not None:
            keep_xyz.append(host(x0[:, :, 0:3]).copy())
        logits = ws.forward(model, x0)
        _lib.call("psg_ce_logp_grad", P(logits), P(labels), 0, B * N, B * N, 13, 1.0 / (B * N), P(dl), None, st())
        dx0 = ws.backward(model, dl)
        last = 1 if t == iters - 1 else 0
        _lib.call("psg_pgd_step_field", P(x0), P(dx0), P(ori_xyz), None, B, N, 0, calpha, ceps, 1.0, last, st())
        if field == "both":
            _lib.call("psg_pgd_step_field", P(x0), P(dx0), P(ori), None, B, N, 3, alpha, eps, 1.0, last, st())
    out = torch.empty(B, 9, N, device="cuda")
    _lib.call("psg_to_channel_major", P(x0), B, 9, N, P(out), st())
    return out


@pytest.mark.parametrize("field", ["coord", "both"])
def test_fused_nb_field_equals_hand_driven_iterations_and_replays_a_graph(net, golden_gcn_nb, field):
    """iters = 6 on a side stream: first iteration eager, one capture, four replays, last eager - the state the same entry points
    leave when they are called one by one, bit for bit; a second call re-uses the graph, another coord_alpha captures anew."""
    from pointsecguard_amd import _lib
    g = golden_gcn_nb
    images = dev(np.ascontiguousarray(g["rooms"].transpose(0, 2, 1)))
    labels = dev(g["labels"].astype(np.int32))
    model, ws = net._packed(), net._workspace(1, N)
    eps, alpha, ceps, calpha, iters = 0.05, 2 / 255, 0.01, 0.004, 6
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        hand = _hand_nb(model, ws, images, labels, field, eps, alpha, ceps, calpha, iters)
        s0 = _lib.capture_stats()
        a1 = ws.nb_attack_field(model, images, labels, FIELDS[field], eps, alpha, ceps, calpha, iters).clone()
        s1 = _lib.capture_stats()
        a2 = ws.nb_attack_field(model, images, labels, FIELDS[field], eps, alpha, ceps, calpha, iters).clone()
        s2 = _lib.capture_stats()
        a3 = ws.nb_attack_field(model, images, labels, FIELDS[field], eps, alpha, ceps, calpha * 0.5, iters).clone()
        s3 = _lib.capture_stats()
        hand3 = _hand_nb(model, ws, images, labels, field, eps, alpha, ceps, calpha * 0.5, iters)
    side.synchronize()
    d = lambda a, b, k: b[k] - a[k]                                       # noqa: E731
    print(field, "capture stats", s0, s1, s2, s3)
    assert d(s0, s1, "captures_tried") == 1 and d(s0, s1, "captures_failed") == 0 and d(s0, s1, "replays") == iters - 2
    assert d(s1, s2, "captures_tried") == 0 and d(s1, s2, "replays") == iters - 2                # the graph is re-used
    assert d(s2, s3, "captures_tried") == 1 and d(s2, s3, "captures_failed") == 0                # another coord_alpha: a new one
    assert same_bits(host(a1), host(hand)) and same_bits(host(a2), host(hand)) and same_bits(host(a3), host(hand3))
    # field invariants
    out, src = host(a1).astype(np.float64), host(images).astype(np.float64)
    assert same_bits(host(a1)[:, 6:9], host(images)[:, 6:9])
    if field == "coord":
        assert same_bits(host(a1)[:, 3:9], host(images)[:, 3:9])
    else:
        assert (out[:, 3:6] != src[:, 3:6]).mean() > 0.5 and out[:, 3:6].min() >= -alpha - ROUND4 and out[:, 3:6].max() <= 1 + alpha + ROUND4
    moved = out[:, 0:3] - src[:, 0:3]
    assert (moved != 0).mean() > 0.5
    assert np.abs(moved).max() <= ceps + calpha + ROUND4                  # the un-projected last step from a projected point
    assert src[:, 0:2].min() < -0.4 and (out[:, 0:2].min() < 0) and out[:, 2].max() > 1.5     # metres: no [0, 1] clamp


def test_nb_field_whole_sign_steps_and_refusals(net, golden_gcn_nb):
    from pointsecguard_amd import _lib
    g = golden_gcn_nb
    images = dev(np.ascontiguousarray(g["rooms"].transpose(0, 2, 1)))
    labels = dev(g["labels"].astype(np.int32))
    model, ws = net._packed(), net._workspace(1, N)
    calpha, iters = 1.0 / 256, 3                                          # (a power of two: the steps add up exactly)
    adv = ws.nb_attack_field(model, images, labels, 1, 0.3, 0.01, 0.5, calpha, iters)
    steps = (host(adv).astype(np.float64)[:, 0:3] - host(images).astype(np.float64)[:, 0:3]) / calpha
    assert np.abs(steps - np.round(steps)).max() <= iters * ROUND4 / calpha and np.abs(np.round(steps)).max() <= iters
    assert (steps != 0).mean() > 0.5
    for bad in (dict(field=0), dict(field=3), dict(iters=0)):
        kw = dict(dict(field=1, iters=2), **bad)
        with pytest.raises(_lib.PsgError):
            ws.nb_attack_field(model, images, labels, kw["field"], 0.3, 0.01, 0.3, 0.01, kw["iters"])
    with pytest.raises(_lib.PsgError):
        _lib.call("psg_gcn_nb_attack_field", model.handle, ws.handle, None, None, 1, 0.3, 0.01, 0.3, 0.01, 2, None, None)


def test_head_graph_follows_the_moved_points(net, golden_gcn_nb):
    """after three hand-driven iterations the head's graph is the kNN graph of the xyz that entered the LAST forward, not the
    clean room's - a frozen head graph (the colour loop's shortcut) fails here"""
    from oracle import resgcn
    g = golden_gcn_nb
    images = dev(np.ascontiguousarray(g["rooms"].transpose(0, 2, 1)))
    labels = dev(g["labels"].astype(np.int32))
    model, ws = net._packed(), net._workspace(1, N)
    seen = []
    _hand_nb(model, ws, images, labels, "coord", 0.0, 0.0, 0.1, 0.02, 3, keep_xyz=seen)
    torch.cuda.synchronize()
    got = host(ws.edges(0))[0]
    assert np.array_equal(got, resgcn.knn_dilated(np.ascontiguousarray(seen[-1][0]), 1))
    clean = resgcn.knn_dilated(np.ascontiguousarray(seen[0][0]), 1)
    assert (got != clean).mean() > 0.05
    # the fused loop rebuilds it too: its last forward saw the same points
    ws.nb_attack_field(model, images, labels, 1, 0.0, 0.0, 0.1, 0.02, 3)
    torch.cuda.synchronize()
    assert np.array_equal(host(ws.edges(0))[0], got)


# =============================================================================== the gradient, the reference's graphs forced
def test_coordinate_gradient_sign_against_the_reference_autograd(net, golden_gcn_room):
    """dx0[:, 0:3] against golden_gcn_room["dx"] (the reference's autograd for a leaf on the whole input): the colour
    channels' bar of tests/test_gpu_resgcn.py::test_forward_backward_with_reference_graphs, on channels 0:3"""
    from pointsecguard_amd import _lib, runtime
    g = golden_gcn_room
    model, ws = net._packed(), net._workspace(1, N)
    ws.set_graphs(dev(np.stack([g["nbr%d" % e].astype(np.int32)[None] for e in range(NB)])))
    try:
        logits = ws.forward(model, dev(g["room"][None]))
        dl = torch.empty_like(logits)
        _lib.call("psg_ce_logp_grad", runtime.ptr(logits), runtime.ptr(dev(g["labels"].astype(np.int32)[None])), 0, N, N, 13, 1.0 / N,
                  runtime.ptr(dl), None, runtime.stream())
        dx = host(ws.backward(model, dl))[0]
    finally:
        ws.set_graphs(None)
    ref = g["dx"]
    agree = float((np.sign(dx[:, 0:3]) == np.sign(ref[:, 0:3])).mean())
    print("sign agreement on channels 0:3: %.5f" % agree)
    assert agree >= 0.999
    assert np.abs(dx[:, 0:3] - ref[:, 0:3]).max() <= 1e-3 * np.abs(ref).max() + 1e-6


def test_teacher_forced_coordinate_step_against_the_oracle(net, gcn_oracle, golden_gcn_nb):
    """one coordinate step under the reference's graphs: GCNOracle.forward / backward + the numpy field step, >= 99.9 % bit-equal"""
    from oracle import resgcn
    from pointsecguard_amd import _lib, runtime
    P, st = runtime.ptr, runtime.stream
    g = golden_gcn_nb
    model, ws = net._packed(), net._workspace(1, N)
    graphs = g["graphs_it0"].astype(np.int32)
    room, labels = g["rooms"][0], g["labels"][0].astype(np.int64)
    calpha, ceps = F(0.004), F(0.01)
    logits, cache = gcn_oracle.forward(room, graphs=[graphs[e] for e in range(NB)])
    dl, _ = resgcn.ce_mean_grad(logits, labels)
    gx = gcn_oracle.backward(cache, dl)[:, 0:3]
    ori = room[:, 0:3]
    stepped = (ori + calpha * np.sign(gx).astype(F)).astype(F)
    want = (ori + np.clip((stepped - ori).astype(F), -ceps, ceps)).astype(F)
    ws.set_graphs(dev(graphs[:, None]))
    try:
        x0 = dev(room[None])
        ori_d = x0[:, :, 0:3].contiguous()
        lg = ws.forward(model, x0)
        dlg = torch.empty_like(lg)
        _lib.call("psg_ce_logp_grad", P(lg), P(dev(labels.astype(np.int32)[None])), 0, N, N, 13, 1.0 / N, P(dlg), None, st())
        dx0 = ws.backward(model, dlg)
        _lib.call("psg_pgd_step_field", P(x0), P(dx0), P(ori_d), None, 1, N, 0, float(calpha), float(ceps), 1.0, 0, st())
        got = host(x0)[0]
    finally:
        ws.set_graphs(None)
    same = float((np.ascontiguousarray(got[:, 0:3]).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)).mean())
    print("teacher-forced coordinate step: bit-equal fraction %.5f" % same)
    assert same >= 0.999
    assert same_bits(got[:, 3:9], room[:, 3:9])


# ======================================================================================= NU windows against hand-driven steps
def _field_mod():
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu_field
    return nu_field


def _hand_step(S, model, ws, step, adam_t, R, nb, field, mode, target, kappa, c_f, c_l2, c_l2x, lr, coord_lr, hist_row, masked):
    """one optimiser step through the per-operation entry points, in the window's order; step constants by value"""
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.attacks.torchattacks.attacks.nu import ADAM_EPS, BETA1, BETA2, ctypes_off
    P, st = runtime.ptr, runtime.stream
    mk = P(S.mask) if masked else None
    both = field == "both"
    _lib.call("psg_nu_coord_apply_rooms", P(S.delta), P(S.ori_xyz), mk, R, N, P(S.active), P(S.x0), st())
    if both:
        _lib.call("psg_nu_tanh_color_rooms", P(S.w), mk, R, N, P(S.x0), st())
    ws.forward(model, S.x0, S.logits)
    _lib.call("psg_gcn_f_loss_grad_rooms", P(S.logits), P(S.labels), target, mk, mode, R, N, 13, kappa, 1.0, c_f, P(S.dlogits),
              P(S.scal[0]), P(S.pred), st())
    ws.backward(model, S.dlogits, S.dx0)
    if both:
        _lib.call("psg_smooth_knn_sym_rooms", ctypes_off(S.x0, 3), 9, N * 9, R, N, nb, P(S.scal[1]), P(S.sgrad), P(S.active),
                  P(S.nn_state), st())
    _lib.call("psg_smooth_knn_xyz_sym_rooms", P(S.x0), 9, N * 9, R, N, nb, P(S.scal[3]), P(S.sgrad_xyz), P(S.active), P(S.nn_xyz), st())
    if both:
        _lib.call("psg_nu_adam_step_rooms", P(S.w), P(S.m), P(S.v), mk, P(S.dx0), P(S.x0), P(S.ori), P(S.sgrad), 1e-4, c_l2, lr, BETA1,
                  BETA2, ADAM_EPS, adam_t, R, N, P(S.active), P(S.scal[2]), st())
    _lib.call("psg_nu_coord_adam_step_rooms_w", P(S.delta), P(S.mx), P(S.vx), mk, P(S.dx0), P(S.sgrad_xyz), 1e-4, c_l2x, coord_lr, BETA1,
              BETA2, ADAM_EPS, adam_t, R, N, P(S.active), P(S.scal[4]), st())
    _lib.call("psg_nu_step_latch", P(S.pred), P(S.labels), target, mk if mode else None, P(S.n_mask) if mode else None, R, 1, N, mode,
              P(S.scal), P(hist_row), P(S.x0), P(S.out), P(S.active), P(S.exit), step, st())
    hist_row[5:7] = S.scal[3:5]
    S.scal[3:5] = 0


def _fresh(F_, x, labels, mk, R, nb, field):
    S = F_._GcnFieldState(x.device, R, N, nb)
    F_.init_state(S, x[:, :, :, 0].contiguous(), torch.from_numpy(labels), mk, field == "both")
    S.out.zero_(); S.pred.fill_(-1); S.nn_state.fill_(-1); S.nn_xyz.fill_(-1)
    S.sgrad_xyz.zero_(); S.sgrad.zero_(); S.dx0.zero_()
    return S


@pytest.mark.parametrize("field", ["coord", "both"])
@pytest.mark.parametrize("variant", ["nu", "tarnu"])
def test_field_windows_equal_hand_driven_steps(net, rooms3, variant, field):
    """31 steps at R = 2: the windows [0], [1..10] (eager), [11..20] (captured), [21..30] (replayed) - their Adam steps and
    latch read the step constants from the device rows - against the same entry points called step by step from here with
    the constants by value; state and integer history bit for bit, the float sums to the rounding of their atomic partials
    (f: 4 workgroup partials; Smooth: one per wave, 256 on colours, 128 on coordinates; L2: 12 per room)."""
    from pointsecguard_amd import _lib
    F_ = _field_mod()
    x, labels, _ = rooms3
    R, steps, lr, coord_lr, kappa = 2, 31, 0.05, 0.004, 0.0
    x, labels = x[:R].contiguous(), labels[:R]
    if variant == "nu":
        nb, mode, target, c_f, c_l2, c_l2x, mk = 10, 0, 0, 0.1, 1.0, 1.0, None
    else:
        nb, mode, target, c_f, c_l2, c_l2x = 5, 2, 6, 1.0, 0.5, 0.25
        mk = np.zeros((R, N), bool)
        mk[0, ::3] = True
        mk[1, 1::2] = True
    model, ws = net._packed(), net._workspace(R, N)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        A = _fresh(F_, x, labels, mk, R, nb, field)
        hist_a = torch.zeros(steps, 7, R, device="cuda")
        zmax = 0.0
        for s in range(steps):
            _hand_step(A, model, ws, s, s + 1, R, nb, field, mode, target, kappa, c_f, c_l2, c_l2x, lr, coord_lr, hist_a[s], mk is not None)
            zmax = max(zmax, float(A.logits.abs().max()))
        B = _fresh(F_, x, labels, mk, R, nb, field)
        hist_b = torch.zeros(steps, 7, R, device="cuda")
        win = F_.window_args(B, model, ws, R, N, field, mode, mode == 2, target, nb, kappa, 1.0, c_f, c_l2, c_l2x, mk is not None)
        for s0, n in ((0, 1), (1, 10), (11, 10), (21, 10)):
            win.step0, win.n_steps, win.adam_t0, win.lr, win.coord_lr = s0, n, s0, lr, coord_lr
            ws.nu_field_window(win, B.graph if n == 10 else None)
            hist_b[s0:s0 + n].copy_(B.hist[:n])
    side.synchronize()
    stats = _lib.capture_stats(B.graph)
    print(variant, field, "graph", stats, "exit steps", host(A.exit), host(B.exit))
    assert stats["replays"] >= 1 and stats["captures_failed"] == 0 and stats["captures_tried"] == 1, stats
    names = ["delta", "mx", "vx", "x0", "pred", "out", "exit", "active", "nn_xyz", "sgrad_xyz", "dx0"]
    if field == "both":
        names += ["w", "m", "v", "nn_state", "sgrad"]
    for name in names:
        assert same_bits(host(getattr(A, name)), host(getattr(B, name))), name
    assert float(A.delta.abs().max()) > 0 and same_bits(host(A.scal), np.zeros((5, R), F))
    on = mk if mk is not None else np.ones((R, N), bool)
    assert (host(A.delta)[~on] == 0).all()
    ha, hb = host(hist_a).astype(np.float64), host(hist_b).astype(np.float64)
    assert np.array_equal(ha[:, :2], hb[:, :2])
    ex = host(A.exit).astype(np.int64)
    live = (ex[None] < 0) | (ex[None] >= np.arange(steps)[:, None])      # [step][room]: the room's loop was still running
    assert (ha[:, 0] > 0).any() and live[:11].all()
    assert (ha[1:, 6][live[1:]] > 0).all() and (ha[0, 6] == 0).all() and (ha[:, 5][live] > 0).all()
    assert (ha[:, 3][live] > 0).all() if field == "both" else (ha[:, 3:5] == 0).all()
    # a sum of p partials in any order: (p - 1) u sum|partials|; |f| <= 2 max|logit| per point, the other terms are >= 0
    assert (np.abs(ha[:, 2] - hb[:, 2]) <= 2 * 3 * U * N * 2 * zmax).all()
    assert (np.abs(ha[:, 3] - hb[:, 3]) <= 2 * 255 * U * np.abs(ha[:, 3])).all()
    assert (np.abs(ha[:, 4] - hb[:, 4]) <= 2 * 11 * U * np.abs(ha[:, 4])).all()
    assert (np.abs(ha[:, 5] - hb[:, 5]) <= 2 * 127 * U * np.abs(ha[:, 5])).all()
    assert (np.abs(ha[:, 6] - hb[:, 6]) <= 2 * 11 * U * np.abs(ha[:, 6])).all()


def test_field_window_refusals(net):
    from pointsecguard_amd import _lib
    F_ = _field_mod()
    model, ws = net._packed(), net._workspace(2, N)
    S = F_._GcnFieldState(torch.device("cuda"), 2, N, 5)
    p = S.w.data_ptr()
    base = dict(model=model.handle.value, ws=ws.handle.value, G=2, N=N, mode=0, neighbour=5, n_steps=1, field=1, delta=p, mx=p, vx=p, ori_xyz=p,
                x0=p, labels=p, logits=p, dlogits=p, dx0=p, sgrad_xyz=p, nn_xyz=p, pred=p, scal=p, hist=p, out=p, active=p, exit_step=p)
    for change in (dict(field=0), dict(field=3), dict(field=2), dict(G=1), dict(N=512), dict(mode=1), dict(mode=3), dict(neighbour=17),
                   dict(n_steps=0), dict(delta=None), dict(nn_xyz=None), dict(ori_xyz=None), dict(sgrad_xyz=None),
                   dict(mode=2, use_target=1, target=13, mask=p, n_mask=p)):
        with pytest.raises(_lib.PsgError):
            ws.nu_field_window(_lib.GcnNuFieldWindowArgs(**dict(base, **change)))


# ================================================================================================= the rooms form
def test_lockstep_equals_rooms_alone_exits_and_generators(net, rooms3):
    """NU_attack(field="coord"), R = 3.  Room 1's labels are (clean prediction + 1) % 13: it leaves at step 0 with the clean room.
    Room 2's labels agree with the clean prediction on 330 points only: 330 / 4096 is just above 1 / 13, so the attack pushes it
    out at a later step - whose snapshot is ori_xyz + delta of THAT step.  Every room equals the call on it alone; the CPU
    generator ends where the same number of forwards alone leaves it and the device generator is not touched."""
    ta = _attacks()
    F_ = _field_mod()
    x, labels, pred = rooms3
    labels = labels.copy()
    labels[1] = (pred[1] + 1) % 13
    labels[2] = (pred[2] + 1) % 13
    labels[2, :330] = pred[2, :330]
    y = torch.from_numpy(labels).cuda()
    kw = dict(c=50.0, kappa=0, steps=25, lr=0.01, field="coord", coord_lr=0.02)
    torch.manual_seed(11)
    torch.cuda.manual_seed(12)
    dev_before = torch.cuda.get_rng_state().clone()
    adv, n = ta.NU_attack(net, **kw).forward_rooms(x, y)
    cpu_after = torch.get_rng_state().clone()
    print("steps run", n)
    assert n[1] == 1 and n[0] > 1 and 1 < n[2] < 25
    assert torch.equal(torch.cuda.get_rng_state(), dev_before)            # no noise draw, no restart draw
    torch.manual_seed(11)
    net.consume_rng(int(n.max()))
    assert torch.equal(torch.get_rng_state(), cpu_after)
    assert same_bits(host(adv)[1], host(x)[1])                            # the exit at step 0 returns the clean room
    assert same_bits(host(adv)[:, 3:9], host(x)[:, 3:9])
    for r in range(3):
        a, k = ta.NU_attack(net, **kw).forward_rooms(x[r:r + 1], y[r:r + 1])
        assert k[0] == n[r], (r, k, n)
        assert same_bits(host(adv)[r], host(a)[0]), r
    one = ta.NU_attack(net, **kw).forward(x[0:1], y[0:1])
    assert same_bits(host(one)[0], host(adv)[0])
    with pytest.raises(ValueError, match="forward_rooms"):
        ta.NU_attack(net, **kw).forward(x, y)
    # the later exit: one-step windows (trace), the state after every step
    seen = {}

    def trace(**t):
        S = t["S"]
        seen[t["step"]] = (host(S.delta).copy(), host(S.x0).copy(), host(S.ori_xyz).copy())

    a2, k2 = F_.gcn_nu_field_attack_rooms(ta.NU_attack(net, **kw), x[2:3], y[2:3], neighbour=10, trace=trace)
    s = int(k2[0]) - 1
    assert k2[0] == n[2] and same_bits(host(a2)[0], host(adv)[2])
    delta_in, (_, x0_s, ori_xyz) = seen[s - 1][0], seen[s]
    assert np.abs(delta_in).max() > 0
    assert same_bits(x0_s[0, :, 0:3], (ori_xyz[0] + delta_in[0]).astype(F))
    assert same_bits(host(a2)[0, :, :, 0], np.ascontiguousarray(x0_s[0].T))


def test_tar_nu_field_past_the_halving(net, rooms3):
    """52 steps of tar_NU_attack(field="both"): after step 50 both learning rates are halved and all moments zeroed, so step 51
    leaves m = (1 - beta1) g and v = (1 - beta2) g^2, v = 0.1 m^2 element by element, on both variables; lr and coord_lr are
    restored on return"""
    ta = _attacks()
    F_ = _field_mod()
    x, labels, pred = rooms3
    mk = _tar_masks(labels, pred)[:1]
    assert mk.sum() > 50
    atk = ta.tar_NU_attack(net, c=1.0, kappa=1000.0, steps=52, lr=0.002, target=None, mask=None, field="both", coord_c=0.5, coord_lr=0.001)
    seen = {}

    def rec(step, row, was_active):
        if step in (50, 51):
            S = next(s for k, s in net._psg_gcn_nu_field_states.items() if k[1] == 1 and k[3] == 5 and k[4] == "both")
            seen[step] = dict(lr=atk.lr, coord_lr=atk.coord_lr, **{k: host(getattr(S, k)).astype(np.float64) for k in ("m", "v", "mx", "vx")})

    adv, n = F_.gcn_nu_field_attack_rooms(atk, x[:1], torch.from_numpy(labels[:1]).cuda(), masks=mk, target=None, neighbour=5,
                                          targeted_variant=True, record=rec)
    assert n[0] == 52 and atk.lr == 0.002 and atk.coord_lr == 0.001
    assert (seen[50]["lr"], seen[50]["coord_lr"]) == (0.002, 0.001) and (seen[51]["lr"], seen[51]["coord_lr"]) == (0.001, 0.0005)
    for m_, v_ in (("m", "v"), ("mx", "vx")):
        assert np.abs(seen[51][m_]).max() > 0
        assert np.allclose(seen[51][v_], 0.1 * seen[51][m_] ** 2, rtol=1e-4, atol=0)
        assert not np.allclose(seen[50][v_], 0.1 * seen[50][m_] ** 2, rtol=1e-2, atol=0)
    moved = host(adv)[0, :, :, 0] != host(x)[0, :, :, 0]
    assert moved[0:6].any() and not moved[6:9].any() and not moved[:, ~mk[0]].any()


# ================================================================================================= the Python surface
@pytest.mark.parametrize("field", ["coord", "both"])
def test_python_surface_of_the_four_attacks(net, rooms3, field):
    ta = _attacks()
    x, labels, pred = rooms3
    x1, y1 = x[:1], torch.from_numpy(labels[:1]).cuda()
    mk = _tar_masks(labels, pred)[0]
    src = host(x1)[0, :, :, 0]
    chans = slice(0, 3) if field == "coord" else slice(0, 6)
    outs = {
        "NB": ta.NB_attack(net, eps=0.05, alpha=0.01, iters=3, field=field, coord_eps=0.02, coord_alpha=0.005)(x1, y1),
        "NB atype": ta.NB_attack(net, eps=0.05, alpha=0.01, iters=3, coord_eps=0.02, coord_alpha=0.005).forward(x1, y1, atype=field.capitalize()),
        "tar_NB": ta.tar_NB_attack(net, eps=0.05, alpha=0.01, iters=3, target=6, mask=mk, field=field, coord_eps=0.02, coord_alpha=0.005)(x1, y1),
        "NU": ta.NU_attack(net, c=0.1, steps=3, lr=0.01, field=field, coord_lr=0.005)(x1, y1),
        "tar_NU": ta.tar_NU_attack(net, c=1.0, kappa=1000.0, steps=3, lr=0.01, target=None, mask=mk, field=field, coord_lr=0.005)(x1, y1),
    }
    assert same_bits(host(outs["NB"]), host(outs["NB atype"]))
    for name, adv in outs.items():
        got = host(adv)[0, :, :, 0]
        assert adv.shape == x1.shape, name
        moved = got != src
        assert moved[chans].any() and not moved[chans.stop:].any(), name
        if name.startswith("tar"):
            assert not moved[:, ~mk].any(), name
    nbm = np.abs(host(outs["tar_NB"])[0, 0:3, :, 0] - src[0:3])
    assert nbm.max() <= 0.015 + 3 * ROUND4                               # three projected steps of 0.005, coord_eps 0.02


def test_field_color_is_the_untouched_colour_path(net, rooms3):
    """field="color" (spelled out or by default) returns the bytes of the colour entry points that this feature left alone"""
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu as gnu
    ta = _attacks()
    x, labels, pred = rooms3
    x1, y1 = x[:1], torch.from_numpy(labels[:1]).cuda()
    mk = _tar_masks(labels, pred)[:1]
    a = ta.NB_attack(net, eps=0.05, alpha=0.01, iters=4, field="color")(x1, y1)
    b = net._workspace(1, N).nb_attack(net._packed(), x1[:, :, :, 0].contiguous(), y1.to(torch.int32), 0.05, 0.01, 4)
    assert same_bits(host(a)[:, :, :, 0], host(b))
    a, na = ta.NU_attack(net, c=0.1, steps=4, lr=0.05, field="color").forward_rooms(x1, y1)
    b, nb_ = gnu.gcn_nu_attack_rooms(ta.NU_attack(net, c=0.1, steps=4, lr=0.05), x1, y1, neighbour=10)
    assert same_bits(host(a), host(b)) and list(na) == list(nb_)
    a, na = ta.tar_NU_attack(net, c=1.0, kappa=1000.0, steps=4, lr=0.05, field="color").forward_rooms(x1, y1, mk)
    b, nb_ = gnu.gcn_nu_attack_rooms(ta.tar_NU_attack(net, c=1.0, kappa=1000.0, steps=4, lr=0.05), x1, y1, masks=mk, target=None,
                                     neighbour=5, targeted_variant=True)
    assert same_bits(host(a), host(b)) and list(na) == list(nb_)
    a = ta.tar_NB_attack(net, eps=0.05, alpha=0.01, iters=3, target=6, mask=mk[0], field="color")(x1, y1)
    from pointsecguard_amd import _lib, runtime
    P, st = runtime.ptr, runtime.stream
    model, ws = net._packed(), net._workspace(1, N)
    x0 = torch.empty(1, N, 9, device="cuda")
    _lib.call("psg_to_point_major", P(x1[:, :, :, 0].contiguous()), 1, 9, N, P(x0), st())
    ori, mask_d, dl = x0[:, :, 3:6].contiguous(), dev(mk[0].astype(np.uint8)), torch.empty(1, N, 13, device="cuda")
    for _ in range(3):
        logits = ws.forward(model, x0)
        assert float((logits.argmax(dim=2)[:, dev(mk[0])] == 6).float().mean()) <= 0.9
        _lib.call("psg_ce_logp_grad", P(logits), None, 6, N, N, 13, 1.0 / N, P(dl), None, st())
        dx0 = ws.backward(model, dl)
        _lib.call("psg_pgd_step", P(x0), P(dx0), P(ori), P(mask_d), 1, N, 0.01, 0.05, -1.0, 0, st())
    assert same_bits(host(a)[0, :, :, 0], np.ascontiguousarray(host(x0)[0].T))
