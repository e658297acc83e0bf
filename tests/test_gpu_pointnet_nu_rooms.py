"""GPU tests of the NU attacks on the vanilla PointNet through device-side windows: `forward` (one attack on a batch) and
`forward_rooms` (one-room attacks in lockstep) against the retained per-step loop, against one call per room, against the
reference's recorded runs (tests/golden/pointnet_{nu,tarnu}.npz), and the two kernels that belong to the feature
(pn_nu_head_kernel through psg_pointnet_nu_head, psg_nu_restart_rooms) on their own.

Images, exit steps and step counts are compared as bit patterns: the kernels and their order are the same on both sides.
The per-step scalar rows {f, Smooth, L2} are sums the kernels finish with float atomics ("Reproducibility"), so
they get rtol = 1e-5, the bar tests/test_gpu_nu.py uses for per-room costs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PN_SEED, ROOM_SEED = 3, 5
N = 4096


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name))


def _new_net():
    from pointsecguard_amd import synthetic
    from pointsecguard_amd.models.pointnet_sem_seg import get_model
    m = get_model(13)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.pointnet_state_dict(PN_SEED).items()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def net():
    return _new_net()


@pytest.fixture(scope="module")
def rooms4():
    from pointsecguard_amd import synthetic
    r = synthetic.make_rooms(4, ROOM_SEED)           # (rooms 0 and 1 are the two rooms of the recorded fixtures)
    return r, synthetic.rule_labels(r)


def _x(r):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(r).transpose(0, 2, 1))).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _clean_pred(net, x):
    with torch.no_grad():
        logp, _ = net(x)
    return logp.argmax(dim=2).cpu().numpy()


def _masks_with_an_early_exit(net, x, labels):
    """tar_NU_attack without a target (the untargeted goal on the mask, target.py:119-121: leave when fewer than 1 / 13 of the
    masked points are still correct).  The synthetic weights predict ONE class for every point, so a mask over the points
    that carry that class as their label starts at accuracy 1 and runs on, and a mask over the other points starts at
    accuracy 0 and leaves at step 0: the last room gets the second kind."""
    pred = _clean_pred(net, x)
    cls = int(np.bincount(pred.ravel()).argmax())
    assert (pred == cls).all()
    masks = labels == cls
    early = x.shape[0] - 1
    masks[early] = ~masks[early]
    return masks, early


def test_forward_rooms_runs_on_pointnet(net, rooms4):
    from pointsecguard_amd.attacks import torchattacks
    x, labels = _x(rooms4[0]), rooms4[1].astype(np.float64)
    adv, n = torchattacks.NU_attack(net, c=0.1, kappa=0, steps=3, lr=0.01).forward_rooms(x, labels)
    assert tuple(adv.shape) == (4, 9, N) and len(n) == 4
    masks = np.zeros((4, N), bool)
    masks[:, ::4] = True
    atk = torchattacks.tar_NU_attack(net, c=0.1, kappa=0, steps=3, lr=0.01, target=4, mask=None)
    adv, n = atk.forward_rooms(x, labels, masks)
    assert tuple(adv.shape) == (4, 9, N) and len(n) == 4
    assert atk.lr == 0.01
    assert np.array_equal(adv[:, 3:6].cpu().numpy()[~np.repeat(masks[:, None], 3, 1)], x[:, 3:6].cpu().numpy()[~np.repeat(masks[:, None], 3, 1)])


def test_lockstep_equals_one_call_per_room_through_restart_and_halving(net, rooms4):
    """The recorded tar_NU settings (c = 0, kappa = 1, lr = 3: the cost stops falling, so restarts run) on the untargeted goal,
    extended past the step-50 halving; one room's mask makes it leave at step 0.  (With a target class these weights give no
    room that leaves early: they predict one class everywhere.)

    The restart noise comes from the device generator, room by room in ascending order at the step it happens.  One call per
    room draws room r's blocks one after the other instead, so from ONE seeding the two sides see the same numbers exactly
    when a single room of the lockstep call draws: (a) every restarting room r in lockstep with the early-exit room, seeded
    like the call on r alone - images and step counts bit for bit; (b) all four rooms in lockstep, where three rooms draw at
    the same steps - step counts, and every channel the noise does not reach (the clamped coordinates and normals), bit for bit."""
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.attacks.torchattacks.attacks import nu as nu_mod
    x, labels = _x(rooms4[0]), rooms4[1].astype(np.float64)
    target, steps = None, 62
    masks, early = _masks_with_an_early_exit(net, x, rooms4[1])
    kw = dict(c=0.0, kappa=1, steps=steps, lr=3.0, target=target)

    def restart_log(into):
        def rec(step, row, extra, who):                      # (row is None: the attacks `who` restart after `step`)
            if row is None:
                into.extend((int(g), step) for g in np.nonzero(who)[0])
        return rec

    single, single_n, single_restarts = {}, {}, {}
    for r in range(4):
        torch.cuda.manual_seed(100 + r)
        a = torchattacks.tar_NU_attack(net, mask=masks[r], **kw)
        log = []
        out, k = nu_mod.nu_attack(a, x[r:r + 1], labels[r:r + 1], masks[r], target, 5, targeted_variant=True, return_steps=True,
                                  record=restart_log(log))
        single[r], single_n[r], single_restarts[r] = out.cpu().numpy()[0], k, [s for _, s in log]
        assert a.lr == 3.0 / 2 ** ((k - 1) // 50), (r, k, a.lr)          # forward leaves the halved lr on the object (target.py:123-125)
    print("steps per room", single_n, "restarts after steps", single_restarts)
    assert single_n[early] == 1 and max(single_n.values()) > 51          # different exit steps; the halving after step 50 was taken
    assert any(single_restarts[r] for r in range(4))
    for r in range(4):                                                   # (a)
        if r == early:
            continue
        pair = [r, early]
        torch.cuda.manual_seed(100 + r)
        a = torchattacks.tar_NU_attack(net, mask=None, **kw)
        out, k = a.forward_rooms(x[pair].contiguous(), labels[pair], masks[pair])
        out = out.cpu().numpy()
        assert a.lr == 3.0                                               # lockstep rooms are fresh objects: lr restored
        assert k[0] == single_n[r] and k[1] == 1, (r, k, single_n[r])
        assert np.array_equal(_bits(out[0]), _bits(single[r])), r
        assert np.array_equal(_bits(out[1]), _bits(single[early])), r
    torch.cuda.manual_seed(11)                                           # (b)
    atk = torchattacks.tar_NU_attack(net, mask=None, **kw)
    log = []
    adv, n = nu_mod.nu_attack_rooms(atk, x, labels, masks, target, 5, targeted_variant=True, record=restart_log(log))
    adv = adv.cpu().numpy()
    assert n[early] == 1 and np.array_equal(_bits(adv[early]), _bits(single[early]))
    geo = [0, 1, 2, 6, 7, 8]
    for r in range(4):
        # whether a room restarts at all is decided before any noise reaches it, and the clamp is idempotent
        assert bool(single_restarts[r]) == any(g == r for g, _ in log), (r, single_restarts[r], log)
        assert np.array_equal(_bits(single[r][geo]), _bits(adv[r][geo])), r
        assert np.array_equal(_bits(adv[r][3:6][:, ~masks[r]]), _bits(single[r][3:6][:, ~masks[r]])), r


def test_nu_lockstep_rooms_leave_at_their_own_steps(net, rooms4):
    """NU_attack (no generator involved): four rooms in lockstep leave at different steps, each with the image and the step
    count of a batch-of-one call on that room"""
    from pointsecguard_amd.attacks import torchattacks
    x, labels = _x(rooms4[0]), rooms4[1].astype(np.float64)
    kw = dict(c=0.1, kappa=0, steps=40, lr=0.01)
    adv, n = torchattacks.NU_attack(net, **kw).forward_rooms(x, labels)
    adv = adv.cpu().numpy()
    print("NU lockstep steps", n)
    assert len(set(n.tolist())) >= 3
    from pointsecguard_amd.attacks.torchattacks.attacks import pointnet as pn
    for r in range(4):
        out, k = pn.nu_attack(torchattacks.NU_attack(net, **kw), x[r:r + 1], labels[r:r + 1], neighbour=10, return_steps=True)
        assert k == n[r], (r, k, n[r])
        assert np.array_equal(_bits(out.cpu().numpy()[0]), _bits(adv[r])), r


def _per_step_loop(net, variant, x, labels, mask, kw, neighbour):
    """the retained per-step loop (pointnet.nu_attack with a trace callback): image, exit step or -1, rows {n_correct, n_hits, f, Smooth, L2}"""
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.attacks.torchattacks.attacks import pointnet as pn
    rows, ex = [], []

    def trace(step, cost, f, smooth, l2, S):
        h = S.hist.cpu().numpy().astype(np.float64)
        rows.append([h[0], h[1], f, smooth, l2])
        ex.append(int(S.exit.item()))

    if variant == "nu":
        atk = torchattacks.NU_attack(net, **kw)
        adv = pn.nu_attack(atk, x, labels, neighbour=neighbour, trace=trace)
    else:
        atk = torchattacks.tar_NU_attack(net, mask=mask, **kw)
        adv = pn.nu_attack(atk, x, labels, mask=mask, target=kw["target"], neighbour=neighbour, targeted_variant=True, trace=trace)
    return adv.cpu().numpy(), ex[-1], np.array(rows), atk.lr


def _windowed(net, variant, x, labels, mask, kw, neighbour):
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.attacks.torchattacks.attacks import pointnet as pn
    rows = []

    def rec(step, row, extra, was_active):
        if row is not None:
            rows.append([row[0, 0], row[1, 0], row[2, 0], row[3, 0], row[4, 0] + extra[0]])

    if variant == "nu":
        atk = torchattacks.NU_attack(net, **kw)
        adv, k = pn.nu_attack(atk, x, labels, neighbour=neighbour, return_steps=True, record=rec)
    else:
        atk = torchattacks.tar_NU_attack(net, mask=mask, **kw)
        adv, k = pn.nu_attack(atk, x, labels, mask=mask, target=kw["target"], neighbour=neighbour, targeted_variant=True,
                              return_steps=True, record=rec)
    return adv.cpu().numpy(), k, np.array(rows), atk.lr


@pytest.mark.parametrize("variant,batch", [("nu", 1), ("nu", 2), ("tarnu", 1), ("tarnu", 2)])
def test_windows_equal_the_per_step_loop(net, rooms4, variant, batch):
    x, labels = _x(rooms4[0][:batch]), rooms4[1][:batch].astype(np.float64)
    mask = None
    if variant == "nu":
        kw, neighbour = dict(c=0.1, kappa=0, steps=23, lr=0.01), 10
    else:
        kw, neighbour = dict(c=0.0, kappa=1, steps=53, lr=3.0, target=4), 5
        mask = np.zeros(N, bool)
        mask[::4] = True
    torch.cuda.manual_seed(7)
    a_img, a_exit, a_rows, a_lr = _per_step_loop(net, variant, x, labels, mask, kw, neighbour)
    torch.cuda.manual_seed(7)
    b_img, b_steps, b_rows, b_lr = _windowed(net, variant, x, labels, mask, kw, neighbour)
    n_loop = a_exit + 1 if a_exit >= 0 else kw["steps"]
    print(variant, batch, "steps", n_loop, b_steps, "lr", a_lr, b_lr)
    assert n_loop == b_steps and a_lr == b_lr
    assert np.array_equal(_bits(a_img), _bits(b_img))
    b_rows = b_rows[:len(a_rows)]                            # (the window may have run up to 9 steps past an exit: speculation)
    assert np.array_equal(a_rows[:, :2], b_rows[:, :2])
    assert np.allclose(a_rows[:, 2:], b_rows[:, 2:], rtol=1e-5, atol=0), np.abs(a_rows[:, 2:] / b_rows[:, 2:] - 1).max()


def test_forward_rooms_reproduces_the_recorded_reference_runs(net, rooms4):
    """the bars of tests/test_gpu_pointnet_attacks.py::test_nu_attacks_run_the_reference_control_flow, on room 0 of the fixtures in
    lockstep with room 1"""
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.attacks.torchattacks.attacks import nu as nu_mod
    g = _golden("pointnet_nu.npz")
    x = _x(rooms4[0][:2])
    labels = np.concatenate([g["labels"], rooms4[1][1:2]]).astype(np.float64)
    costs = []
    atk = torchattacks.NU_attack(net, c=0.1, kappa=0, steps=6, lr=0.01)
    rec = lambda step, row, extra, act: costs.append(row[2, 0] + 0.1 * row[3, 0] + 0.1 * (row[4, 0] + extra[0])) if row is not None else None
    adv, n = nu_mod.nu_attack_rooms(atk, x, labels, None, None, 10, record=rec)
    assert n[0] == int(g["n_steps_run"])
    assert np.allclose(costs, g["costs"], rtol=1e-4, atol=0.02)
    assert np.abs(adv[:1].cpu().numpy() - g["adv_final"]).max() <= 1e-3
    t = _golden("pointnet_tarnu.npz")
    labels = np.concatenate([t["labels"], rooms4[1][1:2]]).astype(np.float64)
    masks = np.stack([t["mask"], t["mask"]])
    costs, extras = [], []
    atk = torchattacks.tar_NU_attack(net, c=0.0, kappa=1, steps=23, lr=3.0, target=4, mask=None)
    rec = lambda step, row, extra, act: (costs.append(row[2, 0]), extras.append(extra[0])) if row is not None else None
    adv, n = nu_mod.nu_attack_rooms(atk, x, labels, masks, 4, 5, targeted_variant=True, record=rec)
    assert n[0] == int(t["n_steps_run"])
    # (c = 0: cost = f.  At lr = 3 the free-running trajectories drift apart step by step, which is why the per-step loop's test
    # compares this run's costs teacher-forced only; the first steps are still within that bar, the rest is printed)
    print("tar_NU free-running cost deviation per step", np.abs(np.array(costs[:21]) / t["costs"][:21] - 1).round(6).tolist())
    assert np.allclose(costs[:3], t["costs"][:3], rtol=1e-4, atol=0.02)
    assert extras[20] == 0.0 and extras[21] > 0.0            # the restart ran after step 20, where the reference's did
    want = t["adv_final"]
    adv = adv.cpu().numpy()
    assert np.array_equal(adv[:1, [0, 1, 2, 6, 7, 8]], want[:, [0, 1, 2, 6, 7, 8]])
    assert np.array_equal(adv[:1, 3:6][:, :, ~t["mask"]], np.clip(x[:1, 3:6].cpu().numpy(), 0, 1)[:, :, ~t["mask"]])


@pytest.mark.parametrize("B,n", [(1, 128), (3, 128), (1, 4096), (3, 4096)])
@pytest.mark.parametrize("use_target", [False, True])
@pytest.mark.parametrize("kappa", [0.0, 1.0])
@pytest.mark.parametrize("tsign", [1.0, -1.0])
def test_head_kernel_equals_the_three_kernel_sequence(B, n, use_target, kappa, tsign):
    """pn_nu_head_kernel against pn_log_softmax_kernel -> psg_nu_f_loss_grad(_rooms) -> pn_log_softmax_bwd_kernel on random
    logits (psg_pointnet_nu_head without / with its scratch arrays): dz and pred bit for bit, the f sums - finished by float
    atomics on both sides - to rtol 1e-5; one sum for the batch and one per room."""
    from pointsecguard_amd import _lib, runtime
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1000 * B + n + 7 * int(use_target))
    logits = torch.randn(B, n, 13, device=dev, generator=g) * 3
    logits[0, :13] = 0.5                                       # ties: every class equal (first arg-max on both sides)
    labels = torch.randint(0, 13, (B, n), device=dev, generator=g, dtype=torch.int32)
    labels[0, 20:40] = logits[0, 20:40].argmax(dim=1).to(torch.int32)          # rows whose label is the arg-max class
    logits[0, 40:50] = torch.tensor([0., 2., -1., 2., 0., 1., -3., .5, .25, 0., 0., -2., 1.], device=dev)     # an exact two-way tie ..
    labels[0, 40:45] = 5                                       # .. for the largest other class (label elsewhere: classes 1 and 3 tie)
    labels[0, 45:50] = 1                                       # .. and with the label on one of the tied classes
    p = runtime.ptr
    for per_room in (0, 1):
        res = []
        for fused in (True, False):
            dz = torch.full((B, n, 13), 7.0, device=dev)
            pred = torch.full((B, n), -1, device=dev, dtype=torch.int32)
            fs = torch.zeros(B if per_room else 1, device=dev)
            sc = [None, None] if fused else [torch.empty(B, n, 13, device=dev), torch.empty(B, n, 13, device=dev)]
            _lib.call("psg_pointnet_nu_head", p(logits), None if use_target else p(labels), 6 if use_target else 0, B, n, per_room,
                      kappa, tsign, p(sc[0]), p(sc[1]), p(dz), p(fs), p(pred), runtime.stream())
            torch.cuda.synchronize()
            res.append((dz.cpu().numpy(), pred.cpu().numpy(), fs.cpu().numpy().astype(np.float64)))
        assert np.array_equal(res[0][1], res[1][1])
        assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])), (_bits(res[0][0]) != _bits(res[1][0])).mean()
        assert np.allclose(res[0][2], res[1][2], rtol=1e-5, atol=0), (res[0][2], res[1][2])
        assert np.abs(res[0][2]).min() > 0 or kappa == 0.0


@pytest.mark.parametrize("flagged", [[1], [0, 2, 3]])
def test_restart_rooms_equals_the_python_restart(flagged):
    """psg_nu_restart_rooms against pointnet.py's restart (index assignment under the boolean mask, clamp_ of all nine
    channels, extra L2 over channels 0:3 and 6:9), for masks that are nearly empty (the first and the last point only), full
    and random, with one and with several flagged rooms; rows = 1 and, for one attack on a batch, rows = 2."""
    from pointsecguard_amd import _lib, runtime
    dev = torch.device("cuda")
    n = 1024 + 128
    rng = np.random.default_rng(3)
    for G, rows in ((4, 1), (4, 2)):
        B = G * rows
        x0 = torch.from_numpy((rng.random((B, n, 9)) * 1.6 - 0.3).astype(np.float32)).to(dev)
        orig = x0.clone() + 0.01
        masks = np.zeros((G, n), bool)
        masks[0, [0, n - 1]] = True
        masks[1] = True
        masks[2] = rng.random(n) < 0.3
        masks[3] = rng.random(n) < 0.7
        k = masks.sum(axis=1)
        blocks = {g: torch.from_numpy(rng.random((rows, 3, int(k[g]))).astype(np.float32)).to(dev) for g in flagged}
        # the Python restart, group by group
        want, want_l2 = x0.clone(), {}
        for g in flagged:
            xs = want[g * rows:(g + 1) * rows]
            col = xs[:, :, 3:6].transpose(1, 2)
            mb = torch.from_numpy(masks[g]).to(dev)
            col[:, :, mb] = col[:, :, mb] + blocks[g]
            xs.clamp_(min=0, max=1)
            d = (xs - orig[g * rows:(g + 1) * rows]).double()
            want_l2[g] = float((d[:, :, 0:3] ** 2).sum().item() + (d[:, :, 6:9] ** 2).sum().item())
        offs, flags, total = np.zeros(G, np.int64), np.zeros(G, np.uint8), 0
        for g in flagged:
            offs[g], flags[g] = total, 1
            total += blocks[g].numel()
        noise = torch.cat([blocks[g].reshape(-1) for g in flagged])
        got = x0.clone()
        l2 = torch.full((G,), -1.0, device=dev)
        d_mask, d_k = torch.from_numpy(masks.astype(np.uint8)).to(dev), torch.from_numpy(k.astype(np.int32)).to(dev)
        d_flags, d_offs = torch.from_numpy(flags).to(dev), torch.from_numpy(offs).to(dev)
        _lib.call("psg_nu_restart_rooms", runtime.ptr(got), runtime.ptr(orig), runtime.ptr(d_mask), runtime.ptr(d_k), runtime.ptr(d_flags),
                  runtime.ptr(noise), runtime.ptr(d_offs), G, rows, n, runtime.ptr(l2), runtime.stream())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy()))          # untouched rooms included
        l2 = l2.cpu().numpy()
        # rows * n * 6 squares in [0, 1.1]: an fp32 sum of T terms in any order is within T * 2^-24 relative of the exact sum
        # (first order); the double-precision sum above stands for the exact one
        tol = rows * n * 6 * 2.0 ** -24
        for g in range(G):
            if g in flagged:
                assert abs(l2[g] - want_l2[g]) <= tol * want_l2[g], (g, l2[g], want_l2[g])
            else:
                assert l2[g] == -1.0


def test_graph_bookkeeping_and_run_to_run(rooms4):
    """41 steps in lockstep: [0], [1..10] eager, [11..20] captured + replayed, [21..30], [31..40] replayed on a side stream; on
    the legacy default stream the capture is refused, counted once, and the windows run eagerly with the same result."""
    from pointsecguard_amd import _lib
    from pointsecguard_amd.attacks import torchattacks
    x, labels = _x(rooms4[0]), rooms4[1].astype(np.float64)
    masks = np.zeros((4, N), bool)
    masks[:, ::4] = True

    def run(net, stream):
        atk = torchattacks.tar_NU_attack(net, c=0.0, kappa=1, steps=41, lr=3.0, target=4, mask=None)
        torch.cuda.manual_seed(3)
        if stream is None:
            adv, n = atk.forward_rooms(x, labels, masks)
            torch.cuda.synchronize()
        else:
            with torch.cuda.stream(stream):
                adv, n = atk.forward_rooms(x, labels, masks)
            stream.synchronize()
        st = next(s for k, s in net._psg_nu_states.items() if k[1] == 4 and k[2] == 1)
        return adv.cpu().numpy(), n, _lib.capture_stats(st.graphs[0])

    side = torch.cuda.Stream()
    x.record_stream(side)
    net_a = _new_net()
    a1, n1, s1 = run(net_a, side)
    print("side stream", s1, "steps", n1)
    assert (n1 == 41).all(), n1
    assert s1["captures_failed"] == 0 and s1["captures_tried"] == 1 and s1["replays"] >= 1, s1
    a2, n2, s2 = run(net_a, side)
    assert np.array_equal(_bits(a1), _bits(a2)) and np.array_equal(n1, n2)               # run to run
    assert s2["replays"] == s1["replays"] + 4 and s2["captures_failed"] == 0, s2
    net_b = _new_net()
    b1, nb, sb = run(net_b, None)
    print("legacy stream", sb)
    assert np.array_equal(_bits(a1), _bits(b1)) and np.array_equal(n1, nb)
    assert sb["captures_failed"] == 1 and sb["replays"] == 0 and sb["eager"] == 4, sb


def test_two_rooms_running_together_one_of_them_restarts(net, rooms4):
    """Two rooms that both run all 30 steps in one lockstep call while only the SECOND one (group 1) restarts, after step 20
    (the first room's cost is still falling there): the single draw of the call is the single draw of the call on that room
    alone, so from one seeding both rooms equal their batch-of-one calls bit for bit, perturbed colours included."""
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.attacks.torchattacks.attacks import nu as nu_mod
    x, labels = _x(rooms4[0]), rooms4[1].astype(np.float64)
    masks, _ = _masks_with_an_early_exit(net, x, rooms4[1])
    kw = dict(c=0.0, kappa=1, steps=30, lr=3.0, target=None)
    pair = [0, 2]
    single = {}
    for r in pair:
        torch.cuda.manual_seed(5)
        log = []
        a = torchattacks.tar_NU_attack(net, mask=masks[r], **kw)
        out, k = nu_mod.nu_attack(a, x[r:r + 1], labels[r:r + 1], masks[r], None, 5, targeted_variant=True, return_steps=True,
                                  record=lambda step, row, extra, who, log=log: log.append(step) if row is None else None)
        single[r] = (out.cpu().numpy()[0], k, log)
    print("restarts after steps", {r: single[r][2] for r in pair})
    assert single[0][1] == 30 and single[2][1] == 30 and single[0][2] == [] and single[2][2] == [20]
    torch.cuda.manual_seed(5)
    log = []
    a = torchattacks.tar_NU_attack(net, mask=None, **kw)
    out, k = nu_mod.nu_attack_rooms(a, x[pair].contiguous(), labels[pair], masks[pair], None, 5, targeted_variant=True,
                                    record=lambda step, row, extra, who: log.append((step, who.tolist())) if row is None else None)
    out = out.cpu().numpy()
    assert log == [(20, [False, True])], log
    assert k.tolist() == [30, 30]
    for i, r in enumerate(pair):
        assert np.array_equal(_bits(out[i]), _bits(single[r][0])), r


def _teacher_window_step(net, g, t, room, mask, target, neighbour, clamp_input):
    """one optimiser step through psg_pointnet_nu_window (n_steps = 1) from the reference's recorded state entering step t:
    returns (cost, w after, gradient) of the masked points"""
    import ctypes
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.attacks.torchattacks.attacks.nu import _NuState
    dev = torch.device("cuda")
    S = _NuState(dev, 1, 1, N, neighbour)
    x0 = torch.from_numpy(np.ascontiguousarray(room[None])).cuda()
    S.ori.copy_(x0[:, :, 3:6])
    S.x0_orig.copy_(x0)
    S.x0.copy_(x0.clamp(0, 1) if clamp_input else x0)          # after the first restart the reference's image is clamped
    _lib.call("psg_nu_inverse_tanh", runtime.ptr(S.x0), 1, N, runtime.ptr(S.w), runtime.stream())
    sel = torch.from_numpy(mask).cuda()
    S.m.zero_(); S.v.zero_(); S.scal.zero_(); S.active.fill_(1); S.exit.fill_(-1)
    S.w[0, sel] = torch.from_numpy(g["s%d_w_before" % t][0].T.copy()).cuda()
    adam_t = int(g["s%d_t" % t])
    if adam_t > 1:
        S.m[0, sel] = torch.from_numpy(g["s%d_m" % (t - 1)][0].T.copy()).cuda()
        S.v[0, sel] = torch.from_numpy(g["s%d_v" % (t - 1)][0].T.copy()).cuda()
    m_prev = S.m[0, sel].cpu().numpy().copy()
    S.labels.copy_(torch.from_numpy(g["labels"].astype(np.int32)).cuda())
    S.mask.copy_(torch.from_numpy(mask.astype(np.uint8))[None])
    S.n_mask.fill_(int(mask.sum()))
    ws = net._workspace(1, N)
    c = float(g["c"])
    a = _lib.PointnetNuWindowArgs(
        model=net._packed().handle.value, ws=ws.handle.value, step0=t, n_steps=1, G=1, rows=1, N=N, mode=2, use_target=1, target=target,
        neighbour=neighbour, warm_first=0, adam_t0=adam_t - 1, fused_head=1, kappa=float(g["kappa"]), tsign=1.0, c_smooth=c, c_l2=c,
        lr=float(g["s%d_lr" % t]), beta1=0.9, beta2=0.999, eps=1e-8, w=S.w.data_ptr(), m=S.m.data_ptr(), v=S.v.data_ptr(),
        mask=S.mask.data_ptr(), n_mask=S.n_mask.data_ptr(), x0=S.x0.data_ptr(), ori=S.ori.data_ptr(), labels=S.labels.data_ptr(),
        logp=None, dlogp=None, dx0=S.dx0.data_ptr(), sgrad=S.sgrad.data_ptr(), pred=S.pred.data_ptr(), scal=S.scal.data_ptr(),
        nn_state=S.nn_state.data_ptr(), hist=S.hist.data_ptr(), out=S.out.data_ptr(), active=S.active.data_ptr(),
        exit_step=S.exit.data_ptr())
    _lib.call("psg_pointnet_nu_window", ctypes.byref(a), None, runtime.stream())
    torch.cuda.synchronize()
    h = S.hist[0, :, 0].cpu().numpy().astype(np.float64)
    extra = float(((S.x0[0, :, [0, 1, 2, 6, 7, 8]] - S.x0_orig[0, :, [0, 1, 2, 6, 7, 8]]).double() ** 2).sum().item())
    cost = h[2] + c * h[3] + c * (h[4] + extra)
    grad = (S.m[0, sel].cpu().numpy() - 0.9 * m_prev) / (1 - 0.9)
    return cost, S.w[0, sel].cpu().numpy(), grad


def test_long_reference_run_restarts_halving_and_exit_step(net, rooms4):
    """tests/golden/pointnet_tarnu_long.npz: the unmodified reference tar_NU_attack(c=0, kappa=1, lr=3, target=4, 62 steps) on room
    0, past the step-50 halving.  Free-running through the windows: the same restart steps, the same lr on the attack object
    after the call (halved once), the same number of optimiser steps, the clamped geometry.  Teacher-forced from the
    reference's recorded state through one-step windows around the first restart and around the halving (fresh moments, Adam's
    step counter back at 1, the halved lr): cost, gradient and updated w within the bars of
    tests/test_gpu_pointnet_attacks.py::_check_step."""
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.attacks.torchattacks.attacks import pointnet as pn
    g = _golden("pointnet_tarnu_long.npz")
    mask, target = g["mask"], int(g["target"])
    x = _x(rooms4[0][:1])
    restarts, costs = [], []

    def rec(step, row, extra, who):
        if row is None:
            restarts.append(step)
        else:
            costs.append(row[2, 0])

    atk = torchattacks.tar_NU_attack(net, c=0.0, kappa=1, steps=int(g["steps"]), lr=3.0, target=target, mask=mask)
    adv, k = pn.nu_attack(atk, x, g["labels"].astype(np.float64), mask=mask, target=target, neighbour=5, targeted_variant=True,
                          return_steps=True, record=rec)
    tests = g["restart_tests"]
    print("restarts after steps", restarts, "reference", g["restart_steps"].tolist(), "steps", k, "lr", atk.lr)
    print("margins cost[s] - cost[s - 10] here", [round(costs[s] - costs[s - 10], 3) for s in tests], "reference",
          g["restart_margins"].round(3).tolist())
    assert restarts == g["restart_steps"].tolist()
    assert k == int(g["n_steps_run"]) and atk.lr == float(g["lr_after"])
    assert np.array_equal(adv.cpu().numpy()[:, [0, 1, 2, 6, 7, 8]], g["adv_geometry"])
    first_restart = int(g["restart_steps"][0])
    for t in [int(t) for t in g["keep"]]:
        if ("s%d_m" % (t - 1)) not in g.files and int(g["s%d_t" % t]) > 1:
            continue                                           # (the first kept step of a block only provides the moments)
        cost, w_after, grad = _teacher_window_step(net, g, t, rooms4[0][0], mask, target, 5, clamp_input=t > first_restart)
        want_cost = float(g["costs"][t])
        assert int(g["s%d_t" % t]) == (t + 1 if t <= 50 else t - 50) and float(g["s%d_lr" % t]) == (3.0 if t <= 50 else 1.5)
        assert abs(cost - want_cost) <= 1e-4 * abs(want_cost) + 0.02, (t, cost, want_cost)
        wg = g["s%d_grad" % t][0].T
        rel = np.abs(grad - wg) / np.maximum(np.abs(wg), 1e-12)
        assert np.median(rel) < 1e-3, (t, np.median(rel))
        wa = g["s%d_w_after" % t][0].T
        tol = 1e-4 * max(1.0, float(g["s%d_lr" % t]) / 0.01)
        assert (np.abs(w_after - wa) <= tol).mean() >= 0.99, (t, (np.abs(w_after - wa) <= tol).mean())
