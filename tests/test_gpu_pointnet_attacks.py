"""GPU tests of the four colour attacks on the vanilla PointNet, against the reference's recorded per-step states
(tests/golden/pointnet_{nb,tarnb,nu,tarnu}.npz, made by tests/golden/make_golden_pointnet.py), and of the drop-in path
of INTEGRATION section 1 (the model module imported by file name, the attack package as top-level `torchattacks`)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PN_SEED, ROOM_SEED = 3, 5
BETA1 = 0.9


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name))


def _net(get_model):
    from pointsecguard_amd import synthetic
    m = get_model(13)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.pointnet_state_dict(PN_SEED).items()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def net():
    from pointsecguard_amd.models.pointnet_sem_seg import get_model
    return _net(get_model)


@pytest.fixture(scope="module")
def rooms():
    from pointsecguard_amd import synthetic
    r = synthetic.make_rooms(2, ROOM_SEED)
    return r, synthetic.rule_labels(r)


def _x(r):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(r).transpose(0, 2, 1))).cuda()


def _project(got, ori, eps):
    return np.clip(ori + np.clip(got - ori, -np.float32(eps), np.float32(eps)), 0, 1).astype(np.float32)


@pytest.mark.parametrize("fixture", ["pointnet_nb.npz", "pointnet_tarnb.npz"])
def test_nb_steps_teacher_forced_against_reference(net, rooms, fixture):
    """the reference's colour state entering iteration i, one fused iteration, projected as the reference projects it:
    bit-equal to the reference's state entering iteration i + 1 on >= 99.9 % of the entries"""
    from pointsecguard_amd.attacks import torchattacks
    g = _golden(fixture)
    x = _x(rooms[0])
    ori = x[:, 3:6].cpu().numpy()
    keep = list(g["keep"])
    n = 0
    for a, i in enumerate(keep):
        if i + 1 not in keep:
            continue
        xi = x.clone()
        xi[:, 3:6] = torch.from_numpy(g["states"][a]).cuda()
        if "mask" in g.files:
            atk = torchattacks.tar_NB_attack(net, eps=0.1, alpha=0.05, iters=1, target=int(g["target"]), mask=g["mask"])
        else:
            atk = torchattacks.NB_attack(net, eps=0.1, alpha=0.05, iters=1)
        got = atk(xi, rooms[1].astype(np.float64))[:, 3:6].cpu().numpy()      # the un-projected step
        want = g["states"][keep.index(i + 1)]
        proj = _project(got, ori, 0.1)
        if "mask" in g.files:
            proj[:, :, ~g["mask"]] = ori[:, :, ~g["mask"]]
        assert (proj.view(np.uint32) == want.view(np.uint32)).mean() >= 0.999, i
        n += 1
    assert n == 3


def _nu_teacher_step(net, g, t, room, mask, mode, target, neighbour, x_in=None):
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.attacks.torchattacks.attacks import pointnet as pn
    N = 4096
    S = pn.NuState(1, N, torch.device("cuda"))
    x0 = torch.from_numpy(np.ascontiguousarray(room[None])).cuda()
    S.ori.copy_(x0[:, :, 3:6])
    if x_in is not None:
        x0 = torch.from_numpy(np.ascontiguousarray(x_in.transpose(0, 2, 1))).cuda()
    S.x0.copy_(x0)
    _lib.call("psg_nu_inverse_tanh", runtime.ptr(S.x0), 1, N, runtime.ptr(S.w), runtime.stream())
    sel = torch.from_numpy(mask).cuda() if mask is not None else torch.ones(N, dtype=torch.bool, device="cuda")

    def put(dst, key):
        dst[0, sel] = torch.from_numpy(g[key][0].T.copy()).cuda()

    put(S.w, "s%d_w_before" % t)
    if t > 0 and ("s%d_m" % (t - 1)) in g.files:
        put(S.m, "s%d_m" % (t - 1))
        put(S.v, "s%d_v" % (t - 1))
    m_prev = S.m[0, sel].cpu().numpy().copy()
    labels = torch.from_numpy(g["labels"].astype(np.int32)).cuda()
    mask_d = torch.from_numpy(mask.astype(np.uint8)).cuda() if mask is not None else None
    n_mask = torch.tensor([int(mask.sum())], dtype=torch.int32, device="cuda") if mask is not None else None
    c = float(g["c"])
    pn.nu_step(net, S, labels, mask_d, n_mask, target, mode, float(g["kappa"]), 1.0, c, neighbour, float(g["s%d_lr" % t]),
               int(g["s%d_t" % t]), t)
    h = S.hist.cpu().numpy().astype(np.float64)
    cost = h[2] + c * h[3] + c * h[4]
    w_after = S.w[0, sel].cpu().numpy()
    grad = (S.m[0, sel].cpu().numpy() - BETA1 * m_prev) / (1 - BETA1)
    return cost, w_after, grad, S


def _check_step(g, t, cost, w_after, grad, extra_cost=0.0):
    want_cost = float(g["costs"][t])
    assert abs(cost + extra_cost - want_cost) <= 1e-4 * abs(want_cost) + 0.02, (t, cost, want_cost)
    wg = g["s%d_grad" % t][0].T
    rel = np.abs(grad - wg) / np.maximum(np.abs(wg), 1e-12)
    assert np.median(rel) < 1e-3, (t, np.median(rel))
    # updated w: tests/test_gpu_nu.py's bar (1e-4 at lr 0.01) in units of the step size: Adam's first steps are ~lr*sign(g),
    # so an entry whose gradient is ~0 can differ by up to 2*lr, and every difference scales with lr
    wa = g["s%d_w_after" % t][0].T
    tol = 1e-4 * max(1.0, float(g["s%d_lr" % t]) / 0.01)
    assert (np.abs(w_after - wa) <= tol).mean() >= 0.99, (t, (np.abs(w_after - wa) <= tol).mean())


def test_nu_steps_teacher_forced(net, rooms):
    g = _golden("pointnet_nu.npz")
    for t in (0, 1, 2):
        cost, w_after, grad, _ = _nu_teacher_step(net, g, t, rooms[0][0], None, 0, None, 10)
        _check_step(g, t, cost, w_after, grad)


def test_tar_nu_steps_teacher_forced_through_restart(net, rooms):
    g = _golden("pointnet_tarnu.npz")
    mask = g["mask"]
    room = rooms[0][0]
    for t in (0, 1, 2, 20, 21, 22):
        x_in = g["input_%d" % t] if t in (21, 22) else None
        cost, w_after, grad, S = _nu_teacher_step(net, g, t, room, mask, 2, int(g["target"]), 5, x_in=x_in)
        _check_step(g, t, cost, w_after, grad)


def test_nu_attacks_run_the_reference_control_flow(net, rooms):
    from pointsecguard_amd.attacks import torchattacks
    g = _golden("pointnet_nu.npz")
    x = _x(rooms[0][:1])
    steps = []
    from pointsecguard_amd.attacks.torchattacks.attacks import pointnet as pn
    atk = torchattacks.NU_attack(net, c=0.1, kappa=0, steps=6, lr=0.01)
    adv = pn.nu_attack(atk, x, g["labels"].astype(np.float64), neighbour=10, trace=lambda **k: steps.append(k["cost"]))
    assert len(steps) == int(g["n_steps_run"])               # the same exit step (here: none, all 6 steps)
    assert np.allclose(steps, g["costs"], rtol=1e-4, atol=0.02)
    assert np.abs(adv.cpu().numpy() - g["adv_final"]).max() <= 1e-3
    t = _golden("pointnet_tarnu.npz")
    atk = torchattacks.tar_NU_attack(net, c=0.0, kappa=1, steps=23, lr=3.0, target=4, mask=t["mask"])
    adv = atk(x, t["labels"].astype(np.float64))
    want = t["adv_final"]
    # after the restart (noise from the device generator here, the CPU one there) only the geometry is comparable:
    # the clamp of all channels to [0, 1] at step 20
    assert np.array_equal(adv[:, [0, 1, 2, 6, 7, 8]].cpu().numpy(), want[:, [0, 1, 2, 6, 7, 8]])
    assert np.array_equal(adv[:, 3:6].cpu().numpy()[:, :, ~t["mask"]], np.clip(x[:, 3:6].cpu().numpy(), 0, 1)[:, :, ~t["mask"]])


def test_integration_flat_import_dispatch(rooms):
    """models/ and attacks/ on sys.path, the model module imported by file name.  The second class
    object this makes must still reach the PointNet kernels from all four attacks."""
    import pointsecguard_amd
    pkg = os.path.dirname(pointsecguard_amd.__file__)
    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    try:
        sys.path[:0] = [os.path.join(pkg, "models"), os.path.join(pkg, "attacks")]
        MODEL = importlib.import_module("pointnet_sem_seg")
        ta = importlib.import_module("torchattacks")
        from pointsecguard_amd.models.pointnet_sem_seg import get_model as pkg_get_model
        assert MODEL.get_model is not pkg_get_model
        net = _net(MODEL.get_model)
        x = _x(rooms[0])
        g = _golden("pointnet_nb.npz")
        adv = ta.NB_attack(net, eps=0.1, alpha=0.05, iters=10)(x, rooms[1].astype(np.float64))
        assert (adv[:, 3:6].cpu().numpy().view(np.uint32) == g["adv_colour"].view(np.uint32)).mean() >= 0.99
        t = _golden("pointnet_tarnb.npz")
        adv = ta.tar_NB_attack(net, eps=0.1, alpha=0.05, iters=10, target=int(t["target"]), mask=t["mask"])(
            x, rooms[1].astype(np.float64))
        assert (adv[:, 3:6].cpu().numpy().view(np.uint32) == t["adv_colour"].view(np.uint32)).mean() >= 0.99
        adv = ta.NU_attack(net, c=0.1, steps=2)(x[:1], rooms[1][:1].astype(np.float64))
        assert adv.shape == (1, 9, 4096)
        mask = np.zeros(4096, bool)
        mask[::4] = True
        adv = ta.tar_NU_attack(net, c=0.1, steps=2, target=4, mask=mask)(x[:1], rooms[1][:1].astype(np.float64))
        assert adv.shape == (1, 9, 4096)
    finally:
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved_mods:
                del sys.modules[k]
