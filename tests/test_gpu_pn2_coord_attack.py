"""GPU tests of the coordinate-field NB attacks (NB_attack / tar_NB_attack field="coord" / "both").

Teacher-forced like check_flips (tests/test_gpu_parity.py): at each of the first iterations the state is OURS, the gradient
the update is judged by is the float64 yardstick's (tests/pn2_ref64.py) on the plan's own index tables for that state.
Updated coordinates must be bit-equal wherever the signs agree; every other entry lies below 3e-3 of the largest gradient
magnitude (the project's bar), and the share of entries excused that way is at most 1 %.  The rooms are the fixture's
(make_rooms(2, 33)), for which the REFERENCE's fp32 gradient agrees in sign with the yardstick on every entry of channels
0:3 (tests/golden/pn2_fullgrad.npz: e_ref).

The reference's loop returns the UN-projected last step (nontarget.py:37-41), so the returned field may sit up to one alpha
outside the eps ball; the states entering every iteration are inside it."""
import os

import numpy as np
import pytest
import torch

import pn2_ref64
from conftest import GOLDEN
from test_gpu_pn2_fullgrad import dev, plan_tables

pytestmark = pytest.mark.gpu

B, N = 2, 4096
EPS, ALPHA, ITERS = np.float32(0.01), np.float32(0.004), 4      # the eps ball clamps from the third step on
FLIP_BAR, SHARE_CAP = 3e-3, 0.01


@pytest.fixture(scope="module")
def setup(weights_sd):
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model
    from pointsecguard_amd.synthetic import make_rooms
    g = dict(np.load(os.path.join(GOLDEN, "pn2_fullgrad.npz")))
    rooms = make_rooms(B, int(g["room_seed"]))
    m = get_model(13)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights_sd.items()})
    return g, rooms, m.cuda().eval()


def host_step(x, grad, ori, eps, alpha, direction, last, clamp01=False, mask=None):
    """The reference's loop body on one field in fp32 (nontarget.py:37-39 / target.py:41-43), from a given gradient."""
    x, ori = x.astype(np.float32), ori.astype(np.float32)
    stepped = (x + np.float32(direction * alpha) * np.sign(grad).astype(np.float32)).astype(np.float32)
    eta = np.clip((stepped - ori).astype(np.float32), -np.float32(eps), np.float32(eps))
    proj = (ori + eta).astype(np.float32)
    if clamp01:
        proj = np.clip(proj, np.float32(0), np.float32(1))
    out = stepped if last else proj
    if mask is not None:
        out = np.where(mask[None, :, None], out, x)
    return out


def run_pieces(model, ws, rooms, labels, starts, sd, target=None, mask=None):
    """The attack's launches one at a time, each step judged against the yardstick; returns the final rooms [B, N, 9]."""
    from pointsecguard_amd import _lib, runtime
    x0 = dev(rooms)
    ori = x0[:, :, 0:3].contiguous()
    ori_np = rooms[:, :, 0:3]
    lab = dev(labels.astype(np.int32))
    mask_d = dev(mask.astype(np.uint8)) if mask is not None else None
    direction = 1.0 if target is None else -1.0
    worst_share = 0.0
    for it in range(ITERS):
        last = it == ITERS - 1
        ws.plan_build(x0, dev(starts[it:it + 1], torch.int32), 1)
        logp = ws.forward(model, 0, x0)
        dlogp = torch.empty_like(logp)
        _lib.call("psg_ce_logp_grad", runtime.ptr(logp), runtime.ptr(lab) if target is None else None, 0 if target is None else target,
                  B * N, B * N if target is None else N, 13, 1.0 / N, runtime.ptr(dlogp), None, runtime.stream())
        dx0 = ws.backward(model, 0, dlogp, full=True)
        torch.cuda.synchronize()
        before = x0.cpu().numpy()
        assert np.abs(before[:, :, 0:3].astype(np.float64) - ori_np).max() <= float(EPS) + np.spacing(np.float32(8.0))
        yard, _ = pn2_ref64.input_grad(sd, before.transpose(0, 2, 1), pn2_ref64.tables_from(plan_tables(ws, B)),
                                       labels=labels if target is None else None, target=target)
        gy = yard[:, 0:3].transpose(0, 2, 1)                                    # [B, N, 3]
        _lib.call("psg_pgd_step_field", runtime.ptr(x0), runtime.ptr(dx0), runtime.ptr(ori), runtime.ptr(mask_d), B, N, 0,
                  float(ALPHA), float(EPS), direction, 1 if last else 0, runtime.stream())
        torch.cuda.synchronize()
        got = x0.cpu().numpy()
        assert np.array_equal(got[:, :, 3:], rooms[:, :, 3:])                   # channels 3:9 untouched
        want = host_step(before[:, :, 0:3], gy, ori_np, EPS, ALPHA, direction, last, mask=mask)
        diff = got[:, :, 0:3].view(np.uint32) != want.view(np.uint32)
        ours = dx0[:, :, 0:3].cpu().numpy()
        moved = np.ones_like(diff) if mask is None else np.broadcast_to(mask[None, :, None], diff.shape)
        share = diff.sum() / moved.sum()
        top = np.abs(gy[moved]).max()
        flipped = float(np.abs(gy[diff]).max() / top) if diff.any() else 0.0
        agree = (np.sign(ours) == np.sign(gy))[moved].mean()
        print("iteration %d: differing entries %.5f (cap %.2f), largest |g| among them %.3e of max (bar %.0e), sign agreement %.6f"
              % (it, share, SHARE_CAP, flipped, FLIP_BAR, agree))
        # an entry differs only where the signs differ
        assert not (diff & (np.sign(ours) == np.sign(gy))).any()
        assert flipped <= FLIP_BAR
        assert share <= SHARE_CAP
        worst_share = max(worst_share, share)
    return x0.cpu().numpy(), worst_share


def test_nb_coord_steps_vs_yardstick_and_public_call(setup, weights_sd, gpu_model):
    from pointsecguard_amd import runtime
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts
    g, rooms, net = setup
    labels = g["labels"].astype(np.int64)
    torch.manual_seed(11)
    starts = draw_fps_starts(B, N, ITERS).numpy()
    state_after = torch.get_rng_state()
    ws = runtime.PN2Workspace(B, N, 1)
    final, _ = run_pieces(gpu_model, ws, rooms, labels, starts, weights_sd)
    # the public call: the same launches, the CPU generator advanced by exactly 4 * iters draws
    images = dev(rooms.transpose(0, 2, 1))
    atk = torchattacks.NB_attack(net, eps=0.3, alpha=0.1, iters=ITERS, field="coord", coord_eps=float(EPS), coord_alpha=float(ALPHA))
    torch.manual_seed(11)
    adv = atk(images, labels.astype(np.float64))
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), state_after)
    out = adv.cpu().numpy()
    assert np.array_equal(out.view(np.uint32), np.ascontiguousarray(final.transpose(0, 2, 1)).view(np.uint32))
    assert np.array_equal(out[:, 3:], rooms.transpose(0, 2, 1)[:, 3:])
    moved = np.abs(out[:, :3].astype(np.float64) - rooms.transpose(0, 2, 1)[:, :3])
    print("coord attack: largest move %.5f (eps %.3f, alpha %.3f), entries outside the eps ball after the un-projected last step: %d"
          % (moved.max(), EPS, ALPHA, int((moved > float(EPS) + 1e-6).sum())))
    assert moved.max() > 0 and moved.max() <= float(EPS) + float(ALPHA) + 1e-6
    # projected as the reference would feed it to a next iteration: inside the ball
    eta = np.clip(out[:, :3] - rooms.transpose(0, 2, 1)[:, :3], -EPS, EPS)
    assert np.abs(eta).max() <= EPS


def test_coord_eps_alpha_fall_back_to_eps_alpha(setup):
    from pointsecguard_amd.attacks import torchattacks
    g, rooms, net = setup
    images, labels = dev(rooms.transpose(0, 2, 1)), g["labels"].astype(np.float64)
    outs = []
    for kw in (dict(eps=float(EPS), alpha=float(ALPHA)), dict(eps=0.5, alpha=0.2, coord_eps=float(EPS), coord_alpha=float(ALPHA))):
        torch.manual_seed(3)
        outs.append(torchattacks.NB_attack(net, iters=2, field="coord", **kw)(images, labels).cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    with pytest.raises(ValueError):
        torchattacks.NB_attack(net, field="normals")


def test_tar_nb_coord_steps_and_mask(setup, weights_sd, gpu_model):
    from pointsecguard_amd import runtime
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts
    g, rooms, net = setup
    labels = g["labels"].astype(np.int64)
    cls = np.bincount(labels[0], minlength=13).argmax()
    mask = labels[0] == cls
    target = int((cls + 1) % 13)
    torch.manual_seed(12)
    starts = draw_fps_starts(B, N, ITERS).numpy()
    state_after = torch.get_rng_state()
    ws = runtime.PN2Workspace(B, N, 1)
    final, _ = run_pieces(gpu_model, ws, rooms, labels, starts, weights_sd, target=target, mask=mask)
    assert np.array_equal(final[:, ~mask], rooms[:, ~mask])                                   # mask respected
    assert (final[:, mask, 0:3] != rooms[:, mask, 0:3]).any()
    atk = torchattacks.tar_NB_attack(net, eps=float(EPS), alpha=float(ALPHA), iters=ITERS, target=target, mask=mask, field="coord")
    torch.manual_seed(12)
    adv = atk(dev(rooms.transpose(0, 2, 1)), labels.astype(np.float64))
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), state_after)
    assert np.array_equal(adv.cpu().numpy().view(np.uint32), np.ascontiguousarray(final.transpose(0, 2, 1)).view(np.uint32))


def test_field_both_moves_both_fields_only(setup):
    from pointsecguard_amd.attacks import torchattacks
    g, rooms, net = setup
    cn = rooms.transpose(0, 2, 1)
    torch.manual_seed(4)
    out = torchattacks.NB_attack(net, eps=0.05, alpha=0.01, iters=3, field="both", coord_eps=float(EPS), coord_alpha=float(ALPHA))(
        dev(cn), g["labels"].astype(np.float64)).cpu().numpy()
    assert np.array_equal(out[:, 6:], cn[:, 6:])
    assert (out[:, :3] != cn[:, :3]).any() and (out[:, 3:6] != cn[:, 3:6]).any()
    assert np.abs(out[:, :3] - cn[:, :3]).max() <= float(EPS) + float(ALPHA) + 1e-6
    assert np.abs(out[:, 3:6] - cn[:, 3:6]).max() <= 0.05 + 0.01 + 1e-6


def test_field_color_is_the_fused_call_byte_for_byte(setup, gpu_model):
    """field="color" (explicit or default) is the parent's path: the same bytes as psg_pn2_nb_attack called directly."""
    from pointsecguard_amd import runtime
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts
    g, rooms, net = setup
    images, labels = dev(rooms.transpose(0, 2, 1)), g["labels"].astype(np.float64)
    outs = []
    for kw in ({}, {"field": "color"}):
        torch.manual_seed(9)
        outs.append(torchattacks.NB_attack(net, eps=0.05, alpha=2 / 255, iters=3, **kw)(images, labels).cpu().numpy())
    torch.manual_seed(9)
    starts = draw_fps_starts(B, N, 3)
    ws = runtime.PN2Workspace(B, N, 3)
    direct = ws.nb_attack(gpu_model, images, dev(g["labels"].astype(np.int32)), starts.cuda(), 0.05, 2 / 255, 3).cpu().numpy()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), direct.view(np.uint32))
