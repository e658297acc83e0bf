"""The remaining paths of the coordinate gradient and the field attacks:
  * PSG_PN2_FPSPLIT=0 - fp_wgrad_kernel reads the coarse level's FEATURE rows at every FP level - in a child process (the
    switch is read once per process), held to the same bars as the default path;
  * PSG_PN2_SPLIT=0 - no dZ1 rows exist: psg_pn2_backward_full refuses with a message;
  * psg_pgd_step_field with channel offset 3 is psg_pgd_step byte for byte;
  * tar_NB_attack(field="both"), teacher-forced on both fields against the float64 yardstick;
  * the vanilla PointNet refuses the coordinate fields."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pn2_ref64
from conftest import GOLDEN
from test_gpu_pn2_coord_attack import host_step
from test_gpu_pn2_fullgrad import dev, plan_tables

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(keyword, extra_env, test_file="test_gpu_pn2_fullgrad.py"):
    env = dict(os.environ)
    for k in ("PSG_PN2_SPLIT", "PSG_PN2_FPSPLIT", "PSG_FP1_WAVE"):
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", test_file), "-x", "-q", "-m", "gpu", "-k",
                           keyword, "-s", "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)


def test_whole_fp_first_layers_meet_the_same_bars():
    out = child("channels_3_to_9 or coordinate_gradient_vs_yardstick or feature_only or two_runs or autograd_switch",
                {"PSG_PN2_FPSPLIT": "0"})
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "5 passed" in out.stdout and "skipped" not in out.stdout.splitlines()[-1]


def test_unsplit_sa_levels_refuse():
    out = child("refuses_without_split", {"PSG_PN2_SPLIT": "0"}, test_file="test_gpu_pn2_fullgrad_paths.py")
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "1 passed" in out.stdout


def test_refuses_without_split(gpu_model):
    """Runs in the child of test_unsplit_sa_levels_refuse under PSG_PN2_SPLIT=0 (there: an error with a message); in the
    default process the same sequence succeeds."""
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import make_rooms
    ws = runtime.PN2Workspace(1, 4096, 1)
    x0 = dev(make_rooms(1, 5))
    ws.plan_build(x0, dev(np.zeros((1, 4, 1)), torch.int32), 1)
    logp = ws.forward(gpu_model, 0, x0)
    dl = torch.zeros_like(logp)
    ws.backward(gpu_model, 0, dl)
    if os.environ.get("PSG_PN2_SPLIT") == "0":
        with pytest.raises(_lib.PsgError, match="PSG_PN2_SPLIT=0"):
            ws.backward(gpu_model, 0, dl, full=True)
    else:
        ws.backward(gpu_model, 0, dl, full=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_field_step_on_colours_is_pgd_step(last, masked):
    from pointsecguard_amd import _lib, runtime
    rng = np.random.default_rng(3)
    B, N = 2, 1024
    x = rng.random((B, N, 9)).astype(np.float32)
    grad = rng.standard_normal((B, N, 9)).astype(np.float32)
    grad[0, :50] = 0
    ori = (x[:, :, 3:6] + rng.uniform(-0.2, 0.2, (B, N, 3))).astype(np.float32)
    mask = dev((rng.random(N) < 0.5).astype(np.uint8)) if masked else None
    outs = []
    for name, extra in (("psg_pgd_step", ()), ("psg_pgd_step_field", (3,))):
        xd, gd, od = dev(x), dev(grad), dev(ori)
        _lib.call(name, runtime.ptr(xd), runtime.ptr(gd), runtime.ptr(od), runtime.ptr(mask), B, N, *extra, 0.03, 0.1, -1.0, last,
                  runtime.stream())
        torch.cuda.synchronize()
        outs.append(xd.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert (outs[0][:, :, 3:6] != x[:, :, 3:6]).any() and np.array_equal(outs[0][:, :, :3], x[:, :, :3])
    # and on the coordinates: no [0, 1] clamp, everything else the same arithmetic
    xd, gd, oc = dev(x * 4 - 2), dev(grad), dev((x[:, :, 0:3] * 4 - 2 + 0.05).astype(np.float32))
    before = xd.cpu().numpy()
    _lib.call("psg_pgd_step_field", runtime.ptr(xd), runtime.ptr(gd), runtime.ptr(oc), runtime.ptr(mask), B, N, 0, 0.03, 0.1, 1.0,
              last, runtime.stream())
    torch.cuda.synchronize()
    m = mask.cpu().numpy().astype(bool) if masked else None
    want = host_step(before[:, :, 0:3], grad[:, :, 0:3], oc.cpu().numpy(), 0.1, 0.03, 1.0, last, mask=m)
    got = xd.cpu().numpy()
    assert np.array_equal(got[:, :, 0:3].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[:, :, 3:], before[:, :, 3:])
    with pytest.raises(_lib.PsgError):
        _lib.call("psg_pgd_step_field", runtime.ptr(xd), runtime.ptr(gd), runtime.ptr(oc), None, B, N, 6, 0.03, 0.1, 1.0, 0,
                  runtime.stream())


def test_tar_nb_both_fields_teacher_forced(weights_sd, gpu_model):
    """tar_NB_attack(field="both"): our state at every iteration, the yardstick's gradient, bit-equal updates of BOTH fields
    wherever the signs agree; flipped entries below 3e-3 of the field's largest magnitude, at most 1 % of the entries."""
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model
    from pointsecguard_amd.synthetic import make_rooms
    g = dict(np.load(os.path.join(GOLDEN, "pn2_fullgrad.npz")))
    B, N, iters = 2, 4096, 3
    rooms = make_rooms(B, int(g["room_seed"]))
    labels = g["labels"].astype(np.int64)
    cls = np.bincount(labels[0], minlength=13).argmax()
    mask, target = labels[0] == cls, int((cls + 1) % 13)
    ceps, calpha, eps, alpha = 0.01, 0.004, 0.02, 0.008
    net = get_model(13)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights_sd.items()})
    net = net.cuda().eval()
    cn = rooms.transpose(0, 2, 1)
    state = rooms.copy()
    for k in range(1, iters + 1):       # the public call for k iterations = k - 1 projected steps + one un-projected
        atk = torchattacks.tar_NB_attack(net, eps=eps, alpha=alpha, iters=k, target=target, mask=mask, field="both",
                                         coord_eps=ceps, coord_alpha=calpha)
        torch.manual_seed(21)
        out = atk(dev(cn), labels.astype(np.float64)).cpu().numpy().transpose(0, 2, 1)
        ws = net._workspace(B, N, 1)    # holds the plan of the call's last iteration, built from `state`
        yard, _ = pn2_ref64.input_grad(weights_sd, state.transpose(0, 2, 1), pn2_ref64.tables_from(plan_tables(ws, B)), target=target)
        gy = yard.transpose(0, 2, 1)
        for lo, e, a, c01 in ((0, ceps, calpha, False), (3, eps, alpha, True)):
            want_last = host_step(state[:, :, lo:lo + 3], gy[:, :, lo:lo + 3], rooms[:, :, lo:lo + 3], e, a, -1.0, True, c01, mask)
            diff = out[:, :, lo:lo + 3].view(np.uint32) != want_last.view(np.uint32)
            gm = np.abs(gy[:, :, lo:lo + 3])
            share = diff.sum() / (mask.sum() * B * 3)
            flipped = float(gm[diff].max() / gm[:, mask].max()) if diff.any() else 0.0
            print("k = %d channels %d:%d differing %.5f (cap 0.01), largest |g| among them %.3e of max (bar 3e-3)" % (k, lo, lo + 3, share, flipped))
            assert flipped <= 3e-3 and share <= 0.01
        assert np.array_equal(out[:, ~mask], rooms[:, ~mask]) and np.array_equal(out[:, :, 6:], rooms[:, :, 6:])
        # our own projected state entering the next iteration: the un-projected last step, projected (nontarget.py:38-39)
        nxt = rooms.copy()
        for lo, e, c01 in ((0, ceps, False), (3, eps, True)):
            eta = np.clip((out[:, :, lo:lo + 3] - rooms[:, :, lo:lo + 3]).astype(np.float32), np.float32(-e), np.float32(e))
            p = (rooms[:, :, lo:lo + 3] + eta).astype(np.float32)
            nxt[:, mask, lo:lo + 3] = (np.clip(p, np.float32(0), np.float32(1)) if c01 else p)[:, mask]
        state = nxt


def test_vanilla_pointnet_refuses_the_coordinate_fields():
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.models import pointnet_sem_seg
    net = pointnet_sem_seg.get_model(13).cuda().eval()
    x = torch.rand(1, 9, 1024, device="cuda")
    y = np.zeros((1, 1024))
    with pytest.raises(NotImplementedError):
        torchattacks.NB_attack(net, iters=1, field="coord")(x, y)
    with pytest.raises(NotImplementedError):
        torchattacks.tar_NB_attack(net, iters=1, target=1, mask=np.ones(1024, bool), field="both")(x, y)
