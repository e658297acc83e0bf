"""GPU tests of psg_pn2_backward_full: the complete coordinate gradient of the PointNet++ SSG network.

Yardstick: tests/pn2_ref64.py (float64, pinned to the reference's autograd by tests/test_pn2_fullgrad_host.py) on the
PLAN'S OWN index tables.  Bars of channels 0:3: the project's colour-gradient bars (tests/test_gpu_parity.py: check_grad)
minus the zero-pattern clause - sign agreement on >= 99.9 % of the entries, every disagreement below 1e-3 of the largest
magnitude, median relative error below 1e-4.  They apply as they stand because the reference's own fp32 autograd sits inside
them with room to spare: e_ref of channels 0:3 = signs agree on 100 % of the entries, no flipped entry, median relative
error 2.28e-05 (tests/golden/pn2_fullgrad.npz: e_ref, e_ref_median; re-measured by the host test).  check_grad has no clause
on the largest error; the reference's own is 3.561e-03 of the largest magnitude (the fp32 noise of the coincident points'
distances), so that clause is 2 x e_ref = 7.12e-03 here: the factor covers another summation order of
the same fp32 terms."""
import os

import numpy as np
import pytest
import torch

import pn2_ref64
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIGN_BAR, FLIP_BAR, MEDIAN_BAR = 0.999, 1e-3, 1e-4


def check_coord_grad(ours, ref, e_ref_max, what):
    """The bars of the module docstring on channels 0:3 ([B, 3, N]); prints every figure before it asserts."""
    agree, flip = coord_bars(ours, ref)
    nz = ref != 0
    median = float(np.median(np.abs(ours - ref)[nz] / np.abs(ref[nz])))
    err = float(np.abs(ours - ref).max() / np.abs(ref).max())
    print("%s 0:3 vs float64: sign agreement %.6f (bar %.3f), largest flipped %.3e (bar %.0e), median relative error %.3e "
          "(bar %.0e), max abs / max mag %.3e (bar 2 x e_ref = %.3e)" % (what, agree, SIGN_BAR, flip, FLIP_BAR, median, MEDIAN_BAR,
                                                                         err, 2 * e_ref_max))
    assert agree >= SIGN_BAR
    assert flip <= FLIP_BAR
    assert median < MEDIAN_BAR
    assert err <= 2 * e_ref_max


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dt is not None:
        t = t.to(dt)
    return t.cuda().contiguous()


def plan_tables(ws, batch):
    """The index tables of plan slot 0 as the yardstick takes them."""
    out = {}
    for l in range(4):
        for what, key in ((0, "fps%d"), (1, "group%d"), (2, "nn_idx%d")):
            out[key % l] = np.stack([ws.plan_tensor(what, l, 0, b).cpu().numpy() for b in range(batch)])
    return out


def coord_bars(ours, ref):
    """(sign agreement share, largest |ref| among disagreeing entries / max |ref|) over channels 0:3."""
    agree = np.sign(ours) == np.sign(ref)
    flip = float(np.abs(ref[~agree]).max() / np.abs(ref).max()) if not agree.all() else 0.0
    return float(agree.mean()), flip


@pytest.fixture(scope="module")
def run(gpu_model, weights_sd):
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import make_rooms
    g = dict(np.load(os.path.join(GOLDEN, "pn2_fullgrad.npz")))
    rooms = make_rooms(2, int(g["room_seed"]))
    assert float(rooms.astype(np.float64).sum()) == float(g["rooms_sum"])
    B, N = 2, 4096
    ws = runtime.PN2Workspace(B, N, 1)
    x0 = dev(rooms)
    ws.plan_build(x0, dev(g["starts"].reshape(1, 4, B), torch.int32), 1)
    logp = ws.forward(gpu_model, 0, x0)
    labels = dev(g["labels"].astype(np.int32))
    dlogp = torch.empty_like(logp)
    _lib.call("psg_ce_logp_grad", runtime.ptr(logp), runtime.ptr(labels), 0, B * N, B * N, 13, 1.0 / N, runtime.ptr(dlogp),
              None, runtime.stream())
    feat = ws.backward(gpu_model, 0, dlogp)
    full = ws.backward(gpu_model, 0, dlogp, full=True)
    torch.cuda.synchronize()
    tables = plan_tables(ws, B)
    yard, _ = pn2_ref64.input_grad(weights_sd, rooms.transpose(0, 2, 1), pn2_ref64.tables_from(tables), labels=g["labels"])
    return dict(g=g, ws=ws, x0=x0, dlogp=dlogp, feat=feat.cpu().numpy().transpose(0, 2, 1), full_t=full,
                full=full.cpu().numpy().transpose(0, 2, 1), yard=yard, tables=tables, rooms=rooms)


def test_plan_tables_are_the_references(run):
    for k, v in run["tables"].items():
        assert np.array_equal(v, run["g"][k].astype(np.int32)), k


def test_channels_3_to_9_are_the_feature_backward_bytes(run):
    assert np.array_equal(run["full"][:, 3:].view(np.uint32), run["feat"][:, 3:].view(np.uint32))


def test_coordinate_gradient_vs_yardstick(run):
    e_ref = run["g"]["e_ref"][0]
    assert e_ref[1] >= 0.9999 and e_ref[2] <= 0.1 * FLIP_BAR, "the reference itself is not inside the bars with room to spare"
    assert run["g"]["e_ref_median"][0] <= 0.5 * MEDIAN_BAR
    ours, ref = run["full"][:, :3], run["yard"][:, :3]
    check_coord_grad(ours, ref, e_ref[0], "backward_full")
    rerr = np.abs(ours - run["g"]["dx"][:, :3]).max() / np.abs(ref).max()
    print("backward_full 0:3 vs the reference's fp32 autograd: max abs / max mag %.3e" % rerr)


def test_feature_only_gradient_fails_the_same_comparison(run):
    """Teeth: psg_pn2_backward's channels 0:3 (the feature path alone) do not meet the bars the full gradient meets."""
    agree, flip = coord_bars(run["feat"][:, :3], run["yard"][:, :3])
    missing = np.abs(run["feat"][:, :3] - run["yard"][:, :3]).max() / np.abs(run["yard"][:, :3]).max()
    print("feature-only 0:3: sign agreement %.4f, largest flipped %.3f, missing part up to %.3f of the largest magnitude"
          % (agree, flip, missing))
    assert agree < SIGN_BAR and flip > FLIP_BAR and missing > 2 * run["g"]["e_ref"][0][0]


def test_two_runs_bit_equal_and_linear(run, gpu_model):
    ws, dlogp = run["ws"], run["dlogp"]
    again = ws.backward(gpu_model, 0, dlogp, full=True)
    twice = ws.backward(gpu_model, 0, (dlogp * 2.0).contiguous(), full=True)
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), run["full_t"].view(torch.int32))
    assert torch.equal(twice, run["full_t"] * 2.0)


def test_autograd_switch(run, weights_sd):
    """get_model.input_grad = "full" is the C call; the default is today's psg_pn2_backward."""
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model
    g = run["g"]
    m = get_model(13)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights_sd.items()})
    m = m.cuda().eval()
    assert m.input_grad == "features"
    grads = {}
    for mode in ("features", "full"):
        m.input_grad = mode
        x = dev(run["rooms"].transpose(0, 2, 1)).requires_grad_(True)
        torch.manual_seed(int(g["seed_rng"]))          # the reference's FPS draws of the fixture: the same plan
        logp, l4 = m(x)
        assert not l4.requires_grad
        logp.backward(run["dlogp"])                    # the upstream gradient the C calls of the fixture `run` were given
        grads[mode] = x.grad.cpu().numpy()
    for mode, want in (("features", run["feat"]), ("full", run["full"])):
        assert np.array_equal(grads[mode].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), mode
    check_coord_grad(grads["full"][:, :3], run["yard"][:, :3], g["e_ref"][0][0], "autograd full")
    m.input_grad = "nonsense"
    with pytest.raises(ValueError):
        m(dev(run["rooms"].transpose(0, 2, 1)))


def test_msg_refuses_instead_of_a_partial_gradient():
    """PSG_PN2_ARCH_MSG: the entry point returns an error with a message, after a forward that would let psg_pn2_backward run."""
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import make_rooms, msg_state_dict
    model = runtime.PN2Model(runtime.fold_state_dict(msg_state_dict(77), msg=True), arch=runtime.ARCH_MSG)
    ws = runtime.PN2Workspace(1, 4096, 1, arch=runtime.ARCH_MSG)
    x0 = dev(make_rooms(1, 5))
    ws.plan_build(x0, dev(np.zeros((1, 4, 1)), torch.int32), 1)
    logp = ws.forward(model, 0, x0)
    dl = torch.zeros_like(logp)
    ws.backward(model, 0, dl)
    with pytest.raises(_lib.PsgError, match="SSG"):
        ws.backward(model, 0, dl, full=True)
    torch.cuda.synchronize()
