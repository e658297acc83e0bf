"""Vanilla PointNet, stage by stage: every kernel launch of csrc/psg_pointnet.hip against the float64 statement of ITS OWN
operation (tests/pointnet_stages_ref64.py, which documents every bound) on ITS OWN inputs, read through the workspace tap
psg_pointnet_debug_ptr.  Every stage is fed what the GPU produced, and the backward stages take the GPU's decisions (ReLU bit
words, act > 0 gates, arg-max sets, pool > 0) as inputs, so a last-bit flip cannot move an entry downstream and every bound
is asserted on EVERY entry.  tests/test_pointnet_stages_host.py shows on the CPU that a float32 evaluation meets every
bound and that eleven single faults each fail at their stage.

Cases (pointnet_stages_ref64.make_case): (B, N) = (1,128) one tile, single-row per-room GEMMs; (3,128) adjacent tiles of
different rooms, ragged 9 / 192-column per-room operands; (2,256) "dup" and (2,128) "const", exact ties in every channel of
all three pools (the shuffle, wave-row and tile levels of the lowest-index rule); (1,384) and (5,640), 3 and 5 tiles.  Each is
one forward and three backwards: both cotangents (dlogp a general standard-normal cotangent, rows not summing to zero),
dtrans_feat = None, and dlogp = 0 (the dtrans_feat path by value).

The end-to-end gradient is compared with float64 autograd through pointnet_ref64.forward with the device's gates and arg-max
sets prescribed, under the bars of test_gpu_pointnet.py (sign agreement >= 0.999 above 1e-6 of the largest magnitude, largest
error <= 1e-3 of it).  The reference's own fp32 autograd, with its decisions prescribed, lies within 2.3e-6 of the largest
magnitude of the float64 gradient (measured on the CPU at these shapes); the figures measured here are printed beside it.

Measured on an MI355X (a record, not a bar; every test prints its own): largest error / bound over the six cases and three runs
  a1 0.296  a2 0.056  pool[0] 0.025  f1 0.003  f2 0.006  trans 0.005  t1 0.433  h 0.319  k1 0.073  k2 0.068  pool[1] 0.035
  fk1 0.004  fk2 0.006  tf 0.014  c2f 0.162  h1pf 0.191  e2 0.078  pool[2] 0.025  part 0.026  gb 0.004  z1 0.059  z2 0.010
  z3 0.021  logits 0.029  logp 0.366  dz4 0.993 (the one rounding of the final difference, u |dz4|, where softmax * sum is small)
  dz3 0.221  dz2 0.038  dz1 0.020  s1 0.008  dg 0.008  dpf 0.018  dtf 0.087  dfk2 0.001  dfk1 0.014  dgk 0.009  dh 0.162
  dxu 0.049  dtrans 0.014  df2 0.212  df1 0.017  dgs 0.008  dx0 0.661
0 of 4 690 944 sign bits differ from the float64 sign; every exact stage, arg-max rule and tile reduce holds; end to end the
largest error is 1.98e-6 of the largest magnitude with both cotangents and 1.40e-6 with dlogp = 0."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pointnet_ref64 as ref64  # noqa: E402
import pointnet_stages_ref64 as S  # noqa: E402

PN_SEED = 3
REFERENCE_OWN = 2.3e-6


@pytest.fixture(scope="module")
def sd():
    from pointsecguard_amd import synthetic
    return synthetic.pointnet_state_dict(PN_SEED)


@pytest.fixture(scope="module")
def folded(sd):
    from pointsecguard_amd import runtime
    return runtime.fold_pointnet_state_dict(sd)


@pytest.fixture(scope="module")
def model(folded):
    from pointsecguard_amd import runtime
    return runtime.PointNetModel(folded)


def snapshot(ws, names):
    t = {}
    for k in names:
        a = ws.debug(k).cpu().numpy()
        t[k] = S.unpack_bits(a.view(np.uint32), S.BITS[k][1]) if k in S.BITS else a
    return t


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def device_runs(model):
    """one forward and three backwards per case, every buffer read through the tap; computed once, shared by the tests"""
    from pointsecguard_amd import runtime
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        B, N, x0, dlogp, dtf = S.make_case(name)
        ws = runtime.PointNetWorkspace(B, N)
        logp, tf = ws.forward(model, cuda(x0))
        fwd = snapshot(ws, S.FWD_FLOAT + S.FWD_INT + tuple(S.BITS))
        runs = []
        for run in S.RUNS:
            dl, up = S.cotangents(run, dlogp, dtf)
            dx0 = ws.backward(model, cuda(dl), cuda(up))
            bwd = snapshot(ws, S.BWD)
            bwd["dx0"] = dx0.cpu().numpy().reshape(B * N, 9)
            runs.append((dl, up, bwd))
        torch.cuda.synchronize()
        cache[name] = dict(B=B, N=N, x0=x0, fwd=fwd, runs=runs, ws=ws, logp=logp.cpu().numpy(), tf=tf.cpu().numpy())
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(S.CASES))
def test_every_stage_within_its_bound(folded, device_runs, name):
    c = device_runs(name)
    B, N, fwd = c["B"], c["N"], c["fwd"]
    rep, reps = S.check_case(S.params(folded), B, N, c["x0"], fwd, c["runs"])
    flips = sum(a for a, _ in rep.flips.values())
    print("%s: sign bits that differ from float64 inside the bound: %d of %d" % (name, flips, sum(b for _, b in rep.flips.values())))
    print("%s: largest error / bound, forward: %s" % (name, " ".join("%s %.3f" % kv for kv in rep.ratio.items())))
    for run, r in zip(S.RUNS, reps):
        print("%s: largest error / bound, backward (%s): %s" % (name, run, " ".join("%s %.3f" % kv for kv in r.ratio.items())))
    assert not rep.fail, rep.fail
    for run, r in zip(S.RUNS, reps):
        assert not r.fail, (run, r.fail)
        assert r.stages == list(S.BWD) + ["dx0"]
    assert len(rep.stages) == 57 and len(rep.flips) == 8
    assert np.array_equal(c["logp"].reshape(B * N, 13), fwd["logp"]) and np.array_equal(c["tf"].reshape(B, 4096), fwd["tf"])
    if name == "dup":
        assert fwd["pidx"].max() < 64
    if name == "const":
        assert not fwd["pidx"].any() and not fwd["part_idx"].any()


def _sign_agree(a, b):
    big = np.abs(b) > 1e-6 * np.abs(b).max()
    return (np.sign(a[big]) == np.sign(b[big])).mean()


@pytest.mark.parametrize("name", list(S.CASES))
def test_input_gradient_against_float64_with_the_device_decisions(sd, device_runs, name):
    c = device_runs(name)
    B, N = c["B"], c["N"]
    dec = ref64.device_decisions(c["fwd"], B, N)
    x = torch.from_numpy(np.ascontiguousarray(c["x0"].transpose(0, 2, 1))).double().requires_grad_(True)
    logp, tf = ref64.forward(sd, x, decide=dec)
    for run, (dl, up, bwd) in zip(S.RUNS, c["runs"]):
        if run == "no_dtf":
            continue
        loss = (logp * torch.from_numpy(dl).double()).sum() + (tf * torch.from_numpy(up).double()).sum()
        want = torch.autograd.grad(loss, x, retain_graph=True)[0].numpy().transpose(0, 2, 1)
        got = bwd["dx0"].reshape(B, N, 9)
        assert np.all(got[:, :, 6:] == 0.0) and np.all(want[:, :, 6:] == 0.0)
        got, want = got[:, :, :6].astype(np.float64), want[:, :, :6]
        err, agree = np.abs(got - want).max() / np.abs(want).max(), _sign_agree(got, want)
        print("%s (%s): largest error %.3g of the largest magnitude (the reference's own fp32 autograd, decisions prescribed: <= %.1e); "
              "sign agreement %.5f" % (name, run, err, REFERENCE_OWN, agree))
        assert agree >= 0.999
        assert err <= 1e-3


def dims(B, N):
    R, T = B * N, B * N // 128
    d = {"a1": (R, 64), "a2": (R, 128), "h": (R, 64), "k1": (R, 64), "k2": (R, 128), "e2": (R, 128), "z1": (R, 512), "z2": (R, 256),
         "z3": (R, 128), "logits": (R, 13), "logp": (R, 13), "x0in": (R, 9), "mh": (R, 2), "m1": (R, 16), "m2": (R, 8), "m3": (R, 4),
         "mf1": (B, 16), "mf2": (B, 8), "mfk1": (B, 16), "mfk2": (B, 8), "pool": (B, 3072), "pidx": (B, 3072), "part_val": (T, 1024),
         "part_idx": (T, 1024), "f1": (B, 512), "f2": (B, 256), "trans": (B, 9), "fk1": (B, 512), "fk2": (B, 256), "tf": (B, 4096),
         "t1": (64, 3 * B), "w1f": (64 * B, 8), "c2f": (128, 64 * B), "h1pf": (512, 64 * B), "gb": (B, 512),
         "dz4": (R, 13), "dz3": (R, 128), "dz2": (R, 256), "dz1": (R, 512), "s1": (B, 512), "dg": (B, 1024), "dpf": (R, 64),
         "ht": (64 * B, N), "dpft": (64 * B, N), "dtf": (B, 4096), "dfk2": (B, 256), "dfk1": (B, 512), "dgk": (B, 1024), "dh": (R, 64),
         "dxu": (R, 8), "dtrans": (B, 9), "df2": (B, 256), "df1": (B, 512), "dgs": (B, 1024)}
    return d


def test_tap_contract(model):
    """NULL with the error string for a null workspace and for unknown codes; the documented row and column counts; and a
    forward / backward give bit-identical logp / dx0 whether or not the tap was read in between"""
    from pointsecguard_amd import _lib, runtime
    lib = _lib.load()
    assert not lib.psg_pointnet_debug_ptr(None, 0, None, None)
    assert b"psg_pointnet_debug_ptr" in lib.psg_last_error() and b"null workspace" in lib.psg_last_error()
    B, N, x0, dlogp, dtf = S.make_case("b3n128")
    ws = runtime.PointNetWorkspace(B, N)
    codes = runtime.PointNetWorkspace.DEBUG
    assert sorted(codes) == sorted(S.FWD_FLOAT + S.FWD_INT + tuple(S.BITS) + S.BWD) and len(set(codes.values())) == len(codes)
    for what in sorted(set(range(-2, 90)) - set(codes.values())) + [1 << 20]:
        rows, cols = ctypes.c_int(-7), ctypes.c_int(-7)
        assert not lib.psg_pointnet_debug_ptr(ws.handle, what, ctypes.byref(rows), ctypes.byref(cols)), what
        assert b"psg_pointnet_debug_ptr: unknown buffer code" in lib.psg_last_error()
        assert rows.value == -7 and cols.value == -7
    want = dims(B, N)
    assert sorted(want) == sorted(codes)
    for k, code in codes.items():
        rows, cols = ctypes.c_int(), ctypes.c_int()
        assert lib.psg_pointnet_debug_ptr(ws.handle, code, ctypes.byref(rows), ctypes.byref(cols)), k
        assert (rows.value, cols.value) == want[k], k
        assert lib.psg_pointnet_debug_ptr(ws.handle, code, None, None), k      # the counts are optional
    x, dl, up = cuda(x0), cuda(dlogp), cuda(dtf)
    logp_a, _ = ws.forward(model, x)
    for k in S.FWD_FLOAT + S.FWD_INT + tuple(S.BITS):
        ws.debug(k)
    dx_a = ws.backward(model, dl, up)
    for k in codes:
        ws.debug(k)
    ws2 = runtime.PointNetWorkspace(B, N)
    logp_b, _ = ws2.forward(model, x)
    dx_b = ws2.backward(model, dl, up)
    logp_c, _ = ws.forward(model, x)                                            # the tapped workspace again, untapped this time
    dx_c = ws.backward(model, dl, up)
    assert torch.equal(logp_a, logp_b) and torch.equal(dx_a, dx_b)
    assert torch.equal(logp_a, logp_c) and torch.equal(dx_a, dx_c)


@pytest.mark.parametrize("targeted", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_fused_nb_attack_is_its_eager_composition(model, targeted, masked):
    """psg_pointnet_nb_attack against the same sequence from the public entry points - psg_to_point_major, then per iteration
    forward, psg_ce_logp_grad, backward, psg_pgd_step with the arguments the fused call passes, then psg_to_channel_major -
    bit for bit.  Non-targeted: CE over all rooms' rows with their labels, ascent; targeted: CE over room 0's rows only with
    the target class, descent; the un-projected step on the last iteration only."""
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd import synthetic
    p, st = runtime.ptr, runtime.stream
    B, N, iters, eps, alpha, target = 3, 128, 3, 0.1, 0.05, 6
    rooms = synthetic.make_rooms(B, 17, num_point=N)
    images = cuda(rooms.transpose(0, 2, 1))
    labels = cuda(synthetic.rule_labels(rooms).astype(np.int32))
    mask = cuda((np.arange(N) % 3 != 0).astype(np.uint8)) if masked else None
    ws = runtime.PointNetWorkspace(B, N)
    fused = ws.nb_attack(model, images, None if targeted else labels, eps, alpha, iters, mask=mask, target=target if targeted else None)
    ws2 = runtime.PointNetWorkspace(B, N)
    x0 = torch.empty(B, N, 9, device="cuda")
    _lib.call("psg_to_point_major", p(images), B, 9, N, p(x0), st())
    ori = x0[:, :, 3:6].contiguous()
    dlogp = torch.empty(B, N, 13, device="cuda")
    for it in range(iters):
        logp, _ = ws2.forward(model, x0)
        _lib.call("psg_ce_logp_grad", p(logp), None if targeted else p(labels), target if targeted else 0, B * N, N if targeted else B * N, 13,
                  1.0 / N, p(dlogp), None, st())
        dx0 = ws2.backward(model, dlogp)
        _lib.call("psg_pgd_step", p(x0), p(dx0), p(ori), p(mask), B, N, alpha, eps, -1.0 if targeted else 1.0, int(it == iters - 1), st())
    eager = torch.empty_like(images)
    _lib.call("psg_to_channel_major", p(x0), B, 9, N, p(eager), st())
    assert torch.equal(fused, eager)
    assert not torch.equal(fused[:, 3:6], images[:, 3:6])
    assert torch.equal(fused[:, :3], images[:, :3]) and torch.equal(fused[:, 6:], images[:, 6:])
    if masked:
        keep = ~mask.bool()
        assert torch.equal(fused[:, 3:6][:, :, keep], images[:, 3:6][:, :, keep])
