"""ResGCN, stage by stage: every launch of psg_gcn_forward / psg_gcn_backward (csrc/psg_resgcn.hip) against the float64
statement of ITS OWN operation (tests/gcn_stages_ref64.py, which documents every bound) on ITS OWN inputs, read through the
workspace tap psg_gcn_debug_ptr, the per-block buffers through the kept copies of psg_gcn_debug_keep.  Every stage is fed what
the GPU produced, and the backward stages take the GPU's decisions (ReLU bit words, arg bytes, graphs, farg) as inputs, so a
last-bit flip cannot move an entry downstream and every bound is asserted on EVERY entry.  tests/test_gcn_stages_host.py
shows on the CPU that a float32 evaluation meets every bound and that thirteen single faults each fail at their stage.

n_blocks = 5 (F = 320: fusion_bwd_kernel runs two z-slices, the second ragged; dense widths reach 256, dilations 4).  Cases
(gcn_stages_ref64.make_case): (1, 96) the bf16 kNN, N off the 64-row chunks; (3, 96) GEMM tiles and the gbias row group straddle
rooms; (2, 112) the exact fused kNN and xp without bp; (2, 200) the matrix kNN, the PQ-fusion fallback, ragged everywhere;
"dup" and "const": exact ties in the kNN, in every edge max and in the global max.  Each case is one forward and two
backwards (a standard-normal dlogits, and dlogits = 0) under debug_keep(True), with dynamic graphs and once more with
teacher-forced graphs that repeat a neighbour in every row.  All six configurations run on (3, 96) and (2, 200), res / edge on
every case.

The end-to-end gradient is compared with the float64 walk of the backward on the device's decisions, under the bars of
test_gpu_resgcn.py (sign agreement >= 0.999 above 1e-6 of the largest magnitude, largest error <= 1e-3 of it).

Measured on an MI355X (a record, not a bar; every test prints its own): largest error / bound over all cases, configurations,
both graph modes and both backward runs
  pq{e} 0.281  y{e} 0.205  sq 0.054  fused 0.023  gb1 0.000  h1 0.020  h2 0.013  logits 0.018  g2 0.257  g1 0.023
  dfeats_head 0.012  g1part 0.036  g1sum 0.318  gfvec 0.001  dfeats_fusion 0.985 (the one rounding of dfeats + part where the
  part is small)  dpq{e} 0.358  state{e} 0.442  dx0 0.276
1 of 20 680 704 sign bits differs from the float64 sign (inside its bound); every exact stage, graph, arg-max and tie rule
holds, on the default path and under PSG_GCN_PQ_FUSION=1, PSG_GCN_EDGE_BWD=atomic and PSG_GEMM_SMALL_BELOW=0
(test_gpu_alt_paths.py).  End to end the largest error is 1.04e-6 of the largest magnitude, sign agreement 1.00000.
No kernel fault was found.  The reference project's own figure (its DenseDeepGCN loaded as tests/golden/make_golden_gcn_variants.py
loads it, n_blocks = 5, fp32 autograd against its float64 run on the fp32 run's graphs, on the CPU at these six cases for
res / edge, plain / edge and dense / mr): 2.5e-7 .. 8.1e-7 of the largest magnitude.  A record, not a bar."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gcn_stages_ref64 as S  # noqa: E402

SEED, NB = 5, S.N_BLOCKS
REFERENCE_OWN = 8.1e-7
BLOCK_CODE, CONV_CODE = {"res": 0, "plain": 1, "dense": 2}, {"edge": 0, "mr": 1}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def nets():
    """(held weights for the reference, device model) per configuration"""
    from pointsecguard_amd import runtime, synthetic
    cache = {}

    def get(block, conv):
        if (block, conv) not in cache:
            sd = synthetic.gcn_state_dict(SEED, NB, block, conv)
            cache[block, conv] = (S.fold(sd, NB, block, conv), runtime.GCNModel(sd, NB, block=BLOCK_CODE[block], conv=CONV_CODE[conv]))
        return cache[block, conv]
    return get


def new_ws(B, N, block, conv):
    from pointsecguard_amd import runtime
    return runtime.GCNWorkspace(B, N, NB, block=BLOCK_CODE[block], conv=CONV_CODE[conv])


def forward_taps(ws, x0, B, N, conv, fixed):
    g = lambda k, e=0: ws.debug(k, e).cpu().numpy()             # noqa: E731
    t = {"x0": x0.reshape(B * N, 9)}
    for k in ("xyz", "feats", "fused", "fmax", "farg", "gb1", "h1", "h2", "logits"):
        t[k] = g(k)
    for k, m in (("mask_f", 1024), ("mask1", 512), ("mask2", 256)):
        t[k] = S.unpack_bits(g(k).view(np.uint32), m)
    for e in range(NB):
        t["nbr%d" % e] = g("nbr", e)
        if conv == "edge":
            t["pq%d" % e], t["arg%d" % e] = g("k_pq", e), g("arg", e)
        else:
            t["cat%d" % e], t["arg_mr%d" % e] = g("k_pq", e), g("arg_mr", e)
            t["mask_mr%d" % e] = S.unpack_bits(g("mask_mr", e).view(np.uint32), 64)
    if not fixed:
        t["sq"], t["xp"] = g("sq"), g("xp")
    return t


def backward_taps(ws, dx0, B, N, conv):
    g = lambda k, e=0: ws.debug(k, e).cpu().numpy()             # noqa: E731
    t = {k: g(k) for k in ("g2", "g1", "g1part", "g1sum", "gfvec")}
    t["dfeats_head"], t["dfeats_fusion"] = g("k_dfeats_head"), g("k_dfeats_fusion")
    for e in range(NB):
        t["dpq%d" % e], t["state%d" % e] = g("k_dpq", e), g("k_state", e)
        if conv == "mr":
            t["gz%d" % e] = g("k_gz", e)
    t["dx0"] = dx0.cpu().numpy().reshape(B * N, 9)
    t["k_dx0"], t["dfeats"], t["gcur"] = g("k_dx0"), g("dfeats"), g("gcur")
    return t


@pytest.fixture(scope="module")
def device_runs(nets):
    """one forward and two backwards per (case, configuration, graphs), every buffer read through the tap; computed once"""
    cache = {}

    def get(name, block, conv, fixed):
        key = (name, block, conv, fixed)
        if key in cache:
            return cache[key]
        _, model = nets(block, conv)
        B, N, x0, dl, graphs = S.make_case(name)
        ws = new_ws(B, N, block, conv)
        ws.debug_keep(True)
        if fixed:
            ws.set_graphs(cuda(graphs))
        logits = ws.forward(model, cuda(x0))
        fwd = forward_taps(ws, x0, B, N, conv, fixed)
        runs = []
        for run in S.RUNS:
            d = S.cotangent(run, dl)
            bwd = backward_taps(ws, ws.backward(model, cuda(d)), B, N, conv)
            runs.append((d, bwd))
        torch.cuda.synchronize()
        cache[key] = dict(B=B, N=N, x0=x0, fwd=fwd, runs=runs, graphs=graphs if fixed else None, logits=logits.cpu().numpy())
        return cache[key]
    return get


CASE_CONFIGS = [(n, b, c) for n in S.CASES for (b, c) in (S.CONFIGS if n in S.ALL_CONFIG_CASES else [("res", "edge")])]


@pytest.mark.parametrize("name,block,conv", CASE_CONFIGS)
def test_every_stage_within_its_bound(nets, device_runs, name, block, conv):
    M, _ = nets(block, conv)
    worst, flips, bits = {}, 0, 0
    for fixed in (False, True):
        c = device_runs(name, block, conv, fixed)
        B, N, fwd = c["B"], c["N"], c["fwd"]
        rep, reps = S.check_case(M, B, N, c["x0"], fwd, c["runs"], graphs=c["graphs"])
        for r in [rep] + reps:
            for k, v in r.ratio.items():
                worst[k] = max(worst.get(k, 0.0), v)
        flips += sum(a for a, _ in rep.flips.values())
        bits += sum(b for _, b in rep.flips.values())
        assert not rep.fail, (fixed, rep.fail)
        assert rep.stages == S.fwd_stages(block, conv, NB, N, fixed)
        for (d, bwd), r in zip(c["runs"], reps):
            assert not r.fail, (fixed, r.fail)
            assert r.stages == S.bwd_stages(block, conv, NB)
            # the persistent taps agree with the kept copies
            assert np.array_equal(bwd["k_dx0"], bwd["dx0"])
            if block == "res" and conv == "edge":
                assert np.array_equal(bwd["dfeats"], bwd["dfeats_fusion"]) and np.array_equal(bwd["gcur"], bwd["state0"])
            else:
                assert np.array_equal(bwd["dfeats"], bwd["state0"])
        assert np.array_equal(c["logits"].reshape(B * N, 13), fwd["logits"])
        if name == "const" and not fixed:                       # the tie rules by value
            assert not fwd["farg"].any()
            assert all(not (fwd["arg%d" % e] & 0x7F).any() for e in range(NB))
        if name == "dup" and not fixed:
            assert fwd["farg"].max() < 64
        if not fixed:
            # (conv = mr scatters its backward with float atomics: dx0 is not bit-reproducible run to run, so its hash is of logits)
            h = hashlib.sha256(fwd["logits"].tobytes() + (c["runs"][0][1]["dx0"].tobytes() if conv == "edge" else b"")).hexdigest()[:16]
            print("hash %s %s/%s %s" % (name, block, conv, h))
    print("%s %s/%s: sign bits that differ from float64 inside the bound: %d of %d" % (name, block, conv, flips, bits))
    print("%s %s/%s: largest error / bound: %s" % (name, block, conv, " ".join("%s %.3f" % kv for kv in worst.items())))


def _sign_agree(a, b):
    big = np.abs(b) > 1e-6 * np.abs(b).max()
    return (np.sign(a[big]) == np.sign(b[big])).mean()


@pytest.mark.parametrize("name,block,conv", CASE_CONFIGS)
def test_input_gradient_against_float64_with_the_device_decisions(nets, device_runs, name, block, conv):
    """The backward is linear in dlogits once the forward's decisions are fixed, so the float64 walk of the backward on the
    device's bit words, arg bytes, graphs and farg IS float64 autograd with the decisions prescribed."""
    M, _ = nets(block, conv)
    for fixed in (False, True):
        c = device_runs(name, block, conv, fixed)
        B, N = c["B"], c["N"]
        for run, (d, bwd) in zip(S.RUNS, c["runs"]):
            want = S.walk_backward(M, c["fwd"], d.reshape(B * N, 13), B, N)[0]["dx0"]
            got = bwd["dx0"].astype(np.float64)
            if run == "zero":
                assert not want.any() and not got.any()
                continue
            err, agree = np.abs(got - want).max() / np.abs(want).max(), _sign_agree(got, want)
            print("%s %s/%s fixed=%d: largest error %.3g of the largest magnitude (the reference's own fp32 autograd: <= %.1e); sign "
                  "agreement %.5f" % (name, block, conv, fixed, err, REFERENCE_OWN, agree))
            assert agree >= 0.999
            assert err <= 1e-3


def dims(B, N, block, conv, e):
    R, F = B * N, 64 * NB
    C = S.plan(block, NB, e)["C"]
    wpq = 2 * C if conv == "mr" else 128
    alt = not (block == "res" and conv == "edge")
    d = {"xyz": (R, 3), "feats": (R, F), "nbr": (R, 16), "arg": (R, 64), "sq": (R, 1), "xp": (R, 64), "fused": (R, 1024), "mask_f": (R, 32),
         "fmax": (B, 1024), "farg": (B, 1024), "gb1": (B, 512), "h1": (R, 512), "mask1": (R, 16), "h2": (R, 256), "mask2": (R, 8),
         "logits": (R, 13), "g2": (R, 256), "g1": (R, 512), "g1part": (B * -(-N // 64), 512), "g1sum": (B, 512), "gfvec": (B, 1024),
         "dfeats": (R, F), "gcur": (R, 64), "k_pq": (R, wpq), "k_dfeats_head": (R, F), "k_dfeats_fusion": (R, F), "k_dpq": (R, wpq),
         "k_state": (R, F if alt else 64), "k_dx0": (R, 9)}
    if conv == "mr":
        d.update({"arg_mr": (R, C), "mask_mr": (R, 2), "k_gz": (R, 64)})
    return d


@pytest.mark.parametrize("block,conv", [("res", "edge"), ("dense", "mr")])
def test_tap_contract(nets, block, conv):
    """NULL with the error string and untouched counts for a null workspace, unknown codes, blocks out of range, mr codes on an
    edge workspace and kept codes with keep off; the documented [rows][cols] of every code and block; logits and dx0
    bit-identical with keep on, with keep off and on a fresh workspace (dx0 of conv = mr: up to its float atomics' order)"""
    from pointsecguard_amd import _lib, runtime
    lib = _lib.load()
    _, model = nets(block, conv)
    assert not lib.psg_gcn_debug_ptr(None, 0, 0, None, None)
    assert b"psg_gcn_debug_ptr: null workspace" in lib.psg_last_error()
    B, N, x0, dl, _ = S.make_case("b2n200")
    ws = new_ws(B, N, block, conv)
    codes = runtime.GCNWorkspace.DEBUG
    assert len(set(codes.values())) == len(codes)

    def refused(code, e, why):
        rows, cols = ctypes.c_int(-7), ctypes.c_int(-7)
        assert not lib.psg_gcn_debug_ptr(ws.handle, code, e, ctypes.byref(rows), ctypes.byref(cols)), (code, e)
        assert why in lib.psg_last_error(), (code, e, lib.psg_last_error())
        assert rows.value == -7 and cols.value == -7

    for what in sorted(set(range(-2, 70)) - set(codes.values())) + [1 << 20]:
        refused(what, 0, b"psg_gcn_debug_ptr: unknown buffer code")
    for e in (-1, NB, 1 << 20):
        refused(codes["feats"], e, b"out of range")
    for k in ("k_pq", "k_dfeats_head", "k_dfeats_fusion", "k_dpq", "k_state", "k_dx0"):
        refused(codes[k], 0, b"psg_gcn_debug_keep on")
    if conv == "edge":
        for k in ("arg_mr", "mask_mr"):
            refused(codes[k], 0, b"conv = mr")
    x, d = cuda(x0), cuda(dl)
    logits_off = ws.forward(model, x).clone()
    dx_off = ws.backward(model, d).clone()
    ws.debug_keep(True)
    ws.debug_keep(True)                                         # a second `on` keeps the arena
    for e in range(NB):
        want = dims(B, N, block, conv, e)
        assert sorted(want) == sorted(k for k in codes if conv == "mr" or k not in ("arg_mr", "mask_mr", "k_gz"))
        for k, shape in want.items():
            rows, cols = ctypes.c_int(), ctypes.c_int()
            assert lib.psg_gcn_debug_ptr(ws.handle, codes[k], e, ctypes.byref(rows), ctypes.byref(cols)), (k, e)
            assert (rows.value, cols.value) == shape, (k, e)
            assert lib.psg_gcn_debug_ptr(ws.handle, codes[k], e, None, None)        # the counts are optional
    if conv == "edge":
        refused(codes["k_gz"], 0, b"conv = mr")
    logits_on = ws.forward(model, x).clone()
    for k in dims(B, N, block, conv, 0):
        ws.debug(k, NB - 1)
    dx_on = ws.backward(model, d).clone()
    ws.debug_keep(False)
    refused(codes["k_pq"], 0, b"psg_gcn_debug_keep on")
    logits_off2 = ws.forward(model, x).clone()
    dx_off2 = ws.backward(model, d).clone()
    ws2 = new_ws(B, N, block, conv)
    logits_new, dx_new = ws2.forward(model, x), ws2.backward(model, d)
    for a in (logits_on, logits_off2, logits_new):
        assert torch.equal(a, logits_off)
    for a in (dx_on, dx_off2, dx_new):
        if conv == "edge":
            assert torch.equal(a, dx_off)
        else:
            # conv = mr scatters the max-relative half with float atomics (mr_bwd_scatter_kernel): two runs of ONE workspace
            # already differ in the summation order.  Every run meets the (in-degree + 5) u bound of its stage entry by entry
            # (test_every_stage_within_its_bound); here: equal to 1e-5 of the largest magnitude (~170 u)
            assert float((a - dx_off).abs().max()) <= 1e-5 * float(dx_off.abs().max())


_CHILD = """
import sys
sys.path.insert(0, %r)
import torch
import test_gpu_gcn_stages as T
from pointsecguard_amd import runtime, synthetic
S = T.S
sd = synthetic.gcn_state_dict(T.SEED, T.NB, "res", "edge")
model = runtime.GCNModel(sd, T.NB)
B, N, x0, dl, _ = S.make_case("b3n96")
ws = T.new_ws(B, N, "res", "edge")
tap = sys.argv[1] == "tap"
if tap:
    ws.debug_keep(True); ws.debug_keep(False); ws.debug("feats")
print("[marker] begin", file=sys.stderr, flush=True)
ws.forward(model, T.cuda(x0))
if tap:
    ws.debug("fused"); ws.debug("nbr", 2)
ws.backward(model, T.cuda(dl))
if tap:
    ws.debug("dfeats")
torch.cuda.synchronize()
print("[marker] end", file=sys.stderr, flush=True)
"""


def test_keep_off_issues_the_launches_of_an_untapped_run():
    """PSG_TRACE_SYNC=1 in a child process: the launch-site sequence of one forward + backward with keep switched on and off
    again and taps read in between equals that of the same child without any tap call"""
    seqs = []
    for mode in ("plain", "tap"):
        env = dict(os.environ, PSG_TRACE_SYNC="1")
        out = subprocess.run([sys.executable, "-c", _CHILD % HERE, mode], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
        body = out.stderr.split("[marker] begin")[1].split("[marker] end")[0]
        seqs.append(re.findall(r"\[psg trace\] launch \d+ at (\S+) issued", body))
    assert len(seqs[0]) >= 30 and seqs[0] == seqs[1], (len(seqs[0]), len(seqs[1]))


def test_attack_entry_points_refuse_while_keep_is_on(nets):
    """psg_gcn_nb_attack, psg_gcn_nb_attack_field, psg_gcn_nu_window and psg_gcn_nu_field_window replay captured forwards:
    PSG_ERR_STATE with a message under keep, and they work again after debug_keep(False)"""
    from pointsecguard_amd import _lib
    from pointsecguard_amd.attacks.torchattacks.attacks.nu import ADAM_EPS, BETA1, BETA2
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks import nu_field as F_
    from pointsecguard_amd import synthetic
    _, model = nets("res", "edge")
    B, N, x0, _, _ = S.make_case("b3n96")
    images = cuda(x0.transpose(0, 2, 1))
    labels = cuda(synthetic.rule_labels(x0).astype(np.int32))
    ws = new_ws(B, N, "res", "edge")
    st = F_._GcnFieldState(torch.device("cuda"), B, N, 5)

    def windows():
        F_.init_state(st, images, labels, None, True)
        st.pred.fill_(-1); st.nn_state.fill_(-1); st.nn_xyz.fill_(-1)
        fw = F_.window_args(st, model, ws, B, N, "both", 0, False, 0, 5, 0.0, 1.0, 0.1, 1.0, 1.0, False)
        fw.step0, fw.n_steps, fw.adam_t0, fw.lr, fw.coord_lr = 0, 1, 0, 0.05, 0.004
        p = lambda t: t.data_ptr()                              # noqa: E731
        cw = _lib.GcnNuWindowArgs(
            model=model.handle.value, ws=ws.handle.value, G=B, N=N, mode=0, use_target=0, target=0, neighbour=5, kappa=0.0, tsign=1.0,
            c_f=0.1, c_smooth=1e-4, c_l2=1.0, lr=0.05, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, w=p(st.w), m=p(st.m), v=p(st.v), mask=None,
            n_mask=p(st.n_mask), x0=p(st.x0), ori=p(st.ori), labels=p(st.labels), logits=p(st.logits), dlogits=p(st.dlogits),
            dx0=p(st.dx0), sgrad=p(st.sgrad), pred=p(st.pred), scal=p(st.scal), nn_state=p(st.nn_state), hist=p(st.hist), out=p(st.out),
            active=p(st.active), exit_step=p(st.exit), step0=0, n_steps=1, adam_t0=0)
        return (lambda: ws.nu_window(cw)), (lambda: ws.nu_field_window(fw))

    calls = {"psg_gcn_nb_attack": lambda: ws.nb_attack(model, images, labels, 0.1, 0.05, 2),
             "psg_gcn_nb_attack_field": lambda: ws.nb_attack_field(model, images, labels, 2, 0.1, 0.05, 0.02, 0.01, 2)}
    calls["psg_gcn_nu_window"], calls["psg_gcn_nu_field_window"] = windows()
    ws.debug_keep(True)
    for who, call in calls.items():
        with pytest.raises(_lib.PsgError) as ei:
            call()
        assert "rc=-3" in str(ei.value) and who in str(ei.value) and "psg_gcn_debug_keep is on" in str(ei.value), str(ei.value)
    ws.debug_keep(False)
    ws2 = new_ws(B, N, "res", "edge")
    assert torch.equal(calls["psg_gcn_nb_attack"](), ws2.nb_attack(model, images, labels, 0.1, 0.05, 2))
    assert torch.equal(calls["psg_gcn_nb_attack_field"](), ws2.nb_attack_field(model, images, labels, 2, 0.1, 0.05, 0.02, 0.01, 2))
    for who in ("psg_gcn_nu_window", "psg_gcn_nu_field_window"):
        calls["psg_gcn_nu_window"], calls["psg_gcn_nu_field_window"] = windows()    # a clean state for each
        calls[who]()
        torch.cuda.synchronize()
        assert torch.isfinite(st.dx0).all() and float(st.dx0.abs().max()) > 0 and int(st.pred.min()) >= 0
