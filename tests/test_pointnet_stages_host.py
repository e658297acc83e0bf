"""CPU tests of the PointNet stage reference (tests/pointnet_stages_ref64.py): a float32 emulation of the whole forward and
backward - the same stage functions with dt = float32, in the device's order, producing the same named buffers - passes
EVERY stage check at every case of tests/test_gpu_pointnet_stages.py, so the derived bounds admit an honest float32
evaluation; eleven single faults injected into that emulation each fail at the stage that is wrong and at nothing upstream
of it; and the stage functions chained in float64 ARE the reference-pinned restatement tests/pointnet_ref64.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pointnet_ref64 as ref64  # noqa: E402
import pointnet_stages_ref64 as S  # noqa: E402

PN_SEED = 3


@pytest.fixture(scope="module")
def sd():
    from pointsecguard_amd import synthetic
    return synthetic.pointnet_state_dict(PN_SEED)


@pytest.fixture(scope="module")
def P(sd):
    from pointsecguard_amd import runtime
    return S.params(runtime.fold_pointnet_state_dict(sd))


def emulate(P, name, dt=np.float32, fwd_faults=(), bwd_faults=(), runs=S.RUNS):
    B, N, x0, dlogp, dtf = S.make_case(name)
    fwd, _ = S.walk_forward(P, x0, B, N, dt=dt, faults=fwd_faults)
    out = []
    for run in runs:
        dl, up = S.cotangents(run, dlogp, dtf)
        bwd, _ = S.walk_backward(P, fwd, dl.reshape(B * N, S.NCLS), None if up is None else up.reshape(B, 4096), B, N, dt=dt,
                                 faults=bwd_faults)
        out.append((dl, up, bwd))
    return B, N, x0, fwd, out


@pytest.fixture(scope="module")
def good(P):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = emulate(P, name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(S.CASES))
def test_float32_emulation_passes_every_stage(P, good, name):
    B, N, x0, fwd, runs = good(name)
    rep, reps = S.check_case(P, B, N, x0, fwd, runs)
    assert not rep.fail, rep.fail
    for run, r in zip(S.RUNS, reps):
        assert not r.fail, (run, r.fail)
        assert r.stages == list(S.BWD) + ["dx0"]
    assert len(rep.stages) == 57 and len(rep.flips) == 8
    flips = sum(a for a, _ in rep.flips.values())
    print("%s: sign bits inside the bound: %d of %d" % (name, flips, sum(b for _, b in rep.flips.values())))
    print("%s: largest error / bound: forward %s" % (name, {k: round(v, 3) for k, v in rep.ratio.items()}))
    for run, r in zip(S.RUNS, reps):
        print("%s / %s: %s" % (name, run, {k: round(v, 3) for k, v in r.ratio.items()}))
    # what the two tie cases are for
    if name == "dup":
        assert fwd["pidx"].max() < 64
        assert np.array_equal(x0[:, 127], x0[:, 128])
        for b in range(B):                                      # 64 distinct rows, each at least twice: every channel is a tie
            _, cnt = np.unique(x0[b], axis=0, return_counts=True)
            assert len(cnt) == 64 and cnt.min() >= 2
    if name == "const":
        assert not fwd["pidx"].any() and not fwd["part_idx"].any()
    # the pool-gate faults below need dead pooled channels, the double count a point that owns two channels
    assert (fwd["pool"][:, :2048] == 0).any()


FWD_FAULTS = {"argmax_last": None, "gate_ge": ["mh.exact", "mh"], "t1_untransposed": ["t1"]}
BWD_FAULTS = {"no_pool_gate_k": "dh", "no_pool_gate_a": "dx0", "dtf_transposed": "dtf", "dtf_dropped": "dtf", "dz4_no_sum": "dz4",
              "dtrans_transposed": "dtrans", "s1_drop_last": "s1", "double_count": "dpf"}


def test_every_fault_is_covered():
    assert sorted(list(FWD_FAULTS) + list(BWD_FAULTS)) == sorted(S.FAULTS)


@pytest.mark.parametrize("name", ["dup", "const"])
def test_last_index_on_ties_fails_the_first_index_rule(P, name):
    """arg-max takes the LAST index on ties (in the tile and across the tiles): rule (ii) fails on all three pools and on
    the tile partials, and nothing else does - value and validity (i) cannot see it"""
    B, N, x0, fwd, _ = emulate(P, name, fwd_faults=("argmax_last",), runs=())
    _, rep = S.walk_forward(P, x0, B, N, taps=fwd)
    want = ["pool[0].first", "pool[1].first", "pool[2].first", "part.first"]
    if N > S.PT:
        want.append("pidx[2].reduce")                           # pool[2].reduce: the tied values are equal
    assert S.failing(rep) == want, rep.fail


@pytest.mark.parametrize("fault", [f for f in FWD_FAULTS if f != "argmax_last"])
def test_forward_fault_fails_at_its_stage(P, fault):
    """gate_ge: the bit of the `h` layer is taken with >= 0 on the stored activation (every bit set), so the words no longer
    equal (activation > 0); t1_untransposed: trans_b instead of trans_b^T in the per-room conv1 weights.  The snapshot is the
    whole wrong network's, as a device with that fault would show it: every later stage is consistent with it and passes"""
    B, N, x0, fwd, runs = emulate(P, "b3n128", fwd_faults=(fault,), runs=("both",))
    rep, reps = S.check_case(P, B, N, x0, fwd, runs)
    assert S.failing(rep) == FWD_FAULTS[fault], rep.fail
    assert not reps[0].fail, reps[0].fail


@pytest.mark.parametrize("fault", list(BWD_FAULTS))
def test_backward_fault_fails_at_its_stage(P, good, fault):
    B, N, x0, fwd, _ = good("b3n128")
    dlogp, dtf = S.make_case("b3n128")[3:]
    for run in S.RUNS:
        dl, up = S.cotangents(run, dlogp, dtf)
        args = (dl.reshape(B * N, S.NCLS), None if up is None else up.reshape(B, 4096), B, N)
        bwd, _ = S.walk_backward(P, fwd, *args, dt=np.float32, faults=(fault,))
        _, rep = S.walk_backward(P, fwd, *args, taps=bwd)
        silent = (fault.startswith("dtf_") and up is None) or (run == "dlogp0" and fault in ("dz4_no_sum", "s1_drop_last", "double_count"))
        assert S.failing(rep) == ([] if silent else [BWD_FAULTS[fault]]), (run, rep.fail)


def _x(x0):
    return torch.from_numpy(np.ascontiguousarray(x0.transpose(0, 2, 1))).double()


@pytest.mark.parametrize("name", ["b3n128", "dup"])
def test_float64_stages_compose_to_the_restatement(sd, name):
    """the stage functions, chained in float64 on the unrounded fold with their own decisions, reproduce
    pointnet_ref64.forward and .grads (NLL, and NLL + 0.001 regulariser through the dtrans_feat addend) to 1e-9; and
    pointnet_ref64.forward with those decisions PRESCRIBED is the same function"""
    from pointsecguard_amd import runtime
    P64 = S.params(runtime.fold_pointnet_state_dict(sd, dtype=np.float64))
    B, N, x0, _, _ = S.make_case(name)
    fwd, _ = S.walk_forward(P64, x0, B, N)
    logp, tf = ref64.forward(sd, _x(x0))
    assert np.abs(fwd["logp"].reshape(B, N, 13) - logp.numpy()).max() <= 1e-9
    assert np.abs(fwd["tf"].reshape(B, 64, 64) - tf.numpy()).max() <= 1e-9
    snap = dict(fwd)
    for k, (act, _) in S.BITS.items():
        snap[k] = fwd[act] > 0
    lp2, tf2 = ref64.forward(sd, _x(x0), decide=ref64.device_decisions(snap, B, N))
    assert np.abs(lp2.numpy() - logp.numpy()).max() <= 1e-12 and np.abs(tf2.numpy() - tf.numpy()).max() <= 1e-12
    labels = torch.from_numpy(np.random.default_rng(2).integers(0, 13, (B, N)))
    dlogp = np.zeros((B * N, 13))
    dlogp[np.arange(B * N), labels.reshape(-1).numpy()] = -1.0 / (B * N)
    for with_reg in (False, True):
        up = None
        if with_reg:
            t = torch.from_numpy(fwd["tf"].reshape(B, 64, 64)).requires_grad_(True)
            (ref64.regulariser(t) * 0.001).backward()
            up = t.grad.numpy().reshape(B, 4096)
        bwd, _ = S.walk_backward(P64, snap, dlogp, up, B, N)
        want = ref64.grads(sd, _x(x0), labels, with_reg=with_reg).numpy().transpose(0, 2, 1)
        got = bwd["dx0"].reshape(B, N, 9)
        assert np.all(got[:, :, 6:] == 0) and np.all(want[:, :, 6:] == 0)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
