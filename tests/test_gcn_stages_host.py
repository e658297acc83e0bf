"""CPU tests of the ResGCN stage reference (tests/gcn_stages_ref64.py): its restatement of the host fold lies within one
rounding per entry of the same fold in float64; the stage functions chained in float64 agree with oracle.resgcn.GCNOracle
(pinned to the reference project's fixtures) on the same graphs for all six configurations; a float32 emulation of the whole
forward and backward - the same stage functions with dt = float32 in two k orders, producing the same named buffers - passes
EVERY stage check at every case of tests/test_gpu_gcn_stages.py, so the derived bounds admit an honest float32 evaluation;
and thirteen single faults injected into that emulation each fail at the stage that is wrong and at nothing upstream of it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gcn_stages_ref64 as S  # noqa: E402
from test_oracle_resgcn_variants import check_dx  # noqa: E402

SEED = 5
NB = S.N_BLOCKS


@pytest.fixture(scope="module")
def models():
    from pointsecguard_amd import synthetic
    cache = {}

    def get(block, conv, faults=(), rounded=True):
        key = (block, conv, tuple(faults), rounded)
        if key not in cache:
            cache[key] = S.fold(synthetic.gcn_state_dict(SEED, NB, block, conv), NB, block, conv, rounded=rounded, faults=faults)
        return cache[key]
    return get


def emulate(M, name, fixed=False, order="plain", fwd_faults=(), bwd_faults=(), runs=S.RUNS, dt=np.float32):
    B, N, x0, dl, graphs = S.make_case(name)
    g = graphs if fixed else None
    fwd, _ = S.walk_forward(M, x0, B, N, dt=dt, faults=fwd_faults, order=order, graphs=g)
    out = []
    for run in runs:
        d = S.cotangent(run, dl)
        bwd, _ = S.walk_backward(M, fwd, d.reshape(B * N, S.NCLS), B, N, dt=dt, faults=bwd_faults, order=order)
        out.append((d, bwd))
    return B, N, x0, fwd, out, g


def _leaves(M):
    for k, v in M.items():
        if k == "edge":
            for e, L in enumerate(v):
                for kk, vv in L.items():
                    yield "edge%d.%s" % (e, kk), vv
        elif isinstance(v, np.ndarray):
            yield k, v


@pytest.mark.parametrize("block,conv", S.CONFIGS)
def test_fold_is_one_rounding_from_the_float64_fold(models, block, conv):
    held, exact = dict(_leaves(models(block, conv))), dict(_leaves(models(block, conv, rounded=False)))
    assert sorted(held) == sorted(exact) and len(held) == 8 * NB + 18
    for k, a in held.items():
        b = exact[k]
        assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape, k
        assert np.all(np.abs(a.astype(np.float64) - b) <= S.U * np.abs(b)), k
    if block == "dense":   # the fold really sums: a later copy of y_0 alone is not the folded column
        assert held["wf"].shape == (1024, 64 * NB)


CASE_CONFIGS = [(n, b, c) for n in S.CASES for (b, c) in (S.CONFIGS if n in S.ALL_CONFIG_CASES else [("res", "edge")])]


@pytest.mark.parametrize("name,block,conv", CASE_CONFIGS)
def test_float32_emulation_passes_every_stage(models, name, block, conv):
    M = models(block, conv)
    worst = {}
    for order in ("plain", "blocks8"):
        for fixed in (False, True):
            B, N, x0, fwd, runs, g = emulate(M, name, fixed, order)
            rep, reps = S.check_case(M, B, N, x0, fwd, runs, graphs=g)
            assert not rep.fail, (order, fixed, rep.fail)
            assert rep.stages == S.fwd_stages(block, conv, NB, N, fixed)
            for r in reps:
                assert not r.fail, (order, fixed, r.fail)
                assert r.stages == S.bwd_stages(block, conv, NB)
            flips = sum(a for a, _ in rep.flips.values())
            assert flips <= S.MASK_CAP * sum(b for _, b in rep.flips.values())
            for r in [rep] + reps:
                for k, v in r.ratio.items():
                    worst[k] = max(worst.get(k, 0.0), v)
            if name == "const" and not fixed:
                assert not fwd["farg"].any()
                assert all(not (fwd["arg%d" % e] & 0x7F).any() for e in range(NB))
    print("%s %s/%s: largest error / bound: %s" % (name, block, conv, " ".join("%s %.3f" % kv for kv in worst.items())))


def test_every_fault_is_covered():
    assert sorted(list(FWD_FAULTS) + list(BWD_FAULTS) + list(FOLD_FAULT_STAGE)) == sorted(S.FAULTS)


def _edge_group(e):
    return {k % e for k in ("y%d", "arg%d.valid", "arg%d.ties", "act%d")}


# fault -> (case, block, conv, the stage that must fail first, what else may fail because it shares the wrong value)
FWD_FAULTS = {
    "gate_ge": ("b3n96", "res", "edge", "mask_f", set()),
    "q_global_row": ("b3n96", "res", "edge", "y1", _edge_group(1)),
    "gb1_room0": ("b3n96", "res", "edge", "h1", {"mask1"}),
    "resid_dropped": ("b3n96", "res", "edge", "y1", set()),
    "resid_twice": ("b3n96", "res", "mr", "y1", set()),
    "gmax_last": ("dup", "res", "edge", "farg", set()),
    "edge_last": None,
}
BWD_FAULTS = {"g1sum_drop_last": ("b3n96", "res", "edge", "g1sum"), "fusion_ignores_mask": ("const", "res", "edge", "dfeats_fusion"),
              "dq_slot0": ("b3n96", "plain", "edge", "dpq1")}
FOLD_FAULT_STAGE = {"dense_fold_skipped": ("dense", "edge", "fwd", "fused", {"mask_f"}),
                    "w1_for_w1mw2": ("res", "edge", "fwd", "pq1", _edge_group(1)),
                    "s1_not_in_wp1a": ("res", "edge", "bwd", "gfvec", set())}


def _assert_fails_at(rep, first, also):
    got = S.failing(rep)
    assert got and got[0] == first and set(got) <= {first} | also, (got, rep.fail[:3])


@pytest.mark.parametrize("fault", [f for f in FWD_FAULTS if FWD_FAULTS[f]])
def test_forward_fault_fails_at_its_stage(models, fault):
    """the snapshot is the whole wrong network's, as a device with that fault would show it: every other stage is consistent
    with it and passes, the backward included"""
    name, block, conv, first, also = FWD_FAULTS[fault]
    M = models(block, conv)
    B, N, x0, fwd, runs, _ = emulate(M, name, fwd_faults=(fault,), runs=("normal",))
    rep, reps = S.check_case(M, B, N, x0, fwd, runs)
    _assert_fails_at(rep, first, also)
    assert not reps[0].fail, reps[0].fail


@pytest.mark.parametrize("name", ["dup", "const"])
@pytest.mark.parametrize("conv", S.CONVS)
def test_last_slot_on_ties_fails_the_first_slot_rule(models, name, conv):
    """the edge arg-max (mr: the max-relative gather) keeps the LAST slot on ties: the tie rule (mr: the exact arg byte)
    fails and nothing else does - the tied values are equal, so value and validity cannot see it"""
    M = models("res", conv)
    B, N, x0, fwd, _, _ = emulate(M, name, fwd_faults=("edge_last",), runs=())
    _, rep = S.walk_forward(M, x0, B, N, taps=fwd)
    got = S.failing(rep)
    want = ["arg%d.ties" % e for e in range(NB)] if conv == "edge" else ["arg_mr%d" % e for e in range(NB)]
    assert got and set(got) <= set(want), rep.fail[:3]
    if name == "const":
        assert got == want


@pytest.mark.parametrize("fault", list(BWD_FAULTS))
def test_backward_fault_fails_at_its_stage(models, fault):
    name, block, conv, stage = BWD_FAULTS[fault]
    M = models(block, conv)
    B, N, x0, fwd, _, _ = emulate(M, name, runs=())
    if fault == "fusion_ignores_mask":                          # needs a pooled channel whose ReLU was off at its arg-max point
        rows = (np.arange(B)[:, None] * N + fwd["farg"]).reshape(-1)
        assert not fwd["mask_f"][rows, np.tile(np.arange(1024), B)].all()
    dl = S.make_case(name)[3]
    for run in S.RUNS:
        d = S.cotangent(run, dl).reshape(B * N, S.NCLS)
        bwd, _ = S.walk_backward(M, fwd, d, B, N, dt=np.float32, faults=(fault,))
        _, rep = S.walk_backward(M, fwd, d, B, N, taps=bwd)
        assert S.failing(rep) == ([] if run == "zero" else [stage]), (run, rep.fail[:3])


@pytest.mark.parametrize("fault", list(FOLD_FAULT_STAGE))
def test_fold_fault_fails_at_its_stage(models, fault):
    """a device that holds a wrongly folded weight, checked with the right fold"""
    block, conv, side, first, also = FOLD_FAULT_STAGE[fault]
    good, bad = models(block, conv), models(block, conv, faults=(fault,))
    B, N, x0, fwd, runs, _ = emulate(bad, "b3n96", runs=("normal",))
    rep, reps = S.check_case(good, B, N, x0, fwd, runs)
    if side == "fwd":
        _assert_fails_at(rep, first, also)
    else:
        assert not rep.fail, rep.fail
        _assert_fails_at(reps[0], first, also)


@pytest.mark.parametrize("block,conv", S.CONFIGS)
def test_float64_walk_agrees_with_the_oracle(models, block, conv):
    """the stage functions chained in float64 on the held weights against GCNOracle (float32 / float64 mixed, edge by edge
    without the split identity) on the walk's graphs, room by room, under the bars of test_oracle_resgcn_variants.py"""
    from oracle import resgcn
    from pointsecguard_amd import synthetic
    M = models(block, conv)
    orc = resgcn.GCNOracle(synthetic.gcn_state_dict(SEED, NB, block, conv), NB, block=block, conv=conv)
    B, N, x0, fwd, runs, _ = emulate(M, "b3n96", runs=("normal",), dt=np.float64)
    dl, bwd = runs[0]
    for b in range(B):
        sl = slice(b * N, (b + 1) * N)
        logits, cache = orc.forward(x0[b], graphs=[fwd["nbr%d" % e][sl] for e in range(NB)])
        want = fwd["logits"][sl]
        assert np.abs(logits - want).max() <= 2e-4 * max(1.0, np.abs(want).max())
        check_dx(orc.backward(cache, dl[b]), bwd["dx0"][sl])
