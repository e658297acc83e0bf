"""Host tests of the lockstep RandLA-Net TBIM / tar_NBattack: the integer exit test against the host loop's double-precision
one, the numpy restatement of the lockstep loop (tests/rla_tbim_ref.py) against TBIM.batch_attack's control flow on scripted
networks, the mutants that restatement must tell apart, and the C ABI of the new entry points."""
import ctypes

import numpy as np
import pytest

import rla_tbim_ref as R

N, NM, TARGET, ORI = 20, 10, 7, 2        # 10 masked points: 9 hits are ON 9/10, 10 are above


def scripted(hits, iteration, seed=0):
    """G = len(hits) clouds; hits[g][it] of cloud g's 10 origin points are predicted as the target in iteration it.  The
    gradient of iteration it is a fixed random field (so every update moves the colours and differs from every other)."""
    G = len(hits)
    rng = np.random.default_rng(seed)
    labels = np.tile(np.r_[np.full(NM, ORI), 3 + np.arange(N - NM) % 3].astype(np.int32), (G, 1))
    mask = (labels == ORI).astype(np.uint8)
    hit_ys = np.where(mask.astype(bool), TARGET, labels).astype(np.int32)
    feat0 = (0.25 + 0.5 * rng.random((G, N, 6))).astype(np.float32)
    grads = rng.standard_normal((iteration + 1, G, N, 6)).astype(np.float32)

    def pred_fn(it, feat):
        p = labels.copy()
        for g in range(G):
            p[g, :hits[g][it]] = TARGET
        return p

    def dfeat_fn(it, feat):
        return grads[it]

    return dict(feat0=feat0, pred_fn=pred_fn, dfeat_fn=dfeat_fn, labels=labels, hit_ys=hit_ys, mask=mask, iteration=iteration)


def per_cloud(case, g, **kw):
    return R.host_loop(case["feat0"][g], lambda it, f: case["pred_fn"](it, None)[g], lambda it, f: case["dfeat_fn"](it, None)[g],
                       case["hit_ys"][g], case["mask"][g], case["iteration"], **kw)


def agrees(case, **mut):
    """Does the (possibly mutated) lockstep loop give every cloud what TBIM.batch_attack's control flow gives it alone?"""
    kw = {k: mut.pop(k) for k in ("l2_metric", "chunk") if k in mut}
    st, hist, feat, steps = R.lockstep(**case, **kw, **mut)
    ok = True
    for g in range(case["labels"].shape[0]):
        pred, adv, n_steps = per_cloud(case, g, **{k: v for k, v in kw.items() if k == "l2_metric"})
        ok &= np.array_equal(st["out_pred"][g], pred) and np.array_equal(st["out_adv"][g], adv) and steps[g] == n_steps
    return bool(ok), st, hist, steps


CAP = 5
SCENARIOS = {
    "exit at it = 1": [[0, 10, 10, 10, 10, 10]],
    "a would-be exit at it = 0": [[10, 4, 5, 10, 10, 10]],
    "exit exactly at the cap": [[0, 1, 2, 3, 9, 10]],
    "no exit": [[0, 1, 2, 3, 9, 9]],
    "on the threshold, then above": [[0, 9, 9, 10, 10, 10]],
    "two clouds leaving at different iterations": [[0, 3, 10, 0, 0, 0], [0, 10, 0, 0, 0, 0], [10, 9, 9, 9, 10, 10], [0, 0, 0, 0, 0, 0]],
}
WANT_EXIT = {"exit at it = 1": [1], "a would-be exit at it = 0": [3], "exit exactly at the cap": [5], "no exit": [-1],
             "on the threshold, then above": [3], "two clouds leaving at different iterations": [2, 1, 4, -1]}


@pytest.mark.parametrize("l2_metric", [0, 1])
@pytest.mark.parametrize("chunk", [1, 2, 10])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_lockstep_reproduces_the_host_loop(name, chunk, l2_metric):
    case = scripted(SCENARIOS[name], CAP)
    ok, st, hist, steps = agrees(case, chunk=chunk, l2_metric=l2_metric)
    assert ok, name
    assert st["exit_step"].tolist() == WANT_EXIT[name]
    assert steps.tolist() == [e + 1 if e >= 0 else CAP + 1 for e in WANT_EXIT[name]]
    assert not st["active"].any() and not st["leaving"].any()
    # the history rows are those of the forward before each update; a retired cloud's rows stay zero
    for g, h in enumerate(SCENARIOS[name]):
        for it in range(hist.shape[0]):
            assert hist[it, g, 1] == (h[it] if it < steps[g] else 0), (g, it)
    # the snapshot's statistics are those of the forward BEFORE the last update
    for g, h in enumerate(SCENARIOS[name]):
        assert st["out_stats"][g, 1] == h[steps[g] - 1]


def test_the_two_quirks_in_numbers():
    """The exiting iteration's update is applied: the snapshot colours differ from the colours the exiting forward saw; a
    cloud at the cap has taken iteration + 1 updates."""
    case = scripted(SCENARIOS["two clouds leaving at different iterations"], CAP)
    st, hist, feat, steps = R.lockstep(**case)
    trace =[case["feat0"][:, :, 3:6]]
    f, ori = case["feat0"].copy(), case["feat0"][:, :, 3:6].copy()
    for it in range(CAP + 1):
        R.bim_step(f, case["dfeat_fn"](it, f), ori, None, 0.5, 0.01, 0)
        trace.append(f[:, :, 3:6].copy())
    for g in range(4):
        assert np.array_equal(st["out_adv"][g], trace[steps[g]][g]) and not np.array_equal(st["out_adv"][g], trace[steps[g] - 1][g])
    assert steps.tolist() == [3, 2, 5, CAP + 1]


MUTANTS = {"snapshot before the update": dict(snapshot="before"), "exit allowed at it = 0": dict(min_it=0),
           ">= in place of >": dict(strict=False), "update withheld from the leaving cloud": dict(update_leaving=False)}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_are_caught(mutant):
    caught = [name for name in SCENARIOS if not agrees(scripted(SCENARIOS[name], CAP), **MUTANTS[mutant])[0]]
    print(mutant, "caught by", caught)
    assert caught, mutant
    # and by the scenario made for it
    made_for = {"exit allowed at it = 0": "a would-be exit at it = 0", ">= in place of >": "on the threshold, then above",
                "snapshot before the update": "exit at it = 1", "update withheld from the leaving cloud": "exit at it = 1"}
    assert made_for[mutant] in caught


def test_a_frozen_cloud_is_not_touched():
    G = 2
    case = scripted([[0, 10, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], CAP)
    labels, hit_ys, mask = case["labels"], case["hit_ys"], case["mask"]
    n_mask = mask.sum(1).astype(np.int32)
    st = R.new_state(G, N)
    feat = case["feat0"].copy()
    for it in (0, 1):
        row = np.zeros((G, 3), np.float32)
        R.latch(st, row, None, labels, hit_ys, mask, n_mask, 9, 10, it, 0, pred=case["pred_fn"](it, feat))
        R.retire(st, feat, 0)
    assert st["active"].tolist() == [0, 1] and st["exit_step"].tolist() == [1, -1]
    keep = {k: v.copy() for k, v in st.items()}
    row = np.full((G, 3), -7.0, np.float32)
    R.latch(st, row, None, labels, hit_ys, mask, n_mask, 9, 10, 2, 1, pred=np.full((G, N), TARGET))
    R.retire(st, feat + 1, 1)
    for k in ("out_adv", "out_pred", "out_stats", "pred", "exit_step"):
        assert np.array_equal(st[k][0], keep[k][0]), k
    assert row[0].tolist() == [-7, -7, -7] and st["exit_step"][1] == 2 and np.array_equal(st["out_adv"][1], feat[1][:, 3:6] + 1)


def test_latch_takes_the_first_maximum():
    labels = np.array([[3, 5, 0, 12]], np.int32)
    z = np.zeros((1, 4, 13), np.float32)
    z[0, 0, [3, 7]] = 2.0            # tie: the first maximum is 3
    z[0, 1, [5, 6]] = 1.0            # tie: the first is 5
    z[0, 3, 12] = 1.0                # (row 2: all equal, the first is 0)
    hit_ys = np.array([[3, 6, 0, 12]], np.int32)
    mask = np.array([[1, 1, 0, 1]], np.uint8)
    st, row = R.new_state(1, 4), np.zeros((1, 3), np.float32)
    R.latch(st, row, z, labels, hit_ys, mask, np.array([3], np.int32), 9, 10, 1, 0)
    assert st["pred"][0].tolist() == [3, 5, 0, 12] and row[0].tolist() == [4, 2, 0] and st["exit_step"][0] == -1


def test_integer_threshold_equals_the_double_test():
    """All 0 <= hits <= points <= 2048, and every hits at points = 8192, 13312 and 40960 (10 * 36864 == 9 * 40960: an equality
    case; 8192 and 13312 have none, 9 * points is no multiple of 10)."""
    tot = np.arange(1, 2049)
    points = np.repeat(tot, tot + 1)
    hits = np.concatenate([np.arange(t + 1) for t in tot])
    assert np.array_equal(R.fires_int(9, 10, hits, points), R.fires_host(hits, points))
    for t in (8192, 13312, 40960):
        h = np.arange(t + 1)
        assert np.array_equal(R.fires_int(9, 10, h, t), R.fires_host(h, t)), t
    assert not R.fires_int(9, 10, 36864, 40960) and R.fires_int(9, 10, 36865, 40960)
    assert not R.fires_int(9, 10, 9, 10) and R.fires_int(9, 10, 10, 10)


NEW_SYMBOLS = ("psg_rla_bim_step_clouds", "psg_rla_tbim_latch_clouds", "psg_rla_tbim_retire_clouds", "psg_rla_tbim_window")


def test_abi_of_the_new_entry_points():
    from pointsecguard_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the argument block mirrors psg_rla_tbim_window_args: 2 handles, 8 ints, 3 floats, 4 bytes of padding, 21 pointers
    assert ctypes.sizeof(_lib.RlaTbimWindowArgs) == 2 * 8 + 8 * 4 + 3 * 4 + 4 + 21 * 8
    assert _lib.RlaTbimWindowArgs.eps.offset == 48 and _lib.RlaTbimWindowArgs.ori.offset == 64


def test_class_has_the_lockstep_method():
    from pointsecguard_amd.randla import attack
    assert callable(attack.TBIM.batch_attack_clouds)
    assert attack.tar_NBattack.batch_attack_clouds is attack.TBIM.batch_attack_clouds
    assert attack.TBIM.EXIT_RATIO == (9, 10) and attack.TBIM.chunk == attack.CHUNK and attack.TBIM.window_hook is None
