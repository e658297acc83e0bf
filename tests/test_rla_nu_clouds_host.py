"""Host tests of the lockstep RandLA-Net NU attacks: the numpy restatement of the latch (tests/rla_nu_ref.py) against
hand-made inputs that tell it from its likely mutants, the integer exit tests against the host loop's double-precision
ones, and the C ABI of the new entry points."""
import ctypes

import numpy as np
import pytest

import rla_nu_ref as R


def one_hot_logits(classes, scale=1.0):
    z = np.zeros(classes.shape + (13,), np.float32)
    np.put_along_axis(z, classes[..., None], scale, -1)
    return z


def hand_case():
    """G = 2 clouds of n = 26 points.  Cloud 0: exactly 2 of 26 correct (13 * 2 == 26: ON the 1/13 threshold); cloud 1: 1 of 26."""
    G, n = 2, 26
    labels = np.tile(np.arange(n) % 13, (G, 1)).astype(np.int32)
    pred = (labels + 1) % 13
    pred[0, :2] = labels[0, :2]
    pred[1, :1] = labels[1, :1]
    logits = one_hot_logits(pred)
    feat = np.random.default_rng(0).random((G, n, 6), dtype=np.float32)
    dist2 = np.array([0.25, 0.5], np.float32)
    return G, n, labels, logits, feat, dist2


def run(step=1, can_exit=1, final=0, **kw):
    G, n, labels, logits, feat, dist2 = hand_case()
    st, row = R.new_state(G, n), np.zeros((G, 3), np.float32)
    R.latch(st, row, logits, labels, labels, None, None, feat, dist2, 0, 1, 13, step, can_exit, final, **kw)
    return st, row, feat


def test_latch_spec_on_hand_case():
    st, row, feat = run()
    assert row.tolist() == [[2, 0, 0.25], [1, 0, 0.5]]
    assert st["exit_step"].tolist() == [-1, 1] and st["active"].tolist() == [1, 0]      # 13 * 2 < 26 is false, 13 * 1 < 26 true
    assert np.array_equal(st["out_adv"][1], feat[1][:, 3:6]) and not st["out_adv"][0].any()
    assert st["out_stats"][1].tolist() == [1, 0, 0.5]


def test_latch_mutants_are_caught():
    spec, _, _ = run()
    # `<=` instead of `<`: cloud 0 sits exactly on the threshold
    mut, _, _ = run(strict=False)
    assert mut["exit_step"].tolist() == [1, 1] != spec["exit_step"].tolist()
    # an exit allowed at evaluation index 0
    spec0, _, _ = run(step=0)
    mut0, _, _ = run(step=0, min_step=0)
    assert spec0["exit_step"].tolist() == [-1, -1] and mut0["exit_step"].tolist() == [-1, 0]
    # can_exit = 0 records, never exits; final snapshots without an exit
    st, row, feat = run(can_exit=0, final=1)
    assert st["exit_step"].tolist() == [-1, -1] and st["active"].tolist() == [1, 1] and row[1].tolist() == [1, 0, 0.5]
    assert np.array_equal(st["out_adv"], feat[:, :, 3:6])


def test_latch_first_maximum_and_mask():
    n = 4
    labels = np.array([[3, 5, 0, 12]], np.int32)
    z = np.zeros((1, n, 13), np.float32)
    z[0, 0, [3, 7]] = 2.0            # tie: first maximum is 3 (correct), last is 7
    z[0, 1, [5, 6]] = 1.0            # tie: first 5 (correct), last 6
    z[0, 2] = 0.0                    # all equal: first 0 (correct), last 12
    z[0, 3, 12] = 1.0
    ys = np.array([[7, 6, 12, 12]], np.int32)
    mask = np.array([[1, 0, 0, 1]], np.uint8)
    feat, dist2 = np.zeros((1, n, 6), np.float32), np.zeros(1, np.float32)
    args = (z, labels, ys, mask, np.array([2], np.int32), feat, dist2, 1, 19, 20, 1, 1, 0)
    st, row = R.new_state(1, n), np.zeros((1, 3), np.float32)
    R.latch(st, row, *args)
    assert st["pred"][0].tolist() == [3, 5, 0, 12] and row[0].tolist() == [4, 1, 0] and st["exit_step"][0] == -1
    # last maximum instead of first
    st2, row2 = R.new_state(1, n), np.zeros((1, 3), np.float32)
    R.latch(st2, row2, *args, argmax="last")
    assert st2["pred"][0].tolist() == [7, 6, 12, 12] and row2[0].tolist() != row[0].tolist()
    # a mask that is ignored: counts hits on unmasked points too
    z3 = one_hot_logits(ys)
    st3, row3 = R.new_state(1, n), np.zeros((1, 3), np.float32)
    R.latch(st3, row3, z3, *args[1:])
    st4, row4 = R.new_state(1, n), np.zeros((1, 3), np.float32)
    R.latch(st4, row4, z3, *args[1:], use_mask=False)
    assert row3[0, 1] == 2 and row4[0, 1] == 4
    assert st3["exit_step"][0] == 1                      # 20 * 2 > 19 * 2


def test_latch_freezes_an_exited_cloud():
    G, n, labels, logits, feat, dist2 = hand_case()
    st, row = R.new_state(G, n), np.zeros((G, 3), np.float32)
    R.latch(st, row, logits, labels, labels, None, None, feat, dist2, 0, 1, 13, 1, 1, 0)
    keep = {k: v.copy() for k, v in st.items()}
    row2 = np.full((G, 3), -7.0, np.float32)
    R.latch(st, row2, logits * 0 + 9, labels, labels, None, None, feat + 1, dist2 + 1, 0, 1, 13, 2, 1, 1)
    for k in ("out_adv", "out_pred", "out_stats", "pred"):
        assert np.array_equal(st[k][1], keep[k][1]), k
    assert st["exit_step"][1] == 1 and row2[1].tolist() == [-7, -7, -7] and row2[0, 2] == 1.25


@pytest.mark.parametrize("mode,num,den", [(0, 1, 13), (1, 19, 20)])
def test_integer_thresholds_equal_the_double_tests(mode, num, den):
    """All 0 <= count <= total <= 2048, and every count at the totals 8192, 13312 (= 13 * 1024: the equality case of mode 0)
    and 40960 (20 * 38912 == 19 * 40960: the equality case of mode 1)."""
    tot = np.arange(1, 2049)
    total = np.repeat(tot, tot + 1)
    count = np.concatenate([np.arange(t + 1) for t in tot])
    assert np.array_equal(R.fires_int(mode, num, den, count, total), R.fires_host(mode, count, total))
    for t in (8192, 13312, 40960):
        c = np.arange(t + 1)
        assert np.array_equal(R.fires_int(mode, num, den, c, t), R.fires_host(mode, c, t)), t
    assert not R.fires_int(0, 1, 13, 1024, 13312) and R.fires_int(0, 1, 13, 1023, 13312)
    assert not R.fires_int(1, 19, 20, 38912, 40960) and R.fires_int(1, 19, 20, 38913, 40960)


NEW_SYMBOLS = ("psg_rla_nu_color_clouds", "psg_rla_nu_adam_clouds", "psg_rla_nu_latch_clouds", "psg_rla_nu_window")


def test_abi_of_the_new_entry_points():
    from pointsecguard_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the argument block mirrors psg_rla_nu_window_args: 2 handles, 8 ints, 2 floats, 22 pointers, no padding
    assert ctypes.sizeof(_lib.RlaNuWindowArgs) == 2 * 8 + 8 * 4 + 2 * 4 + 22 * 8
    assert _lib.RlaNuWindowArgs.xs.offset == 56


def test_classes_have_the_lockstep_methods_and_keep_the_one_cloud_guard():
    from pointsecguard_amd.randla import attack
    assert callable(attack.NUattack.batch_attack_clouds) and callable(attack.tar_NUattack.batch_attack_clouds)
    assert attack.NUattack.EXIT_RATIO == (1, 13) and attack.tar_NUattack.EXIT_RATIO == (19, 20)
    assert attack.CHUNK == 10


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t", [1, 7])
def test_adam64_is_pinned_to_the_oracle(t, masked):
    """The float64 restatement of the Adam step (rla_nu_ref.adam64, the yardstick of the GPU test of the kernel) against
    oracle/randla_net.nu_adam_step on 50 points: the oracle's mixed float32 / float64 evaluation takes no more roundings than
    the kernel, so it lies inside the counted bound."""
    from oracle import randla_net as O
    rng = np.random.default_rng(50 + t)
    n, c, lr = 50, 0.5, 0.01
    xs = rng.random((n, 3), dtype=np.float32)
    dws = (0.3 * rng.standard_normal((n, 3))).astype(np.float32)
    m = (0.1 * rng.standard_normal((n, 3))).astype(np.float32)
    v = (0.01 * rng.random((n, 3))).astype(np.float32)
    dscore = rng.standard_normal((n, 3)).astype(np.float32)
    mask = (rng.random(n) < 0.4) if masked else None
    adv, _ = O.nu_color(xs, dws, mask)
    dist2 = np.float32(((adv.astype(np.float64) - xs) ** 2).sum())
    w_o, m_o, v_o, dist = O.nu_adam_step(xs, dws, m, v, t, dscore, c, lr, mask)
    assert abs(dist - np.sqrt(np.float64(dist2))) <= 2.0 ** -24 * dist
    oracle_consts = (np.float32(1 - 0.9), np.float32(1 - 0.999))          # (adam64's docstring: the kernel's differ in the last bits)
    (w_r, m_r, v_r), (e_w, e_m, e_v) = R.adam64(xs, dws, m, v, adv, dscore, dist2, c, lr, t, mask, one_minus=oracle_consts)
    for name, got, ref, bound in (("d_ws", w_o, w_r, e_w), ("m", m_o, m_r, e_m), ("v", v_o, v_r, e_v)):
        err = np.abs(got.astype(np.float64) - ref)
        print(name, "largest error / bound", float((err / bound).max()), "largest bound / |value|", float((bound / np.abs(ref)).max()))
        assert (err <= bound).all(), name
    # the bound resolves the last bits of a constant: with the kernel's 1 - 0.999f (1.3e-5 below float32(0.001)) the oracle's v
    # no longer fits it
    (_, _, v_k), (_, _, e_vk) = R.adam64(xs, dws, m, v, adv, dscore, dist2, c, lr, t, mask)
    assert (np.abs(v_o.astype(np.float64) - v_k) > e_vk).any()
    assert R.adam_lr_t(lr, t) == np.float32(lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
    if masked:      # a masked-out point: no gradient, the moments only decay
        off = ~mask
        assert np.array_equal(m_r[off], np.float64(R.B1) * m[off]) and np.array_equal(v_r[off], np.float64(R.B2) * v[off])
