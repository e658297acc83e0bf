"""GPU tests of the whole-scene NU attack kernels (csrc/psg_scene_nu.hip) on their own, against tests/scene_nu_ref.py: the
ordered sums, the latch's counters / decision / snapshot and every byte that must stay are compared bit for bit; w / m / v /
c / w_init against the float64 reference fed the float32 sums, within attack_ref64.bound (LOG_RATIO, TANH_RATIO, SQRT_RATIO:
the constants measured for the same logf / tanhf / sqrtf in psg_attack.hip).  Every case runs twice and must repeat.

Inputs: scene_ref.hand_made_index (700 points, 5003 slots, point 5 never occurring, point 9 occurring 3000 times), clean
colours at 0, 1, 1 / 255 and 254 / 255, the order-sensitive triple 1, 1e8, -1e8 in both gradients."""
import numpy as np
import pytest
import torch

import scene_nu_ref as ref
import scene_ref

pytestmark = pytest.mark.gpu
F = np.float32


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda().contiguous()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits_or_nan(a, b):
    nan = np.isnan(a)                                             # (a NaN's payload is not part of the contract)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def word(value):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def lists():
    from pointsecguard_amd import runtime
    idx, n_scene = scene_ref.hand_made_index()
    off, ent = scene_ref.occ_lists(idx, n_scene)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_off, d_ent = runtime.scene_occ_build(dev(idx), n_scene, bad)
    assert int(bad.item()) == 0 and np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_ent.cpu().numpy(), ent)
    return idx, n_scene, off, ent, d_off, d_ent


def report(what, got, want, e):
    r = ref.ratio(got, want, e)
    print("%s: largest error / first-order bound %.4f" % (what, r))
    ok = ref.within(got, want, e)
    assert ok.all(), "%s: %d entries outside the bound, largest error / first-order bound %.4f" % (what, int((~ok).sum()), r)


def test_init(lists):
    from pointsecguard_amd import runtime
    idx, n_scene = lists[:2]
    c0 = ref.nu_step_case(7, idx, n_scene, False)[4]
    want, e = ref.init64(c0)
    outs = []
    for _ in range(2):
        w = torch.full((n_scene, 3), float("nan"), dtype=torch.float32, device="cuda")
        runtime.scene_nu_init(dev(c0), w)
        outs.append(w.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    report("w_init", outs[0], want, e)
    assert (outs[0][c0 == 0] == -np.inf).all() and (outs[0][c0 == 1] == np.inf).all() and np.isinf(outs[0]).sum() == (c0 == 0).sum() + (c0 == 1).sum()


@pytest.mark.parametrize("masked", [False, True])
def test_colour(lists, masked):
    from pointsecguard_amd import runtime
    idx, n_scene, off, ent, d_off, d_ent = lists
    w, _, _, _, _, _, _, mask = ref.nu_step_case(7, idx, n_scene, True)
    msk = mask if masked else None
    c_in = np.random.default_rng(1).random((n_scene, 3)).astype(F)
    c_in[::5] = np.nan                                            # bytes, not values, are kept
    want, e, written = ref.colour64(w, c_in, off, msk)
    d_mask = dev(mask.astype(np.uint8)) if masked else None
    outs = []
    for _ in range(2):
        c = dev(c_in)
        runtime.scene_nu_colour(dev(w), d_mask, d_off, word(1), c)
        outs.append(c.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    assert not written[5] and 0 < written.sum() < n_scene
    assert np.array_equal(bits(outs[0][~written]), bits(c_in[~written]))
    report("c (masked %d)" % masked, outs[0][written], want[written], e[:, written])
    assert (outs[0][written][np.isposinf(w[written])] == 1).all() and (outs[0][written][np.isneginf(w[written])] == 0).all()
    c = dev(c_in)                                                 # active == 0 leaves every byte
    runtime.scene_nu_colour(dev(w), d_mask, d_off, word(0), c)
    assert np.array_equal(bits(c.cpu().numpy()), bits(c_in))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("step,warm", ref.STEP_CASES)
def test_step(lists, step, warm, masked):
    from pointsecguard_amd import runtime
    idx, n_scene, off, ent, d_off, d_ent = lists
    w, m, v, c, c0, dx0, sgrad, mask = ref.nu_step_case(7, idx, n_scene, warm)
    msk = mask if masked else None
    d_mask = dev(mask.astype(np.uint8)) if masked else None
    w64, m64, v64, we, me, ve, gf, gs = ref.step64(w, m, v, c, c0, dx0, sgrad, off, ent, msk, ref.CW, ref.LR, step)
    on = ref.moves(off, msk)

    def run(active, with_sums=True):
        wd, md, vd = dev(w), dev(m), dev(v)
        gfd = torch.full((n_scene, 3), float("nan"), dtype=torch.float32, device="cuda") if with_sums else None
        gsd = torch.full((n_scene, 3), float("nan"), dtype=torch.float32, device="cuda") if with_sums else None
        runtime.scene_nu_step(wd, md, vd, dev(c), dev(c0), d_mask, d_off, d_ent, dev(dx0), dev(sgrad), ref.CW, ref.LR, ref.BETA1,
                              ref.BETA2, ref.ADAM_EPS, step, word(active), gfd, gsd)
        return [t.cpu().numpy() if t is not None else None for t in (wd, md, vd, gfd, gsd)]

    first, second = run(1), run(1)
    for a, b in zip(first, second):
        assert same_bits_or_nan(a, b)
    gw, gm, gv, ggf, ggs = first
    # the two ordered sums, bit for bit: the triple sums to 0 in slot order (1 the other way round), +0 where nothing moves
    assert same_bits_or_nan(ggf, gf) and same_bits_or_nan(ggs, gs)
    p = np.nonzero((off[1:] - off[:-1]) == 3)[0][0]
    assert on[p] and (bits(ggf[p]) == 0).all() and (bits(ggs[p]) == 0).all()
    assert (bits(ggf[~on]) == 0).all() and (bits(ggs[~on]) == 0).all() and np.isnan(ggf).any()
    # points that do not move keep their bytes
    assert not on[5] and on.sum() < n_scene
    for got, before in ((gw, w), (gm, m), (gv, v)):
        assert np.array_equal(bits(got[~on]), bits(before[~on]))
    what = "step %d masked %d" % (step, masked)
    report(what + " w", gw[on], w64[on], we[:, on])
    report(what + " m", gm[on], m64[on], me[:, on])
    report(what + " v", gv[on], v64[on], ve[:, on])
    moved = on[:, None] & np.isfinite(w) & np.isfinite(gw)
    assert (bits(gw)[moved] != bits(w)[moved]).mean() > 0.5
    # without the optional outputs the step is the same; active == 0 leaves every byte, the NaN-filled outputs included
    for a, b in zip(run(1, with_sums=False)[:3], first[:3]):
        assert same_bits_or_nan(a, b)
    idle = run(0)
    for got, before in zip(idle[:3], (w, m, v)):
        assert np.array_equal(bits(got), bits(before))
    assert np.isnan(idle[3]).all() and np.isnan(idle[4]).all()


@pytest.mark.parametrize("rows", [5003, 300001])
@pytest.mark.parametrize("masked", [False, True])
def test_latch(lists, masked, rows):
    """5003 slots: one pass of the counting grid; 300 001 (a whole room's worth, no multiple of 64): more than its 1024
    workgroups of 256 take in one pass, so the grid-stride loop runs"""
    from pointsecguard_amd import runtime
    idx, n_scene = lists[:2]
    if rows != idx.size:
        idx = np.concatenate([idx, np.random.default_rng(2).integers(0, n_scene, rows - idx.size).astype(np.int32)])
        assert idx.size == rows > 1024 * 256 and rows % 64
    pred, labels, target, mask, c = ref.latch_case(5, idx, n_scene)
    msk = mask if masked else None
    d_mask = dev(mask.astype(np.uint8)) if masked else None
    n_hits, n_counted = ref.latch_counts(pred, labels, target, idx, msk)
    assert 1 < n_hits < n_counted and (n_counted == idx.size) == (not masked)
    past = n_hits - 1 if masked else n_hits + 1
    snap_in = np.full((n_scene, 3), np.nan, F)

    def run(num, den, step, active, exit_in=-1):
        snap = dev(snap_in)
        counters = torch.zeros(2, dtype=torch.int32, device="cuda")
        hist = torch.full((2,), -1, dtype=torch.int64, device="cuda")           # 0xFF bytes
        ex, act = word(exit_in), word(active)
        runtime.scene_nu_latch(dev(pred), None if masked else dev(labels), target, dev(idx), d_mask, num, den, step, dev(c), snap,
                               counters, hist, ex, act)
        return snap.cpu().numpy(), counters.cpu().tolist(), hist.cpu().tolist(), int(ex.item()), int(act.item())

    # equality holds, one count past it fires; (0, 1) can never fire below (and always above), (1, 1) the other way round
    for num, den, fires in ((n_hits, n_counted, False), (past, n_counted, True), (0, 1, masked), (1, 1, not masked)):
        outs = [run(num, den, 6, 1) for _ in range(2)]
        assert same_bits_or_nan(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:]
        snap, counters, hist, ex, act = outs[0]
        want_hist, want_snap, want_exit, want_active = ref.latch(pred, labels, target, idx, msk, num, den, 6, c, snap_in, -1, 1)
        assert (want_exit, want_active) == ((6, 0) if fires else (-1, 1))
        assert hist == list(want_hist) and counters == [0, 0] and (ex, act) == (want_exit, want_active)
        assert same_bits_or_nan(snap, want_snap) and (np.isnan(snap).all() != fires)
    # active == 0 leaves every byte: history row, snapshot, exit step
    snap, counters, hist, ex, act = run(past, n_counted, 7, 0, exit_in=6)
    assert np.isnan(snap).all() and counters == [0, 0] and hist == [-1, -1] and (ex, act) == (6, 0)


def test_refusals():
    from pointsecguard_amd import _lib, runtime
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    two = torch.zeros(2, dtype=torch.int64, device="cuda")
    f = torch.zeros(3, dtype=torch.float32, device="cuda")
    too_many = (2 ** 31 - 1) // 9 + 1
    with pytest.raises(_lib.PsgError, match="INT_MAX / 9"):
        _lib.call("psg_scene_nu_step", runtime.ptr(f), runtime.ptr(f), runtime.ptr(f), runtime.ptr(f), runtime.ptr(f), None,
                  runtime.ptr(one), runtime.ptr(one), runtime.ptr(f), runtime.ptr(f), too_many, 1, 1e-4, 0.01, 0.9, 0.999, 1e-8, 1,
                  runtime.ptr(one), None, None, runtime.stream())
    with pytest.raises(_lib.PsgError, match="INT_MAX / 9"):
        _lib.call("psg_scene_nu_latch", runtime.ptr(one), runtime.ptr(one), 0, None, None, too_many, 1, 1, 13, 0, runtime.ptr(f),
                  runtime.ptr(f), runtime.ptr(one), runtime.ptr(two), runtime.ptr(one), runtime.ptr(one), runtime.stream())
    with pytest.raises(_lib.PsgError, match="den > 0"):
        _lib.call("psg_scene_nu_latch", runtime.ptr(one), runtime.ptr(one), 0, None, None, 1, 1, 1, 0, 0, runtime.ptr(f),
                  runtime.ptr(f), runtime.ptr(one), runtime.ptr(two), runtime.ptr(one), runtime.ptr(one), runtime.stream())
    with pytest.raises(_lib.PsgError):
        runtime.scene_nu_init(torch.zeros(4, 3))                  # no CPU path
