"""CPU tests of the whole-scene NU attack: the references of tests/scene_nu_ref.py against brute force,
against float64 autograd of the cost as it is stated and against double-precision quotients; the mutants each of them must
catch ON THE INPUTS THE GPU KERNEL TESTS USE; and the refusals that need no device."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import scene_nu_ref as ref
import scene_ref
from test_gpu_harness import synth_scene

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits_or_nan(a, b):
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


@pytest.fixture(scope="module")
def hand_made():
    idx, n_scene = scene_ref.hand_made_index()
    off, ent = scene_ref.occ_lists(idx, n_scene)
    return idx, n_scene, off, ent


def test_ordered_sums_vs_brute_force(hand_made):
    idx, n_scene, off, ent = hand_made
    _, _, _, _, _, dx0, sgrad, mask = ref.nu_step_case(7, idx, n_scene, True)
    for msk in (None, mask):
        gf, gs = ref.ordered_sums(dx0, sgrad, off, ent, msk)
        want_f, want_s = np.zeros((n_scene, 3), F), np.zeros((n_scene, 3), F)
        with np.errstate(invalid="ignore", over="ignore"):
            for e, p in enumerate(idx.tolist()):                  # ascending slot order IS list order
                if msk is None or msk[p]:
                    want_f[p] = (want_f[p] + dx0[e, 3:6]).astype(F)
                    want_s[p] = (want_s[p] + sgrad[e]).astype(F)
        assert same_bits_or_nan(gf, want_f) and same_bits_or_nan(gs, want_s)
        assert (gf[5] == 0).all() and (gs[5] == 0).all()           # the point without a slot
    # the order-sensitive triple: 1 + 1e8 - 1e8 is 0 ascending, 1 descending, in both sums
    p = np.nonzero((off[1:] - off[:-1]) == 3)[0][0]
    up = ref.ordered_sums(dx0, sgrad, off, ent, None)
    down = ref.ordered_sums(dx0, sgrad, off, ent, None, mutant="descending")
    assert (up[0][p] == 0).all() and (up[1][p] == 0).all() and (down[0][p] == 1).all() and (down[1][p] == 1).all()


def exact_sum_case(seed, idx, n_scene):
    """gradients on a grid of 2^-12 below 2^3: every float32 partial sum of up to 3000 of them is exact in any order, so the
    float32 sums ARE the real sums and the stated cost can be compared without a term for them"""
    rng = np.random.default_rng(seed)
    dx0 = np.zeros((idx.size, 9), F)
    dx0[:, 3:6] = rng.integers(-2 ** 14, 2 ** 14, (idx.size, 3)) / 2.0 ** 12
    sgrad = (rng.integers(-2 ** 14, 2 ** 14, (idx.size, 3)) / 2.0 ** 12).astype(F)
    c0 = (np.floor(rng.random((n_scene, 3)) * 254.0 + 1.0) / 255.0).astype(F)       # inside (0, 1): finite w
    w = (np.arctanh(2.0 * c0.astype(np.float64) - 1.0) + 0.05 * rng.standard_normal((n_scene, 3))).astype(F)
    m = (rng.standard_normal((n_scene, 3)) * 1e-2).astype(F)
    v = (rng.random((n_scene, 3)) * 1e-3).astype(F)
    c = (0.5 * (np.tanh(w.astype(np.float64)) + 1.0)).astype(F)
    return w, m, v, c, c0, dx0, sgrad, rng.random(n_scene) < 0.5


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_assembly_is_the_gradient_of_the_stated_cost(hand_made, step, masked):
    """L2 once per point, f-loss and Smooth gradients summed over the slots: float64 autograd of
    sum_e <dx0[e] + cw sgrad[e], col[idx[e]]> + cw sum_p |col_p - c0_p|^2 against the restatement (float32 sums exact here)."""
    idx, n_scene, off, ent = hand_made
    w, m, v, c, c0, dx0, sgrad, mask = exact_sum_case(3, idx, n_scene)
    msk = mask if masked else None
    cw = 0.05                                                      # an L2 / Smooth weight at which both terms show
    gf, gs = ref.ordered_sums(dx0, sgrad, off, ent, msk)
    on = ref.moves(off, msk)
    for name, d3, g in (("f", dx0[:, 3:6], gf), ("smooth", sgrad, gs)):     # exact: the float64 sums are the same numbers
        want = np.zeros((n_scene, 3))
        np.add.at(want, idx, d3.astype(np.float64))
        assert np.array_equal(g.astype(np.float64)[on], want[on]), name
    w64, m64, v64, we, me, ve, _, _ = ref.step64(w, m, v, c, c0, dx0, sgrad, off, ent, msk, cw, ref.LR, step)
    ws, ms, vs = ref.stated_cost_step64(w, m, v, c0, dx0, sgrad, idx, msk, cw, ref.LR, step)
    # (the stated cost evaluates col from w in float64, the kernel reads the stored float32 colour: half an ulp of c, which
    # the model's first rounding of `diff` covers twice over)
    for name, a, b, e in (("w", w64, ws, we), ("m", m64, ms, me), ("v", v64, vs, ve)):
        print("step %d masked %d %s: stated cost vs float64 reference, error / first-order bound %.4f" % (
            step, masked, name, ref.ratio(a, b, e)))
        assert ref.within(a, b, e).all(), name
    assert np.array_equal(w64[~on], w[~on].astype(np.float64)) and np.array_equal(ws[~on], w[~on].astype(np.float64))
    # the per-slot L2 term and the first-slot Smooth term are NOT that gradient
    for mutant in ("l2_per_slot", "smooth_first_slot_only", "drop_last"):
        wm, mm, _, _, _, _, _, _ = ref.step64(w, m, v, c, c0, dx0, sgrad, off, ent, msk, cw, ref.LR, step, mutant=mutant)
        assert not (ref.within(wm, ws, we).all() and ref.within(mm, ms, me).all()), mutant
    # and the float32 restatement, one operation per line, lies within the model of the float64 reference
    w32, m32, v32, _, _ = ref.step32(w, m, v, c, c0, dx0, sgrad, off, ent, msk, cw, ref.LR, step)
    for name, a, b, e in (("w", w32, w64, we), ("m", m32, m64, me), ("v", v32, v64, ve)):
        assert ref.within(a, b, e).all(), name


def gpu_step_inputs(hand_made):
    idx, n_scene, off, ent = hand_made
    for step, warm in ref.STEP_CASES:
        state = ref.nu_step_case(7, idx, n_scene, warm)
        for masked in (False, True):
            yield step, state[:7], (state[7] if masked else None)


def test_float32_restatement_within_the_bound_on_the_gpu_inputs(hand_made):
    idx, n_scene, off, ent = hand_made
    for step, (w, m, v, c, c0, dx0, sgrad), msk in gpu_step_inputs(hand_made):
        w64, m64, v64, we, me, ve, gf, gs = ref.step64(w, m, v, c, c0, dx0, sgrad, off, ent, msk, ref.CW, ref.LR, step)
        w32, m32, v32, gf32, gs32 = ref.step32(w, m, v, c, c0, dx0, sgrad, off, ent, msk, ref.CW, ref.LR, step)
        assert same_bits_or_nan(gf, gf32) and same_bits_or_nan(gs, gs32)
        for name, a, b, e in (("w", w32, w64, we), ("m", m32, m64, me), ("v", v32, v64, ve)):
            assert ref.within(a, b, e).all(), (step, name)
        on = ref.moves(off, msk)
        assert on.sum() < n_scene and (bits(w32[~on]) == bits(w[~on])).all() and (bits(m32[~on]) == bits(m[~on])).all()
        assert np.isinf(w32).any() and np.isnan(w32).any()           # clean colours 0 and 1; the NaN gradient
        if step == 1:
            assert (bits(w32[on]) != bits(w[on])).any()


def test_every_mutant_shows_on_the_gpu_inputs(hand_made):
    """bits for the sums, the bound for w / m / v: on the very inputs tests/test_gpu_scene_nu_kernels.py feeds the kernel"""
    idx, n_scene, off, ent = hand_made
    shown = {mutant: 0 for mutant in ref.SUM_MUTANTS + ref.STEP_MUTANTS}
    n_cases = 0
    for step, (w, m, v, c, c0, dx0, sgrad), msk in gpu_step_inputs(hand_made):
        n_cases += 1
        w64, m64, v64, we, me, ve, gf, gs = ref.step64(w, m, v, c, c0, dx0, sgrad, off, ent, msk, ref.CW, ref.LR, step)
        for mutant in shown:
            try:
                wm, mm, vm, _, _, _, gfm, gsm = ref.step64(w, m, v, c, c0, dx0, sgrad, off, ent, msk, ref.CW, ref.LR, step,
                                                           mutant=mutant)
            except ZeroDivisionError:                              # bias_late at step 1: a step of size lr / (1 - beta1^0)
                assert (mutant, step) == ("bias_late", 1)
                shown[mutant] += 1
                continue
            if mutant in ref.SUM_MUTANTS:
                shown[mutant] += not (same_bits_or_nan(gf, gfm) and same_bits_or_nan(gs, gsm))
            else:
                shown[mutant] += not (ref.within(wm, w64, we).all() and ref.within(mm, m64, me).all() and ref.within(vm, v64, ve).all())
    print("cases (of %d) in which each mutant leaves the bits / the bound: %s" % (n_cases, shown))
    n_warm = 2 * sum(1 for _, warm in ref.STEP_CASES if warm)
    for mutant, n in shown.items():
        # a mask-related mutant can only show in the masked cases; the per-slot L2 term only where the colours have left the
        # clean ones (before step 1 c - c0 is the rounding of tanh_space(inverse_tanh_space(c0)): nothing to multiply);
        # everything else in every case
        want = {"moves_unmasked": n_cases // 2, "l2_per_slot": n_warm}.get(mutant, n_cases)
        assert n == want and n > 0, (mutant, n)


# ------------------------------------------------------------------------------------------------ the exit latch
RATIOS = [(1, 13), (9, 10), (0, 1), (1, 2), (3, 7), (1, 1), (13, 13), (2, 1)]


def test_integer_exit_rule_vs_double_quotients_exhaustively():
    for rows in range(0, 201):
        for n in range(0, rows + 1):
            for num, den in RATIOS:
                for targeted in (False, True):
                    assert ref.latch_fire(n, rows, num, den, targeted) == ref.latch_fire_quotients(n, rows, num, den, targeted), (
                        n, rows, num, den, targeted)
    for rows in range(1, 201):                                     # (0, 1) can never fire below; nothing fires on equality
        assert not ref.latch_fire(0, rows, 0, 1, False) and not ref.latch_fire(rows, rows, 1, 1, True)
        assert not ref.latch_fire(rows, 13 * rows, 1, 13, False) and not ref.latch_fire(9 * rows, 10 * rows, 9, 10, True)


def test_integer_exit_rule_on_the_listed_inputs_and_the_float_mutant():
    differs = []
    for n, rows, num, den in ref.LATCH_INPUTS:
        assert n * den < 2 ** 63 and num * rows < 2 ** 63          # the kernel's 64-bit products hold them
        for targeted in (False, True):
            exact = (Fraction(n, rows) > Fraction(num, den) if targeted else Fraction(n, rows) < Fraction(num, den)) if rows else False
            assert ref.latch_fire(n, rows, num, den, targeted) == exact, (n, rows, num, den, targeted)
            if ref.latch_fire(n, rows, num, den, targeted, mutant="latch_float_division") != exact:
                differs.append((n, rows, num, den, targeted))
    print("latch_float_division differs from the integer rule on %d listed inputs: %s" % (len(differs), differs))
    assert differs, "latch_float_division is indistinguishable on the listed inputs"
    # on the exhaustive small range a float32 quotient agrees with the integer rule: only the large counts tell them apart
    small = [(n, rows, num, den, t) for rows in range(1, 201) for n in range(rows + 1) for num, den in RATIOS for t in (False, True)
             if ref.latch_fire(n, rows, num, den, t, mutant="latch_float_division") != ref.latch_fire(n, rows, num, den, t)]
    print("latch_float_division on rows <= 200: %d differences" % len(small))


def test_latch_state_and_first_exit(hand_made):
    idx, n_scene, off, ent = hand_made
    pred, labels, target, mask, c = ref.latch_case(5, idx, n_scene)
    snap0 = np.full((n_scene, 3), np.nan, F)
    for msk in (None, mask):
        n_hits, n_counted = ref.latch_counts(pred, labels, target, idx, msk)
        brute = [(pred[e] == target) if msk is not None else (pred[e] == labels[e]) for e in range(idx.size)
                 if msk is None or msk[idx[e]]]
        assert (n_hits, n_counted) == (int(np.sum(brute)), len(brute)) and 0 < n_hits < n_counted
        # equality does not fire, one count past it does
        hold = ref.latch(pred, labels, target, idx, msk, n_hits, n_counted, 3, c, snap0, -1, 1)
        assert hold[0] == (n_hits, n_counted) and hold[2:] == (-1, 1) and hold[1] is snap0
        past = (n_hits - 1, n_counted) if msk is not None else (n_hits + 1, n_counted)
        fired = ref.latch(pred, labels, target, idx, msk, past[0], past[1], 3, c, snap0, -1, 1)
        assert fired[2:] == (3, 0) and np.array_equal(bits(fired[1]), bits(c))
        assert ref.latch(pred, labels, target, idx, msk, past[0], past[1], 4, c, snap0, 3, 0) == (None, snap0, 3, 0)
    hist = np.array([[50, 100], [20, 100], [7, 100], [8, 100]])
    assert ref.first_exit(hist, 1, 13, False) == 2 and ref.first_exit(hist, 0, 1, False) == -1
    assert ref.first_exit(hist, 9, 10, True) == -1 and ref.first_exit(hist, 1, 5, True) == 0


# ------------------------------------------------------------------------------------------------ refusals, no device
def test_refusals_without_a_device():
    from pointsecguard_amd import _lib, harness
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    from pointsecguard_amd.models import pointnet2_sem_seg, pointnet2_sem_seg_msg, pointnet_sem_seg
    pn2 = pointnet2_sem_seg.get_model(13).eval()                   # on the CPU: there is no CPU path
    atk = SceneNUAttack(pn2)
    assert (atk.c, atk.kappa, atk.steps, atk.lr, atk.batch_size, atk.neighbour, atk.check_every) == (1e-4, 0.0, 1000, 0.01, 8, 10, 10)
    assert atk.exit_below == (1, 13) and atk.exit_above == (9, 10) and atk.target is None and atk.origin is None
    assert SceneNUAttack(pn2, target=2, origin=5).neighbour == 5 and SceneNUAttack(pn2, target=2, origin=5, neighbour=7).neighbour == 7
    SceneNUAttack(pointnet2_sem_seg_msg.get_model(13).eval(), steps=2)
    ds = harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": synth_scene(21, 2048, 0.9, 0.9)})
    np.random.seed(3)
    data, label, _, index = ds[0]
    with pytest.raises(_lib.PsgError):
        atk(torch.from_numpy(data.astype(F)), torch.from_numpy(index.astype(np.int32)), torch.from_numpy(label.astype(np.int32)),
            ds.scene_points_list[0][:, 3:6], ds.semantic_labels_list[0])
    with pytest.raises(_lib.PsgError):
        harness.evaluate_whole_scene_consistent(pn2, ds, lambda m: SceneNUAttack(m, steps=1), log=lambda *_: None)
    vanilla = pointnet_sem_seg.get_model(13).eval()
    with pytest.raises(NotImplementedError):
        SceneNUAttack(vanilla)
    from pointsecguard_amd.randla.network import RandLAModel
    from pointsecguard_amd.resgcn.sem_seg_dense.architecture import DenseDeepGCN
    for cls in (RandLAModel, DenseDeepGCN):                        # (bare instances: the refusal looks at the type alone)
        with pytest.raises(NotImplementedError):
            SceneNUAttack(cls.__new__(cls))
    with pytest.raises(ValueError):
        SceneNUAttack(pn2, target=3)                               # targeted needs the origin class as well
    with pytest.raises(ValueError):
        SceneNUAttack(pn2, origin=3)
    with pytest.raises(ValueError):
        SceneNUAttack(pn2, target=13, origin=3)
    for kw in (dict(steps=0), dict(batch_size=0), dict(check_every=0), dict(steps=-3), dict(exit_below=(1, 0)),
               dict(exit_above=(9, 0)), dict(exit_below=(1, -13)), dict(neighbour=17)):
        with pytest.raises(ValueError):
            SceneNUAttack(pn2, **kw)
