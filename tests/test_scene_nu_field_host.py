"""CPU tests of the coordinate field of the whole-scene NU attack: the references of
tests/scene_nu_field_ref.py against brute force and against float64 autograd of the cost as it is stated; the mutants each of
them must catch ON THE INPUTS THE GPU KERNEL TEST USES; and the refusals that need no device."""
import numpy as np
import pytest

import scene_nu_field_ref as ref
import scene_ref

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
    _, _, _, dx0, sgrad, mask = ref.field_step_case(7, idx, n_scene, True)
    for msk in (None, mask):
        gx, gs = ref.ordered_sums(dx0, sgrad, off, ent, msk)
        want_x, want_s = np.zeros((n_scene, 3), F), np.zeros((n_scene, 3), F)
        with np.errstate(invalid="ignore", over="ignore"):
            for e, p in enumerate(idx.tolist()):                  # ascending slot order IS list order
                if msk is None or msk[p]:
                    want_x[p] = (want_x[p] + dx0[e, 0:3]).astype(F)
                    want_s[p] = (want_s[p] + sgrad[e]).astype(F)
        assert same_bits_or_nan(gx, want_x) and same_bits_or_nan(gs, want_s)
        assert (gx[5] == 0).all() and (gs[5] == 0).all()           # the point without a slot
    # channels 3:9 of the block gradients are not read
    other = dx0.copy()
    other[:, 3:9] = F(7)
    assert same_bits_or_nan(ref.ordered_sums(other, sgrad, off, ent, None)[0], ref.ordered_sums(dx0, sgrad, off, ent, None)[0])
    # the order-sensitive triple: 1 + 1e8 - 1e8 is 0 ascending, 1 descending, in both sums
    p = np.nonzero((off[1:] - off[:-1]) == 3)[0][0]
    up = ref.ordered_sums(dx0, sgrad, off, ent, None)
    down = ref.ordered_sums(dx0, sgrad, off, ent, None, mutant="descending")
    assert (up[0][p] == 0).all() and (up[1][p] == 0).all() and (down[0][p] == 1).all() and (down[1][p] == 1).all()
    assert np.isnan(up[0]).any() and np.isnan(up[1]).any()


def exact_sum_case(seed, idx, n_scene):
    """gradients on a grid of 2^-12 below 2^3: every float32 partial sum of up to 3000 of them is exact in any order, so the
    float32 sums ARE the real sums and the stated cost can be compared without a term for them"""
    rng = np.random.default_rng(seed)
    dx0 = rng.standard_normal((idx.size, 9)).astype(F)
    dx0[:, 0:3] = rng.integers(-2 ** 14, 2 ** 14, (idx.size, 3)) / 2.0 ** 12
    sgrad = (rng.integers(-2 ** 14, 2 ** 14, (idx.size, 3)) / 2.0 ** 12).astype(F)
    delta = (rng.standard_normal((n_scene, 3)) * 0.05).astype(F)
    m = (rng.standard_normal((n_scene, 3)) * 1e-2).astype(F)
    v = (rng.random((n_scene, 3)) * 1e-3).astype(F)
    return delta, m, v, dx0, sgrad, rng.random(n_scene) < 0.5


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_assembly_is_the_gradient_of_the_stated_cost(hand_made, step, masked):
    """L2 once per point, f-loss and Smooth_xyz gradients summed over the slots: float64 autograd of
    sum_e <dx0[e][0:3] + coord_c sgrad[e], delta[idx[e]]> + coord_c sum_p |delta_p|^2 against the restatement (float32 sums
    exact here)."""
    idx, n_scene, off, ent = hand_made
    delta, m, v, dx0, sgrad, mask = exact_sum_case(3, idx, n_scene)
    msk = mask if masked else None
    cc = 0.05                                                      # an L2 / Smooth weight at which both terms show
    gx, gs = ref.ordered_sums(dx0, sgrad, off, ent, msk)
    on = ref.moves(off, msk)
    for name, d3, g in (("f", dx0[:, 0:3], gx), ("smooth", sgrad, gs)):     # exact: the float64 sums are the same numbers
        want = np.zeros((n_scene, 3))
        np.add.at(want, idx, d3.astype(np.float64))
        assert np.array_equal(g.astype(np.float64)[on], want[on]), name
    d64, m64, v64, de, me, ve, _, _ = ref.step64(delta, m, v, dx0, sgrad, off, ent, msk, cc, ref.COORD_LR, step)
    ds, ms, vs = ref.stated_cost_step64(delta, m, v, dx0, sgrad, idx, msk, cc, ref.COORD_LR, step)
    for name, a, b, e in (("delta", d64, ds, de), ("m", m64, ms, me), ("v", v64, vs, ve)):
        print("step %d masked %d %s: stated cost vs float64 reference, error / first-order bound %.4f" % (
            step, masked, name, ref.ratio(a, b, e)))
        assert ref.within(a, b, e).all(), name
    assert np.array_equal(d64[~on], delta[~on].astype(np.float64)) and np.array_equal(ds[~on], delta[~on].astype(np.float64))
    # the per-slot L2 term, the first-slot Smooth term and a shortened list are NOT that gradient
    for mutant in ("l2_per_slot", "smooth_first_slot_only", "drop_last"):
        dm, mm = ref.step64(delta, m, v, dx0, sgrad, off, ent, msk, cc, ref.COORD_LR, step, mutant=mutant)[:2]
        assert not (ref.within(dm, ds, de).all() and ref.within(mm, ms, me).all()), mutant
    # and the float32 restatement, one operation per line, lies within the model of the float64 reference
    d32, m32, v32, _, _ = ref.step32(delta, m, v, dx0, sgrad, off, ent, msk, cc, ref.COORD_LR, step)
    for name, a, b, e in (("delta", d32, d64, de), ("m", m32, m64, me), ("v", v32, v64, ve)):
        assert ref.within(a, b, e).all(), name


def gpu_step_inputs(hand_made):
    idx, n_scene, off, ent = hand_made
    for step, warm in ref.STEP_CASES:
        state = ref.field_step_case(7, idx, n_scene, warm)
        for masked in (False, True):
            yield step, state[:5], (state[5] if masked else None)


def test_float32_restatement_within_the_bound_on_the_gpu_inputs(hand_made):
    idx, n_scene, off, ent = hand_made
    for step, (delta, m, v, dx0, sgrad), msk in gpu_step_inputs(hand_made):
        d64, m64, v64, de, me, ve, gx, gs = ref.step64(delta, m, v, dx0, sgrad, off, ent, msk, ref.COORD_C, ref.COORD_LR, step)
        d32, m32, v32, gx32, gs32 = ref.step32(delta, m, v, dx0, sgrad, off, ent, msk, ref.COORD_C, ref.COORD_LR, step)
        assert same_bits_or_nan(gx, gx32) and same_bits_or_nan(gs, gs32)
        for name, a, b, e in (("delta", d32, d64, de), ("m", m32, m64, me), ("v", v32, v64, ve)):
            assert ref.within(a, b, e).all(), (step, name)
        on = ref.moves(off, msk)
        assert on.sum() < n_scene and (bits(d32[~on]) == bits(delta[~on])).all() and (bits(m32[~on]) == bits(m[~on])).all()
        assert np.isnan(d32).any()                                 # the NaN gradient
        assert (bits(d32[on]) != bits(delta[on])).mean() > 0.5
        # the written-out gradient the mutants are built from is the reference's when nothing is wrong with it
        moved = ref.step64(delta, m, v, dx0, sgrad, off, ent, msk, ref.COORD_C, ref.COORD_LR, step)
        assert ref.within(moved[0], d64, de).all()


def test_every_mutant_shows_on_the_gpu_inputs(hand_made):
    """bits for the sums, the bound for delta / m / v: on the very inputs tests/test_gpu_scene_nu_field_kernels.py feeds the
    kernel"""
    idx, n_scene, off, ent = hand_made
    shown = {mutant: 0 for mutant in ref.SUM_MUTANTS + ref.STEP_MUTANTS}
    n_cases = 0
    for step, (delta, m, v, dx0, sgrad), msk in gpu_step_inputs(hand_made):
        n_cases += 1
        d64, m64, v64, de, me, ve, gx, gs = ref.step64(delta, m, v, dx0, sgrad, off, ent, msk, ref.COORD_C, ref.COORD_LR, step)
        for mutant in shown:
            try:
                dm, mm, vm, _, _, _, gxm, gsm = ref.step64(delta, m, v, dx0, sgrad, off, ent, msk, ref.COORD_C, ref.COORD_LR, step,
                                                           mutant=mutant)
            except ZeroDivisionError:                              # bias_late at step 1: a step of size lr / (1 - beta1^0)
                assert (mutant, step) == ("bias_late", 1)
                shown[mutant] += 1
                continue
            if mutant in ref.SUM_MUTANTS:
                shown[mutant] += not (same_bits_or_nan(gx, gxm) and same_bits_or_nan(gs, gsm))
            else:
                shown[mutant] += not (ref.within(dm, d64, de).all() and ref.within(mm, m64, me).all() and ref.within(vm, v64, ve).all())
    print("cases (of %d) in which each mutant leaves the bits / the bound: %s" % (n_cases, shown))
    n_warm = 2 * sum(1 for _, warm in ref.STEP_CASES if warm)
    for mutant, n in shown.items():
        # a mask-related mutant can only show in the masked cases; the per-slot L2 term only where delta has left zero
        # (before step 1 there is nothing to multiply); everything else in every case
        want = {"moves_unmasked": n_cases // 2, "l2_per_slot": n_warm}.get(mutant, n_cases)
        assert n == want and n > 0, (mutant, n)


# ------------------------------------------------------------------------------------------------ refusals, no device
def test_refusals_without_a_device():
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    from pointsecguard_amd.models import pointnet2_sem_seg, pointnet2_sem_seg_msg
    pn2 = pointnet2_sem_seg.get_model(13).eval()
    atk = SceneNUAttack(pn2)
    assert atk.field == "color" and atk.last_delta is None and (atk.coord_c, atk.coord_lr) == (atk.c, atk.lr)
    atk = SceneNUAttack(pn2, c=3e-4, lr=0.02, field="coord")
    assert atk.field == "coord" and (atk.coord_c, atk.coord_lr) == (3e-4, 0.02)       # the fall-backs
    atk = SceneNUAttack(pn2, field="both", coord_c=0.0, coord_lr=0.5)
    assert (atk.c, atk.lr, atk.coord_c, atk.coord_lr) == (1e-4, 0.01, 0.0, 0.5)
    msg = pointnet2_sem_seg_msg.get_model(13).eval()
    SceneNUAttack(msg, steps=2, field="color")
    for field in ("coord", "both"):
        with pytest.raises(NotImplementedError, match="psg_pn2_backward_full refuses MSG"):
            SceneNUAttack(msg, field=field)
    with pytest.raises(ValueError):
        SceneNUAttack(pn2, field="xyz")
    for kw in (dict(coord_lr=0.0), dict(coord_lr=-0.01), dict(coord_c=-1e-4), dict(lr=0.0), dict(c=-1.0), dict(coord_lr=float("nan"))):
        with pytest.raises(ValueError):
            SceneNUAttack(pn2, field="coord", **kw)
    with pytest.raises(ValueError):
        SceneNUAttack(pn2, coord_lr=0.0)                             # a bad value is refused under the colour field too
    # the symbol is bound with the header's argument list
    from pointsecguard_amd import _lib
    assert len(_lib.SIGNATURES["psg_scene_nu_field_step"][1]) == 20
