"""GPU tests of psg_scene_nu_field_step (csrc/psg_scene_nu.hip) on its own, against
tests/scene_nu_field_ref.py: the two ordered sums and every byte that must stay are compared bit for bit; delta / m / v against
the float64 reference fed the float32 sums, within the bound tests/test_gpu_nu_field_kernels.py applies to
psg_nu_coord_adam_step_rooms (attack_ref64.bound of nu_field_ref64.coord_adam_step's error model).  Every case runs twice and
must repeat.

Inputs: scene_ref.hand_made_index (700 points, 5003 slots, point 5 never occurring, point 9 occurring 3000 times), the
order-sensitive triple 1, 1e8, -1e8 and a NaN in both gradients, outputs pre-filled with NaN / 0xFF."""
import numpy as np
import pytest
import torch

import scene_nu_field_ref as ref
import scene_ref
from test_gpu_scene_nu_kernels import bits, dev, lists, report, same_bits_or_nan, word  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("step,warm", ref.STEP_CASES)
def test_field_step(lists, step, warm, masked):
    from pointsecguard_amd import runtime
    idx, n_scene, off, ent, d_off, d_ent = lists
    delta, m, v, dx0, sgrad, mask = ref.field_step_case(7, idx, n_scene, warm)
    assert np.isnan(dx0[:, 0:3]).any() and np.isnan(sgrad).any()
    msk = mask if masked else None
    d_mask = dev(mask.astype(np.uint8)) if masked else None
    d64, m64, v64, de, me, ve, gx, gs = ref.step64(delta, m, v, dx0, sgrad, off, ent, msk, ref.COORD_C, ref.COORD_LR, step)
    on = ref.moves(off, msk)

    def run(active, with_sums=True):
        dd, md, vd = dev(delta), dev(m), dev(v)
        filled = lambda: torch.full((n_scene, 3), float("nan"), dtype=torch.float32, device="cuda")      # noqa: E731
        gxd, gsd = (filled(), filled()) if with_sums else (None, None)
        runtime.scene_nu_field_step(dd, md, vd, d_mask, d_off, d_ent, dev(dx0), dev(sgrad), ref.COORD_C, ref.COORD_LR, ref.BETA1,
                                    ref.BETA2, ref.ADAM_EPS, step, word(active), gxd, gsd)
        return [t.cpu().numpy() if t is not None else None for t in (dd, md, vd, gxd, gsd)]

    first, second = run(1), run(1)
    for a, b in zip(first, second):
        assert same_bits_or_nan(a, b)
    gd, gm, gv, ggx, ggs = first
    # the two ordered sums, bit for bit: the triple sums to 0 in slot order (1 the other way round), +0 where nothing moves
    assert same_bits_or_nan(ggx, gx) and same_bits_or_nan(ggs, gs)
    p = np.nonzero((off[1:] - off[:-1]) == 3)[0][0]
    assert on[p] and (bits(ggx[p]) == 0).all() and (bits(ggs[p]) == 0).all()
    assert (bits(ggx[~on]) == 0).all() and (bits(ggs[~on]) == 0).all() and np.isnan(ggx).any()
    # points that do not move keep their bytes
    assert not on[5] and on.sum() < n_scene
    for got, before in ((gd, delta), (gm, m), (gv, v)):
        assert np.array_equal(bits(got[~on]), bits(before[~on]))
    what = "field step %d masked %d" % (step, masked)
    report(what + " delta", gd[on], d64[on], de[:, on])
    report(what + " m", gm[on], m64[on], me[:, on])
    report(what + " v", gv[on], v64[on], ve[:, on])
    moved = on[:, None] & np.isfinite(gd)
    assert (bits(gd)[moved] != bits(delta)[moved]).mean() > 0.5
    # without the optional outputs the step is the same; active == 0 leaves every byte, the NaN-filled outputs included
    for a, b in zip(run(1, with_sums=False)[:3], first[:3]):
        assert same_bits_or_nan(a, b)
    idle = run(0)
    for got, before in zip(idle[:3], (delta, m, v)):
        assert np.array_equal(bits(got), bits(before))
    assert np.isnan(idle[3]).all() and np.isnan(idle[4]).all()


def test_untouched_bytes_survive_a_0xff_fill(lists):
    """delta / m / v pre-filled with 0xFF bytes (a NaN with a payload): what does not move keeps the payload"""
    from pointsecguard_amd import runtime
    idx, n_scene, off, ent, d_off, d_ent = lists
    _, _, _, dx0, sgrad, mask = ref.field_step_case(7, idx, n_scene, False)
    on = ref.moves(off, mask)
    ff = np.full((n_scene, 3), 0xFFFFFFFF, np.uint32).view(F)
    dd, md, vd = dev(ff), dev(ff), dev(ff)
    runtime.scene_nu_field_step(dd, md, vd, dev(mask.astype(np.uint8)), d_off, d_ent, dev(dx0), dev(sgrad), ref.COORD_C, ref.COORD_LR,
                                ref.BETA1, ref.BETA2, ref.ADAM_EPS, 1, word(1))
    for t in (dd, md, vd):
        assert (bits(t.cpu().numpy())[~on] == 0xFFFFFFFF).all()


def test_refusals():
    from pointsecguard_amd import _lib, runtime
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    f = torch.zeros(3, dtype=torch.float32, device="cuda")
    too_many = (2 ** 31 - 1) // 9 + 1

    def call(rows, step, delta=f):
        _lib.call("psg_scene_nu_field_step", runtime.ptr(delta), runtime.ptr(f), runtime.ptr(f), None, runtime.ptr(one), runtime.ptr(one),
                  runtime.ptr(f), runtime.ptr(f), rows, 1, 1e-4, 0.01, 0.9, 0.999, 1e-8, step, runtime.ptr(one), None, None,
                  runtime.stream())

    with pytest.raises(_lib.PsgError, match="INT_MAX / 9"):
        call(too_many, 1)
    with pytest.raises(_lib.PsgError):
        call(1, 0)                                                # Adam's step count starts at 1
    with pytest.raises(_lib.PsgError):
        call(1, 1, delta=None)
    with pytest.raises(_lib.PsgError):
        runtime.scene_nu_field_step(torch.zeros(4, 3), f, f, None, one, one, f, f, 1e-4, 0.01, 0.9, 0.999, 1e-8, 1, one)      # no CPU path
