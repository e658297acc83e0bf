"""GPU tests of the four whole-scene attack kernels (csrc/psg_scene.hip) on their own, bit for bit against tests/scene_ref.py:
occurrence lists, scene colours into the block slots, the dlogp row mask and the ordered-sum PGD step."""
import numpy as np
import pytest
import torch

import scene_ref
from test_gpu_harness import synth_scene

pytestmark = pytest.mark.gpu
F = np.float32


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda().contiguous()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def slicer_index():
    from pointsecguard_amd import harness
    ds = harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": synth_scene(11, 5000, 1.6, 1.2)})
    np.random.seed(3)
    index = ds[0][3]
    assert index.shape == (18, 1024)
    return index.reshape(-1).astype(np.int32), 5000


def occ_build(idx, n_scene):
    from pointsecguard_amd import runtime
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    off, ent = runtime.scene_occ_build(dev(idx), n_scene, bad)
    torch.cuda.synchronize()
    return off.cpu().numpy(), ent.cpu().numpy(), int(bad.item())


@pytest.mark.parametrize("case", ["slicer", "hand_made"])
def test_occ_build_equals_stable_argsort(slicer_index, case):
    idx, n_scene = slicer_index if case == "slicer" else scene_ref.hand_made_index()
    want_off, want_ent = scene_ref.occ_lists(idx, n_scene)
    off, ent, bad = occ_build(idx, n_scene)
    assert bad == 0
    assert np.array_equal(off, want_off) and np.array_equal(ent, want_ent)
    assert np.array_equal(ent, np.argsort(idx, kind="stable"))
    off2, ent2, _ = occ_build(idx, n_scene)                       # the lists do not depend on scheduling
    assert np.array_equal(off, off2) and np.array_equal(ent, ent2)


def test_occ_build_flags_an_index_out_of_range():
    idx, n_scene = scene_ref.hand_made_index()
    for wrong in (n_scene, -1, 2 ** 31 - 1):
        broken = idx.copy()
        broken[[17, 4000]] = wrong
        off, ent, bad = occ_build(broken, n_scene)
        assert bad == 1
        # the valid slots still form their lists; the two bad ones are in none, the tail of occ_ent holds -1
        valid = np.nonzero((broken >= 0) & (broken < n_scene))[0]
        want = valid[np.argsort(broken[valid], kind="stable")]
        assert off[-1] == valid.size and np.array_equal(ent[:valid.size], want) and (ent[valid.size:] == -1).all()


def test_colour_to_blocks_keeps_the_other_channels(slicer_index):
    from pointsecguard_amd import runtime
    idx, n_scene = slicer_index
    rng = np.random.default_rng(1)
    rgb = rng.random((n_scene, 3)).astype(F)
    x = rng.standard_normal((idx.size, 9)).astype(F)
    x[3, 0], x[4, 7] = np.nan, -0.0                               # bytes, not values, are kept
    want = scene_ref.colour_to_blocks(rgb, idx, x)
    outs = []
    for _ in range(2):
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        xd = dev(x).reshape(18, 1024, 9)
        runtime.scene_colour_to_blocks(dev(rgb), dev(idx).reshape(18, 1024), xd, bad)
        outs.append(xd.cpu().numpy().reshape(-1, 9))
        assert int(bad.item()) == 0
    assert np.array_equal(bits(outs[0]), bits(want)) and np.array_equal(bits(outs[0]), bits(outs[1]))
    assert np.array_equal(bits(outs[0][:, :3]), bits(x[:, :3])) and np.array_equal(bits(outs[0][:, 6:]), bits(x[:, 6:]))
    # a bad index raises the flag and leaves its row alone
    broken = idx.copy()
    broken[5] = n_scene
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    xd = dev(x)
    runtime.scene_colour_to_blocks(dev(rgb), dev(broken), xd, bad)
    assert int(bad.item()) == 1 and np.array_equal(bits(xd.cpu().numpy()[5]), bits(x[5]))


def test_rows_mask(slicer_index):
    from pointsecguard_amd import runtime
    idx, n_scene = slicer_index
    rng = np.random.default_rng(2)
    dlogp = rng.standard_normal((idx.size, 13)).astype(F)
    mask = rng.random(n_scene) < 0.3
    want = scene_ref.rows_mask(dlogp, idx, mask)
    outs = []
    for _ in range(2):
        d = dev(dlogp)
        runtime.scene_rows_mask(d, dev(idx), dev(mask.astype(np.uint8)))
        outs.append(d.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(want)) and np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("direction", [1.0, -1.0])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_pgd_step_bit_for_bit(masked, last, direction):
    """Gradients with exact zeros, a pair that cancels, a NaN, an order-sensitive triple; colours at the faces of the eps ball
    and of [0, 1]; a point without a slot and one with 3000 (tests/scene_ref.py: step_case)."""
    from pointsecguard_amd import runtime
    idx, n_scene = scene_ref.hand_made_index()
    alpha, eps = 0.05, 0.1
    c, c0, dx0, mask = scene_ref.step_case(7, idx, n_scene, eps=eps)
    off, ent = scene_ref.occ_lists(idx, n_scene)
    want, want_g = scene_ref.scene_step(c, c0, dx0, off, ent, mask if masked else None, alpha, eps, direction, bool(last))
    assert not np.array_equal(bits(want), bits(c))
    outs = []
    for _ in range(2):
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_off, d_ent = runtime.scene_occ_build(dev(idx), n_scene, bad)
        cd, g = dev(c), torch.full((n_scene, 3), 7.0, dtype=torch.float32, device="cuda")
        runtime.scene_pgd_step(cd, dev(c0), dev(mask.astype(np.uint8)) if masked else None, d_off, d_ent, dev(dx0), alpha, eps,
                               direction, last, gsum_out=g)
        outs.append((cd.cpu().numpy(), g.cpu().numpy()))
    got, got_g = outs[0]
    assert np.array_equal(bits(got), bits(want))
    nan = np.isnan(want_g)
    assert nan.any() and np.array_equal(np.isnan(got_g), nan)             # (a NaN's payload is not part of the contract)
    assert np.array_equal(bits(got_g)[~nan], bits(want_g)[~nan])
    assert np.array_equal(bits(got), bits(outs[1][0])) and np.array_equal(bits(got_g)[~nan], bits(outs[1][1])[~nan])
    # the point without a slot did not move; without gsum_out the step is the same
    assert np.array_equal(bits(got[5]), bits(c[5]))
    cd = dev(c)
    runtime.scene_pgd_step(cd, dev(c0), dev(mask.astype(np.uint8)) if masked else None, d_off, d_ent, dev(dx0), alpha, eps,
                           direction, last)
    assert np.array_equal(bits(cd.cpu().numpy()), bits(want))


def test_rows_beyond_the_slot_range_are_refused():
    from pointsecguard_amd import _lib, runtime
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    f = torch.zeros(3, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.PsgError, match="INT_MAX / 9"):
        _lib.call("psg_scene_pgd_step", runtime.ptr(f), runtime.ptr(f), None, runtime.ptr(one), runtime.ptr(one), runtime.ptr(f),
                  (2 ** 31 - 1) // 9 + 1, 1, 0.05, 0.1, 1.0, 0, None, runtime.stream())
    with pytest.raises(_lib.PsgError):
        runtime.scene_occ_build(torch.zeros(4, dtype=torch.int32), 4, one)          # no CPU path
