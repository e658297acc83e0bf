"""GPU tests of the two coordinate-field kernels of the whole-scene attack (csrc/psg_scene.hip: psg_scene_delta_to_blocks,
psg_scene_field_step) on their own, bit for bit against tests/scene_field_ref.py."""
import numpy as np
import pytest
import torch

import scene_field_ref
import scene_ref
from test_gpu_harness import synth_scene

pytestmark = pytest.mark.gpu
F = np.float32
ALPHA, EPS = 0.05, 0.1


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


@pytest.fixture(scope="module")
def indices(slicer_index):
    return {"slicer": slicer_index, "hand_made": scene_ref.hand_made_index()}


@pytest.mark.parametrize("case", ["slicer", "hand_made"])
def test_delta_to_blocks_bit_for_bit(indices, case):
    from pointsecguard_amd import runtime
    idx, n_scene = indices[case]
    rng = np.random.default_rng(1)
    delta = (rng.standard_normal((n_scene, 3)) * 0.1).astype(F)
    delta[::5] = F(0)
    x_clean = rng.standard_normal((idx.size, 9)).astype(F)
    x = rng.standard_normal((idx.size, 9)).astype(F)
    x[3, 4], x[4, 7] = np.nan, -0.0                               # bytes, not values, are kept in channels 3:9
    want = scene_field_ref.delta_to_blocks(delta, idx, x_clean, x)
    outs = []
    for _ in range(2):
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        xd, cd = dev(x), dev(x_clean)
        runtime.scene_delta_to_blocks(dev(delta), dev(idx), cd, xd, bad)
        outs.append(xd.cpu().numpy())
        assert int(bad.item()) == 0
        assert np.array_equal(bits(cd.cpu().numpy()), bits(x_clean))          # the clean blocks are read only
    assert np.array_equal(bits(outs[0]), bits(want)) and np.array_equal(bits(outs[0]), bits(outs[1]))
    assert np.array_equal(bits(outs[0][:, 3:]), bits(x[:, 3:]))               # channels 3:9 untouched
    assert not np.array_equal(bits(outs[0][:, :3]), bits(x_clean[:, :3]))
    # delta = 0: the clean coordinates bit for bit
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    xd = dev(x)
    runtime.scene_delta_to_blocks(torch.zeros(n_scene, 3, device="cuda"), dev(idx), dev(x_clean), xd, bad)
    assert np.array_equal(bits(xd.cpu().numpy()[:, :3]), bits(x_clean[:, :3]))


def test_delta_to_blocks_flags_an_index_out_of_range(indices):
    from pointsecguard_amd import runtime
    idx, n_scene = indices["hand_made"]
    rng = np.random.default_rng(2)
    delta = rng.standard_normal((n_scene, 3)).astype(F)
    x_clean = rng.standard_normal((idx.size, 9)).astype(F)
    x = rng.standard_normal((idx.size, 9)).astype(F)
    for wrong in (n_scene, -1, 2 ** 31 - 1):
        broken = idx.copy()
        broken[[17, 4000]] = wrong
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        xd = dev(x)
        runtime.scene_delta_to_blocks(dev(delta), dev(broken), dev(x_clean), xd, bad)
        got = xd.cpu().numpy()
        assert int(bad.item()) == 1
        assert np.array_equal(bits(got[[17, 4000]]), bits(x[[17, 4000]]))     # the bad rows are left alone
        ok = np.ones(idx.size, bool)
        ok[[17, 4000]] = False
        want = scene_field_ref.delta_to_blocks(delta, idx, x_clean, x)
        assert np.array_equal(bits(got[ok]), bits(want[ok]))


@pytest.mark.parametrize("direction", [1.0, -1.0])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", ["slicer", "hand_made"])
def test_field_step_bit_for_bit(indices, case, masked, last, direction):
    """Gradients with exact zeros, a pair that cancels, a NaN, the order-sensitive triple; displacements at both faces of
    the eps ball; (hand-made index) a point without a slot and one with 3000."""
    from pointsecguard_amd import runtime
    idx, n_scene = indices[case]
    delta, dx0, mask = scene_field_ref.field_case(7, idx, n_scene, eps=EPS)
    off, ent = scene_ref.occ_lists(idx, n_scene)
    want, want_g = scene_field_ref.field_step(delta, dx0, off, ent, mask if masked else None, ALPHA, EPS, direction, bool(last))
    assert not np.array_equal(bits(want), bits(delta))
    md = dev(mask.astype(np.uint8)) if masked else None
    outs = []
    for _ in range(2):
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_off, d_ent = runtime.scene_occ_build(dev(idx), n_scene, bad)
        dd, g = dev(delta), torch.full((n_scene, 3), 7.0, dtype=torch.float32, device="cuda")
        runtime.scene_field_step(dd, md, d_off, d_ent, dev(dx0), ALPHA, EPS, direction, last, gsum_out=g)
        outs.append((dd.cpu().numpy(), g.cpu().numpy()))
    got, got_g = outs[0]
    assert np.array_equal(bits(got), bits(want))
    nan = np.isnan(want_g)
    assert nan.any() and np.array_equal(np.isnan(got_g), nan)             # (a NaN's payload is not part of the contract)
    assert np.array_equal(bits(got_g)[~nan], bits(want_g)[~nan])
    assert np.array_equal(bits(got), bits(outs[1][0])) and np.array_equal(bits(got_g)[~nan], bits(outs[1][1])[~nan])
    if case == "hand_made":
        assert np.array_equal(bits(got[5]), bits(delta[5]))               # the point without a slot did not move
    if masked:
        assert np.array_equal(bits(got[~mask]), bits(delta[~mask]))
    if not last:
        assert np.abs(got).max() <= F(EPS)
    dd = dev(delta)                                                       # without gsum_out the step is the same
    runtime.scene_field_step(dd, md, d_off, d_ent, dev(dx0), ALPHA, EPS, direction, last)
    assert np.array_equal(bits(dd.cpu().numpy()), bits(want))


def test_rows_beyond_the_slot_range_are_refused():
    from pointsecguard_amd import _lib, runtime
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    f = torch.zeros(9, dtype=torch.float32, device="cuda")
    too_many = (2 ** 31 - 1) // 9 + 1
    with pytest.raises(_lib.PsgError, match="INT_MAX / 9"):
        _lib.call("psg_scene_field_step", runtime.ptr(f), None, runtime.ptr(one), runtime.ptr(one), runtime.ptr(f), too_many, 1,
                  0.05, 0.1, 1.0, 0, None, runtime.stream())
    with pytest.raises(_lib.PsgError, match="INT_MAX / 9"):
        _lib.call("psg_scene_delta_to_blocks", runtime.ptr(f), runtime.ptr(one), runtime.ptr(f), too_many, 1, runtime.ptr(f),
                  runtime.ptr(one), runtime.stream())
    for rows in (0, -1):
        with pytest.raises(_lib.PsgError, match="INT_MAX / 9"):
            _lib.call("psg_scene_field_step", runtime.ptr(f), None, runtime.ptr(one), runtime.ptr(one), runtime.ptr(f), rows, 1,
                      0.05, 0.1, 1.0, 0, None, runtime.stream())
    with pytest.raises(_lib.PsgError):
        runtime.scene_delta_to_blocks(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 9), torch.zeros(4, 9),
                                      one)                                # no CPU path
    torch.cuda.synchronize()
