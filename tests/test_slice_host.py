"""CPU tests of the device slicer's contract: tests/slice_ref.py - count, ascending members, gather in
double with one rounding, driven by harness.slice_plan - against the reference's recorded blocks (tests/golden/harness.npz) and
against ScannetDatasetWholeScene.__getitem__ on crafted scenes whose premises are asserted here, and the mutants it must catch.
Everything is compared for equality, generator state included."""
import os

import numpy as np
import pytest

import slice_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "harness.npz")
NAMES = ("data", "label", "smpw", "index")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


def fixture_dataset(g):
    from pointsecguard_amd.harness import ScannetDatasetWholeScene
    names = [str(n) for n in g["file_list"]]
    return ScannetDatasetWholeScene(None, block_points=int(g["block_points"]), split="test", test_area=5, stride=0.5, block_size=1.0,
                                    padding=0.001, scenes={n: g["scene%d" % i].copy() for i, n in enumerate(names)})


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def assert_same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), \
            (what, name)


@pytest.fixture(scope="module")
def crafted():
    return slice_ref.crafted_scenes()


def cases(g, crafted):
    """(name, dataset, scene index, seed) of every case: the two fixture scenes and the crafted ones"""
    fx = fixture_dataset(g)
    out = [("fixture%d" % si, fx, si, 100 + si) for si in range(len(fx))]
    return out + [(name, slice_ref.dataset(room), 0, 7) for name, room in crafted.items()]


def run(fn, seed):
    np.random.seed(seed)
    out = fn()
    return out, np.random.get_state()


def test_reference_fixture(g):
    ds = fixture_dataset(g)
    assert int(g["block_points"]) == 256
    for si in range(len(ds)):
        got, state = run(lambda: slice_ref.slice_scene(ds, si), 100 + si)
        want = (g["data_room%d" % si].astype(np.float32), g["label_room%d" % si].astype(np.int32),
                g["sample_weight%d" % si].astype(np.float32), g["index_room%d" % si].astype(np.int32))
        assert_same(got, want, "reference, scene %d" % si)
        host, host_state = run(lambda: slice_ref.host_item(ds, si), 100 + si)
        assert_same(got, host, "__getitem__, scene %d" % si)
        assert same_state(state, host_state)


def test_premises_of_the_crafted_scenes(crafted):
    from pointsecguard_amd import harness
    counts, grids = {}, {}
    for name, room in crafted.items():
        ds = slice_ref.dataset(room)
        cmin, cmax = room[:, :3].min(axis=0), room[:, :3].max(axis=0)
        w, c, grid = slice_ref.cells(cmin, cmax, ds.block_size, ds.stride, ds.padding)
        hw, hc, gx, gy = harness.slice_cells(cmin, cmax, ds.block_size, ds.stride, ds.padding)
        assert np.array_equal(w, hw) and np.array_equal(c, hc) and grid == (gx, gy)
        counts[name], grids[name] = slice_ref.count(room[:, 0], room[:, 1], w), grid
    bp = slice_ref.DS_KW["block_points"]
    assert grids["one_point_cell"] == (3, 1) and counts["one_point_cell"][2] == 1 and counts["one_point_cell"][0] > bp
    assert grids["exact_multiple"] == (1, 1) and counts["exact_multiple"][0] == 2 * bp
    assert grids["hole"] == (3, 1) and counts["hole"][1] == 0 and counts["hole"][0] > 0 and counts["hole"][2] > 0
    # the six probes: on either bound and one ulp inside count, one ulp outside does not
    w, bx = slice_ref.boundary_xs()
    room = crafted["window_edges"]
    assert np.array_equal(room[:6, 0], np.array(list(bx.values()))) and grids["window_edges"] == (3, 1)
    assert bx["lo_out"] < bx["lo"] < bx["lo_in"] and bx["hi_in"] < bx["hi"] < bx["hi_out"]
    inside = slice_ref.members(room[:, 0], room[:, 1], w[None])[0]
    assert [k in inside for k in range(6)] == [True, True, False, True, True, False]
    # the last column is clamped to the wall: its unclamped end lies beyond the max corner
    room = crafted["clamped_column"]
    assert grids["clamped_column"][0] == 4 and 0.0 + 3 * 0.5 + 1.0 > room[:, 0].max() == 2.3
    assert grids["narrow"][0] == 1 and crafted["narrow"][:, 0].max() < 1.0
    assert crafted["n257"].shape[0] == 257 and crafted["n4097"].shape[0] == 4097


def test_crafted_scenes_match_the_host_slicer(g, crafted):
    for name, ds, si, seed in cases(g, crafted):
        before = ds.scene_points_list[si].copy()
        got, state = run(lambda: slice_ref.slice_scene(ds, si), seed)
        host, host_state = run(lambda: slice_ref.host_item(ds, si), seed)
        assert_same(got, host, name)
        assert same_state(state, host_state), name
        assert np.array_equal(ds.scene_points_list[si], before)


def test_slice_plan_is_the_slicers_draws():
    """the plan argument itself, on counts that cover: no padding (a permutation is still drawn), padding with replacement,
    exact multiples, one member, empty cells"""
    from pointsecguard_amd import harness
    bp = 64
    counts = [64, 0, 1, 128, 20, 0, 33, 65, 640]
    np.random.seed(11)
    src_pos, first_block, nb = harness.slice_plan(counts, bp)
    state = np.random.get_state()
    np.random.seed(11)
    want = []
    for cnt in counts:
        if cnt == 0:
            continue
        inside = np.arange(cnt)                      # the slicer's own statements, on positions
        total = int(np.ceil(inside.size / bp)) * bp
        extra = total - inside.size
        fill = np.random.choice(inside, extra, replace=extra > inside.size)
        idx = np.concatenate((inside, fill))
        np.random.shuffle(idx)
        want.append(idx)
    assert same_state(state, np.random.get_state())
    assert src_pos.dtype == np.int32 and np.array_equal(src_pos, np.concatenate(want))
    assert nb == 1 + 1 + 2 + 1 + 1 + 2 + 10 and first_block.tolist() == [0, 1, 1, 2, 4, 5, 5, 6, 8]


@pytest.mark.parametrize("mutant", slice_ref.MUTANTS)
def test_mutants_are_caught(g, crafted, mutant):
    failed = []
    for name, ds, si, seed in cases(g, crafted):
        host, host_state = run(lambda: slice_ref.host_item(ds, si), seed)
        try:
            got, state = run(lambda: slice_ref.slice_scene(ds, si, mutant=mutant), seed)
        except (ValueError, IndexError):
            failed.append(name)
            continue
        same = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, host)) and same_state(state, host_state)
        if not same:
            failed.append(name)
    print("%s fails %s" % (mutant, failed))
    assert failed, "the mutant %s passes every case" % mutant
    expected = {"no_draw_without_padding": "exact_multiple", "draw_for_empty": "hole", "strict_window": "window_edges",
                "start_before_clamp": "clamped_column", "float32": "clamped_column", "reciprocal": "clamped_column"}
    if mutant in expected:
        assert expected[mutant] in failed


def test_float32_and_reciprocal_premises(crafted):
    """the scene the two arithmetic mutants are caught on holds entries where they differ from double-then-round"""
    room = crafted["clamped_column"]
    x, z, cmax = room[:, 0], room[:, 2], room[:, :3].max(axis=0)
    f = np.float32
    centre = f(0.0 + 1.0 / 2.0)                          # the first column's
    assert ((x.astype(f) - centre) != (x - np.float64(centre)).astype(f)).any()
    assert cmax[2] == 2.8 and z[0] == slice_ref.reciprocal_probe(2.8)
    assert f(z[0] / cmax[2]) != f(z[0] * (1.0 / cmax[2]))


def test_refusals():
    from pointsecguard_amd import harness
    with pytest.raises(ValueError):
        harness.slice_plan([0, 0, 0], 64)
    with pytest.raises(ValueError):
        harness.slice_plan([], 64)
    ds = slice_ref.dataset(slice_ref.crafted_scenes()["hole"])
    for fn in (harness.evaluate_whole_scene, harness.evaluate_whole_scene_consistent):
        with pytest.raises(ValueError, match="slicer"):
            fn(None, ds, None, slicer="bogus")           # before any device work: there is no classifier to touch

    class Plain:
        block_points = 64

        def __len__(self):
            return 0
    with pytest.raises(TypeError, match="device_item"):
        harness.evaluate_whole_scene(None, Plain(), None, slicer="device")
