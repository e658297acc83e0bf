"""Grid sub-sampling and sub-cloud projection, host side: the numpy float32 restatement (tests/grid_ref.py) against the
output of the reference's own native code (tests/golden/grid_sub.npz, written by tests/golden/make_golden_grid.py), the
mutants that comparison must catch, the projection's restatement against sklearn's KDTree, and the refusals the Python
surface makes before any device work.  The device side is tests/test_gpu_grid.py.

Equality bar: barycentres and mean features bit-equal (rows matched by a lexicographic sort: the reference's order is its
hash map's); labels equal on every cell whose most frequent label is unique, and on a tied cell the reference's label is
one of the tied values and the restatement's is the smallest of them."""
import os

import numpy as np
import pytest

import grid_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "grid_sub.npz")
NAMES = ("room", "neg", "tiny")
TIE_CAP = 0.05


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLD))


def case(fx, name):
    return fx[name + "_points"], fx[name + "_colors"], fx[name + "_labels"], float(fx[name + "_dl"])


def check_against_fixture(fx, name, **mutant):
    """Raises AssertionError where the restatement (or a mutant of it) and the reference's output disagree."""
    p, col, lab, dl = case(fx, name)
    got = grid_ref.grid_sub_sampling(p, col, lab, dl, **mutant)
    rp, rf, rl, _ = grid_ref.canonical(fx[name + "_sub_points"], fx[name + "_sub_colors"], fx[name + "_sub_labels"])
    gp, gf, gl, o = grid_ref.canonical(got["sub_points"], got["sub_features"], got["sub_labels"])
    assert gp.shape == rp.shape, "number of occupied cells: %d against the reference's %d" % (len(gp), len(rp))
    assert grid_ref.same_bits(gp, rp), "barycentres differ in %d rows" % int((gp.view(np.uint32) != rp.view(np.uint32)).any(1).sum())
    assert grid_ref.same_bits(gf, rf), "mean features differ"
    tied = got["tied"][o]
    assert np.array_equal(gl[~tied], rl[~tied]), "labels differ on cells without a tie"
    vox_of = np.argsort(o)[got["voxel_of_point"]]            # canonical row of every input point
    lab2 = lab.reshape(len(p), -1)
    for v, c in zip(*np.nonzero(tied)):
        vals, cnt = np.unique(lab2[vox_of == v, c], return_counts=True)
        top = vals[cnt == cnt.max()]
        assert len(top) > 1
        assert rl[v, c] in top, "the reference's label of a tied cell is not among the tied values"
        assert gl[v, c] == top.min(), "the restatement's label of a tied cell is not the smallest tied value"
    return got


@pytest.mark.parametrize("name", NAMES)
def test_restatement_vs_reference_fixture(fx, name):
    got = check_against_fixture(fx, name)
    ties = float(got["tied"].any(axis=1).mean())
    print("%s: %d cells, %.2f %% with tied labels" % (name, len(got["count"]), 100 * ties))
    assert ties <= TIE_CAP


@pytest.mark.parametrize("mutant", ({"reverse": True}, {"origin_floor": False}, {"bary_div": True}, {"ties_largest": True}),
                         ids=lambda m: next(iter(m)))
def test_mutants_are_caught(fx, mutant):
    """Sums in reverse input order, origin = min corner without the floor, sum / count for the barycentre, ties to the
    largest label: each must fail the comparison on every fixture that can show it (`room`: on all of these)."""
    with pytest.raises(AssertionError):
        check_against_fixture(fx, "room", **mutant)


def test_restatement_properties(fx):
    p, col, lab, dl = case(fx, "tiny")
    a = grid_ref.grid_sub_sampling(p, col, lab, dl)
    assert a["sub_labels"].shape == (len(a["count"]), 1) and a["sub_labels"].dtype == np.int32
    assert a["count"].sum() == len(p) and np.array_equal(np.bincount(a["voxel_of_point"]), a["count"])
    key = grid_ref.cell_keys(p, dl)
    first = np.r_[True, np.diff(a["voxel_of_point"][np.argsort(key, kind="stable")]) > 0]
    assert first.sum() == len(a["count"])                                     # rows ascend with the key
    two = grid_ref.grid_sub_sampling(p, None, np.stack([lab, -lab], 1), dl)   # label dimensions vote independently
    assert np.array_equal(two["sub_labels"][:, 0], a["sub_labels"][:, 0])


def test_negative_cell_index_is_clamped():
    """min = the float32 below fl(-396 * 0.04): floor(min * (1 / dl)) * dl rounds ABOVE the minimum, the cell index of the minimum is -1 in the
    reference's formula (undefined there); the restatement - and the device - count it as cell 0."""
    dl = np.float32(0.04)
    x = np.nextafter(np.float32(-396) * dl, np.float32(-np.inf))
    origin, n, cell = grid_ref.grid_of(np.array([[x, 0, 0], [x + 1, 1, 1]], np.float32), dl)
    assert origin[0] > x and np.floor((x - origin[0]) / dl) == -1
    assert cell.min() == 0 and (n >= 1).all()


def test_nearest_restatement_vs_kdtree(fx):
    """sklearn's KDTree.query works on float64 copies, the restatement in float32: where their indices differ, the two
    candidates' float64 squared distances must agree within a relative 2^-20.

    Bound: the float32 distance of one candidate carries at most four roundings of relative size 2^-24 on its value (the
    subtraction, the square, two additions - all terms are non-negative, so relative errors do not amplify): at most
    (1 + 2^-24)^4 - 1 < 2^-21.9 beside its exact value.  The float32 argmin prefers candidate b over the float64 winner a
    only if fl(d_b) <= fl(d_a), hence d_b (1 - 2^-21.9) <= d_a (1 + 2^-21.9), so d_a <= d_b <= d_a (1 + 2^-20.8) < d_a (1 + 2^-20)."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    for name in NAMES:
        p, col, lab, dl = case(fx, name)
        sub = grid_ref.grid_sub_sampling(p, None, None, dl)["sub_points"]
        got = grid_ref.nearest_sub_point(sub, p)
        want = neighbors.KDTree(sub).query(p, k=1, return_distance=False)[:, 0]
        diff = np.nonzero(got != want)[0]
        p64, s64 = p.astype(np.float64), sub.astype(np.float64)
        dg = ((p64[diff] - s64[got[diff]]) ** 2).sum(1)
        dw = ((p64[diff] - s64[want[diff]]) ** 2).sum(1)
        print("%s: %d of %d indices differ from the KDTree's" % (name, len(diff), len(p)))
        assert np.all(np.abs(dg - dw) <= dw * 2.0 ** -20)


def test_nearest_restatement_ties_to_lower_index():
    sub = np.array([[1, 0, 0], [-1, 0, 0], [0, 5, 0], [-1, 0, 0]], np.float32)
    assert list(grid_ref.nearest_sub_point(sub, np.array([[0, 0, 0], [-1, 0, 0], [0, 4, 0]], np.float32))) == [0, 1, 2]


def test_host_refusals(monkeypatch):
    """Wrong shapes, a grid_size that is not a positive finite number, mismatched N and CPU tensors are refused before any
    device call (the library is never asked: its call entry is replaced by one that fails the test)."""
    import torch
    from pointsecguard_amd import _lib
    from pointsecguard_amd.randla import grid
    from pointsecguard_amd.randla.helper_tool import DP

    def no_device(*a, **k):
        raise AssertionError("device call")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    p = np.zeros((8, 3), np.float32)
    for bad in (np.zeros((8, 2), np.float32), np.zeros(8, np.float32), np.zeros((0, 3), np.float32), np.zeros((2, 8, 3), np.float32)):
        with pytest.raises(ValueError):
            DP.grid_sub_sampling(bad, grid_size=0.1)
    for f, lab in ((np.zeros((7, 3)), None), (np.zeros(8), None), (None, np.zeros(7, np.int32)), (None, np.zeros((8, 1, 1), np.int32)),
                   (np.zeros((8, 0)), None)):
        with pytest.raises(ValueError):
            DP.grid_sub_sampling(p, f, lab, grid_size=0.1)
    for g in (0.0, -0.04, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            DP.grid_sub_sampling(p, grid_size=g)
    t = torch.zeros(8, 3)
    with pytest.raises(_lib.PsgError):
        grid.grid_sub_sampling_device(t, grid_size=0.1)
    with pytest.raises(_lib.PsgError):
        grid.nearest_sub_point(t, t, 0.1)
    with pytest.raises(_lib.PsgError):
        grid.grid_sub_sampling_device(p, grid_size=0.1)      # not a tensor at all
