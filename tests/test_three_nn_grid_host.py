"""The grid 3-NN's walk and stop rule (three_nn_grid_kernel, psg_geometry.hip), restated in numpy float32
(tests/three_nn_grid_ref.py), return what the plain scan returns on every shared input - and three mutants of the walk do
not: the inputs are able to tell a wrong stop rule, a missing error term and a missing tie rule from the real thing.

The distances come from the oracle's square_distance (the kernels' expansion, with its fused multiply-adds)."""
import numpy as np
import pytest

import three_nn_grid_ref as R


@pytest.fixture(scope="module")
def inputs():
    from oracle import pn2
    out = {}
    with np.errstate(all="ignore"):
        for name, (fine, coarse) in R.cases().items():
            d = pn2.square_distance(fine, coarse)
            out[name] = (fine, coarse, d, R.scan_three_nn(d))
    return out


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def mutant_fails_on(inputs, **kw):
    with np.errstate(all="ignore"):
        return [n for n, (fine, coarse, d, want) in inputs.items() if not same(R.grid_three_nn(fine, coarse, d, **kw)[:2], want)]


def test_numpy_scan_is_the_oracle_scan(inputs):
    from oracle import pn2
    for name, (fine, coarse, d, want) in inputs.items():
        with np.errstate(all="ignore"):
            oi, _ = pn2.three_nn(fine, coarse)
        assert np.array_equal(want[0], oi), name


def test_walk_equals_scan(inputs):
    stats = {}
    with np.errstate(all="ignore"):
        for name, (fine, coarse, d, want) in inputs.items():
            idx, dist, visited, shells = R.grid_three_nn(fine, coarse, d)
            assert same((idx, dist), want), (name, np.nonzero((idx != want[0]).any(1))[0][:8])
            stats[name] = (visited.mean(), visited.max(), shells.max())
    print({k: "%.1f / %d candidates, %d shells" % v for k, v in stats.items()})
    assert stats["offset"][2] > 1                       # the error term widened the walk ..
    assert stats["one_cell_far"][1] == 64               # .. the longest walk reached every point ..
    assert stats["inf_coarse"][2] == 0 and stats["min"][1] == 3      # .. and a non-finite cloud is the scan (no grid)


def test_kernel_schedule_equals_scan(inputs):
    """Queries in cell order, 64 to a wave, the wave's box before a lane's own walk - the form the kernel runs."""
    with np.errstate(all="ignore"):
        for name, (fine, coarse, d, want) in inputs.items():
            idx, dist, visited, shells = R.grid_three_nn(fine, coarse, d, waves=True)
            assert same((idx, dist), want), (name, np.nonzero((idx != want[0]).any(1))[0][:8])
    assert mutant_fails_on(inputs, waves=True, zero_err=True) and mutant_fails_on(inputs, waves=True, d_only=True, order=lambda m: m[::-1])


def test_lattice_tie_is_a_tie_across_the_first_block(inputs):
    fine, coarse, d, (idx, dist) = inputs["lattice_tie"]
    block = R.lattice_tie_case()[2]
    assert not block[0] and d[0, 0] == dist[0, 2] and 0 in idx[0]              # point 0: outside the block, ties the third best, is taken
    assert ((d[0] == dist[0, 2]) & block).any()                                # a point inside the block has the same distance


def test_walk_order_does_not_matter(inputs):
    """The kernel's order inside a cell is whatever the counting sort's atomics gave: reversed and shuffled runs."""
    rng = np.random.default_rng(1)
    with np.errstate(all="ignore"):
        for name in ("identical", "cube", "lattice_tie", "dense_offset"):
            fine, coarse, d, want = inputs[name]
            for order in (lambda m: m[::-1], rng.permutation):
                assert same(R.grid_three_nn(fine, coarse, d, order=order)[:2], want), name


def test_mutants_are_told_apart(inputs):
    failed = {"zero_err": mutant_fails_on(inputs, zero_err=True), "d_only": mutant_fails_on(inputs, d_only=True, order=lambda m: m[::-1]),
              "stop_ge": mutant_fails_on(inputs, stop_ge=True)}
    print("mutants fail on:", failed)
    assert "dense_offset" in failed["zero_err"] or "offset" in failed["zero_err"]
    assert "cube" in failed["d_only"] and "identical" in failed["d_only"]
    # `>=` in the stop rule: NOT told apart by any input, and not counted.  It differs from `>` only when L^2 - err equals
    # the third-best d exactly AND an unvisited point computes that same d with a lower j; err is three times the
    # expansion's real rounding bound, so a point at least L away never computes a d as low as L^2 - err.  The strict `>`
    # is kept because it needs no such margin to be right.
    assert failed["stop_ge"] == []
