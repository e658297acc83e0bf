"""Farthest-point sampling, host side: the oracle (oracle.pn2.fps) and the numpy restatement of the kernel's documented rule
(tests/fps_step_ref.py) make the expected lowest-index choices on the tie clouds that tests/test_gpu_fps_step.py runs on the
device, agree with each other on every cloud of that file, and return index 0 once every key is 0."""
import numpy as np
import pytest

import fps_step_ref as ref


def both(xyz, s, start):
    from oracle import pn2
    a = pn2.fps(xyz, s, start)
    b = ref.fps_rule(xyz, s, start)
    assert a.dtype == np.int32 and np.array_equal(a, b)
    return a


def test_lattice_picks_are_the_lowest_index_of_their_position_then_zero():
    (_, xyz, s, start), = [c for c in ref.tie_cases() if c[0] == "lattice_256"]
    for p in range(xyz.shape[0]):
        distinct = len({tuple(r) for r in xyz[p]})
        assert distinct < 80
        idx = both(xyz[p], 80, start[p])
        assert np.array_equal(idx[:s], both(xyz[p], s, start[p]))
        for i in idx[1:]:
            assert not (xyz[p, :i] == xyz[p, i]).all(axis=1).any(), i       # no equal point below the pick
        assert len(set(idx[:distinct].tolist())) == distinct               # every position once ..
        assert (idx[distinct:] == 0).all() and idx[distinct:].size > 0      # .. then every key is 0: index 0


def test_twins_resolve_to_the_lower_twin_and_the_lower_half():
    (_, xyz, s, start), = [c for c in ref.tie_cases() if c[0] == "twins_4096_p256"]
    n = xyz.shape[1]
    assert np.array_equal(xyz[:, 1::16], xyz[:, 0::16]) and np.array_equal(xyz[:, n // 2:], xyz[:, :n // 2])
    for p in (0, 1, 100, 255):
        idx = both(xyz[p], s, start[p])
        assert idx[0] == start[p]
        assert (idx[1:] < n // 2).all() and (idx[1:] % 16 != 1).all()


def test_all_points_taken_then_index_zero():
    xyz, start = ref.uniform(1, 37, 3)
    idx = both(xyz[0], 37, start[0])
    assert sorted(idx.tolist()) == list(range(37))                          # S = N: a permutation
    dup = np.concatenate([xyz[0], xyz[0][:5]])                              # 42 points, 37 positions
    idx = both(dup, 42, 40)
    assert idx[0] == 40 and (idx[37:] == 0).all()


@pytest.mark.parametrize("case", ref.path_cases()[:7] + ref.edge_cases(), ids=lambda c: c[0])
def test_oracle_equals_the_rule(case):
    _, xyz, s, start = case
    both(xyz[0], s, start[0])


def test_non_finite_rule_never_updates_from_nan_or_inf():
    xyz, start = ref.non_finite(9)
    for p in range(2):
        idx = ref.fps_rule(xyz[p], 16, start[p])
        # the NaN point's and the inf point's distances stay at 1e10 (d < dist is false for them): the lower one is picked
        # at step 1, its NaN distances update nothing, and it is picked again for good
        assert idx[0] == start[p] and (idx[1:] == 77).all()
