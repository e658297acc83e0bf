"""How the channel-ordered max-pool transpose of the packed SA backward (psg_pn2_kernels.cuh: sa_bwd_packed_chan) deals a
workgroup's groups to its waves, restated in numpy (tests/sa_poolt_order_ref.py) and checked on the CPU:

  rooms     over the packed workgroups of levels 1 - 3 of the rooms of tests/test_gpu_sa_poolt_order.py (those of
            tests/sa_pack_bwd_levels_rooms.py: both forwards of its plan, both rooms): every group lies in exactly one range,
            every range holds at most 32 rows, every live row is stored once at its packed row, and the shapes the GPU test
            counts on occur - a workgroup of one group, the cap of 16 groups with one-row groups among them (lattice,
            clusters: 16 groups of ONE row each do not occur at levels 1 - 3 of these rooms, that shape is among the extremes
            below), P - 1 rows, an unaligned workgroup of full groups, a group across a 32-row block; and (from the oracle's
            activations) valid rows that are the arg-max of no channel, the rows without an item;
  extremes  16 x 1 row, 2 x 32 rows, 1 + 31 + 32 rows, 63 rows in groups that force more ranges than slots;
  mutants   a dealing that drops a group, and one whose range overflows 32 rows, are caught by the same check."""
import numpy as np
import pytest

import sa_pack_bwd_levels_rooms as lr
import sa_pack_rooms as spr
import sa_poolt_order_ref as por

LEVELS = (1, 2, 3)


@pytest.fixture(scope="module")
def workgroups(oracle_net):
    """{(kind, level): [counts of the groups of a packed workgroup]} over the GPU test's rooms, forwards and levels"""
    out = {}
    for ki, kind in enumerate(lr.ROOM_KINDS):
        rooms, starts = lr.rooms_and_starts(ki, kind)
        for f in range(2):
            for b in range(lr.B):
                geom = oracle_net.geometry(rooms[b][:, 0:3], [int(starts[f, l, b]) for l in range(4)])
                for lvl in LEVELS:
                    cnt = spr.valid_counts(geom["group"][lvl], lr.N_SRC[lvl])
                    seg = spr.segmentation(cnt, spr.SA_P[lvl])
                    for i in range(int(seg[0])):
                        out.setdefault((kind, lvl), []).append((int(seg[1 + i]), np.asarray(cnt[int(seg[1 + i]):int(seg[2 + i])])))
    return out


def test_every_workgroup_of_the_rooms_is_dealt_whole(workgroups):
    seen = {"one_group": 0, "cap_with_one_row_groups": 0, "p_minus_1": 0, "unaligned_full": 0, "two_ranges_in_a_slot": 0, "across_block": 0}
    for (kind, lvl), wgs in workgroups.items():
        P, nr = spr.SA_P[lvl], por.slots(lvl)
        for first, c in wgs:
            assert 0 < len(c) <= spr.GCAP and c.sum() <= P
            ranges = por.deal(c, nr)
            por.check(c, ranges, nr)
            seen["one_group"] += len(c) == 1
            seen["cap_with_one_row_groups"] += len(c) == spr.GCAP and bool((c == 1).any())
            seen["p_minus_1"] += c.sum() == P - 1
            seen["unaligned_full"] += (c == 32).all() and len(c) == P // 32 and first % (P // 32) != 0
            seen["two_ranges_in_a_slot"] += len(ranges) > nr
            st = np.concatenate([[0], np.cumsum(c)])
            seen["across_block"] += bool(((st[:-1] // 32) != ((st[1:] - 1) // 32)).any())
    for k in ("one_group", "cap_with_one_row_groups", "p_minus_1", "unaligned_full", "across_block"):
        assert seen[k] > 0, (k, seen)           # (a changed room must not make the GPU test vacuous)


def test_valid_rows_without_an_item_occur(oracle_net):
    """a valid row that is the arg-max of no live channel of its group holds no item: the pass must still store it, as zeros"""
    rooms, starts = lr.rooms_and_starts(0, lr.ROOM_KINDS[0])
    geom = oracle_net.geometry(rooms[0][:, 0:3], [int(starts[0, l, 0]) for l in range(4)])
    _, cache = oracle_net.forward(rooms[0], geom)
    free = {}
    for lvl in LEVELS:
        cnt = spr.valid_counts(geom["group"][lvl], lr.N_SRC[lvl])
        acts, _ = cache["sa"][lvl]
        h = np.asarray(acts[-1]).reshape(lr.S_LVL[lvl], 32, -1)
        best, first = h.max(axis=1), h.argmax(axis=1)
        named = np.zeros((lr.S_LVL[lvl], 32), bool)
        g, c = np.nonzero(best > 0)
        named[g, first[g, c]] = True
        valid = np.arange(32)[None, :] < cnt[:, None]
        free[lvl] = int((valid & ~named).sum())
    assert free[1] > 0, free        # (level 1: 128 channels for up to 32 rows; the wider levels name nearly every row)


@pytest.mark.parametrize("lvl", LEVELS)
@pytest.mark.parametrize("cnt", [(1,) * 16, (32, 32), (1, 31, 32), (31,), (1,), (30, 1, 1, 1, 29, 1), (1, 1, 1, 1, 1, 1, 28, 29),
                                 (16, 15), (2,) * 15 + (1,)])
def test_extremes(lvl, cnt):
    c = np.asarray(cnt)
    nr = por.slots(lvl)     # (the dealing does not depend on P: rows past a level's workgroup size only add ranges)
    ranges = por.deal(c, nr)
    por.check(c, ranges, nr)
    if cnt == (1,) * 16:
        assert len(ranges) == nr and all(r[2] - r[1] == 16 // nr for r in ranges)      # balanced by groups
    if cnt == (1, 1, 1, 1, 1, 1, 28, 29) and nr == 4:
        assert len(ranges) == 5 and ranges[4][0] == 0                                  # slot 0 runs a second range


def test_a_dropped_group_is_caught():
    c = np.asarray((3, 4, 5, 6))
    ranges = por.deal(c, 4)
    with pytest.raises(AssertionError):
        por.check(c, ranges[:1] + ranges[2:], 4)
    mutant = [(s, ga, gb if gb != 2 else 1, row0, rows) for s, ga, gb, row0, rows in por.deal(c, 2)]
    with pytest.raises(AssertionError):
        por.check(c, mutant, 2)


def test_an_overflowing_range_is_caught():
    c = np.asarray((20, 20, 20))
    with pytest.raises(AssertionError, match="32 accumulators"):
        por.check(c, por.deal(c, 2, cap=64), 2)        # (per = 2 groups a range without the row cap: 40 rows)
    por.check(c, por.deal(c, 2), 2)
