"""What the packed SA backward of SSG levels 1 - 3 (psg_pn2_kernels.cuh: sa_bwd_packed_kernel with SPV > 0) relies on, and what
the rooms of tests/test_gpu_sa_pack_bwd_levels.py are meant to hold, stated with the ORACLE's own routines (CPU, no GPU):

  rooms     with the GPU test's seeds and starts (both forwards of its plan, both rooms), the level 1 - 3 segmentations hold
            a workgroup at the cap of 16 groups (level 1: clump, lattice, clusters), a workgroup of exactly P - 1 rows at all
            three levels, a group across a 32-row block (level 1), aligned workgroups of full groups (shrunk: every workgroup at
            all three levels; clump: level 1, next to packed ones), surplus workgroups in every kind but shrunk, and (twofull,
            room 0, forward 0) an unaligned workgroup of two full groups at level 1;
  arg-max   computed in numpy from the oracle's grouped activations: the first sample that attains a positive maximum of a
            (group, channel) lies below the group's count - the sparse stream never names a row the packed kernel skips;
  schedule  the numpy restatement of the batch schedule (sa_pack_bwd_levels_rooms.batch_schedule) sends every valid row to
            exactly one packed row, in row order, from the batch that owns its group, and zero-fills exactly the tail."""
import numpy as np
import pytest

import sa_pack_bwd_levels_rooms as lr
import sa_pack_rooms as spr

LEVELS = (1, 2, 3)


@pytest.fixture(scope="module")
def geometries(oracle_net):
    """per room kind: [(forward, room, geometry)] over the two forwards of the GPU test's plan and its two rooms"""
    out = {}
    for ki, kind in enumerate(lr.ROOM_KINDS):
        rooms, starts = lr.rooms_and_starts(ki, kind)
        out[kind] = [(f, b, rooms[b], oracle_net.geometry(rooms[b][:, 0:3], [int(starts[f, l, b]) for l in range(4)]))
                     for f in range(2) for b in range(lr.B)]
    return out


def _found(geometries, kind, lvl, only=None):
    res = []
    for f, b, _, geom in geometries[kind]:
        if only is None or (f, b) == only:
            res.append(lr.premises(spr.valid_counts(geom["group"][lvl], lr.N_SRC[lvl]), spr.SA_P[lvl]))
    return res


def test_workgroup_shapes_of_levels_1_to_3(geometries):
    for kind in ("clump", "lattice", "clusters"):
        assert max(p["cap"] for p in _found(geometries, kind, 1)) == spr.GCAP, kind
    assert max(p["cap"] for kind in lr.ROOM_KINDS for p in _found(geometries, kind, 2)) >= 8
    assert max(p["cap"] for kind in lr.ROOM_KINDS for p in _found(geometries, kind, 3)) >= 6
    for lvl in LEVELS:
        assert any(p["p_minus_1"] for kind in lr.ROOM_KINDS for p in _found(geometries, kind, lvl)), lvl
    assert any(p["crosses_block"] for kind in lr.ROOM_KINDS for p in _found(geometries, kind, 1))
    for lvl in LEVELS:
        gx = lr.S_LVL[lvl] // (spr.SA_P[lvl] // 32)
        for p in _found(geometries, "shrunk", lvl):       # nothing to skip: every workgroup aligned and full
            assert p["used"] == gx and p["full_aligned"] and not p["full_unaligned"] and not p["p_minus_1"], (lvl, p)
        for kind in lr.ROOM_KINDS:
            if kind != "shrunk":
                assert all(0 < p["used"] < gx for p in _found(geometries, kind, lvl)), (kind, lvl)
    clump = _found(geometries, "clump", 1)
    assert any(p["full_aligned"] for p in clump), clump    # (next to packed ones: used < gx above)


def test_twofull_holds_an_unaligned_workgroup_of_two_full_groups(geometries):
    (p,) = _found(geometries, "twofull", 1, only=(0, 0))
    assert p["full_unaligned"], p


@pytest.mark.parametrize("kind", lr.ROOM_KINDS)
def test_arg_max_lies_below_the_count(oracle_net, geometries, kind):
    _, _, room, geom = geometries[kind][0]
    _, cache = oracle_net.forward(room, geom)
    for lvl in LEVELS:
        cnt = spr.valid_counts(geom["group"][lvl], lr.N_SRC[lvl])
        acts, _ = cache["sa"][lvl]
        h = np.asarray(acts[-1]).reshape(lr.S_LVL[lvl], 32, -1)
        best, first = h.max(axis=1), h.argmax(axis=1)            # (argmax: the first sample that attains it)
        live = best > 0
        assert live.any()
        assert (first[live] < np.broadcast_to(cnt[:, None], first.shape)[live]).all(), (kind, lvl)


@pytest.mark.parametrize("kind", lr.ROOM_KINDS)
def test_batch_schedule_places_every_valid_row_once(geometries, kind):
    for f, b, _, geom in geometries[kind]:
        for lvl in LEVELS:
            P = spr.SA_P[lvl]
            cnt = spr.valid_counts(geom["group"][lvl], lr.N_SRC[lvl])
            seg = spr.segmentation(cnt, P)
            for i in range(int(seg[0])):
                c = cnt[int(seg[1 + i]):int(seg[2 + i])]
                nrows = int(c.sum())
                assert nrows <= P and len(c) <= spr.GCAP
                dest, owner, tail = lr.batch_schedule(c, P)
                assert np.array_equal(owner, np.arange(len(c)) // (P // 32))
                valid = np.arange(32)[None, :] < c[:, None]
                assert (dest[~valid] == -1).all()
                assert np.array_equal(dest[valid], np.arange(nrows))     # each packed row once, group by group in row order
                assert np.array_equal(np.sort(np.concatenate([dest[valid], tail])), np.arange((nrows + 31) // 32 * 32))
