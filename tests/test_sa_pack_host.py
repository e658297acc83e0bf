"""What the packed SA forward (psg_pn2_kernels.cuh: sa_fwd_packed_kernel) relies on, stated with the ORACLE's own routines
(CPU, no GPU), on every room of tests/test_gpu_sa_pack.py:

  premise   the valid rows of a group are its LEADING rows and there is at least one: rows k >= cnt repeat member 0, rows
            0 < k < cnt do not (query_ball_point, pointnet_util.py:104-106);
  forward   a padding row's activations are bit-for-bit those of row 0 of its group, in every layer;
  pool      the maximum over the valid rows alone, and the lowest row that attains it, are the oracle's pooled value and arg-max;
  backward  the grouped-input gradient rows of the padding rows are exactly zero.

Plus the greedy workgroup segmentation's invariants (sa_pack_rooms.segmentation, the numpy restatement of sa_pack_plan_kernel)."""
import numpy as np
import pytest

import sa_pack_rooms as spr
from oracle import pn2


@pytest.fixture(scope="module", params=spr.ROOM_KINDS)
def room_run(request, oracle_net):
    kind = request.param
    room = spr.rooms_of(kind, 1, 1000)[0]
    rng = np.random.default_rng(17)
    starts = [int(rng.integers(0, n)) for n in (4096, 1024, 256, 64)]
    geom = oracle_net.geometry(room[:, 0:3], starts)
    _, cache = oracle_net.forward(room, geom)
    return kind, geom, cache


def test_valid_rows_lead_and_groups_are_not_empty(room_run):
    kind, geom, _ = room_run
    n_src = (4096, 1024, 256, 64)
    for lvl in range(4):
        g = np.asarray(geom["group"][lvl])
        cnt = spr.valid_counts(g, n_src[lvl])
        assert cnt.min() >= 1 and cnt.max() <= 32
        assert (g[:, 0] < n_src[lvl]).all(), "no empty ball in these rooms"
        k = np.arange(32)[None, :]
        pad = k >= cnt[:, None]
        same = g == g[:, :1]
        assert (same[pad]).all(), (kind, lvl, "a row behind the valid ones is not a copy of member 0")
        assert not same[(k > 0) & ~pad].any(), (kind, lvl, "a copy of member 0 among the leading rows")
    if kind == "shrunk":
        assert (spr.valid_counts(geom["group"][0], 4096) == 32).all(), "every level-0 ball of the shrunk room is full"
    if kind == "clump":
        c0 = spr.valid_counts(geom["group"][0], 4096)
        d = np.abs(np.diff(c0))
        assert (c0 == 1).sum() > 50 and (c0 == 32).sum() > 50 and (d == 31).sum() >= 4, "groups of 1 next to groups of 32"


def test_padding_rows_copy_row0_and_pool_over_valid_rows_is_the_oracle(room_run, oracle_net):
    kind, geom, cache = room_run
    n_src = (4096, 1024, 256, 64)
    rng = np.random.default_rng(3)
    L = pn2.lib()
    for lvl in range(4):
        g = np.asarray(geom["group"][lvl])
        S = g.shape[0]
        cnt = spr.valid_counts(g, n_src[lvl])
        acts, arg = cache["sa"][lvl]
        pad = (np.arange(32)[None, :] >= cnt[:, None]).ravel()
        for a in acts:
            rows = a.reshape(S, 32, -1)
            row0 = np.broadcast_to(rows[:, :1], rows.shape).reshape(S * 32, -1)
            assert np.array_equal(a.view(np.uint32)[pad], np.ascontiguousarray(row0).view(np.uint32)[pad]), (kind, lvl)
        z = acts[-1].reshape(S, 32, -1)
        valid = np.arange(32)[None, :, None] < cnt[:, None, None]
        zv = np.where(valid, z, -np.inf)
        out = zv.max(axis=1)
        am = zv.argmax(axis=1)                                    # first = lowest row that attains the maximum
        ref_out = cache["sa_out"][lvl + 1]
        assert np.array_equal(out.astype(np.float32).view(np.uint32), ref_out.view(np.uint32)), (kind, lvl)
        pos = ref_out > 0
        assert np.array_equal(am[pos], np.asarray(arg)[pos]), (kind, lvl)
        assert (am < cnt[:, None]).all()
        # backward: the oracle's max-pool transpose and MLP backward leave the padding rows exactly zero
        c = ref_out.shape[1]
        dfeat = rng.standard_normal((S, c)).astype(np.float32)
        dh = np.empty((S * 32, c), np.float32)
        L.orc_maxpool_bwd(pn2._fp(dfeat), pn2._ip(arg), S, 32, c, pn2._fp(dh))
        drows = oracle_net._mlp_bwd("sa%d" % (lvl + 1), acts, dh)
        assert not drows[pad].any(), (kind, lvl)
        assert drows[~pad].any()


def test_segmentation_invariants(room_run):
    kind, geom, _ = room_run
    n_src = (4096, 1024, 256, 64)
    for lvl in range(4):
        P = spr.SA_P[lvl]
        cnt = spr.valid_counts(geom["group"][lvl], n_src[lvl])
        S = len(cnt)
        seg = spr.segmentation(cnt, P)
        n = int(seg[0])
        firsts = seg[1:2 + n]
        assert 1 <= n <= S // (P // 32), "the unpacked grid is the worst case"
        assert firsts[0] == 0 and firsts[-1] == S and (np.diff(firsts) > 0).all()
        for i in range(n):
            lo, hi = int(firsts[i]), int(firsts[i + 1])
            rows = int(cnt[lo:hi].sum())
            assert hi - lo <= spr.GCAP
            assert rows < P or (rows == P and hi - lo == P // 32 and (cnt[lo:hi] == 32).all()), "P rows only as full groups"
            if i + 1 < n:                                         # closed because the next group did not fit
                assert hi - lo >= P // 32
                assert hi - lo == spr.GCAP or not spr.fits(rows, hi - lo, int(cnt[hi]), P)
        if kind == "shrunk" and lvl == 0:
            assert n == S // (P // 32) and np.array_equal(firsts, np.arange(n + 1) * (P // 32)), "segmentation equals the unpacked one"
