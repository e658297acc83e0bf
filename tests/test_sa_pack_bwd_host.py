"""What the packed SA backward (psg_pn2_kernels.cuh: sa_bwd_packed_kernel) relies on, and what its rooms are built to hold,
stated with the ORACLE's own routines (CPU, no GPU):

  rooms     lattice: every level-0 group has one valid row, and every packed workgroup holds the cap of 16 groups in one block;
            clusters (the seed and FPS start tests/test_gpu_sa_pack_bwd.py uses): a level-0 group's valid rows are its cluster's
            size capped at 32, and the level-0 segmentation holds a workgroup of exactly P - 1 rows, an aligned and an unaligned
            workgroup of P / 32 full groups, and a group whose rows cross a 32-row block;
  backward  in every room kind and at every level the oracle's grouped-input gradient is exactly zero on every row at or behind
            cnt[s], and no arg-max index of a channel that gets gradient points there: the rows the packed backward does not run
            are rows whose result is zero and is never stored."""
import numpy as np
import pytest

import sa_pack_bwd_rooms as sbr
import sa_pack_rooms as spr
from oracle import pn2

N_SRC = (4096, 1024, 256, 64)


def _geometry(oracle_net, kind, start0):
    room = sbr.rooms_of(kind, 1, 1000)[0]
    rng = np.random.default_rng(17)
    starts = [int(rng.integers(0, n)) for n in N_SRC]
    if start0 is not None:
        starts[0] = start0
    return room, oracle_net.geometry(room[:, 0:3], starts)


def test_lattice_groups_hold_one_row_and_workgroups_the_cap(oracle_net):
    _, geom = _geometry(oracle_net, "lattice", None)
    cnt = spr.valid_counts(geom["group"][0], 4096)
    assert (cnt == 1).all()
    seg = spr.segmentation(cnt, spr.SA_P[0])
    n = int(seg[0])
    assert n == 1024 // spr.GCAP and np.array_equal(seg[1:2 + n], np.arange(n + 1) * spr.GCAP)


def test_clusters_hold_the_workgroup_shapes(oracle_net):
    room, geom = _geometry(oracle_net, "clusters", sbr.CLUSTERS_START0)
    g = np.asarray(geom["group"][0])
    cnt = spr.valid_counts(g, 4096)
    # a group is its centroid's cluster: the points closer than 0.1 m, capped at 32
    xyz = room[:, 0:3].astype(np.float64)
    size = (np.linalg.norm(xyz[g[:, 0]][:, None, :] - xyz[None, :, :], axis=2) < 0.1).sum(axis=1)
    assert set(np.unique(size)) <= set(sbr.CLUSTER_SIZES)
    assert np.array_equal(cnt, np.minimum(size, 32))
    assert set(np.unique(cnt)) == {1, 2, 31, 32}
    found = sbr.level0_premises(cnt, spr.SA_P[0])
    assert all(found.values()), found


@pytest.mark.parametrize("kind", sbr.ROOM_KINDS)
def test_rows_behind_the_valid_ones_get_no_gradient(oracle_net, kind):
    room, geom = _geometry(oracle_net, kind, sbr.CLUSTERS_START0 if kind == "clusters" else None)
    _, cache = oracle_net.forward(room, geom)
    rng = np.random.default_rng(3)
    L = pn2.lib()
    for lvl in range(4):
        g = np.asarray(geom["group"][lvl])
        S = g.shape[0]
        cnt = spr.valid_counts(g, N_SRC[lvl])
        acts, arg = cache["sa"][lvl]
        out = cache["sa_out"][lvl + 1]
        arg = np.asarray(arg)
        assert (arg[out > 0] < np.broadcast_to(cnt[:, None], arg.shape)[out > 0]).all(), (kind, lvl, "an arg-max behind cnt")
        c = out.shape[1]
        dfeat = rng.standard_normal((S, c)).astype(np.float32)
        dh = np.empty((S * 32, c), np.float32)
        L.orc_maxpool_bwd(pn2._fp(dfeat), pn2._ip(arg), S, 32, c, pn2._fp(dh))
        pad = (np.arange(32)[None, :] >= cnt[:, None]).ravel()
        assert not dh[pad].any(), (kind, lvl, "the pool's transpose reaches a row behind cnt")
        drows = oracle_net._mlp_bwd("sa%d" % (lvl + 1), acts, dh)
        assert not drows[pad].any(), (kind, lvl)
        assert drows[~pad].any()
