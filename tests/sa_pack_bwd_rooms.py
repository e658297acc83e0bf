"""Rooms for the packed SA backward (psg_pn2_kernels.cuh: sa_bwd_packed_kernel): the five kinds of tests/sa_pack_rooms.py and two
more, built so that the level-0 segmentation holds the workgroup shapes the packed backward treats differently.  Shared by
tests/test_sa_pack_bwd_host.py (CPU, the oracle's routines: it states the premises below and fails if the seed loses one) and
tests/test_gpu_sa_pack_bwd.py."""
import numpy as np

import sa_pack_rooms as spr

ROOM_KINDS = spr.ROOM_KINDS + ("lattice", "clusters")
CLUSTER_SIZES = (1, 2, 31, 32, 40)
# room 0 of clusters_rooms(., CLUSTERS_SEED) with its level-0 FPS begun at point CLUSTERS_START0: the level-0 segmentation holds a
# workgroup of exactly P - 1 rows, an aligned and an unaligned workgroup of P / 32 full groups, and a group whose rows cross a
# 32-row block (tests/test_sa_pack_bwd_host.py)
CLUSTERS_SEED = 2017
CLUSTERS_START0 = 0


def lattice_rooms(batch, seed):
    """4096 points on a 16 x 16 x 16 lattice of 0.12 m (each moved by less than 0.005 m, so that no two distances tie): every
    point is alone in its 0.1 m ball, every level-0 group has one valid row, and a packed workgroup holds the cap of 16 groups
    in one 32-row block."""
    rng = np.random.default_rng(seed)
    g = np.arange(16) * 0.12
    gx, gy, gz = np.meshgrid(g - 0.9, g - 0.9, g + 0.1, indexing="ij")
    lattice = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    rooms = np.empty((batch, 4096, 9), np.float32)
    for b in range(batch):
        xyz = lattice + (rng.random((4096, 3)) - 0.5) * 0.009
        room = np.concatenate([xyz, rng.random((4096, 6))], axis=1).astype(np.float32)
        rooms[b] = room[rng.permutation(4096)]
    return rooms


def cluster_sizes(rng):
    """sizes from CLUSTER_SIZES that add up to 4096"""
    sizes, left = [], 4096
    while left >= 40:
        sizes.append(int(rng.choice(CLUSTER_SIZES)))
        left -= sizes[-1]
    for c in (32, 31, 2, 1):
        while left >= c:
            sizes.append(c)
            left -= c
    return sizes


def clusters_rooms(batch, seed):
    """Tight clusters (inside a 0.02 m cube: well inside a 0.1 m ball) on a 0.3 m lattice, sizes from CLUSTER_SIZES: the ball of
    a level-0 centroid holds exactly its cluster, so a group's valid rows are its cluster's size, capped at 32."""
    rng = np.random.default_rng(seed)
    g = np.arange(7) * 0.3
    gx, gy, gz = np.meshgrid(g - 0.9, g - 0.9, g + 0.1, indexing="ij")
    sites = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)          # 343 sites, about 195 clusters
    rooms = np.empty((batch, 4096, 9), np.float32)
    for b in range(batch):
        sizes = cluster_sizes(rng)
        centre = sites[rng.permutation(len(sites))[:len(sizes)]]
        xyz = np.repeat(centre, sizes, axis=0) + (rng.random((4096, 3)) - 0.5) * 0.02
        room = np.concatenate([xyz, rng.random((4096, 6))], axis=1).astype(np.float32)
        rooms[b] = room[rng.permutation(4096)]
    return rooms


def rooms_of(kind, batch, seed):
    if kind == "lattice":
        return lattice_rooms(batch, seed)
    if kind == "clusters":
        return clusters_rooms(batch, CLUSTERS_SEED)
    return spr.rooms_of(kind, batch, seed)


def level0_premises(cnt, P=128):
    """Which of the workgroup shapes the packed backward distinguishes occur in the segmentation of the counts cnt [S]."""
    seg = spr.segmentation(cnt, P)
    n = int(seg[0])
    firsts = seg[1:2 + n]
    found = {"p_minus_1": False, "full_aligned": False, "full_unaligned": False, "crosses_block": False}
    for i in range(n):
        lo, hi = int(firsts[i]), int(firsts[i + 1])
        c = cnt[lo:hi]
        rows = int(c.sum())
        if rows == P - 1:
            found["p_minus_1"] = True
        if rows == P:
            found["full_aligned" if lo % (P // 32) == 0 else "full_unaligned"] = True
        st = np.concatenate([[0], np.cumsum(c)])
        if rows < P and ((st[:-1] // 32) != ((st[1:] - 1) // 32)).any():
            found["crosses_block"] = True
    return found
