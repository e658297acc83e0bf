"""Rooms, starts and the numpy restatement of the batch schedule for the packed SA backward of SSG levels 1 - 3
(psg_pn2_kernels.cuh: sa_bwd_packed_kernel with SPV > 0, sa_bwd_packed_sparse).  Shared by tests/test_sa_pack_bwd_levels_host.py
(CPU, the oracle's routines) and tests/test_gpu_sa_pack_bwd_levels.py.

The room kinds are the seven of tests/sa_pack_bwd_rooms.py with that test's seeds and starts, and one more, "twofull": a clump room
whose level-1 segmentation (FPS of levels 0 and 1 begun at point 0) holds an UNALIGNED workgroup of two full groups - the one
level-1 shape (64 rows in two blocks on the packed path, no padding row) the seven are not built to hold."""
import numpy as np

import sa_pack_bwd_rooms as sbr
import sa_pack_rooms as spr

ROOM_KINDS = sbr.ROOM_KINDS + ("twofull",)
TWOFULL_SEED = 3000                 # found by a search over clump_rooms seeds from 3000 on and level-1 starts 0 - 7: the first hit
TWOFULL_STARTS = (0, 0)             # FPS starts of levels 0 and 1 of room 0, forward 0
B, N, ITERS = 2, 4096, 3
N_SRC = (4096, 1024, 256, 64)
S_LVL = (1024, 256, 64, 16)


def rooms_of(kind, batch, seed):
    if kind == "twofull":
        return spr.clump_rooms(batch, TWOFULL_SEED)
    return sbr.rooms_of(kind, batch, seed)


def rooms_and_starts(ki, kind):
    """the rooms [B][N][9] and FPS starts [ITERS][4][B] of room kind number ki, as both tests use them"""
    rooms = rooms_of(kind, B, 1000 + ki)
    rng = np.random.default_rng(50 + ki)
    starts = np.stack([rng.integers(0, n, (ITERS, B)) for n in N_SRC], axis=1).astype(np.int32)
    if kind == "clusters":
        starts[0, 0, 0] = sbr.CLUSTERS_START0
    if kind == "twofull":
        starts[0, 0:2, 0] = TWOFULL_STARTS
    return rooms, starts


def premises(cnt, P):
    """level0_premises of tests/sa_pack_bwd_rooms.py at any level, plus the most groups in a workgroup and the workgroups in use"""
    found = sbr.level0_premises(cnt, P)
    seg = spr.segmentation(cnt, P)
    n = int(seg[0])
    found["cap"] = int(np.diff(seg[1:2 + n]).max())
    found["used"] = n
    return found


def batch_schedule(cnt_wg, P):
    """What sa_bwd_packed_sparse does with a packed workgroup whose groups hold cnt_wg valid rows: the groups pass through the
    sparse stream in batches of G = P / 32; row k of group g lands in packed row gstart[g] + k where k < cnt_wg[g] and is not
    written otherwise; the tail of the last 32-row block is zero-filled once.  Returns (dest [ng][32] packed row or -1,
    owner [ng] batch of a group, tail rows zero-filled)."""
    G = P // 32
    ng = len(cnt_wg)
    gstart = np.concatenate([[0], np.cumsum(cnt_wg)]).astype(np.int64)
    nrows = int(gstart[-1])
    dest = np.full((ng, 32), -1, np.int64)
    owner = np.empty(ng, np.int64)
    for g0 in range(0, ng, G):                      # one batch
        for g in range(g0, min(g0 + G, ng)):
            owner[g] = g0 // G
            k = np.arange(32)
            dest[g] = np.where(k < cnt_wg[g], gstart[g] + k, -1)
    tail = np.arange(nrows, (nrows + 31) // 32 * 32)
    return dest, owner, tail
