"""Rooms and the numpy restatement of the plan tables for the packed SA forward (psg_pn2_kernels.cuh: sa_pack_plan_kernel,
sa_fwd_packed_kernel).  Shared by tests/test_sa_pack_host.py (CPU, the oracle's routines) and tests/test_gpu_sa_pack.py."""
import numpy as np

from pointsecguard_amd.synthetic import make_rooms, make_rooms_with_duplicates

SA_P = (128, 64, 32, 32)          # grouped rows per SA workgroup at SSG levels 0 - 3 (psg_pn2.hip: make_ssg)
GCAP = 16                         # groups per packed workgroup at most (SA_PACK_GCAP)
ROOM_KINDS = ("uniform", "structured", "duplicates", "shrunk", "clump")


def clump_rooms(batch, seed):
    """One dense clump (3721 points inside a 0.15 m sphere: every ball there is full) plus 375 points on a 0.2 m lattice, most
    of them alone in their 0.1 m ball: FPS interleaves the two, so groups of 1 lie next to groups of 32 and runs of either
    cross 32-row blocks and workgroups."""
    rng = np.random.default_rng(seed)
    gx, gy, gz = np.meshgrid(np.arange(5) * 0.2 - 0.4, np.arange(5) * 0.2 - 0.4, np.arange(15) * 0.2 + 0.1, indexing="ij")
    lattice = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(np.float32)
    rooms = np.empty((batch, 4096, 9), np.float32)
    for b in range(batch):
        n = 4096 - lattice.shape[0]
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts = np.array([0.1, 0.1, 1.5]) + d * (0.15 * rng.random((n, 1)) ** (1.0 / 3.0))
        xyz = np.concatenate([lattice, pts.astype(np.float32)], axis=0)
        room = np.concatenate([xyz, rng.random((4096, 6), dtype=np.float32)], axis=1).astype(np.float32)
        rooms[b] = room[rng.permutation(4096)]
    return rooms


def rooms_of(kind, batch, seed):
    if kind == "uniform":
        return make_rooms(batch, seed)
    if kind == "structured":
        return make_rooms(batch, seed, structured=True)
    if kind == "duplicates":
        return make_rooms_with_duplicates(batch, seed)
    if kind == "shrunk":            # every level-0 ball holds 64 x the points: all groups full, nothing to skip
        r = make_rooms(batch, seed)
        r[..., 0:3] *= np.float32(0.25)
        return r
    if kind == "clump":
        return clump_rooms(batch, seed)
    raise ValueError(kind)


def valid_counts(gidx, n_src):
    """cnt[s] of a group table [S][32]: the leading rows up to the first k > 0 that repeats member 0; an empty ball
    (member 0 = n_src) counts as 32."""
    gidx = np.asarray(gidx)
    rep = gidx[:, 1:] == gidx[:, :1]
    cnt = np.where(rep.any(axis=1), rep.argmax(axis=1) + 1, 32)
    return np.where(gidx[:, 0] >= n_src, 32, cnt).astype(np.int32)


def fits(rows, g, c, P):
    """may a group of c valid rows join a workgroup that holds g groups and `rows` rows"""
    return rows + c < P or (rows + c == P and rows == 32 * g and g + 1 == P // 32)


def descriptors(cnt, seg, P):
    """What a packed workgroup reads: {first group | groups << 16, cnt - 1 of its groups in five bits each, six to a word};
    all zero for the workgroups behind the last one in use."""
    out = np.zeros((len(cnt) // (P // 32), 4), np.int64)
    for i in range(int(seg[0])):
        lo, hi = int(seg[1 + i]), int(seg[2 + i])
        out[i, 0] = lo | ((hi - lo) << 16)
        for g in range(hi - lo):
            out[i, 1 + g // 6] |= (int(cnt[lo + g]) - 1) << (5 * (g % 6))
    return out.astype(np.int32)


def segmentation(cnt, P, gcap=GCAP):
    """Greedy workgroups over consecutive groups while the valid rows stay below P and within gcap groups; P rows only as
    P / 32 full groups.  The table {workgroups in use, first group of each, S}, zero-padded to S / (P / 32) + 2 entries."""
    S = len(cnt)
    firsts, s = [], 0
    while s < S:
        firsts.append(s)
        rows = g = 0
        while s < S and g < gcap and fits(rows, g, int(cnt[s]), P):
            rows += int(cnt[s])
            s += 1
            g += 1
    out = np.zeros(S // (P // 32) + 2, np.int32)
    out[0] = len(firsts)
    out[1:1 + len(firsts)] = firsts
    out[1 + len(firsts)] = S
    return out
