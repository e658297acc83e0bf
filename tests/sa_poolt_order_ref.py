"""The numpy restatement of how the channel-ordered max-pool transpose of a packed SA backward workgroup deals its groups
(psg_pn2_kernels.cuh: sa_bwd_packed_chan).  Shared by tests/test_sa_poolt_order_host.py and tests/test_gpu_sa_poolt_order.py.

A workgroup's waves are (range slot) x (64-column slice of C2): NR = NW / SPV slots.  The groups are cut in order into ranges, a
new range after per = ceil(ng / NR) groups or where the next group would take the range past 32 rows (the 32 row accumulators of a
lane); range i goes to slot i % NR.  A range stores its rows [row0, row0 + rows) of the packed buffer, once."""
import numpy as np

NW = {1: 4, 2: 4, 3: 8}                 # waves of the SSG SA backward workgroups, levels 1 - 3
SPV = {1: 1, 2: 2, 3: 4}                # 64-column slices of C2 = 64 / 128 / 256
ROW_CAP = 32


def slots(lvl):
    return NW[lvl] // SPV[lvl]


def deal(cnt_wg, nr, per=None, cap=ROW_CAP):
    """ranges [(slot, first group, end group, first packed row, rows)] of a workgroup whose groups hold cnt_wg rows"""
    ng = len(cnt_wg)
    if per is None:
        per = (ng + nr - 1) // nr
    out = []
    ga = row0 = rows = 0
    for i in range(ng + 1):
        cnt = int(cnt_wg[i]) if i < ng else 0
        if i > ga and (i == ng or i - ga == per or rows + cnt > cap):
            out.append((len(out) % nr, ga, i, row0, rows))
            row0 += rows
            rows = 0
            ga = i
        rows += cnt
    return out


def check(cnt_wg, ranges, nr):
    """what the kernel relies on: every group in exactly one range, in order; at most 32 rows a range; every live row of the
    workgroup stored exactly once, at the packed row the forward gave it; slots dealt round-robin"""
    ng = len(cnt_wg)
    gstart = np.concatenate([[0], np.cumsum(cnt_wg)]).astype(np.int64)
    owner = np.zeros(ng, np.int64)
    stored = np.zeros(int(gstart[-1]), np.int64)
    for i, (slot, ga, gb, row0, rows) in enumerate(ranges):
        assert 0 <= ga < gb <= ng and slot == i % nr
        assert 0 < rows <= ROW_CAP, "a range of %d rows does not fit a lane's 32 accumulators" % rows
        assert row0 == gstart[ga] and rows == gstart[gb] - gstart[ga]
        owner[ga:gb] += 1
        stored[row0:row0 + rows] += 1
    assert (owner == 1).all(), "a group in no range or in two"
    assert (stored == 1).all(), "a live row stored never or twice"
