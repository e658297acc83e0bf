#!/usr/bin/env python3
"""How many grouped rows of the SSG set-abstraction levels are padding (CPU, the oracle's FPS and ball query).

query_ball_point fills a group of 32 with copies of its first member; the packed SA forward (psg_pn2_kernels.cuh:
sa_fwd_packed_kernel) runs the valid rows only.  Per level this prints the valid rows per group (mean / max / share of full
groups) and the share of 32-row blocks left after the plan's greedy segmentation (tests/sa_pack_rooms.py: segmentation).

usage: tools/sa_pad_count.py [ROOMS.npy | --seed N [--structured]] [--rooms R]
ROOMS.npy holds float32 [R][4096][9] point-major rooms; without it, synthetic.make_rooms(R, seed)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sa_pack_rooms as spr               # noqa: E402
from oracle import pn2                    # noqa: E402
from pointsecguard_amd.synthetic import make_rooms   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rooms_file", nargs="?")
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--structured", action="store_true")
    ap.add_argument("--rooms", type=int, default=2)
    a = ap.parse_args()
    rooms = np.load(a.rooms_file)[:a.rooms] if a.rooms_file else make_rooms(a.rooms, a.seed, structured=a.structured)
    rng = np.random.default_rng(a.seed)
    n_src = (4096, 1024, 256, 64)
    stat = [[] for _ in range(4)]
    for room in rooms:
        xyz = np.ascontiguousarray(room[:, 0:3], np.float32)
        for lvl, (npoint, radius, nsample) in enumerate(pn2.SA_CFG):
            new_xyz = np.ascontiguousarray(xyz[pn2.fps(xyz, npoint, int(rng.integers(0, n_src[lvl])))])
            cnt = spr.valid_counts(pn2.ball_query(radius, nsample, xyz, new_xyz), n_src[lvl])
            seg = spr.segmentation(cnt, spr.SA_P[lvl])
            firsts = seg[1:2 + int(seg[0])]
            blocks = sum((int(cnt[lo:hi].sum()) + 31) // 32 for lo, hi in zip(firsts[:-1], firsts[1:]))
            stat[lvl].append((cnt.mean(), cnt.max(), (cnt == 32).mean(), blocks / npoint, int(seg[0]) / (npoint // (spr.SA_P[lvl] // 32))))
            xyz = new_xyz
    print("level groups  valid rows/group: mean  max  full   32-row blocks kept   workgroups in use")
    for lvl in range(4):
        s = np.array(stat[lvl])
        print("%5d %6d %22.1f %4d %5.0f%% %20.2f %19.2f" % (lvl, pn2.SA_CFG[lvl][0], s[:, 0].mean(), s[:, 1].max(),
                                                        100 * s[:, 2].mean(), s[:, 3].mean(), s[:, 4].mean()))


if __name__ == "__main__":
    main()
