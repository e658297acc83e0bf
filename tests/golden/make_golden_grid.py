"""Generate tests/golden/grid_sub.npz with the REFERENCE's own grid sub-sampling: its sources
(RandLA-Net/utils/cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp and cpp_utils/cloud/cloud.cpp) are
compiled where they lie, together with the small driver below, into a temporary directory (build container only).

    python tests/golden/make_golden_grid.py [path of the reference checkout]

Cases (np.random.default_rng(7), drawn in this order): `room` 20 000 points uniform in 3 x 2 x 1.5 m, the first third snapped
to the plane z = 0.02, dl = 0.04; `neg` 5 000 points of the unit cube shifted by -0.53, dl = 0.1; `tiny` 257 points of a
0.3 m cube, the first third on z = 0.02, dl = 0.05.  Colours are integers 0..255 as float32, labels floor(x / 0.5) % 13 with
5 % of the points relabelled at random.  Stored: the inputs and the reference's outputs, in the reference's (hash map) order.

Label ties (equally frequent labels in a cell) are where the reference's answer is an accident of its hash map; a fixture may
have them in at most 5 % of its cells (asserted here and in tests/test_grid_host.py).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import grid_ref  # noqa: E402

TIE_CAP = 0.05

DRIVER = r"""
// in:  int32 N, fdim, ldim; float dl; float points[N][3]; float features[N][fdim]; int32 labels[N][ldim]
// out: int32 M; float sub_points[M][3]; float sub_features[M][fdim]; int32 sub_labels[M][ldim]
#include <cstdio>
#include "grid_subsampling/grid_subsampling.h"
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int hdr[3]; float dl;
    if (!f || fread(hdr, 4, 3, f) != 3 || fread(&dl, 4, 1, f) != 1) return 1;
    const size_t N = hdr[0], fd = hdr[1], ld = hdr[2];
    vector<PointXYZ> pts(N), sub;
    vector<float> feat(N * fd), sfeat;
    vector<int> lab(N * ld), slab;
    if (fread(pts.data(), 12, N, f) != N || fread(feat.data(), 4, N * fd, f) != N * fd || fread(lab.data(), 4, N * ld, f) != N * ld) return 2;
    fclose(f);
    grid_subsampling(pts, sub, feat, sfeat, lab, slab, dl, 0);
    FILE *o = fopen(argv[2], "wb");
    const int M = (int)sub.size();
    fwrite(&M, 4, 1, o);
    fwrite(sub.data(), 12, sub.size(), o);
    fwrite(sfeat.data(), 4, sfeat.size(), o);
    fwrite(slab.data(), 4, slab.size(), o);
    fclose(o);
    return 0;
}
"""


def build_driver(ref, tmp):
    wrap = os.path.join(ref, "RandLA-Net", "utils", "cpp_wrappers")
    src = os.path.join(tmp, "driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "grid_ref_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-w", "-I", os.path.join(wrap, "cpp_subsampling"), src,
                           os.path.join(wrap, "cpp_subsampling", "grid_subsampling", "grid_subsampling.cpp"),
                           os.path.join(wrap, "cpp_utils", "cloud", "cloud.cpp"), "-o", exe])
    return exe


def run_reference(exe, tmp, points, features, labels, dl):
    fd = 0 if features is None else features.shape[1]
    lab = None if labels is None else labels.reshape(len(points), -1)
    ld = 0 if lab is None else lab.shape[1]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(points), fd, ld], np.int32).tobytes() + np.float32(dl).tobytes() + points.astype(np.float32).tobytes())
        if fd:
            f.write(features.astype(np.float32).tobytes())
        if ld:
            f.write(lab.astype(np.int32).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    M = int(np.frombuffer(raw, np.int32, 1)[0])
    sub = np.frombuffer(raw, np.float32, M * 3, 4).reshape(M, 3).copy()
    sf = np.frombuffer(raw, np.float32, M * fd, 4 + M * 12).reshape(M, fd).copy()
    sl = np.frombuffer(raw, np.int32, M * ld, 4 + M * 12 + M * fd * 4).reshape(M, ld).copy()
    return sub, sf, sl


def make_inputs():
    rng = np.random.default_rng(7)
    out = {}
    for name, n, box, shift, plane, dl in (("room", 20000, (3.0, 2.0, 1.5), 0.0, True, 0.04), ("neg", 5000, (1.0, 1.0, 1.0), -0.53, False, 0.1),
                                           ("tiny", 257, (0.3, 0.3, 0.3), 0.0, True, 0.05)):
        p = (rng.random((n, 3), dtype=np.float32) * np.array(box, np.float32) + np.float32(shift)).astype(np.float32)
        if plane:
            p[:n // 3, 2] = np.float32(0.02)
        col = rng.integers(0, 256, (n, 3)).astype(np.float32)
        lab = (np.floor(p[:, 0] / np.float32(0.5)).astype(np.int64) % 13).astype(np.int32)
        flip = rng.random(n) < 0.05
        lab[flip] = rng.integers(0, 13, int(flip.sum())).astype(np.int32)
        out[name] = (p, col, lab, dl)
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref, tmp)
        for name, (p, col, lab, dl) in make_inputs().items():
            sub, sf, sl = run_reference(exe, tmp, p, col, lab, dl)
            mine = grid_ref.grid_sub_sampling(p, col, lab, dl)
            ties = float(mine["tied"].any(axis=1).mean())
            assert ties <= TIE_CAP, "%s: %.1f %% of the cells have tied labels (cap %.0f %%)" % (name, 100 * ties, 100 * TIE_CAP)
            exact = grid_ref.same_bits(grid_ref.canonical(sub)[0], grid_ref.canonical(mine["sub_points"])[0])
            print("%s: N=%d M=%d tied cells %.2f %% restatement bit-equal: %s" % (name, len(p), len(sub), 100 * ties, exact))
            out.update({name + "_points": p, name + "_colors": col, name + "_labels": lab, name + "_dl": np.float32(dl),
                        name + "_sub_points": sub, name + "_sub_colors": sf, name + "_sub_labels": sl})
    path = os.path.join(HERE, "grid_sub.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
