"""psg_ce_row.cuh (the CE-on-log-probs row shared by ce_logp_grad_kernel and the fused fp1 + head launch of the PointNet++ NB
loop) compiled for the HOST in a tiny stand-alone program and compared with a numpy float32 restatement of
ce_logp_grad_kernel's loop: maximum, sum of exp in class order 0 .. 12, (z - m) - lse, exp, (p - onehot) * scale.

Every float32 operation of the restatement is the one the C++ expression performs, in its order, and expf / logf are the C
library's own (the program and the restatement call the same libm), so the comparison is EXACT: a changed order of the sum, a
contracted multiply-add or a re-associated (z - m) - lse shows as a differing bit on at least one of the rows.  No GPU."""
import ctypes
import ctypes.util
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
NC = 13
f32 = np.float32

MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "psg_ce_row.cuh"
// stdin: lines "<active> <y> <scale bits> <13 x logp bits>" (hex); stdout: "<term bits> <13 x g bits>" per line
int main()
{
    unsigned act, sb, zb[13];
    int y;
    while (scanf("%u %d %x", &act, &y, &sb) == 3) {
        float lp[13], g[13], scale;
        memcpy(&scale, &sb, 4);
        for (int c = 0; c < 13; ++c) { if (scanf("%x", &zb[c]) != 1) return 1; memcpy(&lp[c], &zb[c], 4); }
        const float term = psg::ce_row_grad(lp, 13, y, scale, act != 0, g);
        unsigned tb;
        memcpy(&tb, &term, 4);
        printf("%08x", tb);
        for (int c = 0; c < 13; ++c) { unsigned gb; memcpy(&gb, &g[c], 4); printf(" %08x", gb); }
        printf("\n");
    }
    return 0;
}
"""


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no C++ compiler on this machine"
    tmp = tmp_path_factory.mktemp("ce_row")
    src, exe = str(tmp / "main.cpp"), str(tmp / "ce_row")
    with open(src, "w") as f:
        f.write(MAIN)
    # -O2 like the library's host code; contraction off as in the header's pragma (a compiler that ignores the pragma included)
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC, src, "-o", exe, "-lm"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _libm():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for fn in (lib.expf, lib.logf):
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return lib


def _restate(lp, y, scale, active, libm):
    """ce_logp_grad_kernel's per-row loop, one float32 operation at a time"""
    if not active:
        return f32(0), np.zeros(NC, f32)
    z = lp.astype(f32)
    m = f32(-np.inf)
    for c in range(NC):
        m = max(m, z[c])
    s = f32(0)
    for c in range(NC):
        s = f32(s + f32(libm.expf(f32(z[c] - m))))
    lse = f32(libm.logf(s))
    g, term = np.zeros(NC, f32), f32(0)
    for c in range(NC):
        lp2 = f32(f32(z[c] - m) - lse)
        p = f32(libm.expf(lp2))
        g[c] = f32(f32(p - f32(1.0 if c == y else 0.0)) * scale)
        if c == y:
            term = f32(f32(-lp2) * scale)
    return term, g


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _rows():
    rng = np.random.default_rng(5)

    def logp(z):      # any row is a valid input; log-probs are what the network hands over
        z = np.asarray(z, np.float64)
        return (z - z.max() - np.log(np.exp(z - z.max()).sum())).astype(f32)

    saturated = np.full(NC, -90.0)
    saturated[3] = 0.0
    rows = [("saturated", logp(saturated), 3, True), ("saturated_wrong_label", logp(saturated), 7, True),
            ("equal_logits", logp(np.zeros(NC)), 4, True), ("label_0", logp(rng.normal(0, 3, NC)), 0, True),
            ("label_12", logp(rng.normal(0, 3, NC)), 12, True), ("beyond_rows_active", logp(rng.normal(0, 3, NC)), 5, False)]
    rows += [("random%d" % i, logp(rng.normal(0, 4, NC)), int(rng.integers(0, NC)), True) for i in range(8)]
    return rows


def test_ce_row_matches_the_float32_restatement(program):
    libm = _libm()
    rows = _rows()
    for scale in (f32(1.0 / 4096), f32(1.0 / 1024)):
        text = "".join("%d %d %08x %s\n" % (act, y, _bits(scale), " ".join("%08x" % _bits(v) for v in lp)) for _, lp, y, act in rows)
        r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(rows)
        for (name, lp, y, act), line in zip(rows, lines):
            got = [int(w, 16) for w in line.split()]
            term, g = _restate(lp, y, scale, act, libm)
            assert got[1:] == [_bits(v) for v in g], (name, got[1:], [_bits(v) for v in g])
            assert got[0] == _bits(term), name
            if not act:
                assert got == [0] * (NC + 1), name
            else:
                gv = np.array([struct.unpack("<f", struct.pack("<I", w))[0] for w in got[1:]], np.float64) / float(scale)
                # softmax - onehot (a saturated row's own class rounds to exactly 0)
                assert abs(gv.sum()) < 1e-5 and gv[y] <= 0 and (np.delete(gv, y) >= 0).all(), name


def test_both_users_call_the_one_function():
    """ce_logp_grad_kernel and fp1_loop_kernel hold no copy of the row arithmetic"""
    attack = open(os.path.join(CSRC, "psg_attack.hip")).read()
    kernels = open(os.path.join(CSRC, "psg_pn2_kernels.cuh")).read()
    assert "ce_row_grad(" in attack and "ce_row_grad(" in kernels
    assert "clang fp contract(off)" in open(os.path.join(CSRC, "psg_ce_row.cuh")).read()
