"""The ResGCN block plan and switch set (pointsecguard_amd/csrc/psg_gcn_plan.h: GcnSwitches, GcnKnnSwitches, gcn_block, gcn_totals) compiled for
the HOST in a tiny stand-alone program - the pattern of tests/test_pn2_paths_host.py: the system compiler, no GPU, no library
loaded into Python; the same program once more under the address + undefined-behaviour sanitizers.

The program prints, for (res | plain | dense) x (edge | mr) at n_blocks = 1, 3, 5, 28, every block's descriptor and the two
totals; with an argument, the switch set as parsed from its environment (one process per setting).

The table below was derived BY HAND from the four places that spelled these facts out before the header existed
(psg_gcn_model_create_cfg: C, arg_off; psg_gcn_ws_create_cfg: c_max, arg_total; psg_gcn_forward: xin, ld, dil, have_sq,
resid, next_path, sq_o; backward_alt: tgt, ld_t), not from the header: res / edge is written out in full, the other
configurations as the columns they change."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
SIZES = (1, 3, 5, 28)
COLS = ("C", "ld", "dil", "in", "tgt", "resid", "have_sq", "sq_out", "feeds_next", "arg_off")

MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "psg_gcn_plan.h"
using namespace psg_gcn;
int main(int argc, char **)
{
    if (argc > 1) {
        auto env_str = [](const char *n) -> const char * { return getenv(n); };
        const GcnSwitches s = read_switches([](const char *n, int d) { const char *v = getenv(n); return v ? atoi(v) : d; }, env_str);
        const GcnKnnSwitches k = read_knn_switches(env_str);
        printf("small_below=%d edge_bwd_atomic=%d pq_fusion=%d no_graph=%d knn_mode=%d knn_bf_max_d=%d knn_stats=%d\n", s.gemm_small_below,
               (int)s.edge_bwd_atomic, (int)s.pq_fusion, (int)s.no_graph, k.mode, k.bf_max_d, (int)k.stats);
        return 0;
    }
    const int sizes[4] = {1, 3, 5, 28};
    for (int block = 0; block < 3; ++block)
        for (int conv = 0; conv < 2; ++conv)
            for (int n : sizes) {
                const GcnCfg g{block, conv, n};
                for (int e = 0; e < n; ++e) {
                    const GcnBlock b = gcn_block(g, e);
                    printf("%d %d %d block %d %d %d %d %d %d %d %d %d %d %zu\n", block, conv, n, e, b.C, b.ld, b.dil, b.in_off, b.tgt_off,
                           (int)b.resid, (int)b.have_sq, (int)b.sq_out, (int)b.feeds_next, b.arg_off);
                }
                const GcnTotals t = gcn_totals(g);
                // the model side's offsets and the workspace side's total are one sum: the last block's offset + its width
                const GcnBlock last = gcn_block(g, n - 1);
                printf("%d %d %d totals %d %zu %zu\n", block, conv, n, t.c_max, t.arg_total, conv ? last.arg_off + (size_t)last.C : t.arg_total);
            }
    return 0;
}
"""

# ---- res / edge, in full.  Columns: C ld dil in tgt resid have_sq sq_out feeds_next arg_off.
# Block 0 reads the 9 input channels (ld 9; its input and gradient target are x0 / dx0, the offsets unused: 0), its graph is the
# xyz kNN (dil 1).  Block e > 0 reads the 64 outputs of block e - 1 (rows of 64 n floats, column 64 (e - 1)) with dilation e, carries
# a residual, finds its norms written by block e - 1's edge pass; every block's edge pass writes norms; all but the last feed a
# next block.  arg_off is an mr quantity: 0.
RES_EDGE = {
    1: [(9, 9, 1, 0, 0, 0, 0, 1, 0, 0)],
    3: [(9, 9, 1, 0, 0, 0, 0, 1, 1, 0), (64, 192, 1, 0, 0, 1, 1, 1, 1, 0), (64, 192, 2, 64, 64, 1, 1, 1, 0, 0)],
    5: [(9, 9, 1, 0, 0, 0, 0, 1, 1, 0), (64, 320, 1, 0, 0, 1, 1, 1, 1, 0), (64, 320, 2, 64, 64, 1, 1, 1, 1, 0),
        (64, 320, 3, 128, 128, 1, 1, 1, 1, 0), (64, 320, 4, 192, 192, 1, 1, 1, 0, 0)],
    28: [(9, 9, 1, 0, 0, 0, 0, 1, 1, 0)] + [(64, 1792, e, 64 * (e - 1), 64 * (e - 1), 1, 1, 1, 1 if e < 27 else 0, 0) for e in range(1, 28)],
}
# totals: widest conv input, arg-max bytes per vertex (9 + 64 per later block; the workspace computed it for every conv kind)
RES_EDGE_TOTALS = {1: (64, 9), 3: (64, 137), 5: (64, 265), 28: (64, 1737)}


def _want(block, conv, n):
    """the hand table of one configuration: res / edge with the columns this configuration changes"""
    rows = [dict(zip(COLS, r)) for r in RES_EDGE[n]]
    c_max, arg_total = RES_EDGE_TOTALS[n]
    for e, r in enumerate(rows):
        if block == "plain":          # PlainDynBlock2d: dilation 1 everywhere, no residual
            r.update(dil=1, resid=0)
        if block == "dense":          # DenseDynBlock2d: block e reads ALL earlier outputs, a prefix of the rows, through the round-1
            r.update(resid=0, have_sq=0, sq_out=0, feeds_next=0)      # kNN path (C != 64): no norms from or for an edge pass
            if e > 0:
                r.update(C=64 * e, **{"in": 0, "tgt": 0})
        if conv == "mr":              # MRConv: no edge pass, so nothing of its by-products; arg-max bytes at the sum of C before
            r.update(have_sq=0, sq_out=0, feeds_next=0, arg_off=sum(q["C"] for q in rows[:e]))
    if block == "dense":
        c_max = max(64, 64 * (n - 1))
        arg_total = 9 + sum(64 * e for e in range(1, n))
    return [tuple(r[c] for c in COLS) for r in rows], (c_max, arg_total)


# (environment, the fields it changes); defaults: the library's before the switch set moved into the header
DEFAULTS = dict(small_below=384, edge_bwd_atomic=0, pq_fusion=0, no_graph=0, knn_mode=2, knn_bf_max_d=27, knn_stats=0)
SWITCH_SETTINGS = {
    "unset": ({}, {}),
    "small_below": ({"PSG_GEMM_SMALL_BELOW": "0"}, dict(small_below=0)),
    "edge_bwd_atomic": ({"PSG_GCN_EDGE_BWD": "atomic"}, dict(edge_bwd_atomic=1)),
    "edge_bwd_other": ({"PSG_GCN_EDGE_BWD": "gather"}, {}),
    "knn_matrix": ({"PSG_GCN_KNN": "matrix"}, dict(knn_mode=0)),
    "knn_f32": ({"PSG_GCN_KNN": "f32"}, dict(knn_mode=1)),
    "knn_bf16": ({"PSG_GCN_KNN": "bf16"}, dict(knn_bf_max_d=1 << 30)),
    "knn_bf_maxd": ({"PSG_GCN_KNN_BF_MAXD": "20"}, dict(knn_bf_max_d=20)),
    "knn_bf16_maxd": ({"PSG_GCN_KNN": "bf16", "PSG_GCN_KNN_BF_MAXD": "12"}, dict(knn_bf_max_d=12)),
    "knn_stats": ({"PSG_GCN_KNN_STATS": "1"}, dict(knn_stats=1)),
    "knn_stats_any_value": ({"PSG_GCN_KNN_STATS": "0"}, dict(knn_stats=1)),      # (set to anything: the library tested for presence)
    "pq_fusion": ({"PSG_GCN_PQ_FUSION": "1"}, dict(pq_fusion=1)),
    "no_graph": ({"PSG_GCN_NO_GRAPH": "1"}, dict(no_graph=1)),
    "no_graph_0": ({"PSG_GCN_NO_GRAPH": "0"}, {}),
}
SWITCHES = ["PSG_GEMM_SMALL_BELOW", "PSG_GCN_EDGE_BWD", "PSG_GCN_KNN", "PSG_GCN_KNN_BF_MAXD", "PSG_GCN_KNN_STATS", "PSG_GCN_PQ_FUSION",
            "PSG_GCN_NO_GRAPH"]


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no C++ compiler on this machine"
    tmp = tmp_path_factory.mktemp("gcn_plan")
    src = str(tmp / "main.cpp")
    with open(src, "w") as f:
        f.write(MAIN)
    exes = []
    for name, flags in (("plan", ["-O2"]), ("plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp / name)
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-I", CSRC, src, "-o", exe] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        exes.append(exe)
    return exes


def _run(exe, env_extra, *args):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    r = subprocess.run([exe] + list(args), env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def plans(programs):
    """per program: {(block, conv, n): ([descriptor rows], (c_max, arg_total, last arg_off + C))}"""
    out = []
    for exe in programs:
        got = {}
        for line in _run(exe, {}):
            w = line.split()
            key = ("res plain dense".split()[int(w[0])], "edge mr".split()[int(w[1])], int(w[2]))
            rows, _ = got.setdefault(key, ([], None))
            if w[3] == "block":
                assert int(w[4]) == len(rows)
                rows.append(tuple(int(v) for v in w[5:]))
            else:
                got[key] = (rows, tuple(int(v) for v in w[4:]))
        out.append(got)
    return out


@pytest.mark.parametrize("conv", ["edge", "mr"])
@pytest.mark.parametrize("block", ["res", "plain", "dense"])
def test_every_block_matches_the_hand_derived_table(plans, block, conv):
    for got in plans:      # the plain build and the sanitizer build
        assert len(got) == 6 * len(SIZES)
        for n in SIZES:
            rows, totals = got[(block, conv, n)]
            want_rows, want_totals = _want(block, conv, n)
            assert len(rows) == n
            wrong = {e: (rows[e], want_rows[e]) for e in range(n) if rows[e] != want_rows[e]}
            assert not wrong, (n, wrong)
            assert totals[:2] == want_totals, (n, totals)


def test_model_offsets_and_workspace_total_are_one_sum(plans):
    """conv = mr: the last block's arg-max offset plus its width IS the workspace's bytes per vertex, and the offsets ascend by C"""
    for got in plans:
        for (block, conv, n), (rows, totals) in got.items():
            assert totals[2] == totals[1], (block, conv, n, totals)
            if conv == "mr":
                off = 0
                for r in rows:
                    assert r[COLS.index("arg_off")] == off
                    off += r[0]
                assert off == totals[1]


@pytest.mark.parametrize("setting", sorted(SWITCH_SETTINGS))
def test_switches_parse_to_the_library_s_meaning(programs, setting):
    env, changes = SWITCH_SETTINGS[setting]
    want = dict(DEFAULTS, **changes)
    for exe in programs:
        (line,) = _run(exe, env, "switches")
        got = {k: int(v) for k, v in (w.split("=") for w in line.split())}
        assert got == want
