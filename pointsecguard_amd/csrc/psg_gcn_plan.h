// Host-only side of the ResGCN unit (psg_resgcn.hip, psg_resgcn_attack.hip): its eight environment switches and the per-block
// plan of the backbone.  Plain C++17 without HIP: tests/test_gcn_plan_host.py builds it into a stand-alone program and checks
// every descriptor and every switch against a hand table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "../../include/psg.h"

namespace psg_gcn {

constexpr int GC = 64;      // n_filters
constexpr int NCLS = 13;
constexpr int KNB = 16;     // k

// ---- the switches (registered in psg_api.hip: kEnvSwitches).  All select between tested paths that compute the same bits, or
// turn on diagnosis.  `env_int(name, default)` / `env_str(name)` are the library's readers (psg_common.h) or, in a host program, getenv.
// Read ONCE per process (psg_resgcn.hip: gcn_switches):
struct GcnSwitches {
    int gemm_small_below = 384;     // PSG_GEMM_SMALL_BELOW: the workgroup count below which launch_gemm takes 64 x 64 tiles (A/B runs)
    bool edge_bwd_atomic = false;   // PSG_GCN_EDGE_BWD=atomic: the EdgeConv max-pass backward as the atomic scatter, not the gather kernel
    // PSG_GCN_PQ_FUSION=1: a block's edge pass also computes the next block's per-vertex product (edge_max_pq_fwd_kernel).
    // Measured on MI355X: 0.21 ms less kernel time per 4-room iteration (8.09 -> 7.89) and +2 % with one launch in flight
    // (10.18 -> 10.39 rooms/s), but -0.7 % at the bench's three launches in flight (12.05 -> 11.96): the small GEMM launches
    // it removes were running inside the idle slots of another launch's kNN kernel.  Off by default for that reason.
    bool pq_fusion = false;
    bool no_graph = false;          // PSG_GCN_NO_GRAPH=1: the NB loops stay eager (no hipGraph of the interior iterations)
};
template <typename EnvInt, typename EnvStr> GcnSwitches read_switches(EnvInt env_int, EnvStr env_str)
{
    GcnSwitches s;
    s.gemm_small_below = env_int("PSG_GEMM_SMALL_BELOW", 384);
    const char *eb = env_str("PSG_GCN_EDGE_BWD");
    s.edge_bwd_atomic = eb && !strcmp(eb, "atomic");
    s.pq_fusion = env_int("PSG_GCN_PQ_FUSION", 0) != 0;
    s.no_graph = env_int("PSG_GCN_NO_GRAPH", 0) != 0;
    return s;
}
// Read at EVERY workspace creation and kept in the workspace: tests/test_gpu_knn_fused.py, tests/test_gpu_knn_bf16.py and
// tools/knn_*.py set them between two workspaces of one process.
struct GcnKnnSwitches {
    // PSG_GCN_KNN: which kernel builds the dilated graph of 64-wide features.  Unset: the bf16-prefilter kernel for every
    // dilation of the network (1..27): since round 6 (2048-bin final ranking) it is the faster one on the
    // network's own features up to d = 27 (148-153 us against 178-184 us per 4-room call at d = 21..27, no tile on the exact
    // path; rounds 4-5 split at 20, where rows of more than 256 finalists started to fall back); the exact fused kernel stays
    // as the in-launch fallback; both give the same graph bit for bit.  =f32 / =bf16 force one kernel for every dilation,
    // =matrix the round-1 path (distance matrix in HBM + selection kernel).
    int mode = 2;          // 1 = exact fused kernel only (=f32), 2 = bf16 prefilter up to bf_max_d, 0 = round-1 path (=matrix)
    int bf_max_d = 27;     // PSG_GCN_KNN_BF_MAXD: the prefilter kernel serves dilations up to this, the exact kernel the rest
    bool stats = false;    // PSG_GCN_KNN_STATS (set to anything): the workspace carries the prefilter kernel's device counters
};
template <typename EnvStr> GcnKnnSwitches read_knn_switches(EnvStr env_str)
{
    GcnKnnSwitches k;
    const char *kv = env_str("PSG_GCN_KNN"), *mode = kv ? kv : "";
    k.mode = !strcmp(mode, "matrix") ? 0 : (!strcmp(mode, "f32") ? 1 : 2);
    k.bf_max_d = !strcmp(mode, "bf16") ? 1 << 30 : 27;
    if (const char *md = env_str("PSG_GCN_KNN_BF_MAXD")) k.bf_max_d = atoi(md);
    k.stats = env_str("PSG_GCN_KNN_STATS") != nullptr;
    return k;
}

// ---- the block plan: what EdgeConv / MRConv block e of a backbone reads and writes, decided HERE and nowhere else (model and
// workspace creation, the forward and both backward loops read it).  Block e writes columns [64 e, 64 e + 64) of the
// workspace's `feats` rows (F = 64 n_blocks floats); its output gradient is the same slice of `dfeats`.
struct GcnCfg { int block, conv, n_blocks; };   // PSG_GCN_BLOCK_*, PSG_GCN_CONV_*
inline bool operator==(const GcnCfg &a, const GcnCfg &b) { return a.block == b.block && a.conv == b.conv && a.n_blocks == b.n_blocks; }
struct GcnBlock {
    int C;            // input width: 9 (head), 64, or dense: all earlier outputs
    int ld;           // floats per input row: 9 (the head reads x0) or F
    int dil;          // dilation of its graph: 1 for the head (xyz kNN, architecture.py:59) and plain blocks (:36), else e (:23,28)
    int in_off;       // e > 0: first column of `feats` it reads (the previous output, or dense: a prefix of the rows)
    int tgt_off;      // e > 0: first column of `dfeats` its input gradient is added to (the head writes dx0 instead)
    bool resid;       // y = conv(x) + x (res blocks but the head)
    bool have_sq;     // the norms (and operand copies) of its input came out of the producing edge pass: no kNN prep launch
    bool sq_out;      // its edge pass writes the norms of its output beside the features (edge convs of res / plain backbones)
    bool feeds_next;  // .. and a next block reads exactly these 64 outputs: its kNN kernel names the operand copies to write too
    size_t arg_off;   // conv = mr: offset of its arg-max bytes per vertex (the sum of C before it), else 0
};
inline int gcn_width(const GcnCfg &g, int e) { return e == 0 ? 9 : (g.block == PSG_GCN_BLOCK_DENSE ? GC * e : GC); }
// arg-max bytes per vertex of the mr blocks before e: the ONE running sum behind GcnBlock::arg_off and GcnTotals::arg_total
inline size_t gcn_arg_bytes(const GcnCfg &g, int e)
{
    size_t s = 0;
    for (int i = 0; i < e; ++i) s += (size_t)gcn_width(g, i);
    return s;
}
inline GcnBlock gcn_block(const GcnCfg &g, int e)
{
    const bool dense = g.block == PSG_GCN_BLOCK_DENSE, mr = g.conv == PSG_GCN_CONV_MR;
    GcnBlock b;
    b.C = gcn_width(g, e);
    b.ld = e == 0 ? 9 : GC * g.n_blocks;
    b.dil = e == 0 || g.block == PSG_GCN_BLOCK_PLAIN ? 1 : e;
    b.in_off = b.tgt_off = e == 0 || dense ? 0 : GC * (e - 1);
    b.resid = e > 0 && g.block == PSG_GCN_BLOCK_RES;
    b.have_sq = e > 0 && !mr && !dense;
    b.sq_out = !mr && !dense;
    b.feeds_next = b.sq_out && e + 1 < g.n_blocks;
    b.arg_off = mr ? gcn_arg_bytes(g, e) : 0;
    return b;
}
struct GcnTotals { int c_max; size_t arg_total; };   // widest conv input (dense: all earlier outputs); arg-max bytes per vertex
inline GcnTotals gcn_totals(const GcnCfg &g)
{
    return GcnTotals{std::max(GC, gcn_width(g, g.n_blocks - 1)), gcn_arg_bytes(g, g.n_blocks)};
}

}  // namespace psg_gcn
