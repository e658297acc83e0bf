// Host-only side of the PointNet++ launches (psg_pn2.hip): the process-wide switch set, the table of SA module kernels, the two
// architecture descriptors, and the ONE decision of which kernel family an SA level runs, forward and backward.  Plain C++17
// without HIP: tests/test_pn2_paths_host.py builds it into a stand-alone program and checks every decision against a hand table.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/psg.h"

// (psg_mlp.cuh's build-time LDS geometry, the same guarded defaults: the packed forward's fit depends on it)
#ifndef PSG_LDS_PAD
#define PSG_LDS_PAD 0
#endif
#ifndef PSG_LDS_SPARE
#define PSG_LDS_SPARE 0
#endif

namespace psg_pn2 {

constexpr int MAXL = PSG_PN2_MSG_NUM_LAYERS;   // the larger of the two layer counts
constexpr int NCLS = PSG_PN2_NUM_CLASSES;
constexpr int kS[4] = {1024, 256, 64, 16};
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------------------------------------ the switch set
// Every process-wide switch of psg_pn2.hip, read ONCE (read_switches) and registered in psg_api.hip (kEnvSwitches).  All but
// `diag` select between tested paths that compute the same bits (A/B runs; the test that runs both is named with each).
constexpr int kPackBwdBuilt = (1 << 0) | (1 << 1) | (1 << 2);
struct Pn2Switches {
    // PSG_PN2_SPLIT: 1 = the first layer of SA levels 1 - 3 split into a per-point feature product and a per-row xyz chunk
    // (sa_fwd_kernel SPLIT), SSG and MSG alike: 8 x fewer points than grouped rows.  Level 0 stays whole: its 9 feature channels
    // are 2 of the module's 14 k8-chunk passes, the rows of T (32 floats) would be a larger gather than the 12 floats it replaces,
    // and its backward writes compact 16-byte colour rows.  0 = whole first layers everywhere
    // (tests/test_gpu_alt_paths.py).  2 (measurement): the FORWARD of SSG level 0 split as well - T0 = W1f . x0 + b1 per point of
    // the room on the vector pipe, gathered into the accumulators like the other levels; its backward stays whole.
    int split = 1;
    // PSG_PN2_FPSPLIT: the first layer of fp1 .. fp3 split across the 3-NN interpolation (fp_layer1_split): its interpolated-part
    // columns run per COARSE point inside the coarser module's kernels, forward and backward; fp4 stays whole (its coarse side is
    // the 16 points of level 4: nothing to fuse into).  0 = whole first layers (tests/test_gpu_alt_paths.py).
    bool fpsplit = true;
    // PSG_FP1_WAVE=1: the wave-private fp1 + head kernels (psg_chain.cuh; they know no split) instead of the cooperative ones.
    // MI355X, 32 rooms: forward 193 vs 193 us, backward 211 vs 189 us, so the cooperative kernels stay the default.
    bool fp1_wave = false;
    // PSG_PN2_PACK: the SSG SA forward kernels run a group's valid rows only (sa_fwd_packed_kernel); 0 = the unpacked kernels
    // (tests/test_gpu_sa_pack.py), which MSG (16-sample scales) always runs.
    bool pack = true;
    // PSG_PN2_PACK_BWD: bit l = the backward of packed level l runs the same packed rows (sa_bwd_packed_kernel) and its forward
    // keys the ReLU masks by packed workgroup.  Unset or 1 = kPackBwdBuilt, 0 = none, L + level digits (L0, L02) = exactly those
    // levels with bit 8 set: a level NAMED that does not fit the packed kernel's configuration is an error at its launch, not a
    // fall-back.  The default set holds the levels whose launch is faster packed in the headline rooms (DESIGN.md section 4,
    // rounds 19 and 27): 0, 1 and 2 - level 2 since its max-pool transpose runs in channel order (82 against 100 us); level 3
    // is slower packed (too few workgroups are left to hide the sparse stream's latency).
    int pack_bwd = kPackBwdBuilt;
    // PSG_PN2_POOLT_ORDER=row: the max-pool transpose of a packed sparse level as batches of row-ordered item lists instead of
    // channel order over all of a workgroup's groups (sa_bwd_packed_chan).  The same bytes (tests/test_gpu_sa_poolt_order.py).
    bool poolt_chan = true;
    // PSG_PN2_POOLT_SPARSE=0: the dense transposed third layer instead of the sparse weight-row stream (SaPath::spv).
    bool poolt_sparse = true;
    // PSG_PN2_L1T_COLOUR=0: a colour-only request at level 0 keeps the transposed first layer on the matrix pipe (sa_l1t_colour).
    bool l1t_colour = true;
    // PSG_PN2_PW_SIZED=0: the per-point launches of the split SA levels on fp_fwd_kernel<32, 8> / pw_bwd_kernel<32, 8> whatever the
    // layer's width, instead of as many waves as the layer has output tiles.  Bit-identical (tests/test_gpu_pw_sized.py).
    bool pw_sized = true;
    // PSG_PN2_BALL_TABLE: 0 = always the direct level-0 ball query, 2 = the per-room table for every plan (the measurement of the
    // threshold), 1 = by plan size (ball_table_route; tests/test_gpu_ball_table.py).  Integer results.
    int ball_table = 1;
    // PSG_PN2_FP1_LOOP=0: three launches even where the fused fp1 + head launch applies (fp1_loop_applies; tests/test_gpu_fp1_loop.py).
    bool fp1_loop = true;
    // PSG_PN2_PGD_FUSE=0: the PGD step as a launch of its own behind the gradient's last gather (dx0_gather_pgd_kernel fuses them).
    bool pgd_fuse = true;
    // PSG_PN2_GRAPH=1: replay a whole NB attack as a hipGraph.  Measured slower than the eager launches and left OFF (psg_pn2_nb_attack).
    bool graph = false;
    // PSG_DIAG: section-skipping timing switches of the module kernels, in `make EXTRA=-DPSG_DIAG_BUILD` libraries only
    // (tools/diag_*.sh); the default library has no way to skip work (psg_pn2_kernels.cuh: PSG_DIAGBIT == 0).
    int diag = 0;
};

// `env_int(name, default)` and `env_str(name)` are the library's registered readers (psg_common.h) or, in a host program, getenv.
template <typename EnvInt, typename EnvStr> Pn2Switches read_switches(EnvInt env_int, EnvStr env_str)
{
    Pn2Switches s;
    s.split = env_int("PSG_PN2_SPLIT", 1);
    s.fpsplit = env_int("PSG_PN2_FPSPLIT", 1) != 0;
    s.fp1_wave = env_int("PSG_FP1_WAVE", 0) != 0;
    s.pack = env_int("PSG_PN2_PACK", 1) != 0;
    if (const char *v = env_str("PSG_PN2_PACK_BWD"); v && *v) {
        const bool by_name = *v == 'L' || *v == 'l';
        s.pack_bwd = by_name ? 1 << 8 : atoi(v) != 0 ? kPackBwdBuilt : 0;
        for (const char *c = v + 1; by_name && *c; ++c)
            if (*c >= '0' && *c <= '3') s.pack_bwd |= 1 << (*c - '0');
    }
    if (const char *v = env_str("PSG_PN2_POOLT_ORDER")) s.poolt_chan = strcmp(v, "row") != 0;
    s.poolt_sparse = env_int("PSG_PN2_POOLT_SPARSE", 1) != 0;
    s.l1t_colour = env_int("PSG_PN2_L1T_COLOUR", 1) != 0;
    s.pw_sized = env_int("PSG_PN2_PW_SIZED", 1) != 0;
    s.ball_table = env_int("PSG_PN2_BALL_TABLE", 1);
    s.fp1_loop = env_int("PSG_PN2_FP1_LOOP", 1) != 0;
    s.pgd_fuse = env_int("PSG_PN2_PGD_FUSE", 1) != 0;
    s.graph = env_int("PSG_PN2_GRAPH", 0) != 0;
#ifdef PSG_DIAG_BUILD
    s.diag = env_int("PSG_DIAG", 0);
#endif
    return s;
}

// ------------------------------------------------------------------------------------- the table of SA module kernels
// One row per distinct SA configuration: points / waves per workgroup, samples per group, tiles a wave may hold across a
// layer's barrier forward and backward, and the kernel variants BUILT for it beside the whole forward and the dense backward,
// which every row has.  psg_pn2.hip instantiates exactly what a row's flags name (run_sa_fwd / run_sa_bwd: sa_visit).
enum : unsigned {
    V_SPLIT = 1,   // sa_fwd_kernel<.., true>: split first layer
    V_PACK0 = 2,   // packed with a whole first layer (SSG level 0): sa_fwd_packed_kernel<P, NW, false(, true)>, sa_bwd_packed_kernel<.., 0>
    V_PACK = 4,    // packed with a split first layer (SSG levels 1 - 3): sa_fwd_packed_kernel<P, NW, true(, true)>, sa_bwd_packed_kernel<.., SPV>
    V_CHAN = 8,    // sa_bwd_packed_kernel<.., SPV + SA_PACK_CHAN>: channel-ordered max-pool transpose
};
struct SaCfg { int P, NW, K, maxt_f, maxt_b; unsigned v; int spv; };
template <int P_, int NW_, int K_, int MF_, int MB_, unsigned V_, int SPV_ = 0> struct SaRow {
    static constexpr int P = P_, NW = NW_, K = K_, MF = MF_, MB = MB_, SPV = SPV_;   // SPV > 0: sa_bwd_sparse_kernel<P, NW, MB, SPV>
    static constexpr unsigned V = V_;
    static constexpr SaCfg cfg() { return SaCfg{P_, NW_, K_, MF_, MB_, V_, SPV_}; }
};
template <class... R> struct SaRowList {
    static constexpr SaCfg cfg[sizeof...(R)] = {R::cfg()...};
    template <class T> static constexpr int index() { int i = 0, f = -1; ((std::is_same<T, R>::value ? f = i++ : i++), ...); return f; }
};
// backward tiles per wave: ceil(widest layer's tiles / waves) (SSG sa2 67->96: 6 tiles on 4 waves; sa3 131->160: 5 on 4; sa4
// 259->288: 9 on 8; MSG first layers transposed: 99 -> 8 tiles, 259 -> 9, 515 -> 17)
using SaSsg1 = SaRow<128, 4, 32, 1, 1, V_SPLIT | V_PACK0>;           // SSG sa1, MSG sa1 scale 1
using SaSsg2 = SaRow<64, 4, 32, 1, 2, V_SPLIT | V_PACK | V_CHAN, 1>; // SSG sa2
using SaSsg3 = SaRow<32, 4, 32, 1, 2, V_SPLIT | V_PACK | V_CHAN, 2>; // SSG sa3
using SaSsg4 = SaRow<32, 8, 32, 1, 2, V_SPLIT | V_PACK, 4>;          // SSG sa4, MSG sa3 scale 1
using SaMsg1a = SaRow<128, 4, 16, 1, 1, 0>;                          // MSG sa1 scale 0 (level 0 is never split in MSG)
using SaMsg2a = SaRow<64, 4, 16, 1, 2, V_SPLIT>;                     // MSG sa2 scale 0
using SaMsg2b = SaRow<64, 8, 32, 1, 1, V_SPLIT>;                     // MSG sa2 scale 1
using SaMsg3a = SaRow<32, 8, 16, 1, 2, V_SPLIT>;                     // MSG sa3 scale 0
using SaMsg4a = SaRow<32, 8, 16, 1, 3, V_SPLIT>;                     // MSG sa4 scale 0
using SaMsg4b = SaRow<32, 8, 32, 2, 3, V_SPLIT>;                     // MSG sa4 scale 1: 384 -> 12 tiles on 8 waves
using SaRows = SaRowList<SaSsg1, SaSsg2, SaSsg3, SaSsg4, SaMsg1a, SaMsg2a, SaMsg2b, SaMsg3a, SaMsg4a, SaMsg4b>;

// -------------------------------------------------------------------------------------------- architecture descriptors
// One ball-query scale of an SA level: its three conv layers, its pooled output's column, its row of the kernel table
struct ScaleDesc {
    int K;          // nsample: 32, or 16 (two groups per 32-point MFMA tile)
    float r2;       // float32(radius**2) with radius**2 evaluated in double, as Python does (pointnet_util.py:102)
    int l0;         // index of the first of its 3 layers
    int c_off;      // first column of its C3 channels in the level's output rows
    int row;        // index into SaRows
    int P, NW, maxt_f, maxt_b;
};
template <class Row> ScaleDesc scale_of(double r, int l0, int c_off)
{
    return ScaleDesc{Row::K, (float)(r * r), l0, c_off, SaRows::index<Row>(), Row::P, Row::NW, Row::MF, Row::MB};
}

struct ArchDesc {
    int id;                 // PSG_PN2_ARCH_*
    int ns;                 // scales per SA level
    ScaleDesc sc[4][2];
    int C[5];               // feature channels of level 0..4
    int n_layers;
    int cin[MAXL], cout[MAXL];
    int fp_first[4], fp_count[4];   // FP module LVL (0 = fp1 .. 3 = fp4): first layer index, layer count
    int fp_maxt_b[4];
    int head;               // conv1; conv2 = head + 1
    bool sa_perm;           // reference concat order is [rel_xyz, feats] (SSG) rather than [feats, rel_xyz] (MSG)
    bool fp4_big;           // fp4's concatenated input exceeds LDS: streamed first / last layer
    int c3(int lvl, int s) const { return cout[sc[lvl][s].l0 + 2]; }
};

inline ArchDesc make_ssg()
{
    ArchDesc a{};
    a.id = PSG_PN2_ARCH_SSG; a.ns = 1; a.n_layers = PSG_PN2_NUM_LAYERS; a.sa_perm = true; a.fp4_big = false;
    const int cin[PSG_PN2_NUM_LAYERS] = {12, 32, 32, 67, 64, 64, 131, 128, 128, 259, 256, 256, 768, 256, 384, 256, 320, 256,
                                         128, 128, 128, 128, 128};
    const int cout[PSG_PN2_NUM_LAYERS] = {32, 32, 64, 64, 64, 128, 128, 128, 256, 256, 256, 512, 256, 256, 256, 256, 256, 128,
                                          128, 128, 128, 128, 13};
    for (int i = 0; i < a.n_layers; ++i) { a.cin[i] = cin[i]; a.cout[i] = cout[i]; }
    const int C[5] = {9, 64, 128, 256, 512};
    for (int i = 0; i < 5; ++i) a.C[i] = C[i];
    a.sc[0][0] = scale_of<SaSsg1>(0.1, 0, 0);
    a.sc[1][0] = scale_of<SaSsg2>(0.2, 3, 0);
    a.sc[2][0] = scale_of<SaSsg3>(0.4, 6, 0);
    a.sc[3][0] = scale_of<SaSsg4>(0.8, 9, 0);
    // layer indices: fp4 12,13  fp3 14,15  fp2 16,17  fp1 18,19,20 (+ head 21,22 fused into fp1)
    const int ff[4] = {18, 16, 14, 12}, fc[4] = {3, 2, 2, 2}, fm[4] = {1, 2, 2, 3};   // fp2 320: 10 tiles on 8 waves; fp3 384: 12; fp4 768: 24
    for (int l = 0; l < 4; ++l) { a.fp_first[l] = ff[l]; a.fp_count[l] = fc[l]; a.fp_maxt_b[l] = fm[l]; }
    a.head = 21;
    return a;
}

inline ArchDesc make_msg()
{
    ArchDesc a{};
    a.id = PSG_PN2_ARCH_MSG; a.ns = 2; a.n_layers = PSG_PN2_MSG_NUM_LAYERS; a.sa_perm = false; a.fp4_big = true;
    const int mlp[4][2][3] = {{{16, 16, 32}, {32, 32, 64}}, {{64, 64, 128}, {64, 96, 128}},
                              {{128, 196, 256}, {128, 196, 256}}, {{256, 256, 512}, {256, 384, 512}}};
    // kernel configurations: every layer of a module must fit maxt tiles per wave (tiles = ceil(width / 32) * P / 32)
    a.sc[0][0] = scale_of<SaMsg1a>(0.05, 0, 0); a.sc[0][1] = scale_of<SaSsg1>(0.1, 0, 0);
    a.sc[1][0] = scale_of<SaMsg2a>(0.1, 0, 0);  a.sc[1][1] = scale_of<SaMsg2b>(0.2, 0, 0);
    a.sc[2][0] = scale_of<SaMsg3a>(0.2, 0, 0);  a.sc[2][1] = scale_of<SaSsg4>(0.4, 0, 0);
    a.sc[3][0] = scale_of<SaMsg4a>(0.4, 0, 0);  a.sc[3][1] = scale_of<SaMsg4b>(0.8, 0, 0);
    a.C[0] = 9;
    int li = 0;
    for (int l = 0; l < 4; ++l) {
        int coff = 0;
        for (int s = 0; s < 2; ++s) {
            a.sc[l][s].l0 = li; a.sc[l][s].c_off = coff;
            int last = a.C[l] + 3;
            for (int j = 0; j < 3; ++j) { a.cin[li] = last; a.cout[li] = mlp[l][s][j]; last = mlp[l][s][j]; ++li; }
            coff += mlp[l][s][2];
        }
        a.C[l + 1] = coff;
    }
    // fp4, fp3, fp2, fp1 (state_dict order), then the head
    const int fin[4] = {a.C[3] + a.C[4], a.C[2] + 256, a.C[1] + 256, 128};
    const int fw[4][3] = {{256, 256, 0}, {256, 256, 0}, {256, 128, 0}, {128, 128, 128}};
    const int fm[4] = {1, 2, 2, 1};   // by LVL: fp1 1; fp2 352 -> 11 tiles on 8 waves; fp3 512 -> 16; fp4 streamed
    for (int q = 0; q < 4; ++q) {
        const int lvl = 3 - q, n = q == 3 ? 3 : 2;
        a.fp_first[lvl] = li; a.fp_count[lvl] = n; a.fp_maxt_b[lvl] = fm[lvl];
        int last = fin[q];
        for (int j = 0; j < n; ++j) { a.cin[li] = last; a.cout[li] = fw[q][j]; last = fw[q][j]; ++li; }
    }
    a.head = li;
    a.cin[li] = 128; a.cout[li] = 128; ++li;
    a.cin[li] = 128; a.cout[li] = NCLS; ++li;
    return a;
}

inline const ArchDesc &arch_of(int id)
{
    static const ArchDesc ssg = make_ssg(), msg = make_msg();
    return id == PSG_PN2_ARCH_MSG ? msg : ssg;
}

// ---------------------------------------------------------------------------------------------- the path decision
// FP module lvl (0 = fp1 .. 3 = fp4) runs its first layer split (Pn2Switches::fpsplit)
inline bool fp_split(const Pn2Switches &sw, int lvl) { return sw.fpsplit && lvl <= 2 && !(lvl == 0 && sw.fp1_wave); }

// The kernel families of an SA module
enum class SaKernel { fwd_whole, fwd_split, fwd_packed, fwd_packed_keys, bwd_dense, bwd_sparse, bwd_packed_dense0,
                      bwd_packed_sparse, bwd_packed_chan, error };

// What SA level `lvl`, scale `sc` of an architecture runs under a switch set: decided HERE and nowhere else.  A model and a
// workspace of one process are created under the same switches, so both read the same answer (psg_pn2.hip: sa_path_of).
struct SaPath {
    bool split_fwd = false;     // forward: per-point product + per-row xyz chunk
    bool split_bwd = false;     // backward stores dZ1 rows, summed per point by pw_bwd_kernel
    bool packed = false;        // the plan builds the level's packed descriptors (SSG under PSG_PN2_PACK)
    bool packed_fwd = false;    // sa_fwd_packed_kernel
    bool packed_keys = false;   // .. with its ReLU masks keyed by packed workgroup: the backward runs packed
    enum Bwd { none, dense0, sparse, chan } packed_bwd = none;
    int spv = 0;                // sparse max-pool transpose: C2 / 64, or 0 for the dense transposed layer
    bool w1c = false;           // a colour-only request runs sa_l1t_colour (level 0)
    // a level named explicitly by PSG_PN2_PACK_BWD that does not fit: the message of the launch that fails, or null
    const char *fwd_error = nullptr, *bwd_error = nullptr;
};

inline SaPath sa_path(const ArchDesc &A, const Pn2Switches &sw, int lvl, int sc)
{
    const ScaleDesc &d = A.sc[lvl][sc];
    const int P = d.P, NW = d.NW, KS = d.K, NT = NW * 64, PB = P / 32;
    const SaCfg &row = SaRows::cfg[d.row];
    auto split_at = [&](int l) { return sw.split != 0 && l >= 1; };
    auto lb = [](int k8, int mb) { return std::max(k8, mb * 4); };
    const int C1 = A.cout[d.l0], C2 = A.cout[d.l0 + 1], C3 = A.cout[d.l0 + 2];
    SaPath p;
    p.split_bwd = split_at(lvl);
    p.split_fwd = p.split_bwd || (sw.split == 2 && A.id == PSG_PN2_ARCH_SSG && lvl == 0);
    p.packed = sw.pack && A.id == PSG_PN2_ARCH_SSG;
    // Packed rows (SSG as shipped: level 0 whole, levels 1 - 3 split); any other first-layer form keeps the unpacked kernels.  LDS:
    // the [P][C3] pool rows over the activation buffer (`blocks`), the row maps behind it, the group starts in pool row P - 1.
    const int blk = P * 8 + PSG_LDS_PAD, nb3 = cdiv(C3, 32);
    const int blocks = std::max(std::max(lb(cdiv(p.split_fwd ? 3 : A.cin[d.l0], 8), cdiv(C1, 32)), lb(cdiv(C1, 8), cdiv(C2, 32))),
                                cdiv(C2, 8)) + PSG_LDS_SPARE;
    p.packed_fwd = p.packed && KS == 32 && d.maxt_f == 1 && p.split_fwd == (lvl >= 1) && nb3 * PB == 2 * NW &&
                   blocks * blk + 2 * P <= (P - 1) * C3 && (P * C3) % blk == 0 && (row.v & (p.split_fwd ? V_PACK : V_PACK0));
    p.w1c = sw.l1t_colour && lvl == 0 && !p.split_bwd && P == 32 * NW && (C1 == 16 || C1 == 32);
    // Max-pool transpose as a sparse weight-row stream where the level's shapes fit it: SSG levels 1 - 3, whose third layers
    // the model also keeps as plain rows (sa1: C2 = 32 is half a wave's lanes; MSG: KS = 16 and C2 = 96 / 196 / 384)
    const bool wr = A.id == PSG_PN2_ARCH_SSG && lvl >= 1;
    p.spv = sw.poolt_sparse && wr && KS == 32 && P <= 64 && (P / KS) * C3 <= NT && C3 % 64 == 0 && (C2 == 64 || C2 == 128 || C2 == 256)
                ? C2 / 64 : 0;
    // Packed backward: the level named by PSG_PN2_PACK_BWD and the plan's descriptors; by default also the configuration the
    // kernel is built for, SSG as shipped (`fits`: level 0 whole under a split level 1; levels 1 - 3 split both ways with the
    // sparse stream and a split level above, or level 3's nninv gather).  Any other keeps the unpacked backward.
    const bool named = p.packed && ((sw.pack_bwd >> lvl) & 1), by_name = (sw.pack_bwd >> 8) != 0;
    const bool fits = lvl == 0 ? !p.split_fwd && !p.split_bwd && split_at(1)
                               : p.split_fwd && p.split_bwd && (lvl == 3 || split_at(lvl + 1)) && p.spv > 0;
    if (!named || !(by_name || fits)) return p;
    p.packed_keys = p.packed_fwd;
    if (!p.packed_fwd) p.fwd_error = "the packed backward (PSG_PN2_PACK_BWD) needs the packed forward, which this configuration does not run";
    // the pooled-output gradient must be plain rows (the split level above sums them per point) or, for the sparse form, level
    // 3's nninv gather of fp4's interpolated-part rows - not the inverse group lists of an unsplit level above
    const bool rows = lvl < 3 && split_at(lvl + 1);
    const bool dense0 = !p.spv && !p.split_bwd && rows && !((A.C[lvl + 1] | d.c_off) & 3) && !(C3 & 7) && (row.v & V_PACK0) && d.maxt_b == 1;
    // sparse: G * C3 == NT (a batch of the packed kernel is one unpacked workgroup's pass), one tile per wave in l3t, l2t and
    // the mask pass.  Channel order where the gradient is plain rows and the row has the kernel (levels 1 and 2).
    const bool sparse = p.spv && p.split_bwd && p.split_fwd && (rows || lvl == 3) && (P / KS) * C3 == NT &&
                        std::max(cdiv(C2, 32), cdiv(C1, 32)) * PB <= NW && (row.v & V_PACK) && row.spv == p.spv;
    if (dense0) p.packed_bwd = SaPath::dense0;
    else if (sparse) p.packed_bwd = (row.v & V_CHAN) && rows && sw.poolt_chan ? SaPath::chan : SaPath::sparse;
    else p.bwd_error = "PSG_PN2_PACK_BWD names a level without a packed backward kernel in this configuration";
    return p;
}

// The kernel family of a launch.  `colour`: a colour-only request (compact rows at level 0), which alone may run sa_l1t_colour.
inline SaKernel sa_fwd_family(const SaPath &p)
{
    if (p.fwd_error) return SaKernel::error;
    if (p.packed_fwd) return p.packed_keys ? SaKernel::fwd_packed_keys : SaKernel::fwd_packed;
    return p.split_fwd ? SaKernel::fwd_split : SaKernel::fwd_whole;
}
inline bool sa_w1c(const SaPath &p, bool colour) { return p.w1c && colour; }
inline int sa_spv(const SaPath &p, bool colour) { return sa_w1c(p, colour) ? 0 : p.spv; }   // (level 0 never streams: spv is 0 there)
inline SaKernel sa_bwd_family(const SaPath &p, bool colour)
{
    if (p.bwd_error) return SaKernel::error;
    if (p.packed_bwd) return (SaKernel)((int)SaKernel::bwd_packed_dense0 + p.packed_bwd - SaPath::dense0);   // (same order)
    return sa_spv(p, colour) ? SaKernel::bwd_sparse : SaKernel::bwd_dense;
}
// The "#variant" of a launch's trace site: "#<row>" and the family, in the suffixes the GPU tests key on (#packed,
// #bwd#packed, #colour, #saN, #chan#saN); %d = lvl + 1, %s = "#colour" where sa_l1t_colour runs (SaKernel order).
struct SaSite { char text[64]; };
inline SaSite sa_site(const SaCfg &r, SaKernel k, int lvl, bool w1c, bool traced = true)
{
    if (!traced) return SaSite{{0}};      // (nobody reads it)
    static const char *const tail[] = {"#whole", "#split", "#packed", "#keys#packed", "#dense%s", "#sparse", "%s#bwd#packed",
                                       "#sa%d#bwd#packed", "#chan#sa%d#bwd#packed", "#error"};
    SaSite s;
    const int n = snprintf(s.text, sizeof s.text, "#p%dw%dk%df%db%d", r.P, r.NW, r.K, r.maxt_f, r.maxt_b);
    if (k == SaKernel::bwd_packed_sparse || k == SaKernel::bwd_packed_chan) snprintf(s.text + n, sizeof s.text - n, tail[(int)k], lvl + 1);
    else snprintf(s.text + n, sizeof s.text - n, tail[(int)k], w1c ? "#colour" : "");
    return s;
}

}  // namespace psg_pn2
