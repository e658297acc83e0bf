// Host side of the PointNet++ sem-seg networks on gfx950: weight packing, workspace layout, geometry plan, forward,
// input-gradient backward and the fused NB attack loop, driven by an architecture descriptor (SSG or MSG).
// Everything is stream-ordered; nothing here synchronises the device except psg_pn2_model_create* (upload).
//
// SSG (PointNet/models/pointnet2_sem_seg.py:9-19 of the reference):
//   sa1 (1024, r .1, 32, 12 ->32,32,64)    sa2 (256, .2, 32, 67 ->64,64,128)
//   sa3 (64, .4, 32, 131->128,128,256)     sa4 (16, .8, 32, 259->256,256,512)
//   fp4 768->256,256   fp3 384->256,256    fp2 320->256,128    fp1 128->128,128,128
//   conv1 128->128 (+bn1, ReLU, eval dropout = id), conv2 128->13, log_softmax
// MSG (PointNet/models/pointnet2_sem_seg_msg.py:10-21): every SA level runs two radii on one FPS sample and
// concatenates their pooled outputs (pointnet_util.py:210-267):
//   sa1 (1024, r .05/.1, K 16/32, 12 ->16,16,32 | 32,32,64)      sa2 (256, .1/.2, 99 ->64,64,128 | 64,96,128)
//   sa3 (64, .2/.4, 259->128,196,256 | 128,196,256)             sa4 (16, .4/.8, 515->256,256,512 | 256,384,512)
//   fp4 1536->256,256   fp3 512->256,256   fp2 352->256,128    fp1 128->128,128,128, same head
#include <algorithm>
#include <cstring>
#include <vector>

#include "psg_common.h"
#include "psg_pn2_paths.h"
#include "psg_pn2_kernels.cuh"
#include "psg_chain.cuh"
#include "psg_pn2_geomgrad.cuh"

using namespace psg;
using namespace psg_pn2;

namespace {

const Pn2Switches &sw()     // the process-wide switches, read once (psg_pn2_paths.h: Pn2Switches documents each)
{
    static const Pn2Switches s = read_switches(psg::env_int, psg::env_str);
    return s;
}
static inline int diag_build_bits() { return sw().diag; }

// What SA level lvl, scale sc of an architecture runs in this process (psg_pn2_paths.h: sa_path), computed once.  The model,
// the workspace layout, the plan and both launch functions read THIS: forward and backward cannot disagree.
const SaPath &sa_path_of(const ArchDesc &A, int lvl, int sc)
{
    static const std::vector<SaPath> t = [] {
        std::vector<SaPath> t(16);       // [arch][level][scale]
        for (int i = 0; i < 16; ++i)
            if ((i & 1) < arch_of(i >> 3).ns) t[i] = sa_path(arch_of(i >> 3), sw(), (i >> 1) & 3, i & 1);
        return t;
    }();
    return t[(A.id == PSG_PN2_ARCH_MSG ? 8 : 0) + lvl * 2 + sc];
}
inline bool arch_split(const ArchDesc &A, int lvl) { return sa_path_of(A, lvl, 0).split_bwd; }       // (both scales of a level alike)
inline bool arch_split_fwd(const ArchDesc &A, int lvl) { return sa_path_of(A, lvl, 0).split_fwd; }
inline bool arch_fp_split(const ArchDesc &, int lvl) { return fp_split(sw(), lvl); }
inline bool arch_pack(const ArchDesc &A) { return sa_path_of(A, 0, 0).packed; }

struct PackedLayer {
    float4 *wf = nullptr;  // forward packing  [mb(cout)][k8(cin)][64]
    float4 *wb = nullptr;  // transposed packing [mb(cin)][k8(cout)][64]
    float *bias = nullptr; // [mb(cout)*32]
    float4 *wf4 = nullptr; // forward packing, k8-major [k8][mb = 4][64] (wave-private chain kernels, psg_chain.cuh)
    float4 *wb4 = nullptr; // transposed packing, k8-major
    float *wr = nullptr;   // plain rows [cout][cin]: the third layers of the SSG SA levels 1 - 3 (sa_pool_t_sparse)
    int cin = 0, cout = 0;
    // K is padded to a multiple of 8 only (tile_mac runs a tail of 1..3 chunks behind its 4-chunk pipeline)
    int k8f() const { return ceil_div(cin, 8); }
    int mbf() const { return ceil_div(cout, 32); }
    int k8b() const { return ceil_div(cout, 8); }
    int mbb() const { return ceil_div(cin, 32); }
};

}  // namespace

struct psg_pn2_model {
    uint64_t gen = psg::next_generation();   // never re-used (psg_common.h): what replayed graphs are keyed on
    psg_ctx *ctx;
    const ArchDesc *arch;
    PackedLayer L[MAXL];
    // split first layers (arch_split): sx = the xyz columns [C1 x 3] (forward packing only), sf = the feature columns
    // [C1 x D] with the layer's bias (forward packing for the per-point product, transposed packing for its gradient)
    PackedLayer sx[4][2], sf[4][2];                      // [level][scale]
    bool split[4] = {false, false, false, false};        // forward and backward split (levels 1-3)
    bool split_fwd[4] = {false, false, false, false};    // forward split (the above, + level 0 under PSG_PN2_SPLIT=2)
    float *w0f = nullptr, *b0f = nullptr;                 // level 0 forward split: W1f [32][9] row-major, b1 [32]
    // split FP first layers (arch_fp_split), by FP level: fa = the skip columns [cout x C1] (forward and transposed packing,
    // the layer's own bias), fb = the interpolated-part columns [cout x C2] (forward packing = one more layer of the COARSER
    // module's forward, transposed packing = one more layer at the front of its backward; zero bias)
    PackedLayer fa[3], fb[3];
    bool fsplit[3] = {false, false, false};
    float *w1feat[2] = {nullptr, nullptr};               // level 0, per scale: the first layer's feature columns as plain rows [C1][9] (sa_l1t_colour)
    float *w1x[4] = {nullptr, nullptr, nullptr, nullptr}; // SSG split levels: the first layer's xyz columns as plain rows [3][C1] (sa_grel_kernel)
    void *arena = nullptr;
};

struct psg_pn2_ws {
    uint64_t gen = psg::next_generation();
    psg_ctx *ctx;
    const ArchDesc *arch;
    int B, N, F;          // batch, points per room, max forwards in the plan
    int Nl[5];            // points at level 0..4
    void *arena = nullptr;
    size_t bytes = 0;
    // plan (per-scale tables are indexed [level][scale]; an SSG level has one scale)
    float *xyz0;          // [B][N][3]
    int32_t *fps[4];      // [F*B][S_l]
    float *xyz[5];        // xyz[l+1]: [F*B][S_l][3]; xyz[0] = xyz0
    int32_t *gidx[4][2];  // [F*B][S_l][K]
    int32_t *pk_cnt[4];   // packed SA forward (arch_pack): [F*B][S_l] valid rows of each group
    int32_t *pk_seg[4];   // [F*B][S_l / G_l + 2] workgroup segmentation (psg_pn2_kernels.cuh: sa_pack_plan_kernel)
    int4 *pk_desc[4];     // [F*B][S_l / G_l] what the packed kernel's workgroups read: one descriptor each
    int32_t *ball0[2];    // per level-0 scale: [B][N][K] the room's ball query with every point as centroid, or null (ball_table_route)
    int32_t *nn_idx[4];   // [F*B][N_l][3]
    float *nn_w[4];
    int32_t *inv_off[4];  // inverse 3-NN lists (CSR by coarse point): [F*B][S_l + 1]
    int2 *inv_ent[4];     // [F*B][3*N_l] {fine point, weight bits}, ascending fine point inside a list
    float *dint[4];       // [B][N_l][C2_l] interpolated-part gradient rows of fp_bwd level l
    int32_t *ginv_off[4][2]; // inverse group lists (CSR by source point, lists sorted by grouped row): [F*B][N_l + 1]
    int32_t *ginv_pos[4][2]; // [F*B][S_l*K] inverse permutation: slot of a grouped row in the concatenated lists
    float *gsa[4][2];     // [B][S_l*K][CG_l] grouped-input gradient rows of sa_bwd level l (CG = 12, then C[l]; split levels: dZ1 rows, C1)
    const float *x0_fwd = nullptr;   // the input rows of the forward in progress (level 0 forward split)
    float *tfeat[4][2];   // split levels, per scale: [B][N_l][C1] per-point first-layer products of the resident forward
    float *dsum[4];       // dsum[l], l = 0..2, when level l + 1 is split: [B][S_l][C_{l+1}] complete gradient of level l's pooled output
    float *tfp[3];        // FP level l split: [B][N_{l+1}][cout1_l] = (coarser module's output) . W1b^T of the resident forward
    int planned = 0;
    // activations of one forward
    float *act[7];        // l1..l4, fp4 out (64 pts), fp3 out (256), fp2 out (1024)
    int actC[7];
    uint8_t *arg[4][2];
    uint16_t *mask[MAXL];
    float *logp, *dlogp;
    // gradients (every buffer has exactly one writer: nothing is zeroed or accumulated into)
    float *dact[7];
    float *dx0;           // [B][N][9]
    // coordinate gradient (psg_pn2_backward_full, SSG): g_rel rows of the split SA levels, dL/dd of the FP levels' three
    // neighbours, and the coordinate gradient of the points of levels 1 - 4
    float4 *grel[4];      // [B][S_l*K] list order (levels 1 - 3)
    float4 *fpg[4];       // [B][N_l]
    float *gxyz[5];       // [B][N_l][3] (levels 1 - 4)
    // attack state
    float *x0, *ori;      // [B][N][9], [B][N][3]
    unsigned long long *dbg;  // diagnostics scratch (diagnostic builds, bit 256), 4 words per workgroup
    int fwd_slot = -1;
    // hipGraph of a whole NB attack (geometry plan + every iteration) on the workspace's own buffers: the caller's labels,
    // FPS starts and mask are copied in first, so that the captured kernels' arguments never change between calls
    int32_t *nb_labels;       // [B][N]
    int32_t *nb_starts;       // [F][4][B]
    uint8_t *nb_mask;         // [N]
    psg::GraphSlot nb;
    struct NbKey { uint64_t model_gen; float eps, alpha; int iters, targeted, target, has_mask, has_labels, pad; } nb_key{};   // (no padding bytes: compared with memcmp)
    bool nb_have_key = false;
    // the graph is captured and replayed on a non-blocking stream of the workspace, fenced against the caller's stream with two
    // events: the reference's harness calls from the legacy default stream, which cannot capture
    hipStream_t nb_stream = nullptr;
    hipEvent_t nb_ev[2] = {nullptr, nullptr};
    // attack loops: module outputs nobody reads are not written (fp2 - fp4 under the FP split: the finer module gathers T rows)
    bool lean = false;        // (set and cleared by psg::pn2_forward_lean only)
    psg::EvLog prof;          // optional per-launch HIP-event timing (psg_pn2_prof_enable); off in normal operation
};

namespace psg {
uint64_t pn2_model_generation(const psg_pn2_model *m) { return m ? m->gen : 0; }
uint64_t pn2_ws_generation(const psg_pn2_ws *ws) { return ws ? ws->gen : 0; }
}  // namespace psg

namespace {

// `perm` maps the packed (LDS-order) input-channel index to the reference's column: LDS order of an SA
// module's grouped input is [feats(D), rel_xyz(3)], the reference concatenates [rel_xyz, feats].
std::vector<int> sa_input_perm(int cin)
{
    std::vector<int> perm(cin);
    const int D = cin - 3;
    for (int c = 0; c < cin; ++c) perm[c] = c < D ? 3 + c : c - D;
    return perm;
}

std::vector<float> pack_fwd(const float *w, int cin, int cout, const std::vector<int> *perm)
{
    const int k8 = ceil_div(cin, 8), mb = ceil_div(cout, 32);
    std::vector<float> out(((size_t)mb * k8 + 4) * 64 * 4, 0.0f);  // + 4 chunks: prefetch over-read slack
    for (int m = 0; m < mb; ++m)
        for (int k = 0; k < k8; ++k)
            for (int lane = 0; lane < 64; ++lane)
                for (int t = 0; t < 4; ++t) {
                    int o = m * 32 + (lane & 31), c = 8 * k + 4 * (lane >> 5) + t;
                    if (o < cout && c < cin)
                        out[(((size_t)m * k8 + k) * 64 + lane) * 4 + t] = w[(size_t)o * cin + (perm ? (*perm)[c] : c)];
                }
    return out;
}

std::vector<float> pack_bwd(const float *w, int cin, int cout, const std::vector<int> *perm)
{
    const int k8 = ceil_div(cout, 8), mb = ceil_div(cin, 32);
    std::vector<float> out(((size_t)mb * k8 + 4) * 64 * 4, 0.0f);  // + 4 chunks: prefetch over-read slack
    for (int m = 0; m < mb; ++m)
        for (int k = 0; k < k8; ++k)
            for (int lane = 0; lane < 64; ++lane)
                for (int t = 0; t < 4; ++t) {
                    int c = m * 32 + (lane & 31), o = 8 * k + 4 * (lane >> 5) + t;
                    if (o < cout && c < cin)
                        out[(((size_t)m * k8 + k) * 64 + lane) * 4 + t] = w[(size_t)o * cin + (perm ? (*perm)[c] : c)];
                }
    return out;
}

// [mb][k8][64] float4 -> [k8_pad][mb][64] float4 (one k8-step of all four 32-row blocks contiguous), k8 zero-padded up to
// k8_pad chunks (the wave-private chain kernels want multiples of 4 on their backward side)
std::vector<float> k8_major_padded(const std::vector<float> &packed, int mb, int k8, int k8_pad)
{
    std::vector<float> out((size_t)mb * k8_pad * 256, 0.0f);
    for (int m = 0; m < mb; ++m)
        for (int k = 0; k < k8; ++k)
            std::copy(packed.begin() + ((size_t)m * k8 + k) * 256, packed.begin() + ((size_t)m * k8 + k + 1) * 256,
                      out.begin() + ((size_t)k * mb + m) * 256);
    return out;
}

FwdLayer fwd_layer(const PackedLayer &p, bool relu, uint16_t *mask)
{
    FwdLayer f;
    f.w = p.wf; f.bias = p.bias; f.mask = mask; f.k8 = p.k8f(); f.mb = p.mbf(); f.relu = relu ? 1 : 0;
    return f;
}
BwdLayer bwd_layer(const PackedLayer &p, const uint16_t *mask)
{
    BwdLayer f;
    f.w = p.wb; f.mask = mask; f.k8 = p.k8b(); f.mb = p.mbb();
    return f;
}

// kernel tags of the per-launch profile (psg_pn2_prof_read)
enum { TAG_SA_FWD = 0, TAG_FP_FWD = 4, TAG_FP_BWD = 8, TAG_SA_BWD = 12, TAG_FPS = 16, TAG_BALL = 17, TAG_NN = 18,
       TAG_GATHER = 19, TAG_CE = 20, TAG_PGD = 21, TAG_ZERO = 22, TAG_PW_FWD = 23, TAG_PW_BWD = 24,
       TAG_GEOM_GREL = 25, TAG_GEOM_WGRAD = 26, TAG_GEOM_GX = 27, TAG_PACK_PLAN = 28, TAG_FP1_LOOP = 29,
       TAG_COUNT = 30 };   // 25-27: psg_pn2_backward_full only; 29: the NB loop's fp1 + head forward, CE and backward in one launch

// Every launch with a dynamic LDS buffer of `blocks8` blocks of `blk` floats goes through here: size check, the shared LDS
// opt-in above 48 KiB, the profile scope and the launch check.  `site` is the CALLER's launch site (PSG_SITE, psg_common.h);
// a launch line that serves several kernels passes the "#variant" chosen at run time, appended when the tracer is on.
template <typename KernelT, typename ArgsT>
int launch_lds(psg_pn2_ws *ws, int tag, const char *site, KernelT kern, dim3 grid, int threads, int blocks8, int blk,
               const ArgsT &args, hipStream_t st, const char *variant = nullptr)
{
    size_t lds = (size_t)blocks8 * blk * sizeof(float);
    if (lds > 160 * 1024) { set_error("LDS request %zu exceeds 160 KiB", lds); return PSG_ERR_ARG; }
    if (lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)kern));
    EvScope prof(&ws->prof, tag, 0.0, st);
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, st, args);
    char full[192];
    if (variant && psg::trace_sync_enabled()) site = (snprintf(full, sizeof full, "%s%s", site, variant), full);
    PSG_LAUNCH_CHECK_AT(site);
    return PSG_OK;
}

inline int layer_blocks(int k8, int mb) { return std::max(k8, mb * 4); }
inline int gsa_stride(const ArchDesc &A, int lvl)
{
    if (arch_split(A, lvl)) return A.cout[A.sc[lvl][0].l0];     // dZ1 rows: the first layer's width
    return lvl == 0 ? 12 : A.C[lvl];
}

// Calls f(Row{}) for row `row` of the kernel table: a compare chain over the type list (psg_pn2_paths.h: SaRows)
template <class F, class... R> int sa_visit(SaRowList<R...>, int row, F &&f)
{
    int rc = PSG_ERR_STATE, i = 0;
    (void)((i++ == row ? (rc = f(R{}), true) : false) || ...);
    return rc;
}

// An SA module's two launches: the kernel FAMILY from the level's path (sa_path_of), the template arguments from the scale's row;
// `if constexpr` on the row's flags keeps the instantiations to what the table names.  Site: the launch line + sa_site's variant.
int run_sa_fwd(psg_pn2_model *m, psg_pn2_ws *ws, int lvl, int sc, int fwd, const float *x0, hipStream_t st)
{
    const ArchDesc &A = *m->arch;
    const ScaleDesc &d = A.sc[lvl][sc];
    const SaPath &path = sa_path_of(A, lvl, sc);
    const int B = ws->B, S = kS[lvl], Np = ws->Nl[lvl], D = A.C[lvl], KS = d.K, P = d.P, NW = d.NW;
    const PackedLayer *L = &m->L[d.l0];
    const size_t prob = (size_t)fwd * B;
    SaFwdArgs a;
    a.diag = diag_build_bits();
    a.xyz = lvl == 0 ? x0 : ws->xyz[lvl] + prob * Np * 3;
    a.xyz_stride = lvl == 0 ? 9 : 3;
    a.feat = lvl == 0 ? x0 : ws->act[lvl - 1];
    a.new_xyz = ws->xyz[lvl + 1] + prob * S * 3;
    a.gidx = ws->gidx[lvl][sc] + prob * S * KS;
    a.out = ws->act[lvl];
    a.ld_out = A.C[lvl + 1];
    a.c_out = d.c_off;
    a.arg = ws->arg[lvl][sc];
    const bool split = path.split_fwd;
    a.l1 = fwd_layer(split ? m->sx[lvl][sc] : L[0], true, ws->mask[d.l0]);
    a.l2 = fwd_layer(L[1], true, ws->mask[d.l0 + 1]);
    a.w3 = L[2].wf; a.b3 = L[2].bias; a.k8_3 = L[2].k8f(); a.nb3 = L[2].mbf();
    a.D = D; a.Np = Np; a.S = S; a.C3 = L[2].cout;
    a.tfeat = split ? ws->tfeat[lvl][sc] : nullptr;
    a.ldt = split ? L[0].cout : 0;
    // one in-place activation buffer: the widest of the layers' K / M extents (psg_mlp.cuh)
    const int blocks = std::max(std::max(layer_blocks(a.l1.k8, a.l1.mb), layer_blocks(a.l2.k8, a.l2.mb)), a.k8_3) + PSG_LDS_SPARE;
    if (a.l1.mb * (P / 32) > d.maxt_f * NW || a.l2.mb * (P / 32) > d.maxt_f * NW || a.nb3 * (P / 32) > 2 * NW) {
        set_error("run_sa_fwd level %d scale %d: more tiles than waves in a layer", lvl, sc);
        return PSG_ERR_STATE;
    }
    const dim3 grid(S / (P / KS), B);
    const int tag = TAG_SA_FWD + lvl;
    const SaKernel fam = sa_fwd_family(path);
    if (fam == SaKernel::error) { set_error("run_sa_fwd level %d: %s", lvl, path.fwd_error); return PSG_ERR_STATE; }
    // packed rows: the [P][C3] pool rows over the activation buffer, the row maps behind the buffer
    const int blk = P * 8 + PSG_LDS_PAD;                           // Lds<P>::BLK
    a.pk_desc = path.packed_fwd ? ws->pk_desc[lvl] + prob * grid.x : nullptr;
    a.pk_tab_off = path.packed_fwd ? blocks * blk : 0;
    const int lds_blocks = path.packed_fwd ? P * a.C3 / blk : blocks;
    const SaSite site = sa_site(SaRows::cfg[d.row], fam, lvl, false, psg::trace_sync_enabled());
    return sa_visit(SaRows{}, d.row, [&](auto row) -> int {
        using R = decltype(row);
        auto go = [&](auto kern) { return launch_lds(ws, tag, PSG_SITE, kern, grid, R::NW * 64, lds_blocks, Lds<R::P>::BLK, a, st, site.text); };
        if constexpr ((R::V & (V_PACK0 | V_PACK)) != 0) {
            if (fam == SaKernel::fwd_packed_keys) return go(sa_fwd_packed_kernel<R::P, R::NW, (R::V & V_PACK) != 0, true>);
            if (fam == SaKernel::fwd_packed) return go(sa_fwd_packed_kernel<R::P, R::NW, (R::V & V_PACK) != 0>);
        }
        if constexpr ((R::V & V_SPLIT) != 0)
            if (fam == SaKernel::fwd_split) return go(sa_fwd_kernel<R::P, R::NW, R::K, R::MF, true>);
        if (fam == SaKernel::fwd_whole) return go(sa_fwd_kernel<R::P, R::NW, R::K, R::MF>);
        set_error("run_sa_fwd: no split kernel for P=%d NW=%d K=%d MAXT=%d", R::P, R::NW, R::K, R::MF);
        return PSG_ERR_STATE;
    });
}

int run_sa_bwd(psg_pn2_model *m, psg_pn2_ws *ws, int lvl, int sc, int fwd, int c_lo, int c_hi, hipStream_t st)
{
    const ArchDesc &A = *m->arch;
    const ScaleDesc &d = A.sc[lvl][sc];
    const SaPath &path = sa_path_of(A, lvl, sc);
    const int B = ws->B, S = kS[lvl], Np = ws->Nl[lvl], D = A.C[lvl], KS = d.K, P = d.P, NW = d.NW;
    const PackedLayer *L = &m->L[d.l0];
    const size_t prob = (size_t)fwd * B;
    SaBwdArgs a{};            // (no nninv gather, no inverse group lists unless set below)
    a.diag = diag_build_bits();
    a.ld = A.C[lvl + 1];
    a.c_off = d.c_off;
    a.dout = ws->dact[lvl];   // skip-link gradient rows written by fp_bwd level lvl + 1
    if (lvl < 3 && m->split[lvl + 1]) {
        a.dout = ws->dsum[lvl];   // skip-link rows + the transposed grouping of level lvl + 1, summed per point by pw_bwd_kernel
    } else if (lvl < 3) {   // plus the transposed grouping of SA level lvl + 1, gathered through its inverse lists
        a.g_rows = kS[lvl + 1] * A.sc[lvl + 1][0].K;
        a.ginv_off = ws->ginv_off[lvl + 1][0] + prob * (S + 1);
        a.gsa = ws->gsa[lvl + 1][0];
        if (A.ns > 1) {
            a.g_rows2 = kS[lvl + 1] * A.sc[lvl + 1][1].K;
            a.ginv_off2 = ws->ginv_off[lvl + 1][1] + prob * (S + 1);
            a.gsa2 = ws->gsa[lvl + 1][1];
        }
    }
    const int C3 = L[2].cout;
    if (P * (C3 / 8) > 4 * NW * 64) {   // sa_bwd_kernel pre-loads at most 4 arg-max tasks per thread
        set_error("run_sa_bwd level %d scale %d: %d max-pool tasks exceed 4 per thread", lvl, sc, P * (C3 / 8));
        return PSG_ERR_STATE;
    }
    const bool colour = lvl == 0 && c_hi - c_lo == 3;   // colour-only: compact float4 rows
    a.gsa_out = ws->gsa[lvl][sc];
    a.gpos_out = ws->ginv_pos[lvl][sc] + prob * S * KS;
    a.cg_out = colour ? 4 : gsa_stride(A, lvl);
    a.split = path.split_bwd ? 1 : 0;
    if (a.split) { c_lo = 0; c_hi = L[0].cout; }   // the rows stored are dZ1 [C1]
    if (lvl == 3) {   // l4_points feed only fp4: its gradient is gathered from fp4's interpolated-part rows
        a.dout = nullptr;
        a.nninv_off = ws->inv_off[3] + prob * (kS[3] + 1);
        a.nninv_ent = ws->inv_ent[3] + prob * ws->Nl[3] * 3;
        a.dint = ws->dint[3];
        a.n_fine = ws->Nl[3];
    }
    a.arg = ws->arg[lvl][sc];
    a.gidx = ws->gidx[lvl][sc] + prob * S * KS;
    a.l3t = bwd_layer(L[2], ws->mask[d.l0 + 1]);
    a.l2t = bwd_layer(L[1], ws->mask[d.l0]);
    a.l1t = bwd_layer(L[0], nullptr);
    a.D = D; a.Np = Np; a.S = S; a.C3 = C3;
    a.c_lo = c_lo; a.c_hi = c_hi;
    // colour-only request at level 0: three of the first layer's columns on the vector pipe (psg_pn2_kernels.cuh: sa_l1t_colour)
    a.w1c = sa_w1c(path, colour) ? m->w1feat[sc] : nullptr;
    a.C1 = L[0].cout;
    // max-pool transpose as a sparse weight-row stream (SaPath::spv).  The sparse pass needs no dZ3 tile: the buffer is sized
    // without l3t's K.
    const int C2 = L[2].cin, NT = NW * 64;
    const int spv = sa_spv(path, colour);
    const int l3_blocks = spv ? a.l3t.mb * 4 : layer_blocks(a.l3t.k8, a.l3t.mb);
    const int main_blocks = std::max(std::max(l3_blocks, layer_blocks(a.l2t.k8, a.l2t.mb)),
                                     a.split ? 0 : layer_blocks(a.l1t.k8, a.l1t.mb)) + PSG_LDS_SPARE;
    a.dsrc_blk = main_blocks;   // the gathered pooled-output gradient is staged behind the activation buffer
    const int blk_floats = P * 8 + PSG_LDS_PAD;
    a.w1c_off = round_up((P / KS) * C3, 4);
    a.pos_off = a.w1c_off + (a.w1c ? round_up(3 * a.C1, 4) : 0);
    // sparse: item list [NT] int2, count / offset table [NW][32], row starts [P + 1]
    a.sp_off = round_up(a.pos_off + P, 4);
    a.w3r = spv ? L[2].wr : nullptr;
    const SaKernel fam = sa_bwd_family(path, colour);
    if (fam == SaKernel::error) { set_error("run_sa_bwd level %d: %s", lvl, path.bwd_error); return PSG_ERR_STATE; }
    // packed backward: the same packed rows as the level's forward, masks at the packed key.  Its row map [P] lies behind the
    // output slots; levels 1 - 3: the first packed row of each group [SA_PACK_GCAP + 1] lies behind the sparse pass's row starts.
    const bool packed = path.packed_bwd != SaPath::none;
    const int staged = spv ? a.sp_off + 2 * NT + NW * 32 + P + 1 + (packed ? SA_PACK_GCAP + 1 : 0) : a.pos_off + P + (packed ? P : 0);
    const int blocks = main_blocks + ceil_div(staged, blk_floats);
    if (std::max(std::max(a.l3t.mb, a.l2t.mb), a.split ? 0 : a.l1t.mb) * (P / 32) > d.maxt_b * NW) {
        set_error("run_sa_bwd level %d scale %d: more than %d tiles per wave in a layer", lvl, sc, d.maxt_b);
        return PSG_ERR_STATE;
    }
    const dim3 grid(S / (P / KS), B);
    const int tag = TAG_SA_BWD + lvl;
    const SaBwdPackedArgs pa{a, packed ? ws->pk_desc[lvl] + prob * grid.x : nullptr};
    const SaSite site = sa_site(SaRows::cfg[d.row], fam, lvl, a.w1c != nullptr, psg::trace_sync_enabled());
    return sa_visit(SaRows{}, d.row, [&](auto row) -> int {
        using R = decltype(row);
        auto go = [&](auto kern, const auto &args) { return launch_lds(ws, tag, PSG_SITE, kern, grid, R::NW * 64, blocks, Lds<R::P>::BLK, args, st, site.text); };
        if constexpr ((R::V & V_CHAN) != 0)
            if (fam == SaKernel::bwd_packed_chan) return go(sa_bwd_packed_kernel<R::P, R::NW, 1, R::SPV + SA_PACK_CHAN>, pa);
        if constexpr ((R::V & (V_PACK0 | V_PACK)) != 0)
            if (fam == SaKernel::bwd_packed_dense0 || fam == SaKernel::bwd_packed_sparse) return go(sa_bwd_packed_kernel<R::P, R::NW, 1, R::SPV>, pa);
        if constexpr (R::SPV != 0)
            if (fam == SaKernel::bwd_sparse && spv == R::SPV) return go(sa_bwd_sparse_kernel<R::P, R::NW, R::MB, R::SPV>, a);
        if (fam == SaKernel::bwd_dense) return go(sa_bwd_kernel<R::P, R::NW, R::MB, R::K>, a);
        set_error("run_sa_bwd: no sparse kernel for P=%d NW=%d MAXT=%d C2=%d", R::P, R::NW, R::MB, C2);
        return PSG_ERR_STATE;
    });
}

// FP module `LVL` (0 = fp1 ... 3 = fp4) upsamples level LVL+1 -> level LVL.
// activation slots: act[0..3] = l1..l4 (SA outputs); act[4] = fp4 out (level 3), act[5] = fp3 out
// (level 2), act[6] = fp2 out (level 1)
inline int fp_out_slot(int lvl) { return 7 - lvl; }          // lvl 3 -> 4, 2 -> 5, 1 -> 6
inline int fp_in2_slot(int lvl) { return lvl == 3 ? 3 : fp_out_slot(lvl + 1); }
// P = points per workgroup.  fp1 + head runs 64 points (two point blocks) where the level's point count allows it, so that
// its 128-wide layers deal PAIRS of tiles on one weight stream (psg_mlp.cuh: tile_mac4x2, deal_pairs); fp2 - fp4 stay at 32
// (their backward's staged gather, fp_bwd_gather_rows, is written for one point block).  Forward and backward must agree on
// P: it decides the ReLU mask layout; both take it from the level's point count.
template <int LVL> struct FpCfg { static constexpr int P = 32, P2 = 32, NW = 8; };
template <> struct FpCfg<0> { static constexpr int P = 32, P2 = PSG_MLP_PAIRS ? 64 : 32, NW = 4; };

// level 0 forward split (PSG_PN2_SPLIT=2): T0[n][c] = b1[c] + sum_k W1f[c][k] x0[n][k], one thread per (point, 4 channels)
__global__ void pw9_fwd_kernel(const float *__restrict__ x0, const float *__restrict__ w, const float *__restrict__ bias, size_t rows,
                               float *__restrict__ out)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * 8) return;
    const size_t n = t >> 3;
    const int c0 = (int)(t & 7) * 4;
    float x[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = x0[n * 9 + k];
    float r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float acc = bias[c0 + u];
#pragma unroll
        for (int k = 0; k < 9; ++k) acc = fmaf(w[(c0 + u) * 9 + k], x[k], acc);
        r[u] = acc;
    }
    *(float4 *)(out + n * 32 + c0) = make_float4(r[0], r[1], r[2], r[3]);
}

// Level-0 ball query of a plan (psg_pn2_plan_build).  A plan of n_forward forwards queries n_forward x 1024 centroids per room,
// every one of them a point of the room; the table route queries each of the room's N points once and copies rows
// (group_from_table_kernel).  It is taken when the plan asks for at least BALL_TABLE_C x N centroids per room: the colour
// attacks' plans (40 forwards: 40 960 against 4 096; the NU plans: 10 or 11 forwards), not a one-forward evaluation plan, and
// not the coordinate attacks, which rebuild a one-forward plan whenever xyz moves (the table would be built for 1024 rows).
// Pn2Switches::ball_table = 0 / 2 forces the direct query / the table.
constexpr int BALL_TABLE_C = 2;
static_assert(1 * 1024 < BALL_TABLE_C * 1024, "a one-forward plan stays on the direct route at every n_point a workspace accepts");
inline bool ball_table_route(int n_forward, int N)
{
    const int mode = sw().ball_table;
    if (mode == 0 || mode == 2) return mode == 2;
    return (long long)n_forward * kS[0] >= (long long)BALL_TABLE_C * N;
}

// Per-point side of a split SA level (arch_split): T = act[lvl - 1] . W1f^T + b1 for the Nl[lvl] points of every room, one
// launch of pw_fwd_kernel (psg_pn2_kernels.cuh): 2 waves per 32-point tile where the layer has 2 output blocks (level 1), else
// 4 waves and one workgroup per 4 output blocks (level 3, 8 blocks: two workgroups per tile, so that 64 rooms' 128 tiles
// cover the chip's 256 CUs).
int run_pw_fwd(psg_pn2_model *m, psg_pn2_ws *ws, int lvl, int sc, int fwd, hipStream_t st)
{
    constexpr int P = 32;
    const PackedLayer &F = m->sf[lvl][sc];
    const int B = ws->B, N = ws->Nl[lvl];
    if (lvl == 0) {
        EvScope prof(&ws->prof, TAG_PW_FWD, 0.0, st);
        const size_t rows = (size_t)B * N;
        hipLaunchKernelGGL(pw9_fwd_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, st, ws->x0_fwd, m->w0f, m->b0f, rows, ws->tfeat[0][0]);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    if (sw().pw_sized) {
        PwFwdArgs p;
        p.in = ws->act[lvl - 1]; p.out = ws->tfeat[lvl][sc];
        p.l = fwd_layer(F, false, nullptr);
        p.N = N; p.D = F.cin; p.C1 = F.cout;
        if (N % P || p.D % 8 || p.C1 % 32) { set_error("run_pw_fwd level %d: unsupported shape", lvl); return PSG_ERR_STATE; }
        if (p.l.mb <= 2) {
            const int blocks = layer_blocks(p.l.k8, 2) + PSG_LDS_SPARE;
            return launch_lds(ws, TAG_PW_FWD, PSG_SITE "#nw2", (pw_fwd_kernel<P, 2>), dim3(N / P, B, 1), 2 * 64, blocks, Lds<P>::BLK, p, st);
        }
        const int blocks = layer_blocks(p.l.k8, 4) + PSG_LDS_SPARE;
        return launch_lds(ws, TAG_PW_FWD, PSG_SITE "#nw4", (pw_fwd_kernel<P, 4>), dim3(N / P, B, ceil_div(p.l.mb, 4)), 4 * 64, blocks, Lds<P>::BLK, p, st);
    }
    constexpr int NW = 8;
    FpFwdArgs a;
    a.feat1 = ws->act[lvl - 1]; a.C1 = F.cin;
    a.feat2 = ws->act[lvl - 1]; a.C2 = 0;
    // (the kernel reads a point's three neighbour entries before it looks at C2: any valid table of N rows per room will do)
    a.nn_idx = ws->nn_idx[lvl] + (size_t)fwd * B * N * 3;
    a.nn_w = ws->nn_w[lvl] + (size_t)fwd * B * N * 3;
    a.N = N; a.S = N;
    a.layer[0] = fwd_layer(F, false, nullptr);
    a.n_layers = 1;
    a.out = ws->tfeat[lvl][sc]; a.Cout = F.cout; a.logp = nullptr; a.n_cls = 0;
    a.tsrc = nullptr; a.ldt = 0; a.out2 = nullptr; a.Cout2 = 0; a.extra = FwdLayer{};
    a.diag = 0; a.dbg = ws->dbg;
    if (a.layer[0].mb > NW || N % P) { set_error("run_pw_fwd level %d: unsupported shape", lvl); return PSG_ERR_STATE; }
    const int blocks = layer_blocks(a.layer[0].k8, a.layer[0].mb) + PSG_LDS_SPARE;
    return launch_lds(ws, TAG_PW_FWD, PSG_SITE, (fp_fwd_kernel<P, NW, false>), dim3(N / P, B), NW * 64, blocks, Lds<P>::BLK, a, st);
}

// dsum[lvl - 1] = dact[lvl - 1] (skip-link rows of the coarser FP module; level 3 feeds fp4 only: its skip part is that gather,
// done in sa_bwd) + (sum of the dZ1 rows of level lvl per source point) . W1f
// (MSG: the second scale of a level adds its product to what the first one wrote)
// Four waves where the transposed layer has at most four output tiles (SSG levels 1 and 2: D = 64 / 128), eight otherwise; a
// point's list is walked by one wave in list order whatever the wave count (pw_bwd_gather_rows), so the sums do not change.
int run_pw_bwd(psg_pn2_model *m, psg_pn2_ws *ws, int lvl, int sc, int fwd, hipStream_t st)
{
    constexpr int P = 32, NW = 8;
    const ArchDesc &A = *m->arch;
    const PackedLayer &F = m->sf[lvl][sc];
    const int B = ws->B, N = ws->Nl[lvl];
    PwBwdArgs a;
    a.ginv_off = ws->ginv_off[lvl][sc] + (size_t)fwd * B * (N + 1);
    a.gsa = ws->gsa[lvl][sc];
    a.g_rows = kS[lvl] * A.sc[lvl][sc].K;
    a.skip = sc == 0 ? ws->dact[lvl - 1] : ws->dsum[lvl - 1];
    a.out = ws->dsum[lvl - 1];
    a.wt = bwd_layer(F, nullptr);
    a.N = N; a.C1 = F.cout; a.D = F.cin;
    if ((a.C1 != 64 && a.C1 != 128 && a.C1 != 256) || a.wt.mb > 2 * NW || N % P || a.D % 32) {
        set_error("run_pw_bwd level %d: unsupported shape", lvl);
        return PSG_ERR_STATE;
    }
    if (sw().pw_sized && a.wt.mb <= 4) {    // (D <= 128: one float4 piece of a skip-link row per thread)
        const int blocks = layer_blocks(a.wt.k8, a.wt.mb) + PSG_LDS_SPARE;
        return launch_lds(ws, TAG_PW_BWD, PSG_SITE "#nw4", (pw_bwd_kernel<P, 4, 1, 1>), dim3(N / P, B), 4 * 64, blocks, Lds<P>::BLK, a, st);
    }
    const int blocks = layer_blocks(a.wt.k8, a.wt.mb) + PSG_LDS_SPARE;
    if (a.wt.mb > NW)       // MSG level 3: 512 feature channels = 16 output tiles on 8 waves
        return launch_lds(ws, TAG_PW_BWD, PSG_SITE, (pw_bwd_kernel<P, NW, 2>), dim3(N / P, B), NW * 64, blocks, Lds<P>::BLK, a, st);
    return launch_lds(ws, TAG_PW_BWD, PSG_SITE, (pw_bwd_kernel<P, NW, 1>), dim3(N / P, B), NW * 64, blocks, Lds<P>::BLK, a, st);
}

template <int LVL, int P>
int run_fp_fwd_p(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, float *logp, hipStream_t st)
{
    constexpr int NW = FpCfg<LVL>::NW;
    const ArchDesc &A = *m->arch;
    const int B = ws->B, N = ws->Nl[LVL], S = ws->Nl[LVL + 1];
    const size_t prob = (size_t)fwd * B;
    const int first = A.fp_first[LVL], head = A.head;
    if (LVL == 0 && sw().fp1_wave) {
        // fp1 + classifier head as a wave-private chain (psg_chain.cuh): one wave per 32 points, no barriers
        Fp1FwdArgs w;
        w.feat2 = ws->act[fp_in2_slot(0)];
        w.nn_idx = ws->nn_idx[0] + prob * N * 3;
        w.nn_w = ws->nn_w[0] + prob * N * 3;
        w.logp = logp;
        for (int i = 0; i < 4; ++i) {
            const int li = i < 3 ? first + i : head;
            const PackedLayer &L = m->L[li];
            w.mask[i] = (unsigned long long *)ws->mask[li];
            w.layer[i].w4 = L.wf4; w.layer[i].bias = L.bias; w.layer[i].k8 = L.k8f();
        }
        w.head = fwd_layer(m->L[head + 1], false, nullptr);
        w.N = N; w.S = S; w.n_cls = NCLS;
        EvScope prof(&ws->prof, TAG_FP_FWD + 0, 0.0, st);
        hipLaunchKernelGGL(fp1_fwd_wave_kernel, dim3(N / 32, B), dim3(64), (size_t)16 * WBLK * sizeof(float), st, w);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    FpFwdArgs a;
    a.feat1 = LVL == 0 ? nullptr : ws->act[LVL > 0 ? LVL - 1 : 0];
    a.C1 = LVL == 0 ? 0 : A.C[LVL];
    a.feat2 = ws->act[fp_in2_slot(LVL)];
    a.C2 = m->L[first].cin - a.C1;
    a.nn_idx = ws->nn_idx[LVL] + prob * N * 3;
    a.nn_w = ws->nn_w[LVL] + prob * N * 3;
    a.N = N; a.S = S;
    int nl = A.fp_count[LVL];
    for (int i = 0; i < nl; ++i)
        a.layer[i] = fwd_layer(m->L[first + i], true, ws->mask[first + i]);
    a.out = nullptr; a.logp = nullptr; a.Cout = 0; a.n_cls = 0;
    a.tsrc = nullptr; a.ldt = 0; a.out2 = nullptr; a.Cout2 = 0; a.extra = FwdLayer{};
    if constexpr (LVL <= 2) if (m->fsplit[LVL]) {
        // this module's first layer split: its interpolated part arrives as rows of T from the coarser module
        a.layer[0] = fwd_layer(m->fa[LVL], true, ws->mask[first]);
        a.layer[0].bias = m->L[first].bias;
        a.tsrc = ws->tfp[LVL]; a.ldt = m->fa[LVL].cout;
    }
    if constexpr (LVL >= 1) if (m->fsplit[LVL - 1]) {
        // the finer module's first layer split: its interpolated-part product, per point of THIS module
        a.extra = fwd_layer(m->fb[LVL - 1], false, nullptr);
        a.out2 = ws->tfp[LVL - 1]; a.Cout2 = m->fb[LVL - 1].cout;
    }
    if (LVL == 0) {
        a.layer[nl] = fwd_layer(m->L[head], true, ws->mask[head]);
        a.layer[nl + 1] = fwd_layer(m->L[head + 1], false, nullptr);
        nl += 2;
        a.logp = logp; a.n_cls = NCLS;
    } else {
        a.out = ws->act[fp_out_slot(LVL)];
        a.Cout = m->L[first + nl - 1].cout;
    }
    a.n_layers = nl;
    const int diag = diag_build_bits();
    a.diag = diag;
    if ((diag & 512) && ((diag >> 16) & 7) != LVL + 1) a.diag &= ~512;   // phase stamps for one module only
    a.dbg = ws->dbg;
    if (diag & 2) for (int i = 0; i < nl; ++i) a.layer[i].mask = nullptr;
    if (diag & 64) for (int i = 0; i < nl; ++i) a.layer[i].k8 = 4;    // timing only: 1/4 .. 1/24 of the MFMAs
    if (diag & 128) for (int i = 0; i < nl; ++i) a.layer[i].relu = 0; // timing only: no ReLU/mask epilogue
    const bool big = LVL == 3 && A.fp4_big;
    int blocks = 0;
    for (int i = 0; i < nl; ++i) {
        // a streamed first layer holds at most 64 blocks of its input at a time (fp_fwd_kernel<.., BIG>)
        const int k8 = (big && i == 0) ? std::min(a.layer[i].k8, 64) : a.layer[i].k8;
        blocks = std::max(blocks, layer_blocks(k8, a.layer[i].mb));
        if (a.layer[i].mb > NW) {     // (P / 32 tiles per wave: fp_fwd_kernel)
            set_error("run_fp_fwd<%d>: more tiles than waves in layer %d", LVL, i);
            return PSG_ERR_STATE;
        }
    }
    if (a.out2) {
        if (a.extra.mb > NW || a.extra.k8 * 8 != a.Cout || a.Cout2 % 4) {
            set_error("run_fp_fwd<%d>: unsupported shape of the finer module's split layer", LVL);
            return PSG_ERR_STATE;
        }
        blocks = std::max(blocks, layer_blocks(a.extra.k8, a.extra.mb));
    }
    if (a.tsrc && (a.ldt % 32 || a.C1 % 8)) { set_error("run_fp_fwd<%d>: unsupported shape of the split first layer", LVL); return PSG_ERR_STATE; }
    if (ws->lean && a.out2) a.out = nullptr;      // (the only reader of this module's output rows is ws.activation())
    blocks += PSG_LDS_SPARE;
    if constexpr (LVL == 3) if (big) {
        if (a.C1 % 4 || a.C2 % 4 || (a.C1 % 512) || !a.feat1) { set_error("run_fp_fwd: streamed fp4 wants C1 a multiple of 512"); return PSG_ERR_STATE; }
        return launch_lds(ws, TAG_FP_FWD + LVL, PSG_SITE, (fp_fwd_kernel<P, NW, true>), dim3(N / P, B), NW * 64, blocks, Lds<P>::BLK, a, st, "#big");
    }
    return launch_lds(ws, TAG_FP_FWD + LVL, PSG_SITE, (fp_fwd_kernel<P, NW, false>), dim3(N / P, B), NW * 64, blocks, Lds<P>::BLK, a, st,
                      a.tsrc ? "#tsrc" : "#whole");
}

template <int LVL, int P>
int run_fp_bwd_p(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *logp, const float *dlogp, hipStream_t st)
{
    constexpr int NW = FpCfg<LVL>::NW;
    const ArchDesc &A = *m->arch;
    const int B = ws->B, N = ws->Nl[LVL], S = ws->Nl[LVL + 1];
    const size_t prob = (size_t)fwd * B;
    const int first = A.fp_first[LVL], cnt = A.fp_count[LVL], head = A.head;
    if (LVL == 0 && sw().fp1_wave) {
        Fp1BwdArgs w;
        w.logp = logp; w.dlogp = dlogp;
        for (int i = 0; i < 4; ++i) w.mask[i] = (const unsigned long long *)ws->mask[i < 3 ? first + i : head];
        for (int i = 0; i < 5; ++i) {   // conv2^T, conv1^T, mlp2^T, mlp1^T, mlp0^T
            const PackedLayer &L = m->L[i < 2 ? head + 1 - i : first + 4 - i];
            w.layer[i].w4 = L.wb4; w.layer[i].bias = nullptr; w.layer[i].k8 = round_up(L.k8b(), 4);
        }
        w.dint_out = ws->dint[0];
        w.N = N; w.n_cls = NCLS;
        EvScope prof(&ws->prof, TAG_FP_BWD + 0, 0.0, st);
        hipLaunchKernelGGL(fp1_bwd_wave_kernel, dim3(N / 32, B), dim3(64), (size_t)16 * WBLK * sizeof(float), st, w);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    FpBwdArgs a;
    a.nn_idx = ws->nn_idx[LVL] + prob * N * 3;
    a.nn_w = ws->nn_w[LVL] + prob * N * 3;
    a.N = N; a.S = S;
    a.C1 = LVL == 0 ? 0 : A.C[LVL];
    a.C2 = m->L[first].cin - a.C1;
    a.dfeat1 = LVL == 0 ? nullptr : ws->dact[LVL > 0 ? LVL - 1 : 0];
    a.dint_out = ws->dint[LVL];
    a.nninv_off = nullptr; a.nninv_ent = nullptr; a.dint = nullptr; a.n_fine = 0;
    int nl = 0;
    a.dout = nullptr; a.mask_last = nullptr; a.logp = nullptr; a.dlogp = nullptr;
    a.Cout = 0; a.n_cls = 0; a.mb_last = 0;
    a.Cg = 0; a.pre = BwdLayer{}; a.split = 0; a.Cd = 0; a.skipT = BwdLayer{};
    if (LVL == 0) {
        a.logp = logp; a.dlogp = dlogp; a.n_cls = NCLS;
        a.layer[nl++] = bwd_layer(m->L[head + 1], ws->mask[head]);          // conv2^T, then bn1/conv1 ReLU mask
        a.layer[nl++] = bwd_layer(m->L[head], ws->mask[first + cnt - 1]);   // conv1^T, then fp1 last ReLU mask
    } else {
        // gradient of this module's output = transpose of the finer module's interpolation, gathered
        constexpr int LF = LVL > 0 ? LVL - 1 : 0;   // the finer FP level
        a.nninv_off = ws->inv_off[LF] + prob * (N + 1);
        a.nninv_ent = ws->inv_ent[LF] + prob * ws->Nl[LF] * 3;
        a.dint = ws->dint[LF];
        a.n_fine = ws->Nl[LF];
        a.mask_last = ws->mask[first + cnt - 1];
        a.Cout = m->L[first + cnt - 1].cout;
        a.mb_last = m->L[first + cnt - 1].mbf();
        a.Cg = a.Cout;
        if (m->fsplit[LF]) {    // the finer module wrote its dZ1 rows: W1b^T (and this module's last ReLU mask) after the gather
            a.pre = bwd_layer(m->fb[LF], a.mask_last);
            a.Cg = m->fb[LF].cout;
            if ((a.Cg != 128 && a.Cg != 256) || a.pre.mb != a.mb_last) {
                set_error("run_fp_bwd<%d>: unsupported shape of the finer module's split layer", LVL);
                return PSG_ERR_STATE;
            }
        }
    }
    const bool fs = LVL <= 2 && m->fsplit[LVL < 3 ? LVL : 0];
    for (int i = cnt - 1; i >= (fs ? 1 : 0); --i)
        a.layer[nl++] = bwd_layer(m->L[first + i], i > 0 ? ws->mask[first + i - 1] : nullptr);
    a.n_layers = nl;
    if (fs) {   // the layers stop at dZ1 (written as this module's interpolated-part rows); the skip columns' transpose follows
        a.split = 1; a.Cd = m->fb[LVL < 3 ? LVL : 0].cout;
        if (a.C1) a.skipT = bwd_layer(m->fa[LVL < 3 ? LVL : 0], nullptr);
        if (a.Cd % 4 || a.C1 % 4) { set_error("run_fp_bwd<%d>: unsupported shape of the split first layer", LVL); return PSG_ERR_STATE; }
    }
    const bool big = LVL == 3 && A.fp4_big;
    const int maxt = A.fp_maxt_b[LVL] * (P / 32);
    int blocks = std::max(a.mb_last * 4, a.Cg / 8);
    for (const BwdLayer *x : {&a.pre, &a.skipT}) {
        if (!x->w) continue;
        blocks = std::max(blocks, layer_blocks(x->k8, x->mb));
        if (x->mb * (P / 32) > maxt * NW) { set_error("run_fp_bwd<%d>: more than %d tiles per wave in a split layer", LVL, maxt); return PSG_ERR_STATE; }
    }
    for (int i = 0; i < nl; ++i) {
        if (big && i == nl - 1) {   // streamed last layer: its input plus a staging area of NW tiles
            blocks = std::max(blocks, a.layer[i].k8 + NW * 4);
            continue;
        }
        blocks = std::max(blocks, layer_blocks(a.layer[i].k8, a.layer[i].mb));
        if (a.layer[i].mb * (P / 32) > maxt * NW) {
            set_error("run_fp_bwd<%d>: more than %d tiles per wave in layer %d", LVL, maxt, i);
            return PSG_ERR_STATE;
        }
    }
    blocks += PSG_LDS_SPARE;
    const dim3 grid(N / P, B);
    auto go = [&](auto kern, const char *variant) {
        return launch_lds(ws, TAG_FP_BWD + LVL, PSG_SITE, kern, grid, NW * 64, blocks, Lds<P>::BLK, a, st, variant);
    };
    if constexpr (LVL == 3) if (big) return go(fp_bwd_kernel<P, NW, 1, true>, "#big");
    // (fp1 + head: 128-wide layers on 4 waves, one tile per wave at 32 points, two tiles = one pair at 64; the 8-wave modules
    // have ragged layers)
    if constexpr (P == 64) {
        if (maxt == 2) return go(fp_bwd_kernel<P, NW, 2, false>, "#p64#t2");
    } else {
        if (maxt == 1) return go(fp_bwd_kernel<P, NW, 1, false>, "#t1");
        if constexpr (LVL > 0) {
            if (maxt == 2) return go(fp_bwd_kernel<P, NW, 2, false>, "#t2");
            if (maxt == 3) return go(fp_bwd_kernel<P, NW, 3, false>, "#t3");
        }
    }
    set_error("run_fp_bwd<%d>: no kernel for MAXT=%d", LVL, maxt);
    return PSG_ERR_STATE;
}

template <int LVL>
int run_fp_fwd(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, float *logp, hipStream_t st)
{
    if constexpr (FpCfg<LVL>::P2 != FpCfg<LVL>::P)
        if (ws->Nl[LVL] % FpCfg<LVL>::P2 == 0) return run_fp_fwd_p<LVL, FpCfg<LVL>::P2>(m, ws, fwd, logp, st);
    return run_fp_fwd_p<LVL, FpCfg<LVL>::P>(m, ws, fwd, logp, st);
}

template <int LVL>
int run_fp_bwd(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *logp, const float *dlogp, hipStream_t st)
{
    if constexpr (FpCfg<LVL>::P2 != FpCfg<LVL>::P)
        if (ws->Nl[LVL] % FpCfg<LVL>::P2 == 0) return run_fp_bwd_p<LVL, FpCfg<LVL>::P2>(m, ws, fwd, logp, dlogp, st);
    return run_fp_bwd_p<LVL, FpCfg<LVL>::P>(m, ws, fwd, logp, dlogp, st);
}

// The NB loop's fp1 + head forward, CE gradient and fp1 + head backward as ONE launch (fp1_loop_kernel, psg_pn2_kernels.cuh)
// where forward and backward share the 64-point tiling: the split fp1 of both architectures (three 128-wide layers without
// skip columns, conv1, the 13-class conv2).  Anything else - PSG_PN2_FPSPLIT=0, the wave-private chain (PSG_FP1_WAVE=1), a
// point count that is no multiple of 64, a diagnostic build, PSG_PN2_FP1_LOOP=0 (A/B runs, tests/test_gpu_fp1_loop.py) - keeps
// the three launches.  The results are the same bits either way.
bool fp1_loop_applies(const psg_pn2_model *m, const psg_pn2_ws *ws)
{
    const bool on = sw().fp1_loop;
#ifdef PSG_DIAG_BUILD
    constexpr bool diag_build = true;     // (the fused kernel has no section-skipping switches)
#else
    constexpr bool diag_build = false;
#endif
    if (!on || diag_build || FpCfg<0>::P2 != 64 || FpCfg<0>::NW != 4 || sw().fp1_wave || !m->fsplit[0] || ws->Nl[0] % 64) return false;
    const ArchDesc &A = *m->arch;
    const int first = A.fp_first[0], head = A.head;
    if (A.fp_count[0] != 3 || NCLS != 13 || m->fa[0].k8f() != 0 || m->fa[0].cout != 128 || m->fb[0].cout != 128) return false;
    for (const PackedLayer *p : {&m->L[first + 1], &m->L[first + 2], &m->L[head]})
        if (p->k8f() != 16 || p->mbf() != 4 || p->k8b() != 16 || p->mbb() != 4) return false;
    const PackedLayer &c2 = m->L[head + 1];
    return c2.k8f() == 16 && c2.mbf() == 1 && c2.k8b() == 2 && c2.mbb() == 4;
}

int run_fp1_loop(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const int32_t *labels, int target, int rows_active, float scale,
                 hipStream_t st)
{
    constexpr int P = 64, NW = 4;
    const ArchDesc &A = *m->arch;
    const int B = ws->B, N = ws->Nl[0], first = A.fp_first[0], head = A.head;
    const size_t prob = (size_t)fwd * B;
    Fp1LoopArgs a{};
    a.fwd.nn_idx = ws->nn_idx[0] + prob * N * 3;
    a.fwd.nn_w = ws->nn_w[0] + prob * N * 3;
    a.fwd.tsrc = ws->tfp[0]; a.fwd.ldt = m->fa[0].cout;
    a.fwd.N = N; a.fwd.S = ws->Nl[1];
    a.fwd.layer[0] = fwd_layer(m->fa[0], true, nullptr);      // (k8 = 0: no skip columns)
    a.fwd.layer[0].bias = m->L[first].bias;
    a.f[0] = fwd_layer(m->L[first + 1], true, nullptr);
    a.f[1] = fwd_layer(m->L[first + 2], true, nullptr);
    a.f[2] = fwd_layer(m->L[head], true, nullptr);
    a.head = fwd_layer(m->L[head + 1], false, nullptr);
    a.t[0] = bwd_layer(m->L[head + 1], nullptr);
    a.t[1] = bwd_layer(m->L[head], nullptr);
    a.t[2] = bwd_layer(m->L[first + 2], nullptr);
    a.t[3] = bwd_layer(m->L[first + 1], nullptr);
    a.labels = labels; a.target = target; a.rows_active = rows_active; a.scale = scale;
    a.dint_out = ws->dint[0];
    a.N = N;
#if PSG_MLP_PAIRS
    return launch_lds(ws, TAG_FP1_LOOP, PSG_SITE, (fp1_loop_kernel<P, NW, NCLS>), dim3(N / P, B), NW * 64, 16 + PSG_LDS_SPARE, Lds<P>::BLK, a, st);
#else   // (the single-tile engine runs fp1 at 32 points: fp1_loop_applies is false, and no paired loop is built)
    set_error("run_fp1_loop: built without the paired k-loop");
    return PSG_ERR_STATE;
#endif
}

__global__ void extract_xyz_kernel(const float *__restrict__ x0, float *__restrict__ xyz, size_t rows)
{
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows * 3; t += (size_t)gridDim.x * blockDim.x)
        xyz[t] = x0[(t / 3) * 9 + (t % 3)];
}

__global__ void extract_color_kernel(const float *__restrict__ x0, float *__restrict__ ori, size_t rows)
{
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows * 3; t += (size_t)gridDim.x * blockDim.x)
        ori[t] = x0[(t / 3) * 9 + 3 + (t % 3)];
}

__global__ void gather_starts_kernel(const int32_t *__restrict__ starts, int32_t *__restrict__ out, int level, int B,
                                     int P)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) out[p] = starts[((size_t)(p / B) * 4 + level) * B + (p % B)];
}

// Level-0 groups of a many-forward plan from the room's ball table (psg_pn2_plan_build): a level-0 centroid IS a point of the
// room (xyz[1] = xyz0[fps]: psg_gather_points copies the three floats), and the ball query of a centroid - the first K
// indices in index order with sqdist(centroid, .) <= r^2 - depends on nothing but the centroid's bits and the room, so
// gidx[p][s][0:K] = table[p % B][fps[p][s]][0:K].  A row is K int32 (128 or 64 bytes): K / 4 lanes copy it as int4, 8 or 16 rows
// per wave; the lanes of a row read the same fps word (one broadcast load).
__global__ void group_from_table_kernel(const int32_t *__restrict__ table, const int32_t *__restrict__ fps, int B, int N, int S,
                                        int K4, size_t rows, int32_t *__restrict__ gidx)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t row = t / K4;
    if (row >= rows) return;
    const int part = (int)(t - row * K4);
    const size_t p = row / S;
    const int4 *src = (const int4 *)(table + ((p % B) * N + (size_t)fps[row]) * K4 * 4);
    ((int4 *)gidx)[t] = src[part];
}

constexpr int INV_NT = 1024;

// Inverse of the 3-NN tables: for every coarse point the (fine point, weight) pairs that interpolate from it,
// as CSR sorted by fine point, so the backward pass can GATHER (fixed summation order, no atomics) what the
// reference's autograd scatter-adds (index_points backward, pointnet_util.py:308).
// One workgroup per problem; counters and the whole entry array are staged in LDS (3 N 16-bit fine indices + 3 N
// weights + S + 1 counters: 78 KiB at N = 4096, S = 1024), so the per-list sort never touches HBM and the lists leave
// the CU as one coalesced stream (the first version sorted in global memory: 640 MB of traffic per launch).
__global__ __launch_bounds__(INV_NT) void build_inv_nn_kernel(const int32_t *__restrict__ nn_idx, const float *__restrict__ nn_w,
                                                              int N, int S, int32_t *__restrict__ inv_off,
                                                              int2 *__restrict__ inv_ent)
{
    extern __shared__ int s_nn[];
    int *s_cnt = s_nn;                                         // [S + 1]
    float *s_wt = (float *)(s_nn + S + 1);                     // [3 N]
    unsigned short *s_fine = (unsigned short *)(s_wt + 3 * N); // [3 N] fine point of every entry (< 8192)
    const size_t p = blockIdx.x;
    const int32_t *idx = nn_idx + p * N * 3;
    const float *w = nn_w + p * N * 3;
    int32_t *off = inv_off + p * (S + 1);
    int2 *ent = inv_ent + p * N * 3;
    for (int i = threadIdx.x; i <= S; i += INV_NT) s_cnt[i] = 0;
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * N; e += INV_NT) atomicAdd(&s_cnt[idx[e]], 1);
    __syncthreads();
    if (threadIdx.x < 64) {   // exclusive scan by one wave: 64 contiguous chunks, then a scan of the chunk sums
        const int lane = threadIdx.x, chunk = (S + 63) / 64, lo = min(S, lane * chunk), hi = min(S, lo + chunk);
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += s_cnt[i];
        int incl = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        int run = incl - sum;
        for (int i = lo; i < hi; ++i) { const int c = s_cnt[i]; s_cnt[i] = run; off[i] = run; run += c; }
        if (lane == 63) { off[S] = incl; s_cnt[S] = incl; }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * N; e += INV_NT) {
        const int pos = atomicAdd(&s_cnt[idx[e]], 1);
        s_fine[pos] = (unsigned short)(e / 3);
        s_wt[pos] = w[e];
    }
    __syncthreads();
    // after the fill s_cnt[i] == end of list i; start = end of list i-1 (0 for i == 0)
    for (int i = threadIdx.x; i < S; i += INV_NT) {
        const int lo = i ? s_cnt[i - 1] : 0, hi = s_cnt[i];
        for (int a = lo + 1; a < hi; ++a) {   // insertion sort by fine point (the fill order above is not deterministic)
            const unsigned short kf = s_fine[a];
            const float kw = s_wt[a];
            int q = a - 1;
            while (q >= lo && s_fine[q] > kf) { s_fine[q + 1] = s_fine[q]; s_wt[q + 1] = s_wt[q]; --q; }
            s_fine[q + 1] = kf; s_wt[q + 1] = kw;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * N; e += INV_NT) ent[e] = make_int2((int)s_fine[e], __float_as_int(s_wt[e]));
}

// Inverse of the group tables: for every source point the grouped rows (group*32 + sample) that gathered it, as
// offsets of a CSR whose lists are sorted by grouped row, plus the inverse permutation `pos` (slot of a grouped row
// in the concatenated lists): sa_bwd stores row r at slot pos[r], so a consumer reads the rows of one point
// contiguously and in a fixed order.  (query_ball_point pads a group by repeating its first member, so a point
// can occur several times in one group: autograd's index backward sums every occurrence; see the kernel body for
// why only the first is listed.)  One workgroup per problem, the whole list array staged in LDS (<= 32768 16-bit row ids + 8193 counters).
__global__ __launch_bounds__(INV_NT) void build_inv_group_kernel(const int32_t *__restrict__ gidx, int n_rows, int n_src,
                                                                 int ks, int32_t *__restrict__ inv_off,
                                                                 int32_t *__restrict__ inv_pos)
{
    const int km = ks - 1;   // ks = samples per group, a power of two
    extern __shared__ int s_inv[];
    int *s_cnt = s_inv;               // [n_src + 1]
    unsigned short *s_ent = (unsigned short *)(s_inv + n_src + 1);   // [n_rows] row ids (< 32768: 16 bits)
    const size_t p = blockIdx.x;
    const int32_t *idx = gidx + p * n_rows;
    int32_t *off = inv_off + p * (n_src + 1);
    int32_t *pos = inv_pos + p * n_rows;
    for (int i = threadIdx.x; i <= n_src; i += INV_NT) s_cnt[i] = 0;
    __syncthreads();
    // Padding rows (sample k > 0 repeating the group's first member) are left out: they duplicate sample 0, the
    // max-pool's lowest-index tie rule never routes gradient to them, so their rows are exactly zero.  pos = -1
    // tells sa_bwd not to store them.  That also bounds a list by the number of GROUPS containing the point.
    for (int e = threadIdx.x; e < n_rows; e += INV_NT) {
        const bool pad = (e & km) != 0 && idx[e] == idx[e & ~km];
        if (!pad) atomicAdd(&s_cnt[idx[e]], 1);
        else pos[e] = -1;
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // exclusive scan by one wave: 64 contiguous chunks, then a scan of the chunk sums
        const int lane = threadIdx.x, chunk = (n_src + 63) / 64, lo = min(n_src, lane * chunk), hi = min(n_src, lo + chunk);
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += s_cnt[i];
        int incl = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        int run = incl - sum;
        for (int i = lo; i < hi; ++i) { const int c = s_cnt[i]; s_cnt[i] = run; off[i] = run; run += c; }
        if (lane == 63) { off[n_src] = incl; s_cnt[n_src] = incl; }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_rows; e += INV_NT) {
        const bool pad = (e & km) != 0 && idx[e] == idx[e & ~km];
        if (!pad) s_ent[atomicAdd(&s_cnt[idx[e]], 1)] = (unsigned short)e;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_src; i += INV_NT) {   // s_cnt[i] is now the END of list i
        const int lo = i ? s_cnt[i - 1] : 0, hi = s_cnt[i];
        for (int a = lo + 1; a < hi; ++a) {   // insertion sort by row id (the fill order above is not deterministic)
            const unsigned short key = s_ent[a];
            int q = a - 1;
            while (q >= lo && s_ent[q] > key) { s_ent[q + 1] = s_ent[q]; --q; }
            s_ent[q + 1] = key;
        }
    }
    __syncthreads();
    const int n_listed = s_cnt[n_src - 1];   // end of the last list
    for (int a = threadIdx.x; a < n_listed; a += INV_NT) pos[s_ent[a]] = a;
}

// dx0[q][c] = sum over the grouped rows of sa1 that gathered point q (c in [c_lo, c_hi)); sa1_bwd stored its rows in
// list order, so the rows of point q are the contiguous slots [off[q], off[q+1]), summed in ascending order.
// COMPACT: rows are {c_lo, c_lo+1, c_lo+2, 0} float4 (attack loop), one thread per point; else rows of `cg` floats
// indexed by channel, one thread per (point, channel).
template <bool COMPACT>
__global__ void dx0_gather_kernel(const int32_t *__restrict__ inv_off, const float *__restrict__ gsa, int g_rows,
                                  const int32_t *__restrict__ inv_off2, const float *__restrict__ gsa2, int g_rows2,
                                  int B, int N, int cg, int c_lo, int c_hi, float *__restrict__ dx0)
{
    const int nc = COMPACT ? 1 : c_hi - c_lo;
    const size_t total = (size_t)B * N * nc;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = c_lo + (int)(t % nc);
        const size_t pq = t / nc;
        const int b = (int)(pq / N), q = (int)(pq - (size_t)b * N);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int list = 0; list < 2; ++list) {   // the MSG network has a second scale of sa1 (after the first)
            const int32_t *offs = list ? inv_off2 : inv_off;
            if (!offs) break;
            const float *rows = list ? gsa2 : gsa;
            const int gr = list ? g_rows2 : g_rows;
            const int32_t *off = offs + (size_t)b * (N + 1) + q;
            const int e1 = off[1];
            for (int e = off[0]; e < e1; e += 8) {
                if (COMPACT) {
                    float4 v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        v[u] = e + u < e1 ? *(const float4 *)(rows + ((size_t)b * gr + e + u) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; }
                } else {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = e + u < e1 ? rows[((size_t)b * gr + e + u) * cg + c] : 0.0f;
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc.x += v[u];
                }
            }
        }
        if (COMPACT) {
            dx0[pq * 9 + c_lo] = acc.x; dx0[pq * 9 + c_lo + 1] = acc.y; dx0[pq * 9 + c_lo + 2] = acc.z;
        } else {
            dx0[pq * 9 + c] = acc.x;
        }
    }
}

// The attack loop's last two launches in one: the compact gather above, then the PGD step of the point's three colours -
// the arithmetic of pgd_step_kernel (psg_attack.hip: sign, step, projection onto the eps ball and [0, 1], the un-projected
// last step of nontarget.py:36-41), on the sum still in registers; dx0 is neither written nor read.
struct PgdFuse {
    float *x;               // [B][N][9]
    const float *ori;       // [B][N][3]
    const uint8_t *mask;    // [N] or null
    float step, eps;        // step = dir * alpha, rounded to fp32 on the host like psg_pgd_step does
    int last;
};
__global__ void dx0_gather_pgd_kernel(const int32_t *__restrict__ inv_off, const float *__restrict__ gsa, int g_rows,
                                      const int32_t *__restrict__ inv_off2, const float *__restrict__ gsa2, int g_rows2,
                                      int B, int N, int c_lo, PgdFuse f)
{
    const size_t total = (size_t)B * N;
    for (size_t pq = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pq < total; pq += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(pq / N), q = (int)(pq - (size_t)b * N);
        if (f.mask && !f.mask[q]) continue;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int list = 0; list < 2; ++list) {
            const int32_t *offs = list ? inv_off2 : inv_off;
            if (!offs) break;
            const float *rows = list ? gsa2 : gsa;
            const int gr = list ? g_rows2 : g_rows;
            const int32_t *off = offs + (size_t)b * (N + 1) + q;
            const int e1 = off[1];
            for (int e = off[0]; e < e1; e += 8) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    v[u] = e + u < e1 ? *(const float4 *)(rows + ((size_t)b * gr + e + u) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; }
            }
        }
        const float g[3] = {acc.x, acc.y, acc.z};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const size_t xi = pq * 9 + c_lo + ch;
            const float sg = g[ch] > 0.0f ? 1.0f : (g[ch] < 0.0f ? -1.0f : 0.0f);
            const float stepped = __fadd_rn(f.x[xi], __fmul_rn(f.step, sg));
            const float o = f.ori[pq * 3 + ch];
            const float eta = fminf(fmaxf(__fsub_rn(stepped, o), -f.eps), f.eps);
            const float proj = fminf(fmaxf(__fadd_rn(o, eta), 0.0f), 1.0f);
            f.x[xi] = f.last ? stepped : proj;
        }
    }
}

void ws_layout(psg_pn2_ws *ws, Bump &bp)
{
    const ArchDesc &A = *ws->arch;
    const int B = ws->B, F = ws->F;
    const size_t PR = (size_t)F * B;
    ws->xyz0 = bp.take<float>((size_t)B * ws->N * 3);
    ws->xyz[0] = ws->xyz0;
    for (int l = 0; l < 4; ++l) {
        ws->fps[l] = bp.take<int32_t>(PR * kS[l]);
        ws->xyz[l + 1] = bp.take<float>(PR * kS[l] * 3);
        ws->nn_idx[l] = bp.take<int32_t>(PR * ws->Nl[l] * 3);
        ws->nn_w[l] = bp.take<float>(PR * ws->Nl[l] * 3);
        ws->inv_off[l] = bp.take<int32_t>(PR * (kS[l] + 1));
        ws->inv_ent[l] = bp.take<int2>(PR * ws->Nl[l] * 3);
        for (int s = 0; s < A.ns; ++s) {
            ws->gidx[l][s] = bp.take<int32_t>(PR * kS[l] * A.sc[l][s].K);
            ws->ginv_off[l][s] = bp.take<int32_t>(PR * (ws->Nl[l] + 1));
            ws->ginv_pos[l][s] = bp.take<int32_t>(PR * kS[l] * A.sc[l][s].K);
        }
    }
    for (int l = 0; l < 4; ++l)
        for (int s = 0; s < A.ns; ++s) ws->gsa[l][s] = bp.take<float>((size_t)B * kS[l] * A.sc[l][s].K * gsa_stride(A, l));
    for (int l = 0; l < 4; ++l) {
        ws->tfeat[l][0] = ws->tfeat[l][1] = nullptr; ws->dsum[l] = nullptr;
        if (arch_split_fwd(A, l))
            for (int s = 0; s < A.ns; ++s) ws->tfeat[l][s] = bp.take<float>((size_t)B * ws->Nl[l] * A.cout[A.sc[l][s].l0]);
        if (arch_split(A, l)) ws->dsum[l - 1] = bp.take<float>((size_t)B * ws->Nl[l] * A.C[l]);
    }
    for (int l = 0; l < 4; ++l) {   // interpolated-part gradient rows of FP module l: C2 = its input minus the skip part
        const int c2 = A.cin[A.fp_first[l]] - (l == 0 ? 0 : A.C[l]);      // (a split module writes its dZ1 rows instead)
        const bool fs = l < 3 && arch_fp_split(A, l);
        ws->dint[l] = bp.take<float>((size_t)B * ws->Nl[l] * (fs ? A.cout[A.fp_first[l]] : c2));
        if (l < 3) ws->tfp[l] = fs ? bp.take<float>((size_t)B * ws->Nl[l + 1] * A.cout[A.fp_first[l]]) : nullptr;
    }
    const int actN[7] = {1024, 256, 64, 16, 64, 256, 1024};
    for (int i = 0; i < 4; ++i) ws->actC[i] = A.C[i + 1];
    for (int lvl = 3; lvl >= 1; --lvl) ws->actC[7 - lvl] = A.cout[A.fp_first[lvl] + A.fp_count[lvl] - 1];
    for (int i = 0; i < 7; ++i) ws->act[i] = bp.take<float>((size_t)B * actN[i] * ws->actC[i]);
    for (int l = 0; l < 4; ++l)
        for (int s = 0; s < A.ns; ++s) ws->arg[l][s] = bp.take<uint8_t>((size_t)B * kS[l] * A.c3(l, s));
    // ReLU masks: one uint16 per (32-channel block, point-lane): rows * mb(cout) * 2 entries
    for (int i = 0; i < A.n_layers; ++i) ws->mask[i] = nullptr;
    for (int l = 0; l < 4; ++l)
        for (int s = 0; s < A.ns; ++s)
            for (int j = 0; j < 3; ++j) {
                const int li = A.sc[l][s].l0 + j;
                ws->mask[li] = bp.take<uint16_t>((size_t)B * kS[l] * A.sc[l][s].K * ceil_div(A.cout[li], 32) * 2);
            }
    for (int lvl = 0; lvl < 4; ++lvl)
        for (int j = 0; j < A.fp_count[lvl]; ++j) {
            const int li = A.fp_first[lvl] + j;
            ws->mask[li] = bp.take<uint16_t>((size_t)B * ws->Nl[lvl] * ceil_div(A.cout[li], 32) * 2);
        }
    for (int li = A.head; li < A.head + 2; ++li)
        ws->mask[li] = bp.take<uint16_t>((size_t)B * ws->Nl[0] * ceil_div(A.cout[li], 32) * 2);
    ws->logp = bp.take<float>((size_t)B * ws->N * NCLS);
    ws->dlogp = bp.take<float>((size_t)B * ws->N * NCLS);
    bp.off = (bp.off + 255) & ~(size_t)255;
    for (int i = 0; i < 7; ++i) ws->dact[i] = bp.take<float>((size_t)B * actN[i] * ws->actC[i]);
    ws->dx0 = bp.take<float>((size_t)B * ws->N * 9);
    bp.off = (bp.off + 255) & ~(size_t)255;
    ws->x0 = bp.take<float>((size_t)B * ws->N * 9);
    ws->ori = bp.take<float>((size_t)B * ws->N * 3);
    ws->dbg = bp.take<unsigned long long>(16 * 8 * 1024);
    ws->nb_labels = bp.take<int32_t>((size_t)B * ws->N);
    ws->nb_starts = bp.take<int32_t>((size_t)F * 4 * B);
    ws->nb_mask = bp.take<uint8_t>((size_t)ws->N);
    for (int l = 0; l < 4; ++l) {   // (behind everything else: the offsets of the buffers above do not depend on them)
        const bool full = A.id == PSG_PN2_ARCH_SSG;
        ws->grel[l] = full && l >= 1 ? bp.take<float4>((size_t)B * kS[l] * A.sc[l][0].K) : nullptr;
        ws->fpg[l] = full ? bp.take<float4>((size_t)B * ws->Nl[l]) : nullptr;
        ws->gxyz[l + 1] = full ? bp.take<float>((size_t)B * ws->Nl[l + 1] * 3) : nullptr;
    }
    ws->gxyz[0] = nullptr;
    for (int l = 0; l < 4; ++l) {
        const bool pk = arch_pack(A);
        ws->pk_cnt[l] = pk ? bp.take<int32_t>(PR * kS[l]) : nullptr;
        ws->pk_seg[l] = pk ? bp.take<int32_t>(PR * (kS[l] / (A.sc[l][0].P / 32) + 2)) : nullptr;
        bp.off = (bp.off + 15) & ~(size_t)15;
        ws->pk_desc[l] = pk ? bp.take<int4>(PR * (kS[l] / (A.sc[l][0].P / 32))) : nullptr;
    }
    // (last of all, for the same reason) the per-room level-0 ball tables, where a plan of this workspace can reach the table route
    for (int s = 0; s < 2; ++s)
        ws->ball0[s] = s < A.ns && ball_table_route(F, ws->N) ? bp.take<int32_t>((size_t)B * ws->N * A.sc[0][s].K) : nullptr;
}

}  // namespace

// ================================================================================== C ABI: model
extern "C" int psg_pn2_model_create_arch(psg_ctx *ctx, int arch, const float *const *weights,
                                         const float *const *biases, int n_layers, psg_pn2_model **out)
{
    PSG_REQUIRE(ctx && weights && biases && out, "psg_pn2_model_create: null argument");
    PSG_REQUIRE(arch == PSG_PN2_ARCH_SSG || arch == PSG_PN2_ARCH_MSG, "psg_pn2_model_create: unknown architecture %d", arch);
    const ArchDesc &A = arch_of(arch);
    PSG_REQUIRE(n_layers == A.n_layers, "psg_pn2_model_create: architecture %d has %d layers, got %d", arch, A.n_layers, n_layers);
    PSG_CHECK_HIP(hipSetDevice(ctx->device));
    auto *m = new psg_pn2_model();
    m->ctx = ctx;
    m->arch = &A;
    auto fail = [&](int rc) { psg_pn2_model_destroy(m); return rc; };     // (frees the arena, if any, and the handle)
    for (int i = 0; i < A.n_layers; ++i)
        if (!weights[i] || !biases[i]) { set_error("psg_pn2_model_create: layer %d is null", i); return fail(PSG_ERR_ARG); }
    // Every weight block is listed ONCE, in arena order: its host copy and where its device pointer goes.  The layout below
    // takes them in this order (256-byte aligned), the arena is their exact sum, and one loop uploads them.
    struct Block { const void *src; size_t bytes; std::function<void(void *)> set; void *dst; };
    std::vector<Block> blocks;
    std::vector<std::vector<float>> host;     // owns the packed copies (a moved vector keeps its data pointer)
    auto add = [&](std::vector<float> v, std::function<void(void *)> set) {
        blocks.push_back({v.data(), v.size() * 4, std::move(set), nullptr});
        host.push_back(std::move(v));
    };
    auto padded_bias = [&](int i) {
        std::vector<float> b(biases[i], biases[i] + A.cout[i]);
        b.resize((size_t)ceil_div(A.cout[i], 32) * 32, 0.0f);
        return b;
    };
    for (int l = 0; l < 4; ++l) { m->split[l] = arch_split(A, l); m->split_fwd[l] = arch_split_fwd(A, l); }
    for (int l = 0; l < 3; ++l) m->fsplit[l] = arch_fp_split(A, l);
    auto cols = [&](int li, int c0, int n) {     // columns [c0, c0 + n) of layer li's rows, as [cout][n]
        std::vector<float> w((size_t)A.cout[li] * std::max(n, 1));
        for (int o = 0; o < A.cout[li]; ++o)
            for (int c = 0; c < n; ++c) w[(size_t)o * n + c] = weights[li][(size_t)o * A.cin[li] + c0 + c];
        return w;
    };
    for (int l = 1; l < 4; ++l) {   // SSG column order of a first layer: [rel_xyz(3), feats(D)]; the xyz columns as [3][C1]
        if (A.id != PSG_PN2_ARCH_SSG || !m->split[l]) continue;
        const int li = A.sc[l][0].l0, cin = A.cin[li], cout = A.cout[li];
        std::vector<float> w1x((size_t)3 * cout);
        for (int o = 0; o < cout; ++o)
            for (int c = 0; c < 3; ++c) w1x[(size_t)c * cout + o] = weights[li][(size_t)o * cin + c];
        add(std::move(w1x), [m, l](void *p) { m->w1x[l] = (float *)p; });
    }
    for (int sc = 0; sc < A.ns; ++sc) {
        const int li = A.sc[0][sc].l0;
        add(cols(li, A.sa_perm ? 3 : 0, A.cin[li] - 3), [m, sc](void *p) { m->w1feat[sc] = (float *)p; });
    }
    // split FP first layers (arch_fp_split): reference column order is [points1 (skip, C1), interpolated (C2)]
    for (int l = 0; l < 3; ++l) {
        if (!m->fsplit[l]) continue;
        const int li = A.fp_first[l], cout = A.cout[li], C1 = l == 0 ? 0 : A.C[l], C2 = A.cin[li] - C1;
        const std::vector<float> wa = cols(li, 0, C1), wbm = cols(li, C1, C2);
        PackedLayer *Fa = &m->fa[l], *Fb = &m->fb[l];
        Fa->cin = C1; Fa->cout = cout;
        Fb->cin = C2; Fb->cout = cout;
        if (C1) {
            add(pack_fwd(wa.data(), C1, cout, nullptr), [Fa](void *p) { Fa->wf = (float4 *)p; });
            add(pack_bwd(wa.data(), C1, cout, nullptr), [Fa](void *p) { Fa->wb = (float4 *)p; });
        }
        add(pack_fwd(wbm.data(), C2, cout, nullptr), [Fb](void *p) { Fb->wf = (float4 *)p; });
        add(pack_bwd(wbm.data(), C2, cout, nullptr), [Fb](void *p) { Fb->wb = (float4 *)p; });
        add(std::vector<float>((size_t)ceil_div(cout, 32) * 32, 0.0f), [Fb](void *p) { Fb->bias = (float *)p; });
    }
    // split first layers (arch_split): reference column order of the layer is [rel_xyz(3), feats(D)] (SSG: sa_perm)
    for (int ls = 0; ls < 8; ++ls) {
        const int l = ls >> 1, s = ls & 1;
        if (!m->split_fwd[l] || s >= A.ns) continue;
        const int li = A.sc[l][s].l0, cout = A.cout[li], D = A.cin[li] - 3;
        std::vector<float> wx = cols(li, A.sa_perm ? 0 : D, 3), wfe = cols(li, A.sa_perm ? 3 : 0, D);
        PackedLayer *X = &m->sx[l][s], *F = &m->sf[l][s];
        X->cin = 3; X->cout = cout;
        F->cin = D; F->cout = cout;
        add(pack_fwd(wx.data(), 3, cout, nullptr), [X](void *p) { X->wf = (float4 *)p; });
        add(pack_fwd(wfe.data(), D, cout, nullptr), [F](void *p) { F->wf = (float4 *)p; });
        add(pack_bwd(wfe.data(), D, cout, nullptr), [F](void *p) { F->wb = (float4 *)p; });
        add(padded_bias(li), [m, X, F, l](void *p) {
            X->bias = F->bias = (float *)p;     // (X's is unused: the bias arrives through T)
            if (l == 0) m->b0f = F->bias;
        });
        if (l == 0) add(std::move(wfe), [m](void *p) { m->w0f = (float *)p; });
    }
    const int fp1 = A.fp_first[0];
    for (int i = 0; i < A.n_layers; ++i) {
        const int cin = A.cin[i], cout = A.cout[i];
        bool sa_first = false, sa_rows = false;
        for (int l = 0; l < 4; ++l)
            for (int s = 0; s < A.ns; ++s) {
                if (A.sc[l][s].l0 == i) sa_first = A.sa_perm;
                if (A.sc[l][s].l0 + 2 == i) sa_rows = A.id == PSG_PN2_ARCH_SSG && l >= 1;   // (SaPath::spv: the levels that may run sparse)
            }
        std::vector<int> perm;
        if (sa_first) perm = sa_input_perm(cin);
        std::vector<float> wf = pack_fwd(weights[i], cin, cout, sa_first ? &perm : nullptr);
        std::vector<float> wb = pack_bwd(weights[i], cin, cout, sa_first ? &perm : nullptr), wf4, wb4;
        if ((i >= fp1 && i < fp1 + 3) || i >= A.head) {   // fp1 + head run as wave-private chains: k8-major packings of the 128-wide sides
            if (cout == 128) wf4 = k8_major_padded(wf, 4, ceil_div(cin, 8), ceil_div(cin, 8));
            wb4 = k8_major_padded(wb, 4, ceil_div(cout, 8), round_up(ceil_div(cout, 8), 4));
        }
        PackedLayer *L = &m->L[i];
        L->cin = cin; L->cout = cout;
        add(std::move(wf), [L](void *p) { L->wf = (float4 *)p; });
        add(std::move(wb), [L](void *p) { L->wb = (float4 *)p; });
        add(padded_bias(i), [L](void *p) { L->bias = (float *)p; });
        if (!wf4.empty()) add(std::move(wf4), [L](void *p) { L->wf4 = (float4 *)p; });
        if (!wb4.empty()) add(std::move(wb4), [L](void *p) { L->wb4 = (float4 *)p; });
        if (sa_rows) blocks.push_back({weights[i], (size_t)cout * cin * 4, [L](void *p) { L->wr = (float *)p; }, nullptr});
    }
    size_t bytes = 0;
    if (int rc = carve_arena(&m->arena, &bytes, "psg_pn2_model_create", [&](Bump &bp) {
            for (Block &b : blocks) b.set(b.dst = bp.take<char>(b.bytes));
        }))
        return fail(rc);
    for (const Block &b : blocks) {
        const hipError_t e = psg::copy_sync(b.dst, b.src, b.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("psg_pn2_model_create: upload failed: %s", hipGetErrorString(e)); return fail(PSG_ERR_HIP); }
    }
    *out = m;
    return PSG_OK;
}

extern "C" int psg_pn2_model_create(psg_ctx *ctx, const float *const *weights, const float *const *biases,
                                    psg_pn2_model **out)
{
    return psg_pn2_model_create_arch(ctx, PSG_PN2_ARCH_SSG, weights, biases, PSG_PN2_NUM_LAYERS, out);
}

extern "C" int psg_pn2_model_destroy(psg_pn2_model *m)
{
    if (!m) return PSG_OK;
    if (m->arena) (void)hipFree(m->arena);
    delete m;
    return PSG_OK;
}

// ============================================================================== C ABI: workspace
extern "C" int psg_pn2_ws_create_arch(psg_ctx *ctx, int arch, int batch, int n_point, int max_forwards, psg_pn2_ws **out)
{
    PSG_REQUIRE(ctx && out, "psg_pn2_ws_create: null argument");
    PSG_REQUIRE(arch == PSG_PN2_ARCH_SSG || arch == PSG_PN2_ARCH_MSG, "psg_pn2_ws_create: unknown architecture %d", arch);
    PSG_REQUIRE(batch > 0 && max_forwards > 0, "psg_pn2_ws_create: batch and max_forwards must be positive");
    PSG_REQUIRE(n_point >= 1024 && n_point <= 8192 && n_point % 128 == 0,
                "psg_pn2_ws_create: n_point=%d must be a multiple of 128 in [1024, 8192]", n_point);
    PSG_CHECK_HIP(hipSetDevice(ctx->device));
    auto *ws = new psg_pn2_ws();
    ws->ctx = ctx; ws->arch = &arch_of(arch); ws->B = batch; ws->N = n_point; ws->F = max_forwards;
    ws->Nl[0] = n_point;
    for (int l = 0; l < 4; ++l) ws->Nl[l + 1] = kS[l];
    if (int rc = carve_arena(&ws->arena, &ws->bytes, "psg_pn2_ws_create", [&](Bump &bp) { ws_layout(ws, bp); })) {
        delete ws;
        return rc;
    }
    *out = ws;
    return PSG_OK;
}

extern "C" int psg_pn2_ws_create(psg_ctx *ctx, int batch, int n_point, int max_forwards, psg_pn2_ws **out)
{
    return psg_pn2_ws_create_arch(ctx, PSG_PN2_ARCH_SSG, batch, n_point, max_forwards, out);
}

extern "C" int psg_pn2_ws_destroy(psg_pn2_ws *ws)
{
    if (!ws) return PSG_OK;
    ws->nb.destroy();
    for (hipEvent_t e : ws->nb_ev) if (e) (void)hipEventDestroy(e);
    if (ws->nb_stream) (void)hipStreamDestroy(ws->nb_stream);
    if (ws->arena) (void)hipFree(ws->arena);
    ws->prof.destroy();
    delete ws;
    return PSG_OK;
}

extern "C" size_t psg_pn2_ws_bytes(const psg_pn2_ws *ws) { return ws ? ws->bytes : 0; }

extern "C" int psg_pn2_debug_read(psg_pn2_ws *ws, unsigned long long *host_out, int n_words)
{
    PSG_REQUIRE(ws && host_out && n_words > 0 && n_words <= 16 * 8 * 1024, "psg_pn2_debug_read: bad argument");
    PSG_CHECK_HIP(hipDeviceSynchronize());
    PSG_CHECK_HIP(psg::copy_sync(host_out, ws->dbg, (size_t)n_words * 8, hipMemcpyDeviceToHost));
    return PSG_OK;
}

extern "C" int psg_pn2_prof_enable(psg_pn2_ws *ws, int on)
{
    PSG_REQUIRE(ws, "psg_pn2_prof_enable: null workspace");
    ws->prof.reset(on != 0);
    return PSG_OK;
}

extern "C" int psg_pn2_prof_read(psg_pn2_ws *ws, int n_tags, double *total_ms, int *counts)
{
    PSG_REQUIRE(ws && total_ms && counts && n_tags >= TAG_COUNT, "psg_pn2_prof_read: need room for %d tags", TAG_COUNT);
    if (ws->prof.read(n_tags, total_ms, counts, nullptr)) { set_error("psg_pn2_prof_read: event query failed"); return PSG_ERR_HIP; }
    return PSG_OK;
}

extern "C" int psg_pn2_plan_build(psg_pn2_ws *ws, const float *x0, const int32_t *starts, int n_forward,
                                  psg_stream stream)
{
    PSG_REQUIRE(ws && x0 && starts, "psg_pn2_plan_build: null argument");
    PSG_REQUIRE(n_forward > 0 && n_forward <= ws->F, "psg_pn2_plan_build: n_forward=%d exceeds workspace capacity %d",
                n_forward, ws->F);
    hipStream_t st = (hipStream_t)stream;
    const int B = ws->B, P = n_forward * B;
    hipLaunchKernelGGL(extract_xyz_kernel, dim3(std::min(1024, ceil_div(B * ws->N * 3, 256))), dim3(256), 0, st, x0,
                       ws->xyz0, (size_t)B * ws->N);
    PSG_LAUNCH_CHECK();
    int rc;
    // starts is [n_forward][4][B]; FPS wants start[p], p = f*B + b, per level: gathered by a tiny
    // kernel into the head of nn_idx[l], which is dead until this level's 3-NN runs (stream order).
    for (int l = 0; l < 4; ++l) {
        const int Np = ws->Nl[l], S = kS[l];
        const int n_clouds = l == 0 ? B : P;
        int32_t *start_l = ws->nn_idx[l];  // scratch: nn_idx[l] is written only after FPS of this level
        hipLaunchKernelGGL(gather_starts_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, starts, start_l, l, B, P);
        PSG_LAUNCH_CHECK();
        {
            EvScope prof(&ws->prof, TAG_FPS, 0.0, st);
            if ((rc = psg_fps(ws->ctx, ws->xyz[l], n_clouds, P, Np, S, start_l, ws->fps[l], st))) return rc;
        }
        {
            EvScope prof(&ws->prof, TAG_GATHER, 0.0, st);
            if ((rc = psg_gather_points(ws->ctx, ws->xyz[l], n_clouds, P, Np, 3, ws->fps[l], S, ws->xyz[l + 1], st)))
                return rc;
        }
        for (int sc = 0; sc < ws->arch->ns; ++sc) {
            const ScaleDesc &d = ws->arch->sc[l][sc];
            // level 0 of a many-forward plan (ball_table_route): the room's own points as the centroid set (S = N), in a profile
            // scope of its own (psg_pn2_prof_read counts one launch more under TAG_BALL), then one row copy per (problem, centroid)
            const bool table = l == 0 && ws->ball0[sc] && ball_table_route(n_forward, Np);
            if (table) {
                PSG_REQUIRE(d.K % 4 == 0, "psg_pn2_plan_build: nsample=%d is no multiple of 4", d.K);
                EvScope prof(&ws->prof, TAG_BALL, 0.0, st);
                if ((rc = psg_ball_query(ws->ctx, ws->xyz0, B, ws->xyz0, B, Np, Np, d.r2, d.K, ws->ball0[sc], st))) return rc;
            }
            EvScope prof(&ws->prof, TAG_BALL, 0.0, st);
            if (table) {
                const size_t rows = (size_t)P * S, items = rows * (d.K / 4);
                hipLaunchKernelGGL(group_from_table_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, ws->ball0[sc],
                                   ws->fps[0], B, Np, S, d.K / 4, rows, ws->gidx[0][sc]);
                PSG_LAUNCH_CHECK_AT(PSG_SITE "#table");
            } else if ((rc = psg_ball_query(ws->ctx, ws->xyz[l], n_clouds, ws->xyz[l + 1], P, Np, S, d.r2, d.K, ws->gidx[l][sc],
                                            st))) {
                return rc;
            }
            const size_t inv_lds = (size_t)(Np + 1) * 4 + (size_t)S * d.K * 2;
            if (inv_lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)build_inv_group_kernel));
            hipLaunchKernelGGL(build_inv_group_kernel, dim3(P), dim3(INV_NT), inv_lds, st, ws->gidx[l][sc], S * d.K, Np, d.K,
                               ws->ginv_off[l][sc], ws->ginv_pos[l][sc]);
            PSG_LAUNCH_CHECK();
            if (ws->pk_cnt[l] && sc == 0) {
                EvScope prof_pack(&ws->prof, TAG_PACK_PLAN, 0.0, st);
                hipLaunchKernelGGL(sa_pack_plan_kernel, dim3(P), dim3(256), 0, st, ws->gidx[l][0], S, Np, d.P, ws->pk_cnt[l],
                                   ws->pk_seg[l], ws->pk_desc[l]);
                PSG_LAUNCH_CHECK();
            }
        }
        {
            EvScope prof(&ws->prof, TAG_NN, 0.0, st);
            if ((rc = psg_three_nn(ws->ctx, ws->xyz[l], n_clouds, ws->xyz[l + 1], P, Np, S, ws->nn_idx[l], ws->nn_w[l],
                                   st)))
                return rc;
            const size_t nn_lds = (size_t)(S + 1) * 4 + (size_t)3 * Np * 6;
            if (nn_lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)build_inv_nn_kernel));
            hipLaunchKernelGGL(build_inv_nn_kernel, dim3(P), dim3(INV_NT), nn_lds, st, ws->nn_idx[l], ws->nn_w[l],
                               Np, S, ws->inv_off[l], ws->inv_ent[l]);
            PSG_LAUNCH_CHECK();
        }
    }
    ws->planned = n_forward;
    return PSG_OK;
}

extern "C" const void *psg_pn2_plan_ptr(const psg_pn2_ws *ws, int what, int level, int forward, int room)
{
    if (!ws || level < 0 || level > 3 || forward < 0 || forward >= ws->F || room < 0 || room >= ws->B) return nullptr;
    const size_t p = (size_t)forward * ws->B + room;
    switch (what) {
    case 0: return ws->fps[level] + p * kS[level];
    case 1: return ws->gidx[level][0] + p * kS[level] * ws->arch->sc[level][0].K;
    case 2: return ws->nn_idx[level] + p * ws->Nl[level] * 3;
    case 3: return ws->nn_w[level] + p * ws->Nl[level] * 3;
    case 4: return ws->xyz[level + 1] + p * kS[level] * 3;
    case 5: return ws->arch->ns > 1 ? ws->gidx[level][1] + p * kS[level] * ws->arch->sc[level][1].K : nullptr;
    case 6: return ws->pk_cnt[level] ? ws->pk_cnt[level] + p * kS[level] : nullptr;
    case 7: return ws->pk_seg[level] ? ws->pk_seg[level] + p * (kS[level] / (ws->arch->sc[level][0].P / 32) + 2) : nullptr;
    case 9: return ws->pk_desc[level] ? ws->pk_desc[level] + p * (kS[level] / (ws->arch->sc[level][0].P / 32)) : nullptr;
    case 8: return forward == 0 ? ws->arg[level][0] + (size_t)room * kS[level] * ws->arch->c3(level, 0) : nullptr;
    default: return nullptr;
    }
}

extern "C" const float *psg_pn2_activation_ptr(const psg_pn2_ws *ws, int which)
{
    if (!ws || which < 0 || which > 6) return nullptr;
    return ws->act[which];
}

extern "C" int psg_pn2_activation_channels(const psg_pn2_ws *ws, int which)
{
    if (!ws || which < 0 || which > 6) return 0;
    return ws->actC[which];
}

// ================================================================================ forward / backward
// Everything of a forward in front of fp1 + head: the four SA levels and fp4 .. fp2 (whose last launch also writes the T rows
// fp1's split first layer gathers)
static int forward_to_fp2(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *x0, hipStream_t st)
{
    int rc;
    ws->x0_fwd = x0;
    for (int l = 0; l < 4; ++l) {
        for (int sc = 0; sc < m->arch->ns; ++sc) {
            if (m->split_fwd[l] && (rc = run_pw_fwd(m, ws, l, sc, fwd, st))) return rc;
            if ((rc = run_sa_fwd(m, ws, l, sc, fwd, x0, st))) return rc;
        }
    }
    if ((rc = run_fp_fwd<3>(m, ws, fwd, nullptr, st))) return rc;
    if ((rc = run_fp_fwd<2>(m, ws, fwd, nullptr, st))) return rc;
    return run_fp_fwd<1>(m, ws, fwd, nullptr, st);
}

extern "C" int psg_pn2_forward(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *x0, float *logp_out,
                               float *l4_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && x0 && logp_out, "psg_pn2_forward: null argument");
    PSG_REQUIRE(m->arch == ws->arch, "psg_pn2_forward: model and workspace were created for different architectures");
    PSG_REQUIRE(fwd >= 0 && fwd < ws->planned, "psg_pn2_forward: plan slot %d not built (planned %d)", fwd, ws->planned);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = forward_to_fp2(m, ws, fwd, x0, st))) return rc;
    if ((rc = run_fp_fwd<0>(m, ws, fwd, ws->logp, st))) return rc;
    if (logp_out != ws->logp)
        PSG_CHECK_HIP(hipMemcpyAsync(logp_out, ws->logp, (size_t)ws->B * ws->N * NCLS * 4, hipMemcpyDeviceToDevice, st));
    if (l4_out)
        PSG_CHECK_HIP(hipMemcpyAsync(l4_out, ws->act[3], (size_t)ws->B * 16 * ws->actC[3] * 4, hipMemcpyDeviceToDevice, st));
    ws->fwd_slot = fwd;
    return PSG_OK;
}

static int backward_impl(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *logp, const float *dlogp,
                         float *dx0, int c_lo, int c_hi, hipStream_t st, const PgdFuse *pgd = nullptr, bool rel0 = false,
                         bool fp1_done = false)
{
    const ArchDesc &A = *m->arch;
    int rc;
    // no gradient buffer is accumulated into: every row has exactly one writer, consumers gather (fixed order)
    // (fp1_done: the fused launch of the NB step has already written fp1's dZ1 rows; logp / dlogp are not read then)
    if (!fp1_done && (rc = run_fp_bwd<0>(m, ws, fwd, logp, dlogp, st))) return rc;
    if ((rc = run_fp_bwd<1>(m, ws, fwd, nullptr, nullptr, st))) return rc;
    if ((rc = run_fp_bwd<2>(m, ws, fwd, nullptr, nullptr, st))) return rc;
    if ((rc = run_fp_bwd<3>(m, ws, fwd, nullptr, nullptr, st))) return rc;
    for (int l = 3; l >= 0; --l) {
        for (int sc = 0; sc < A.ns; ++sc) {
            // (rel0, psg_pn2_backward_full: level 0 also stores the three rel_xyz columns 9..11 of its rows; same values in 0..8)
            if ((rc = run_sa_bwd(m, ws, l, sc, fwd, l ? 0 : c_lo, l ? A.C[l] : (rel0 ? A.C[0] + 3 : c_hi), st))) return rc;
            if (m->split[l] && (rc = run_pw_bwd(m, ws, l, sc, fwd, st))) return rc;
        }
    }
    {
        EvScope prof(&ws->prof, TAG_ZERO, 0.0, st);   // (tag kept: the slot that used to be the gradient memset)
        const bool compact = c_hi - c_lo == 3;
        const size_t total = (size_t)ws->B * ws->N * (compact ? 1 : c_hi - c_lo);
        const dim3 grid((unsigned)std::min<size_t>(8192, (total + 255) / 256));
        const size_t po = (size_t)fwd * ws->B * (ws->N + 1);
        const int32_t *off = ws->ginv_off[0][0] + po;
        const int32_t *off2 = A.ns > 1 ? ws->ginv_off[0][1] + po : nullptr;
        const float *gsa2 = A.ns > 1 ? ws->gsa[0][1] : nullptr;
        const int gr = kS[0] * A.sc[0][0].K, gr2 = A.ns > 1 ? kS[0] * A.sc[0][1].K : 0;
        if (compact && pgd)
            hipLaunchKernelGGL(dx0_gather_pgd_kernel, grid, dim3(256), 0, st, off, ws->gsa[0][0], gr, off2, gsa2, gr2, ws->B, ws->N, c_lo, *pgd);
        else if (compact)
            hipLaunchKernelGGL(dx0_gather_kernel<true>, grid, dim3(256), 0, st, off, ws->gsa[0][0], gr, off2, gsa2, gr2, ws->B,
                               ws->N, 4, c_lo, c_hi, dx0);
        else
            hipLaunchKernelGGL(dx0_gather_kernel<false>, grid, dim3(256), 0, st, off, ws->gsa[0][0], gr, off2, gsa2, gr2, ws->B,
                               ws->N, gsa_stride(A, 0), c_lo, c_hi, dx0);
        PSG_LAUNCH_CHECK();
    }
    return PSG_OK;
}

// What every backward entry point `who` asks of its (non-null) handles: one architecture, and forward `fwd` is the one whose
// activations, masks and log-probs the workspace holds.
static int require_resident(const psg_pn2_model *m, const psg_pn2_ws *ws, int fwd, const char *who)
{
    PSG_REQUIRE(m->arch == ws->arch, "%s: model and workspace were created for different architectures", who);
    if (ws->fwd_slot != fwd) {
        set_error("%s: forward %d is not the one resident in the workspace (%d)", who, fwd, ws->fwd_slot);
        return PSG_ERR_STATE;
    }
    return PSG_OK;
}

extern "C" int psg_pn2_backward(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *dlogp, float *dx0_out,
                                psg_stream stream)
{
    PSG_REQUIRE(m && ws && dlogp && dx0_out, "psg_pn2_backward: null argument");
    if (int rc = require_resident(m, ws, fwd, "psg_pn2_backward")) return rc;
    // the log_softmax backward reads the log-probs of the resident forward, kept in ws->logp
    return backward_impl(m, ws, fwd, ws->logp, dlogp, dx0_out, 0, 9, (hipStream_t)stream);
}

// The geometric paths of the coordinate gradient, added to channels 0:3 of dx0 (which hold the feature-path gradient):
// psg_pn2_geomgrad.cuh.  Levels from the coarsest down: a level's gradient is complete before it goes down through fps.
static int geometry_grad(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, float *dx0, hipStream_t st)
{
    const ArchDesc &A = *m->arch;
    const int B = ws->B;
    const size_t prob = (size_t)fwd * B;
    auto xyz_of = [&](int l) { return l == 0 ? ws->xyz0 : ws->xyz[l] + prob * ws->Nl[l] * 3; };
    // level 0 is not split: its rows are the grouped-input gradient in LDS channel order [feats(C[0]), rel_xyz(3)]
    const int ld0 = gsa_stride(A, 0), rel0_col = A.C[0];
    for (int l = 1; l < 4; ++l) {   // g_rel rows of the split levels
        const int C1 = A.cout[A.sc[l][0].l0], g_rows = kS[l] * A.sc[l][0].K;
        EvScope prof(&ws->prof, TAG_GEOM_GREL, 0.0, st);
        hipLaunchKernelGGL(sa_grel_kernel, dim3(std::min(256, ceil_div(g_rows, GG_NT / GG_LANES)), B), dim3(GG_NT),
                           (size_t)3 * C1 * sizeof(float), st, ws->gsa[l][0], ws->ginv_off[l][0] + prob * (ws->Nl[l] + 1), ws->Nl[l],
                           g_rows, m->w1x[l], C1, ws->grel[l]);
        PSG_LAUNCH_CHECK();
    }
    for (int l = 0; l < 4; ++l) {   // dL/dd of every fine point's three neighbours
        const bool fs = l < 3 && m->fsplit[l];
        const int C = fs ? A.cout[A.fp_first[l]] : A.cin[A.fp_first[l]] - (l == 0 ? 0 : A.C[l]);
        const float *src = fs ? ws->tfp[l] : ws->act[fp_in2_slot(l)];
        EvScope prof(&ws->prof, TAG_GEOM_WGRAD, 0.0, st);
        hipLaunchKernelGGL(fp_wgrad_kernel, dim3(std::min(512, ceil_div(ws->Nl[l], GG_NT / GG_LANES)), B), dim3(GG_NT), 0, st,
                           ws->dint[l], src, C, ws->nn_idx[l] + prob * ws->Nl[l] * 3, xyz_of(l), xyz_of(l + 1), ws->Nl[l],
                           ws->Nl[l + 1], ws->fpg[l]);
        PSG_LAUNCH_CHECK();
    }
    for (int L = 4; L >= 0; --L) {
        GxArgs a{};
        const int n = ws->Nl[L];
        a.n = n;
        a.xyz = xyz_of(L);
        if (L <= 3) {
            a.src_off = ws->ginv_off[L][0] + prob * (n + 1);
            a.src_n = kS[L] * A.sc[L][0].K;
            if (L == 0) { a.src_rows = ws->gsa[0][0]; a.src_ld = ld0; a.src_col = rel0_col; }
            else { a.src_rows = (const float *)ws->grel[L]; a.src_ld = 4; a.src_col = 0; }
            a.nn_idx = ws->nn_idx[L] + prob * n * 3;
            a.fpg = ws->fpg[L];
            a.xyz_c = xyz_of(L + 1);
            a.n_c = ws->Nl[L + 1];
        }
        if (L >= 1) {
            const int lf = L - 1;
            a.K = A.sc[lf][0].K;
            a.grp_n = kS[lf] * a.K;
            a.grp_pos = ws->ginv_pos[lf][0] + prob * a.grp_n;
            if (lf == 0) { a.grp_rows = ws->gsa[0][0]; a.grp_ld = ld0; a.grp_col = rel0_col; }
            else { a.grp_rows = (const float *)ws->grel[lf]; a.grp_ld = 4; a.grp_col = 0; }
            a.n_f = ws->Nl[lf];
            a.cinv_off = ws->inv_off[lf] + prob * (n + 1);
            a.cinv_ent = ws->inv_ent[lf] + prob * a.n_f * 3;
            a.f_nn_idx = ws->nn_idx[lf] + prob * a.n_f * 3;
            a.f_fpg = ws->fpg[lf];
            a.xyz_f = xyz_of(lf);
        }
        a.out = L == 0 ? dx0 : ws->gxyz[L];
        a.out_ld = L == 0 ? 9 : 3;
        a.accumulate = L == 0 ? 1 : 0;
        EvScope prof(&ws->prof, TAG_GEOM_GX, 0.0, st);   // (with the level's gx_fps_down_kernel)
        hipLaunchKernelGGL(gx_level_kernel, dim3(std::min(2048, ceil_div(B * n, GG_NT))), dim3(GG_NT), 0, st, a, B);
        PSG_LAUNCH_CHECK();
        if (L <= 3) {
            static_assert(GX_FPS_MAX_S >= 1024, "gx_fps_down_kernel holds a room's FPS table (kS[L] entries) in LDS");
            PSG_REQUIRE(kS[L] <= GX_FPS_MAX_S, "psg_pn2_backward_full: level %d has more coarse points than gx_fps_down_kernel holds", L);
            hipLaunchKernelGGL(gx_fps_down_kernel, dim3(B), dim3(GG_NT), 0, st,
                               (const float *)ws->gxyz[L + 1], (const int32_t *)(ws->fps[L] + prob * kS[L]), B, kS[L], n, a.out, a.out_ld);
            PSG_LAUNCH_CHECK();
        }
    }
    return PSG_OK;
}

extern "C" int psg_pn2_backward_full(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *dlogp, float *dx0_out,
                                     psg_stream stream)
{
    PSG_REQUIRE(m && ws && dlogp && dx0_out, "psg_pn2_backward_full: null argument");
    PSG_REQUIRE(m->arch->id == PSG_PN2_ARCH_SSG, "psg_pn2_backward_full: the coordinate gradient is implemented for the SSG "
                "network only (MSG: use psg_pn2_backward, whose channels 0:3 exclude the geometric paths)");
    PSG_REQUIRE(m->split[1] && m->split[2] && m->split[3] && m->w1x[1] && m->w1x[2] && m->w1x[3],
                "psg_pn2_backward_full: needs the split first layers of SA levels 1 - 3 (model created under PSG_PN2_SPLIT=0)");
    PSG_REQUIRE(ws->grel[1] && arch_split(*ws->arch, 1), "psg_pn2_backward_full: workspace created under PSG_PN2_SPLIT=0");
    PSG_REQUIRE(!m->split[0] && gsa_stride(*m->arch, 0) == m->arch->C[0] + 3,
                "psg_pn2_backward_full: level 0's rows are expected whole, [feats, rel_xyz]");
    if (int rc = require_resident(m, ws, fwd, "psg_pn2_backward_full")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = backward_impl(m, ws, fwd, ws->logp, dlogp, dx0_out, 0, 9, st, nullptr, true)) return rc;
    return geometry_grad(m, ws, fwd, dx0_out, st);
}

// The colour channels (3..5) of the input gradient only: what the NU loop's Adam step reads (psg_attack.hip: nu_window_steps).
// Same launches as psg_pn2_backward except at level 0: compact 16-byte rows, the first layer's three colour columns on the vector
// pipe, one gather thread per point; dx0_out[.][3..5] are written, the other six channels of a row are left untouched.
namespace psg {
int pn2_full_grad_check(const psg_pn2_model *m, const psg_pn2_ws *ws, const char *who)
{
    PSG_REQUIRE(m && ws, "%s: null model / workspace", who);
    PSG_REQUIRE(m->arch->id == PSG_PN2_ARCH_SSG && ws->arch->id == PSG_PN2_ARCH_SSG,
                "%s: the coordinate gradient is implemented for the SSG network only", who);
    PSG_REQUIRE(m->split[1] && m->split[2] && m->split[3] && m->w1x[1] && m->w1x[2] && m->w1x[3] && !m->split[0] && ws->grel[1] &&
                    arch_split(*ws->arch, 1),
                "%s: needs the split first layers of SA levels 1 - 3 (model or workspace created under PSG_PN2_SPLIT=0)", who);
    return PSG_OK;
}
// psg_pn2_forward without the module outputs only ws.activation() reads (the NU loop)
int pn2_forward_lean(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *x0, float *logp_out, psg_stream stream)
{
    if (!ws) return psg_pn2_forward(m, ws, fwd, x0, logp_out, nullptr, stream);
    ws->lean = true;
    const int rc = psg_pn2_forward(m, ws, fwd, x0, logp_out, nullptr, stream);
    ws->lean = false;
    return rc;
}
int pn2_backward_colour(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *dlogp, float *dx0_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && dlogp && dx0_out, "pn2_backward_colour: null argument");
    if (int rc = require_resident(m, ws, fwd, "pn2_backward_colour")) return rc;
    return backward_impl(m, ws, fwd, ws->logp, dlogp, dx0_out, 3, 6, (hipStream_t)stream);
}
}  // namespace psg

// The attack loop's own launches one at a time through the C ABI (round 6; include/psg.h): what psg_pn2_nb_attack runs per
// iteration, so that a teacher-forced test drives exactly the kernels the benchmark times
extern "C" int psg_pn2_forward_lean(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *x0, float *logp_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && x0, "psg_pn2_forward_lean: null argument");
    return psg::pn2_forward_lean(m, ws, fwd, x0, logp_out, stream);
}
extern "C" int psg_pn2_backward_colour(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *dlogp, float *dx0_out, psg_stream stream)
{
    return psg::pn2_backward_colour(m, ws, fwd, dlogp, dx0_out, stream);
}
extern "C" int psg_pn2_backward_colour_pgd(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *dlogp, float *x, const float *ori,
                                           const uint8_t *mask, float alpha, float eps, float dir, int last, psg_stream stream)
{
    PSG_REQUIRE(m && ws && dlogp && x && ori, "psg_pn2_backward_colour_pgd: null argument");
    PSG_REQUIRE(dir == 1.0f || dir == -1.0f, "psg_pn2_backward_colour_pgd: dir must be +1 or -1");
    if (int rc = require_resident(m, ws, fwd, "psg_pn2_backward_colour_pgd")) return rc;
    const PgdFuse pf{x, ori, mask, dir * alpha, eps, last ? 1 : 0};
    return backward_impl(m, ws, fwd, ws->logp, dlogp, ws->dx0, 3, 6, (hipStream_t)stream, &pf);
}

// ====================================================================================== NB attack
// One PGD iteration of the NB / tar_NB loop on plan slot `fwd` (nontarget.py:29-39, target.py:31-43): lean forward, loss
// gradient, colour backward with the step applied to x.  Written once: psg_pn2_nb_attack's loop body is this call and nothing
// else, and psg_pn2_nb_step exports it for the teacher-forced tests.
//   non-targeted: CE_sum over all rooms / N (nontarget.py:34); targeted: CE_mean of room 0 (target.py:36-39)
// Where fp1 + head runs as one launch there and back (fp1_loop_applies), the forward stops in front of fp1, the fused launch
// takes the loss gradient with it, and the backward starts behind fp1; ws->logp, ws->dlogp and the four masks of fp1 + head are
// not written then, so no forward is resident for the general backward entry points afterwards.
static int nb_step(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, float *x, const float *ori, const int32_t *labels, const uint8_t *mask,
                   float alpha, float eps, int targeted, int target, bool last, hipStream_t st)
{
    const int B = ws->B, N = ws->N, rows = B * N;
    const int rows_active = targeted ? N : rows;
    const float scale = 1.0f / (float)N, dir = targeted ? -1.0f : 1.0f;
    const bool fused = fp1_loop_applies(m, ws);
    int r;
    if (fused) {
        PSG_REQUIRE(fwd >= 0 && fwd < ws->planned, "psg_pn2_nb_step: plan slot %d not built (planned %d)", fwd, ws->planned);
        ws->lean = true;
        r = forward_to_fp2(m, ws, fwd, x, st);
        ws->lean = false;
        ws->fwd_slot = -1;
        if (r) return r;
        if ((r = run_fp1_loop(m, ws, fwd, labels, target, rows_active, scale, st))) return r;
    } else {
        if ((r = psg::pn2_forward_lean(m, ws, fwd, x, ws->logp, st))) return r;
        EvScope prof(&ws->prof, TAG_CE, 0.0, st);
        if ((r = psg_ce_logp_grad(ws->logp, labels, target, rows, rows_active, NCLS, scale, ws->dlogp, nullptr, st))) return r;
    }
    // (the PGD step rides on the gradient's last gather: dx0_gather_pgd_kernel; PSG_PN2_PGD_FUSE=0: two launches)
    if (sw().pgd_fuse) {
        const PgdFuse pf{x, ori, mask, dir * alpha, eps, last ? 1 : 0};
        return backward_impl(m, ws, fwd, ws->logp, ws->dlogp, ws->dx0, 3, 6, st, &pf, false, fused);
    }
    if ((r = backward_impl(m, ws, fwd, ws->logp, ws->dlogp, ws->dx0, 3, 6, st, nullptr, false, fused))) return r;
    EvScope prof(&ws->prof, TAG_PGD, 0.0, st);
    return psg_pgd_step(x, ws->dx0, ori, mask, B, N, alpha, eps, dir, last, st);
}

extern "C" int psg_pn2_nb_step(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, float *x, const float *ori, const int32_t *labels,
                               const uint8_t *mask, float alpha, float eps, int targeted, int target, int last, psg_stream stream)
{
    PSG_REQUIRE(m && ws && x && ori, "psg_pn2_nb_step: null argument");
    PSG_REQUIRE(m->arch == ws->arch, "psg_pn2_nb_step: model and workspace were created for different architectures");
    PSG_REQUIRE(targeted || labels, "psg_pn2_nb_step: labels required for the non-targeted step");
    PSG_REQUIRE(!targeted || (target >= 0 && target < NCLS), "psg_pn2_nb_step: target class %d out of range", target);
    PSG_REQUIRE(fwd >= 0 && fwd < ws->planned, "psg_pn2_nb_step: plan slot %d not built (planned %d)", fwd, ws->planned);
    return nb_step(m, ws, fwd, x, ori, targeted ? nullptr : labels, mask, alpha, eps, targeted, target, last != 0, (hipStream_t)stream);
}

// The dZ1 rows of fp1 [batch][n_point][128] as the last backward (or fused step) left them: what fp2's backward gathers.
// Read-only, for the tests.
extern "C" const float *psg_pn2_fp1_grad_ptr(const psg_pn2_ws *ws)
{
    return ws ? ws->dint[0] : nullptr;
}

extern "C" int psg_pn2_nb_attack(psg_pn2_model *m, psg_pn2_ws *ws, const float *images, const int32_t *labels,
                                 const int32_t *starts, const uint8_t *mask, float eps, float alpha, int iters,
                                 int targeted, int target, float *adv_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && images && starts && adv_out, "psg_pn2_nb_attack: null argument");
    PSG_REQUIRE(m->arch == ws->arch, "psg_pn2_nb_attack: model and workspace were created for different architectures");
    PSG_REQUIRE(targeted || labels, "psg_pn2_nb_attack: labels required for the non-targeted attack");
    PSG_REQUIRE(iters > 0 && iters <= ws->F, "psg_pn2_nb_attack: iters=%d exceeds workspace capacity %d", iters, ws->F);
    hipStream_t st = (hipStream_t)stream;
    const int B = ws->B, N = ws->N;
    int rc;
    // ---- inputs into the workspace's own buffers (what the captured graph below reads)
    if ((rc = psg_to_point_major(images, B, 9, N, ws->x0, st))) return rc;
    if (!targeted) PSG_CHECK_HIP(hipMemcpyAsync(ws->nb_labels, labels, (size_t)B * N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    PSG_CHECK_HIP(hipMemcpyAsync(ws->nb_starts, starts, (size_t)iters * 4 * B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (mask) PSG_CHECK_HIP(hipMemcpyAsync(ws->nb_mask, mask, (size_t)N, hipMemcpyDeviceToDevice, st));
    const int32_t *labels_ws = targeted ? nullptr : ws->nb_labels;
    const uint8_t *mask_ws = mask ? ws->nb_mask : nullptr;
    // ---- the attack proper: colours aside, geometry of all iterations, iters x (forward, CE gradient, backward, step)
    auto body = [&](hipStream_t st) -> int {         // (`st`: the caller's stream, or the workspace's graph stream)
        int r;
        hipLaunchKernelGGL(extract_color_kernel, dim3(std::min(1024, ceil_div(B * N * 3, 256))), dim3(256), 0, st, ws->x0,
                           ws->ori, (size_t)B * N);
        PSG_LAUNCH_CHECK();
        if ((r = psg_pn2_plan_build(ws, ws->x0, ws->nb_starts, iters, st))) return r;
        for (int it = 0; it < iters; ++it)
            if ((r = nb_step(m, ws, it, ws->x0, ws->ori, labels_ws, mask_ws, alpha, eps, targeted, target, it == iters - 1, st))) return r;
        return PSG_OK;
    };
    // Pn2Switches::graph (off): a harness that calls the attack batch after batch (NB_nontarget_test_semseg.py:169-171) repeats
    // exactly these ~1 300 launches with exactly these arguments, so the second call with a key captures them into a hipGraph
    // kept in the workspace and later calls replay it (same bits: tests/test_gpu_api.py).  On this runtime the replay is SLOWER:
    // one 8-room attack at a time 324 -> 307 rooms/s, four in flight 541 -> 386.
    const bool use_graph = sw().graph && !psg::trace_sync_enabled();
    if (use_graph && B <= 16 && !ws->prof.on) {
        const psg_pn2_ws::NbKey key{m->gen, eps, alpha, iters, targeted ? 1 : 0, targeted ? target : 0, mask ? 1 : 0, targeted ? 0 : 1, 0};
        const bool same = ws->nb_have_key && memcmp(&key, &ws->nb_key, sizeof(key)) == 0;
        if (same && !ws->nb.capture_failed) {
            if (!ws->nb_stream) {
                PSG_CHECK_HIP(hipStreamCreateWithFlags(&ws->nb_stream, hipStreamNonBlocking));
                for (hipEvent_t &e : ws->nb_ev) PSG_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            }
            hipStream_t gs = ws->nb_stream;
            // the graph stream starts after everything the caller's stream holds so far (the copies above included) ..
            PSG_CHECK_HIP(hipEventRecord(ws->nb_ev[0], st));
            PSG_CHECK_HIP(hipStreamWaitEvent(gs, ws->nb_ev[0], 0));
            if (ws->nb.exec || ws->nb.capture(gs, [&] { return body(gs); })) {
                PSG_CHECK_HIP(ws->nb.replay(gs));
                // (the host-side state the eager body leaves)
                ws->planned = iters; ws->fwd_slot = fp1_loop_applies(m, ws) ? -1 : iters - 1; ws->x0_fwd = ws->x0;
                // .. and the caller's stream goes on after the attack
                PSG_CHECK_HIP(hipEventRecord(ws->nb_ev[1], gs));
                PSG_CHECK_HIP(hipStreamWaitEvent(st, ws->nb_ev[1], 0));
                return psg_to_channel_major(ws->x0, B, 9, N, adv_out, st);
            }
        }
        if (!same) {
            PSG_CHECK_HIP(ws->nb.forget(st));
            ws->nb_key = key;
            ws->nb_have_key = true;
        }
        ws->nb.note_eager();
    }
    if ((rc = body(st))) return rc;
    return psg_to_channel_major(ws->x0, B, 9, N, adv_out, st);
}
