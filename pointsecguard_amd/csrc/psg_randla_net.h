// Internal (not part of the C ABI): the model and workspace handles of RandLA-Net (psg_randla_net.hip owns and fills them),
// read by the attack drivers of psg_randla_attack.hip, with the two things those drivers call back into the network unit for.
#pragma once
#include <vector>

#include "psg_common.h"

constexpr int RL = 5;            // encoder levels
constexpr int RK = 16;           // neighbours
constexpr int RNCLS = 13;

struct RLayer {
    float *w = nullptr;    // [cout][cin]  BatchNorm scale folded in
    float *wt = nullptr;   // [cin][cout]
    float *b = nullptr;    // [cout] folded bias, or null
    int cin = 0, cout = 0;
};

struct EncLayers { RLayer mlp1, lfa_mlp1, att1_fc, att1_mlp, lfa_mlp2, att2_fc, att2_mlp, mlp2, shortcut; };

struct psg_rla_model {
    uint64_t gen = psg::next_generation();   // never re-used (psg_common.h): what the replayed BIM iteration is keyed on
    psg_ctx *ctx;
    RLayer fc0, decoder0, dec[RL], fc1, fc2, fc;
    EncLayers enc[RL];
    std::vector<void *> allocs;
};

struct LevelBuf {
    int n = 0, n_sub = 0, d = 0, h = 0, d_in = 0;   // n, n_sub: rows of ALL clouds of the workspace (B * per-cloud counts)
    int nc = 0, nc_sub = 0;                         // per cloud
    float *xyz = nullptr;                           // [B][nc][3]: the level's points, cloud by cloud
    int32_t *neigh = nullptr, *up = nullptr;   // [n][16], [n][1] (row numbers of this level / of the next); pool = a cloud's first nc_sub rows
    // transposes of the two index arrays (the geometry is fixed for a whole attack, so they are built once per cloud): for every
    // row j of this level the edges e = p * 16 + k with neigh[e] == j, ascending (inv_off [n + 1], inv_ent [n * 16]); for every row
    // t of the next level the rows n with up[n] == t, ascending (invu_off [n_sub + 1], invu_ent [n]).  The backward pass GATHERS
    // through them in that fixed order instead of scattering with float atomics: bit-reproducible, and faster.
    int32_t *inv_off = nullptr, *inv_ent = nullptr, *invu_off = nullptr, *invu_ent = nullptr;
    // the same for the edges of the SAMPLED points only (the max-pool reads just those): entries i = r * 16 + k, r a sampled row
    int32_t *invp_off = nullptr, *invp_ent = nullptr;
    float *relpos, *fxyz1, *fxyz2;             // [n*16][10], [n*16][h] x2
    float *fpc, *cat1, *a1, *agg1, *fagg1, *cat2, *a2, *agg2, *fagg2, *m2, *sc, *enc, *samp;
    uint32_t *m_fpc, *m_fagg1, *m_fagg2, *m_enc;
    uint8_t *arg;
    float *d_enc, *d_samp;                     // gradients w.r.t. enc [n][2d] and samp [n_sub][2d]
    float *d_fpc, *d_fagg1;                    // [n][h]
    // full workspaces only (psg_rla_ws_create_full), the position-branch gradient: sign words of fxyz1 / fxyz2 [16n][ceil(h/32)],
    // G2 / G1 [16n][h] (gradients of the pre-activations of LFAmlp2 / LFAmlp1), g_rp [16n][10], what every edge hands to its
    // point i and to its neighbour j ([16n] float4 each), gxyz [n][3]
    uint32_t *m_fxyz1 = nullptr, *m_fxyz2 = nullptr;
    float *G1 = nullptr, *G2 = nullptr, *g_rp = nullptr, *gxyz = nullptr;
    float4 *side_i = nullptr, *side_j = nullptr;
};

struct psg_rla_ws {
    uint64_t gen = psg::next_generation();   // never re-used (psg_common.h): what a replayed NU window is keyed on
    psg_ctx *ctx;
    int N = 0;                      // rows of all clouds: B * Nc
    int B = 1, Nc = 0;              // clouds per workspace (independent: every index stays inside its cloud), points per cloud
    void *arena = nullptr;
    size_t bytes = 0;
    float *xyz_all;                 // [B][Nc][3]; a level's points are the first Nc / ratio points of each cloud
    float *xyz_last;                // [B][nc5][3]: the sub-sampled points of the last level
    LevelBuf lv[RL];
    float *f0; uint32_t *m_f0;      // fc0 output [N][8]
    float *dec0; uint32_t *m_dec0;  // decoder_0 output [n5][1024]
    float *dec_cat[RL], *dec_out[RL]; uint32_t *m_dec[RL];
    float *fc1o, *fc2o; uint32_t *m_fc1, *m_fc2;
    float *logits, *dlogits;
    float *scratch_a, *scratch_b;   // [max edges * d] gradient scratch (dcat / ds), also decoder d_cat
    float *d_f0, *d_dec0, *d_dec_out[RL], *d_fc1o, *d_fc2o;
    char *acc = nullptr; size_t acc_bytes = 0;   // the contiguous block of gradient accumulators
    float *feat, *dfeat, *ori, *delta, *norms;   // attack state: [N][6], [N][6], [N][3], [N][3], [2][B] (l_2: squared gradient / delta norm per cloud)
    int32_t *labels;
    bool cloud_set = false, have_fwd = false;
    bool fuse16 = true;           // PSG_RLA_NO_FUSE16=1: the unfused chain at level 0 too (A/B runs, tests)
    bool split = true;            // PSG_RLA_NO_SPLIT=1: levels 1-4 through the gather + per-edge score GEMM chain (A/B runs)
    bool use_inv = true;          // PSG_RLA_ATOMICS=1: the scatter kernels with float atomics instead of the inverse-list gathers
    bool full = false;            // psg_rla_ws_create_full: the buffers of the coordinate gradient, level 0 on the unfused chain
    size_t scratch_bytes = 0;     // of scratch_a and of scratch_b
    psg::EvLog prof;              // psg_rla_prof_enable
    uint64_t xyz_branch_model = 0;   // generation number (not the address: a freed model's address can come back) of the model whose xyz-branch features (fxyz1 / fxyz2) are resident
    // hipGraph of one BIM iteration (forward, loss gradient, backward, update: ~150 short launches), valid for the
    // (model, eps, alpha, metric) below; every captured kernel works on workspace buffers, so it is cloud-independent
    psg::GraphSlot bim;
    uint64_t bim_model_gen = 0;      // the model's generation number, not its address (psg_common.h)
    float bim_eps = 0.f, bim_alpha = 0.f;
    int bim_metric = -1;
};

namespace {

// dst[r][d0 .. d0 + nc) = src[r][c0 .. c0 + nc): used by the backward pass and by the BIM loop's set-up
__global__ void copy_cols_kernel(const float *__restrict__ src, int ld_s, int c0, int nc, size_t rows, float *__restrict__ dst, int ld_d, int d0)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * nc) return;
    const size_t r = t / nc;
    const int c = (int)(t % nc);
    dst[r * ld_d + d0 + c] = src[r * ld_s + c0 + c];
}

inline unsigned blocks_for(size_t total) { return (unsigned)((total + 255) / 256); }

}  // namespace

namespace psg {

// The index pyramid of the reference's tf_map (main_S3DIS.py:198-207) and the relative position encodings, from the
// cloud in ws->xyz_all.
int build_pyramid(psg_rla_ws *ws, psg_stream stream);

struct ProfBind {   // routes rl_gemm's scopes to the workspace of the call in progress
    EvLog *prev;
    explicit ProfBind(psg_rla_ws *ws);
    ~ProfBind();
};

}  // namespace psg
