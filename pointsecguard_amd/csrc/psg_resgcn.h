// Internal (not part of the C ABI): the model and workspace handles of ResGCN (psg_resgcn.hip owns and fills them), read by
// the attack drivers of psg_resgcn_attack.hip, with what those drivers call back into the network unit for.
#pragma once
#include <tuple>
#include "psg_common.h"
#include "psg_gcn_plan.h"

struct EdgeLayer {
    float *wcat;    // [128][C]: rows 0..63 = W1 - W2, rows 64..127 = W2
    float *bcat;    // [128] = [b, 0]
    float *wcat_t;  // [C][128] (transpose, for the input gradient)
    float *wcat_k8 = nullptr;   // C == 64: wcat as MFMA operand blocks [k / 8][128][8] (edge_max_pq_fwd_kernel)
    float *scale, *shift;  // eval BatchNorm after the ReLU
    float *w = nullptr, *b = nullptr;   // conv = mr: plain [64][2C] weight and [64] bias of the BasicConv
    float *w_t = nullptr;               // conv = mr: [2C][64] transpose (input gradient)
};

struct psg_gcn_model {
    uint64_t gen = psg::next_generation();   // never re-used (psg_common.h): what the replayed NB iteration is keyed on
    psg_ctx *ctx;
    psg_gcn::GcnCfg cfg;                  // block / conv kind (architecture.py:26-39, torch_vertex.py:44-49), n_blocks
    std::vector<EdgeLayer> edge;
    float *wf, *bf, *sf, *tf;             // fusion 1792 -> 1024
    float *wp1, *bp1, *s1, *t1;           // prediction.0: 2816 -> 512 (columns: [fusion 1024 | feats 1792])
    float *wp2, *bp2, *s2, *t2;           // 512 -> 256
    float *wp3, *bp3;                     // 256 -> 13
    float *wp3_t;                         // [256][13]
    float *wp2_st;                        // [512][256]: W2^T with BatchNorm scale s2 folded (by W2's output row)
    float *wp1b_st;                       // [1792][512]: W1b^T with s1 folded
    float *wp1a_st;                       // [1024][512]: (s1 * W1a)^T (for the fusion-vector gradient)
    int fdim;                             // 64 * n_blocks
    void *arena = nullptr;                // every weight block above, one allocation
};

constexpr int kGcnFieldColour = 0;    // the NB loop's field beside PSG_NU_FIELD_COORD (1) and PSG_NU_FIELD_BOTH (2)
struct NbKey {   // what a captured NB iteration is valid for
    uint64_t model_gen = 0;          // the model's generation number, not its address (psg_common.h)
    int field = 0;
    float eps = 0.f, alpha = 0.f, coord_eps = 0.f, coord_alpha = 0.f;
    bool fixed_graphs = false;
    auto tie() const { return std::tie(model_gen, field, eps, alpha, coord_eps, coord_alpha, fixed_graphs); }
    bool operator==(const NbKey &o) const { return tie() == o.tie(); }
};
// hipGraph of one interior PGD iteration (forward, CE, backward, step): ~300 short launches replayed as one graph launch
struct NbGraph { psg::GraphSlot slot; NbKey key; };

struct psg_gcn_ws {
    uint64_t gen = psg::next_generation();   // never re-used: what the replayed NU windows are keyed on (psg_common.h)
    psg_ctx *ctx;
    int B, N, fdim;
    psg_gcn::GcnCfg cfg;
    int pq_w = 128;            // row width of pq / dpq: 128, or 2 * (widest conv input) for conv = mr
    uint8_t *arg_mr = nullptr; // conv = mr: [sum_e C_e][B*N] winning neighbour of every (layer, vertex, channel)
    uint32_t *mask_mr = nullptr; // conv = mr: [n_blocks][B*N][2] ReLU bits of every layer's conv output
    void *arena = nullptr;
    size_t bytes = 0;
    float *feats, *dfeats;     // [B*N][fdim]
    float *dist;               // [B*N][N]
    float *sq;                 // [B*N]
    float *xp;                 // [B*N][64] the current block's features in fp32 MFMA operand order (exact fused kNN)
    void *bp;                  // [B*N/32][9][64] 16-byte bf16 hi / lo / augmented fragments (prefilter kNN, psg_knn_ops.cuh)
    psg_gcn::GcnKnnSwitches knn;   // as the environment stood at creation; mode 0 also where the device does not grant the kernels' LDS
    unsigned long long *knn_stats = nullptr;   // knn.stats: device counters of the prefilter kernel
    float *pq, *dpq;           // [B*N][128]
    float *pq2 = nullptr;      // second [P | Q] buffer: a block's edge pass writes the NEXT block's products while it reads its own
    float *dpq2;               // second [B*N][128] gradient buffer of the default (res / edge) backward's ping-pong
    int32_t *nbr;              // [n_blocks][B*N][16]
    uint8_t *arg;              // [n_blocks][B*N][64]
    float *fused;              // [B*N][1024]
    uint32_t *mask_f, *mask1, *mask2;
    float *fmax; int32_t *farg; // [B][1024]
    unsigned long long *fkeys;  // [B][1024] packed (value, ~row) keys of the global max
    float *gb1;                // [B][512]
    float *h1, *h2;            // [B*N][512], [B*N][256]
    float *g2, *g1;            // backward buffers [B*N][256], [B*N][512]
    float *g1sum, *gfvec;      // [B][512], [B][1024]
    float *g1part;             // [B][ceil(N / 64)][512] per-chunk column sums (added up in chunk order)
    float *gcur;               // [B*N][64]
    float *logits, *dlogits;   // [B*N][13]
    float *x0, *ori, *dx0;     // attack state [B*N][9], [B*N][3], [B*N][9]
    float *xyz;                // [B*N][3]
    float *ori_xyz;            // [B*N][3] the clean coordinates of the coordinate-field NB loop
    int32_t *nb_labels;        // [B*N] the attack's labels, copied so that the captured kernels' arguments never change
    bool have_fwd = false;
    bool fixed_graphs = false;  // psg_gcn_set_graphs: forward uses the supplied neighbour tables
    bool head_graph_frozen = false;  // inside a colour attack loop: xyz never changes, the head's xyz kNN graph is kept
    // the colour loop's graph and the field loop's, a holder each: one survives a call of the other
    NbGraph nb, nbf;
    psg::EvLog prof;           // psg_gcn_prof_enable
    // psg_gcn_debug_keep: a second arena of per-block copies of what the loops overwrite (null = off, the one pointer the host
    // path tests per block).  Strides per block: pq_w floats per row for k_pq / k_dpq, fdim for k_state.
    void *keep = nullptr;
    float *k_pq, *k_dpq;       // [n_blocks][B*N][pq_w]: every block's [P | Q] (mr: cat) and [dP | dQ] (mr: dcat)
    float *k_gz;               // [n_blocks][B*N][64]: conv = mr, every block's mr_dz output
    float *k_state;            // [n_blocks] slots of B*N*fdim floats: after block e, gcur packed [B*N][64] (res / edge) or dfeats [B*N][fdim]
    float *k_dfh, *k_dff;      // [B*N][fdim]: dfeats as the prediction head left it, and after the fusion transpose
    float *k_dx0;              // [B*N][9]
};

const psg_gcn::GcnSwitches &gcn_switches();   // read at the first call
inline bool gcn_same_cfg(const psg_gcn_model *m, const psg_gcn_ws *ws) { return m->cfg == ws->cfg; }
// The NB prologue's copies out of ws->x0 (point-major rows of 9): colours -> ws->ori and, `xyz`, coordinates -> ws->ori_xyz
int gcn_extract_clean(psg_gcn_ws *ws, bool xyz, hipStream_t st);
// the attack entry points capture and replay forwards: refused while psg_gcn_debug_keep is on (PSG_ERR_STATE), PSG_OK otherwise
int gcn_keep_refuses(const psg_gcn_ws *ws, const char *who);
