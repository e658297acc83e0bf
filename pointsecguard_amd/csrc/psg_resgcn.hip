// ResGCN-28 (dense DeepGCN) semantic-segmentation network on gfx950: the model, the workspace, forward, input-gradient
// backward and the per-operator entry points.  Its kernels are psg_resgcn_kernels.cuh, its handles psg_resgcn.h, the per-block
// plan and the switch set psg_gcn_plan.h, the attack loops psg_resgcn_attack.hip.  Reference (paths relative to its ResGCN directory):
//   gcn_lib/dense/torch_edge.py:32-79   pairwise_distance, dense_knn_matrix, DenseDilated(KnnGraph)
//   gcn_lib/dense/torch_nn.py:55-98     BasicConv (Conv -> ReLU -> BatchNorm), batched_index_select
//   gcn_lib/dense/torch_vertex.py:23-100 EdgeConv2d, DynConv2d, ResDynBlock2d
//   sem_seg_dense/architecture.py:58-68  DenseDeepGCN.forward
//
// MI355X-first choices:
//   * EdgeConv uses the split identity W.[x_i, x_j - x_i] = (W1 - W2) x_i + W2 x_j: one 64->128 GEMM per
//     vertex ([P | Q]) instead of a 128->64 GEMM per EDGE (16x fewer MACs), then a gather kernel does
//     relu(P_i + Q_j) -> BatchNorm affine -> max over the 16 neighbours (+ residual) in one pass.
//   * the feature-space kNN distance matrix is an fp32 MFMA GEMM whose accumulation order is the
//     ascending-k fmaf chain of a CPU sgemm (bit-identical distances for bit-identical features); the
//     top-(k*d) selection is an in-LDS bitonic sort of (distance, index) keys per row, ties -> lowest index.
//   * backward exploits structure: the global max-pool makes the fusion layer's gradient 1024-sparse
//     (one point per channel), so its 1792x1024 transpose GEMM collapses to 1024 scaled row additions;
//     the broadcast fusion term of the first prediction layer becomes a per-room bias (forward) and a
//     column sum + mat-vec (backward).
#include "psg_resgcn.h"
using namespace psg;
using namespace psg_gcn;
#include "psg_resgcn_kernels.cuh"

const GcnSwitches &gcn_switches()
{
    static const GcnSwitches sw = read_switches(psg::env_int, psg::env_str);   // once per process, at the first use of any
    return sw;
}

namespace {

void bn_affine(const float *g, const float *b, const float *mu, const float *var, int n, std::vector<float> &s,
               std::vector<float> &t)
{
    s.resize(n); t.resize(n);
    for (int i = 0; i < n; ++i) {
        double sc = (double)g[i] / sqrt((double)var[i] + 1e-5);
        s[i] = (float)sc;
        t[i] = (float)((double)b[i] - (double)mu[i] * sc);
    }
}

// out[k][o] = W[o][col0 + k] (* s[o]): a [rows][ld] weight's columns col0 .. col0 + cols transposed for an input-gradient
// pass, the BatchNorm scale of the layer's output rows folded in where `s` is given
std::vector<float> transposed(const float *W, int rows, int ld, int col0, int cols, const std::vector<float> &s = {})
{
    std::vector<float> out((size_t)rows * cols);
    for (int o = 0; o < rows; ++o)
        for (int k = 0; k < cols; ++k) {
            const float w = W[(size_t)o * ld + col0 + k];
            out[(size_t)k * rows + o] = s.empty() ? w : w * s[o];
        }
    return out;
}

enum GcnTag { GT_KNN = 0, GT_KNN_OTHER, GT_VERTEX_GEMM, GT_EDGE_MAX, GT_HEAD, GT_BACKWARD, GT_COUNT };

// which kernel builds the dilated graph of C-wide features: the bf16-prefilter kernel (default), the exact fused kernel
// (PSG_GCN_KNN=f32, and sizes the prefilter does not take), or -1 = the round-1 path (distance matrix in HBM + selection
// kernel: the xyz graph of the head, dense blocks, PSG_GCN_KNN=matrix)
int knn_path(const psg_gcn_ws *ws, int C, int d)
{
    if (ws->knn.mode == 0 || C != 64) return -1;
    if (ws->knn.mode == 2 && d <= ws->knn.bf_max_d && knn_shape_ok(ws->N, KNB, d, KNN_PATH_BF16)) return KNN_PATH_BF16;
    return knn_shape_ok(ws->N, KNB, d, KNN_PATH_F32) ? KNN_PATH_F32 : -1;
}

// pairwise_distance, torch_edge.py:32-42: x [B][N][ld] (C used columns) -> out [B][N][N] = (|x_i|^2 + (-2 x_i.x_j)) + |x_j|^2 with
// the reference's fp32 order (norms in torch.sum's order - written to sq [B*N] unless `have_sq` -, dot products as the ascending-k
// fmaf chain); distances never cross rooms
int pairwise_distance(const float *x, int ld, int B, int N, int C, float *sq, bool have_sq, float *out, hipStream_t st)
{
    const size_t rows = (size_t)B * N;
    if (!have_sq) {
        hipLaunchKernelGGL(sumsq_rows_kernel, dim3(ceil_div((int)rows, 256)), dim3(256), 0, st, x, ld, C, rows, sq);
        PSG_LAUNCH_CHECK();
    }
    for (int b = 0; b < B; ++b) {
        GemmArgs a = gemm_args(x + (size_t)b * N * ld, ld, x + (size_t)b * N * ld, ld, out + (size_t)b * N * N, N, N, C, N);
        a.sq = sq + (size_t)b * N;
        if (int rc = launch_gemm<2, 2, EPI_KNN_DIST, true>(a, st)) return rc;
    }
    return PSG_OK;
}

// have_sq: ws->sq (and, on the fused paths, ws->xp / ws->bp) already hold the norms / operand copies of x (the forward
// pass gets them from the producing edge_max_fwd kernel)
int knn_graph(psg_gcn_ws *ws, const float *x, int ld, int C, int d, int32_t *out, hipStream_t st, bool have_sq = false)
{
    const size_t rows = (size_t)ws->B * ws->N;
    const int path = knn_path(ws, C, d);
    if (path >= 0) {
        KnnBuffers buf;
        buf.xp = ws->xp; buf.bp = ws->bp; buf.sq = ws->sq; buf.stats = ws->knn_stats; buf.x = x; buf.ld = ld;
        if (!have_sq) PSG_CHECK_HIP(knn_prep_launch(x, ld, rows, buf, path == KNN_PATH_BF16, st));
        EvScope prof(&ws->prof, GT_KNN, 2.0 * ws->B * (double)ws->N * ws->N * 64.0, st);
        PSG_CHECK_HIP(knn_launch(buf, ws->B, ws->N, KNB, d, out, (KnnPath)path, st));
        return PSG_OK;
    }
    EvScope prof(&ws->prof, GT_KNN_OTHER, 2.0 * ws->B * (double)ws->N * ws->N * C, st);   // round-1 path, xyz graph
    if (int rc = pairwise_distance(x, ld, ws->B, ws->N, C, ws->sq, have_sq, ws->dist, st)) return rc;
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)ceil_div((int)rows, KS_WAVES)), dim3(KS_WAVES * 64), 0, st, ws->dist,
                       ws->N, rows, KNB, d, out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

}  // namespace

// ============================================================================================ model
// tensors (host pointers, fp32), in this order:
//   for each EdgeConv e = 0 (head) .. n_blocks-1:  conv.weight [64][2C], conv.bias [64], bn.weight, bn.bias,
//                                                 bn.running_mean, bn.running_var [64]      (C = 9 for e = 0, else 64)
//   fusion_block: weight [1024][64*n_blocks], bias, bn x4 [1024]
//   prediction.0: weight [512][1024 + 64*n_blocks], bias, bn x4 [512]
//   prediction.1: weight [256][512], bias, bn x4 [256]
//   prediction.3: weight [13][256], bias [13]
//
// block = dense (DenseDynBlock2d, torch_vertex.py:103-115): EdgeConv e reads ALL earlier outputs (C = 64 e) and the
// fusion / prediction.0 layers see every block's growing concatenation, i.e. output y_j of block j (64 channels)
// occurs n_blocks - j times among their input columns (architecture.py:62-63 with :112-115).  Those duplicate columns
// are summed on the host into one [.., 64 * n_blocks] weight: W_eff[:, y_j] = sum_{i >= j} W[:, copy of y_j in cur_i],
// so everything downstream of the backbone is the same computation as for block = res.
extern "C" int psg_gcn_model_create_cfg(psg_ctx *ctx, const float *const *tensors, int n_tensors, int n_blocks, int block,
                                        int conv, psg_gcn_model **out)
{
    PSG_REQUIRE(ctx && tensors && out, "psg_gcn_model_create: null argument");
    PSG_REQUIRE(block >= PSG_GCN_BLOCK_RES && block <= PSG_GCN_BLOCK_DENSE, "psg_gcn_model_create: unknown block kind %d", block);
    PSG_REQUIRE(conv == PSG_GCN_CONV_EDGE || conv == PSG_GCN_CONV_MR, "psg_gcn_model_create: unknown conv kind %d", conv);
    PSG_REQUIRE(n_blocks >= 1 && n_blocks <= 64, "psg_gcn_model_create: n_blocks out of range");
    PSG_REQUIRE(n_tensors == 6 * n_blocks + 6 + 6 + 6 + 2, "psg_gcn_model_create: expected %d tensors, got %d",
                6 * n_blocks + 20, n_tensors);
    for (int i = 0; i < n_tensors; ++i) PSG_REQUIRE(tensors[i], "psg_gcn_model_create: tensor %d is null", i);
    PSG_CHECK_HIP(hipSetDevice(ctx->device));
    auto *m = new psg_gcn_model();
    m->ctx = ctx; m->cfg = GcnCfg{block, conv, n_blocks}; m->fdim = GC * n_blocks;
    m->edge.resize(n_blocks);
    // every weight block of the model, listed once (where its device pointer goes, its host values); the arena is carved from the list
    std::vector<std::pair<float **, std::vector<float>>> blocks;
    auto add = [&](float *&dst, std::vector<float> v) { blocks.emplace_back(&dst, std::move(v)); };
    auto vec = [](const float *p, size_t n) { return std::vector<float>(p, p + n); };
    // eval BatchNorm (weight, bias, running mean, running var at t[0..3]) as a scale and a shift block; returns the scale
    auto add_bn = [&](const float *const *t, int n, float *&scale, float *&shift) {
        std::vector<float> s, h;
        bn_affine(t[0], t[1], t[2], t[3], n, s, h);
        add(scale, s); add(shift, std::move(h));
        return s;
    };
    int ti = 0;
    for (int e = 0; e < n_blocks; ++e, ti += 6) {
        const int C = gcn_block(m->cfg, e).C;
        const float *W = tensors[ti], *b = tensors[ti + 1];
        std::vector<float> wcat((size_t)2 * GC * C), bcat(2 * GC, 0.0f), wk(C == GC ? (size_t)2 * GC * C : 0);
        for (int o = 0; o < GC; ++o) {
            bcat[o] = b[o];
            for (int c = 0; c < C; ++c) {
                const float w1 = W[(size_t)o * 2 * C + c], w2 = W[(size_t)o * 2 * C + C + c];
                wcat[(size_t)o * C + c] = w1 - w2;
                wcat[(size_t)(GC + o) * C + c] = w2;
            }
        }
        for (size_t r = 0; r < 2 * GC && C == GC; ++r)
            for (int c = 0; c < C; ++c) wk[((size_t)(c >> 3) * 2 * GC + r) * 8 + (c & 7)] = wcat[r * C + c];
        EdgeLayer &L = m->edge[e];
        add(L.wcat_t, transposed(wcat.data(), 2 * GC, C, 0, C));
        add(L.wcat, std::move(wcat)); add(L.bcat, std::move(bcat));
        if (C == GC) add(L.wcat_k8, std::move(wk));
        add_bn(tensors + ti + 2, GC, L.scale, L.shift);
        if (conv == PSG_GCN_CONV_MR) {
            add(L.w, vec(W, (size_t)GC * 2 * C)); add(L.b, vec(b, GC)); add(L.w_t, transposed(W, GC, 2 * C, 0, 2 * C));
        }
    }
    const int F = m->fdim;
    // fold the duplicated feature columns of a dense backbone (see above): src has `lead` leading columns kept as
    // they are, then the concatenation cur_0 | cur_1 | ... with cur_i = y_0 .. y_i
    std::vector<std::vector<float>> folded;
    auto fold_dense = [&](const float *W, int rows, int lead) -> const float * {
        if (block != PSG_GCN_BLOCK_DENSE) return W;
        const int fd = GC * n_blocks * (n_blocks + 1) / 2;
        std::vector<float> o((size_t)rows * (lead + F), 0.0f);
        for (int r = 0; r < rows; ++r) {
            const float *src = W + (size_t)r * (lead + fd);
            float *dst = o.data() + (size_t)r * (lead + F);
            for (int k = 0; k < lead; ++k) dst[k] = src[k];
            std::vector<double> acc(F, 0.0);
            int off = lead;
            for (int i = 0; i < n_blocks; ++i) {
                for (int k = 0; k < GC * (i + 1); ++k) acc[k] += (double)src[off + k];
                off += GC * (i + 1);
            }
            for (int k = 0; k < F; ++k) dst[lead + k] = (float)acc[k];
        }
        folded.push_back(std::move(o));
        return folded.back().data();
    };
    // a head layer [rows][cols] at tensors[ti]: weight (lead >= 0: over the feature concatenation behind `lead` columns,
    // folded), bias and, where `s` is given, its BatchNorm; returns the weight as uploaded and the scale, for the transposes
    struct HeadLayer { const float *W; std::vector<float> s; };
    auto head_layer = [&](int rows, int cols, int lead, float *&w, float *&b, float **s, float **t) {
        HeadLayer h{lead >= 0 ? fold_dense(tensors[ti], rows, lead) : tensors[ti], {}};
        add(w, vec(h.W, (size_t)rows * cols)); add(b, vec(tensors[ti + 1], rows));
        if (s) h.s = add_bn(tensors + ti + 2, rows, *s, *t);
        ti += 6;
        return h;
    };
    head_layer(1024, F, 0, m->wf, m->bf, &m->sf, &m->tf);
    const HeadLayer p1 = head_layer(512, 1024 + F, 1024, m->wp1, m->bp1, &m->s1, &m->t1);
    const HeadLayer p2 = head_layer(256, 512, -1, m->wp2, m->bp2, &m->s2, &m->t2);
    const HeadLayer p3 = head_layer(NCLS, 256, -1, m->wp3, m->bp3, nullptr, nullptr);
    // transposes for the input-gradient pass, BatchNorm scales folded in
    add(m->wp3_t, transposed(p3.W, NCLS, 256, 0, 256));
    add(m->wp2_st, transposed(p2.W, 256, 512, 0, 512, p2.s));
    add(m->wp1b_st, transposed(p1.W, 512, 1024 + F, 1024, F, p1.s));
    add(m->wp1a_st, transposed(p1.W, 512, 1024 + F, 0, 1024, p1.s));
    // one arena (256-byte aligned blocks), a host image of it, one upload
    size_t bytes = 0;
    if (int rc = carve_arena(&m->arena, &bytes, "psg_gcn_model_create", [&](Bump &bp) {
            for (auto &w : blocks) *w.first = bp.take<float>(w.second.size());
        })) {
        delete m;
        return rc;
    }
    std::vector<char> host(bytes);
    for (auto &w : blocks) memcpy(host.data() + ((char *)*w.first - (char *)m->arena), w.second.data(), w.second.size() * 4);
    if (psg::copy_sync(m->arena, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        psg_gcn_model_destroy(m);
        set_error("psg_gcn_model_create: weight upload failed");
        return PSG_ERR_HIP;
    }
    *out = m;
    return PSG_OK;
}

extern "C" int psg_gcn_model_create(psg_ctx *ctx, const float *const *tensors, int n_tensors, int n_blocks, psg_gcn_model **out)
{
    return psg_gcn_model_create_cfg(ctx, tensors, n_tensors, n_blocks, PSG_GCN_BLOCK_RES, PSG_GCN_CONV_EDGE, out);
}

extern "C" int psg_gcn_model_destroy(psg_gcn_model *m)
{
    if (!m) return PSG_OK;
    if (m->arena) (void)hipFree(m->arena);
    delete m;
    return PSG_OK;
}

// ======================================================================================== workspace
extern "C" int psg_gcn_ws_create_cfg(psg_ctx *ctx, int batch, int n_point, int n_blocks, int block, int conv, psg_gcn_ws **out)
{
    PSG_REQUIRE(ctx && out, "psg_gcn_ws_create: null argument");
    PSG_REQUIRE(block >= PSG_GCN_BLOCK_RES && block <= PSG_GCN_BLOCK_DENSE && (conv == PSG_GCN_CONV_EDGE || conv == PSG_GCN_CONV_MR),
                "psg_gcn_ws_create: unknown block / conv kind");
    PSG_REQUIRE(batch > 0 && n_blocks >= 1, "psg_gcn_ws_create: bad sizes");
    PSG_REQUIRE(n_point >= 16 * n_blocks && n_point <= 4096,
                "psg_gcn_ws_create: n_point=%d must be in [k*max dilation = %d, 4096]", n_point, 16 * n_blocks);
    PSG_CHECK_HIP(hipSetDevice(ctx->device));
    auto *ws = new psg_gcn_ws();
    ws->ctx = ctx; ws->B = batch; ws->N = n_point; ws->fdim = GC * n_blocks;
    ws->cfg = GcnCfg{block, conv, n_blocks};
    ws->knn = read_knn_switches(psg::env_str);
    // the fused kNN kernels need 129 KB of dynamic LDS (raised once, outside any stream capture); a device that does
    // not grant it keeps the round-1 path (distance matrix in HBM + selection kernel)
    if (ws->knn.mode && knn_setup() != hipSuccess) { (void)hipGetLastError(); ws->knn.mode = 0; }
    const GcnTotals tot = gcn_totals(ws->cfg);
    ws->pq_w = conv == PSG_GCN_CONV_MR ? std::max(128, 2 * tot.c_max) : 128;
    const size_t R = (size_t)batch * n_point;
    auto layout = [&](Bump &bp) {
        ws->feats = bp.take<float>(R * ws->fdim); ws->dfeats = bp.take<float>(R * ws->fdim);
        ws->dist = bp.take<float>(R * n_point); ws->sq = bp.take<float>(R);
        ws->xp = (float *)bp.take<char>(knn_xp_bytes(R)); ws->bp = bp.take<char>(knn_bp_bytes(R));
        ws->knn_stats = ws->knn.stats ? bp.take<unsigned long long>(8) : nullptr;
        ws->pq = bp.take<float>(R * ws->pq_w); ws->pq2 = bp.take<float>(R * 2 * GC);
        ws->dpq = bp.take<float>(R * ws->pq_w); ws->dpq2 = bp.take<float>(R * 2 * GC);
        if (conv == PSG_GCN_CONV_MR) {
            ws->arg_mr = bp.take<uint8_t>(R * tot.arg_total); ws->mask_mr = bp.take<uint32_t>((size_t)n_blocks * R * 2);
        }
        ws->nbr = bp.take<int32_t>((size_t)n_blocks * R * KNB); ws->arg = bp.take<uint8_t>((size_t)n_blocks * R * GC);
        ws->fused = bp.take<float>(R * 1024);
        ws->mask_f = bp.take<uint32_t>(R * 32); ws->mask1 = bp.take<uint32_t>(R * 16); ws->mask2 = bp.take<uint32_t>(R * 8);
        ws->fmax = bp.take<float>((size_t)batch * 1024); ws->farg = bp.take<int32_t>((size_t)batch * 1024);
        ws->fkeys = bp.take<unsigned long long>((size_t)batch * 1024); ws->gb1 = bp.take<float>((size_t)batch * 512);
        ws->h1 = bp.take<float>(R * 512); ws->h2 = bp.take<float>(R * 256);
        ws->g2 = bp.take<float>(R * 256); ws->g1 = bp.take<float>(R * 512);
        ws->g1sum = bp.take<float>((size_t)batch * 512); ws->g1part = bp.take<float>((size_t)batch * ceil_div(n_point, 64) * 512);
        ws->gfvec = bp.take<float>((size_t)batch * 1024); ws->gcur = bp.take<float>(R * GC);
        ws->logits = bp.take<float>(R * NCLS); ws->dlogits = bp.take<float>(R * NCLS);
        ws->x0 = bp.take<float>(R * 9); ws->ori = bp.take<float>(R * 3); ws->dx0 = bp.take<float>(R * 9);
        ws->xyz = bp.take<float>(R * 3); ws->nb_labels = bp.take<int32_t>(R); ws->ori_xyz = bp.take<float>(R * 3);
    };
    if (int rc = carve_arena(&ws->arena, &ws->bytes, "psg_gcn_ws_create", layout)) {
        delete ws;
        return rc;
    }
    if (ws->knn_stats) (void)psg::memset_sync(ws->knn_stats, 0, 8 * sizeof(unsigned long long));
    *out = ws;
    return PSG_OK;
}

extern "C" int psg_gcn_ws_create(psg_ctx *ctx, int batch, int n_point, int n_blocks, psg_gcn_ws **out)
{
    return psg_gcn_ws_create_cfg(ctx, batch, n_point, n_blocks, PSG_GCN_BLOCK_RES, PSG_GCN_CONV_EDGE, out);
}

extern "C" int psg_gcn_ws_destroy(psg_gcn_ws *ws)
{
    if (!ws) return PSG_OK;
    ws->nb.slot.destroy();
    ws->nbf.slot.destroy();
    if (ws->arena) (void)hipFree(ws->arena);
    if (ws->keep) (void)hipFree(ws->keep);
    ws->prof.destroy();
    delete ws;
    return PSG_OK;
}

// Diagnostic counters of the bf16-prefilter kNN kernel since the last reset (workspaces created with PSG_GCN_KNN_STATS=1;
// otherwise all zero): [0] 32-query tiles, [1] tiles that took the exact path, [2] rows ranked on the fast path,
// [3] finalists (exact distances evaluated), [4] row cuts, [5] entries held at the end of the stream.  Synchronises.
extern "C" int psg_gcn_knn_stats(psg_gcn_ws *ws, unsigned long long *host_out8, int reset)
{
    PSG_REQUIRE(ws && host_out8, "psg_gcn_knn_stats: null argument");
    for (int i = 0; i < 8; ++i) host_out8[i] = 0ull;
    if (!ws->knn_stats) return PSG_OK;
    PSG_CHECK_HIP(hipDeviceSynchronize());
    PSG_CHECK_HIP(psg::copy_sync(host_out8, ws->knn_stats, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) PSG_CHECK_HIP(psg::memset_sync(ws->knn_stats, 0, 8 * sizeof(unsigned long long)));
    return PSG_OK;
}

extern "C" size_t psg_gcn_ws_bytes(const psg_gcn_ws *ws) { return ws ? ws->bytes : 0; }

// per-launch HIP-event profile (tags: 0 fused kNN kernel, 1 other kNN launches (xyz graph / round-1 path), 2 per-vertex
// [P|Q] GEMM, 3 edge max, 4 fusion + prediction, 5 backward); while enabled the attack loop stays eager (no hipGraph)
extern "C" int psg_gcn_prof_enable(psg_gcn_ws *ws, int on)
{
    PSG_REQUIRE(ws, "psg_gcn_prof_enable: null workspace");
    ws->prof.reset(on != 0);
    return PSG_OK;
}

extern "C" int psg_gcn_prof_read(psg_gcn_ws *ws, int n_tags, double *total_ms, int *counts, double *flops)
{
    PSG_REQUIRE(ws && total_ms && counts && n_tags >= GT_COUNT, "psg_gcn_prof_read: need room for %d tags", GT_COUNT);
    if (ws->prof.read(n_tags, total_ms, counts, flops)) { set_error("psg_gcn_prof_read: event query failed"); return PSG_ERR_HIP; }
    return PSG_OK;
}

extern "C" const int32_t *psg_gcn_edge_ptr(const psg_gcn_ws *ws, int block)
{
    if (!ws || block < 0 || block >= ws->cfg.n_blocks) return nullptr;
    return ws->nbr + (size_t)block * ws->B * ws->N * KNB;
}

extern "C" int psg_gcn_set_graphs(psg_gcn_ws *ws, const int32_t *nbr, psg_stream stream)
{
    PSG_REQUIRE(ws, "psg_gcn_set_graphs: null workspace");
    if (!nbr) { ws->fixed_graphs = false; return PSG_OK; }
    PSG_CHECK_HIP(hipMemcpyAsync(ws->nbr, nbr, (size_t)ws->cfg.n_blocks * ws->B * ws->N * KNB * 4, hipMemcpyDeviceToDevice,
                                 (hipStream_t)stream));
    ws->fixed_graphs = true;
    return PSG_OK;
}

extern "C" const float *psg_gcn_feats_ptr(const psg_gcn_ws *ws) { return ws ? ws->feats : nullptr; }

// unit op: torch.max_pool2d(x, [N, 1]) of DenseDeepGCN.forward (architecture.py:64) on point-major rows: per room and
// channel the maximum over the N points and the row that holds it (lowest row on equal values)
extern "C" int psg_global_max(const float *x, int B, int N, int C, unsigned long long *scratch, float *out_max,
                              int32_t *out_arg, psg_stream stream)
{
    PSG_REQUIRE(x && scratch && out_max && out_arg && B > 0 && N > 0 && C > 0 && C % 64 == 0,
                "psg_global_max: bad argument (C must be a multiple of 64)");
    hipStream_t st = (hipStream_t)stream;
    PSG_CHECK_HIP(hipMemsetAsync(scratch, 0, (size_t)B * C * 8, st));
    hipLaunchKernelGGL(colmax_partial_kernel, dim3(C / 64, ceil_div(N, 64), B), dim3(256), 0, st, x, N, C, 64, scratch);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(colmax_decode_kernel, dim3(ceil_div(B * C, 256)), dim3(256), 0, st, scratch, (size_t)B * C, out_max, out_arg);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// unit op: dilated dense kNN graph of point-major features x [B][N][C] (torch_edge.py:45-79)
extern "C" int psg_gcn_knn(psg_gcn_ws *ws, const float *x, int C, int dilation, int32_t *out_idx, psg_stream stream)
{
    PSG_REQUIRE(ws && x && out_idx, "psg_gcn_knn: null argument");
    PSG_REQUIRE(C >= 1 && dilation >= 1 && KNB * dilation <= ws->N, "psg_gcn_knn: k*dilation=%d exceeds N=%d",
                KNB * dilation, ws->N);
    return knn_graph(ws, x, C, C, dilation, out_idx, (hipStream_t)stream);
}

// ---- per-operator entry points behind the stand-alone forwards of the reference's public modules (the whole-network
// entry points below fuse them): thin launches of the same kernels on the caller's tensors.

// pairwise_distance (above) of x [B][N][C]; sq: scratch [B*N]
extern "C" int psg_gcn_pairwise_distance(const float *x, int B, int N, int C, float *sq, float *out, psg_stream stream)
{
    PSG_REQUIRE(x && sq && out && B > 0 && N > 0 && C > 0, "psg_gcn_pairwise_distance: bad argument");
    return pairwise_distance(x, C, B, N, C, sq, false, out, (hipStream_t)stream);
}

// EdgeConv2d.forward, torch_vertex.py:31-35 with BasicConv's Conv -> ReLU -> BatchNorm(eval) (torch_nn.py:55-75):
// y[i] = max_k ( scale * relu(W . [x_i, x_j - x_i] + b) + shift ),  j = nbr[i][k], 16 neighbours, 64 output channels.
// x [R][ld_x] (C used columns), R = rooms * N, nbr room-local; wcat [128][C] = [W1 - W2 ; W2], bcat [128] = [b, 0]
// (the split identity, built by the caller); pq: scratch [R][128]; arg [R][64] for the backward.
extern "C" int psg_edgeconv_fwd(const float *x, int ld_x, int R, int N, int C, const int32_t *nbr, const float *wcat,
                                const float *bcat, const float *scale, const float *shift, float *pq, float *out, int ld_out,
                                uint8_t *arg, psg_stream stream)
{
    PSG_REQUIRE(x && nbr && wcat && bcat && scale && shift && pq && out && arg && R > 0 && N > 0 && C > 0 && R % N == 0,
                "psg_edgeconv_fwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    GemmArgs a = gemm_args(x, ld_x, wcat, C, pq, 2 * GC, R, C, 2 * GC);
    a.bias = bcat;
    int rc;
    if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
    hipLaunchKernelGGL(edge_max_fwd_kernel, dim3(ceil_div((int)((size_t)R * GC), 256)), dim3(256), 0, st, pq, nbr, scale, shift,
                       (const float *)nullptr, 0, out, ld_out, arg, N, (size_t)R * GC, (float *)nullptr, (float *)nullptr,
                       (unsigned short *)nullptr);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// its input gradient: dy [R][ld_dy] -> dx [R][C]; wcat_t [C][128] = wcat transposed; dpq: scratch [R][128]
extern "C" int psg_edgeconv_bwd(const float *dy, int ld_dy, int R, int N, int C, const int32_t *nbr, const uint8_t *arg,
                                const float *scale, const float *wcat_t, float *dpq, float *dx, int ld_dx, psg_stream stream)
{
    PSG_REQUIRE(dy && nbr && arg && scale && wcat_t && dpq && dx && R > 0 && N > 0 && C > 0 && R % N == 0,
                "psg_edgeconv_bwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    { const int rc0 = launch_edge_max_bwd(dy, ld_dy, nbr, arg, scale, dpq, N, (size_t)R, st); if (rc0) return rc0; }
    GemmArgs a = gemm_args(dpq, 2 * GC, wcat_t, 2 * GC, dx, ld_dx, R, 2 * GC, C);
    return launch_gemm<4, 1, EPI_LINEAR, false>(a, st);
}

// MRConv2d's gather, torch_vertex.py:16-19: cat [R][2C] = [x_i, max_k (x_j - x_i)], arg [R][C] = winning neighbour (first
// on ties); the BasicConv that follows is psg_pw_mlp_fwd (Conv -> ReLU -> BatchNorm through its scale / shift).
extern "C" int psg_mrconv_gather_fwd(const float *x, int ld_x, int R, int N, int C, const int32_t *nbr, float *cat, uint8_t *arg,
                                     psg_stream stream)
{
    PSG_REQUIRE(x && nbr && cat && arg && R > 0 && N > 0 && C > 0 && R % N == 0, "psg_mrconv_gather_fwd: bad argument");
    const size_t tot = (size_t)R * C;
    hipLaunchKernelGGL(mr_gather_fwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ld_x, C, nbr,
                       cat, arg, N, tot);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// its transpose: dx[i] = dcat_x[i] - dcat_m[i], then dx[nbr(i, k*)] += dcat_m[i]   (dx [R][ld_dx], fully written)
extern "C" int psg_mrconv_gather_bwd(const float *dcat, int R, int N, int C, const int32_t *nbr, const uint8_t *arg, float *dx,
                                     int ld_dx, psg_stream stream)
{
    PSG_REQUIRE(dcat && nbr && arg && dx && R > 0 && N > 0 && C > 0 && R % N == 0, "psg_mrconv_gather_bwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const size_t tot = (size_t)R * C;
    const unsigned grid = (unsigned)((tot + 255) / 256);
    hipLaunchKernelGGL(mr_bwd_self_kernel, dim3(grid), dim3(256), 0, st, dcat, C, dx, ld_dx, (const float *)nullptr, 0, 1, tot);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(mr_bwd_scatter_kernel, dim3(grid), dim3(256), 0, st, dcat, C, nbr, arg, dx, ld_dx, N, tot);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// ==================================================================================== forward / backward
int gcn_extract_clean(psg_gcn_ws *ws, bool xyz, hipStream_t st)
{
    const size_t R = (size_t)ws->B * ws->N;
    hipLaunchKernelGGL(extract_color3_kernel, dim3(ceil_div((int)(R * 3), 256)), dim3(256), 0, st, ws->x0, ws->ori, R);
    PSG_LAUNCH_CHECK();
    if (!xyz) return PSG_OK;
    hipLaunchKernelGGL(extract3_kernel, dim3(ceil_div((int)(R * 3), 256)), dim3(256), 0, st, ws->x0, ws->ori_xyz, R);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_gcn_forward(psg_gcn_model *m, psg_gcn_ws *ws, const float *x0, float *logits_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && x0 && logits_out, "psg_gcn_forward: null argument");
    PSG_REQUIRE(gcn_same_cfg(m, ws), "psg_gcn_forward: model / workspace configuration mismatch");
    hipStream_t st = (hipStream_t)stream;
    const int B = ws->B, N = ws->N, F = ws->fdim;
    const size_t R = (size_t)B * N;
    const int g256 = ceil_div((int)(R * GC), 256);
    int rc;
    hipLaunchKernelGGL(extract3_kernel, dim3(ceil_div((int)(R * 3), 256)), dim3(256), 0, st, x0, ws->xyz, R);
    PSG_LAUNCH_CHECK();
    const bool mr = m->cfg.conv == PSG_GCN_CONV_MR, fuse_pq = gcn_switches().pq_fusion;
    bool pq_ready = false;     // this block's [P | Q] was written by the previous block's edge pass
    for (int e = 0; e < m->cfg.n_blocks; ++e) {
        const EdgeLayer &L = m->edge[e];
        const GcnBlock P = gcn_block(m->cfg, e);
        int32_t *nbr = ws->nbr + (size_t)e * R * KNB;
        const float *xin = e == 0 ? x0 : ws->feats + P.in_off;
        // the block's graph (the head's on xyz).  The norms of a 64-wide EdgeConv output come out of its max kernel.
        if (!ws->fixed_graphs && !(e == 0 && ws->head_graph_frozen) &&
            (rc = knn_graph(ws, e == 0 ? ws->xyz : xin, e == 0 ? 3 : P.ld, e == 0 ? 3 : P.C, P.dil, nbr, st, P.have_sq)))
            return rc;
        float *yout = ws->feats + (size_t)e * GC;
        const float *resid = P.resid ? xin : nullptr;
        if (!mr) {
            // [P | Q] = x . [W1 - W2 ; W2]^T + [b, 0]: a GEMM launch, unless the previous block's edge pass has produced it
            float *pq_cur = (e & 1) ? ws->pq2 : ws->pq, *pq_nxt = (e & 1) ? ws->pq : ws->pq2;
            if (!pq_ready) {
                GemmArgs a = gemm_args(xin, P.ld, L.wcat, P.C, pq_cur, 2 * GC, (int)R, P.C, 2 * GC);
                a.bias = L.bcat;
                EvScope prof(&ws->prof, GT_VERTEX_GEMM, 2.0 * R * P.C * 2.0 * GC, st);
                if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
            }
            // the next block's kNN kernel decides which operand copies this kernel writes beside the features
            const int next_path = (!ws->fixed_graphs && P.feeds_next) ? knn_path(ws, GC, gcn_block(m->cfg, e + 1).dil) : -1;
            // fused with the next block's per-vertex product when that block reads exactly this block's 64 outputs
            const bool fuse_next = fuse_pq && P.feeds_next && R % EMF_V == 0;
            EvScope prof(&ws->prof, GT_EDGE_MAX, fuse_next ? 2.0 * R * GC * 2.0 * GC : 0.0, st);
            float *sq_o = (ws->fixed_graphs || !P.sq_out) ? nullptr : ws->sq;
            float *xp_o = next_path >= 0 ? ws->xp : nullptr;
            unsigned short *bp_o = next_path == KNN_PATH_BF16 ? (unsigned short *)ws->bp : nullptr;
            if (fuse_next) {
                hipLaunchKernelGGL(edge_max_pq_fwd_kernel, dim3((unsigned)(R / EMF_V)), dim3(EMF_T), 0, st, pq_cur, nbr, L.scale, L.shift,
                                   resid, F, yout, F, ws->arg + (size_t)e * R * GC, N, sq_o, xp_o, bp_o, m->edge[e + 1].wcat_k8,
                                   m->edge[e + 1].bcat, pq_nxt);
                PSG_LAUNCH_CHECK();
            } else {
                hipLaunchKernelGGL(edge_max_fwd_kernel, dim3(g256), dim3(256), 0, st, pq_cur, nbr, L.scale, L.shift, resid, F, yout, F,
                                   ws->arg + (size_t)e * R * GC, N, R * GC, sq_o, xp_o, bp_o);
                PSG_LAUNCH_CHECK();
            }
            pq_ready = fuse_next;
        } else {
            // MRConv2d: BasicConv(cat[x, max_k (x_j - x_i)]) per vertex (+ x for a residual block)
            if ((rc = psg_mrconv_gather_fwd(xin, P.ld, (int)R, N, P.C, nbr, ws->pq, ws->arg_mr + P.arg_off * R, stream))) return rc;
            GemmArgs a = gemm_args(ws->pq, 2 * P.C, L.w, 2 * P.C, yout, F, (int)R, 2 * P.C, GC);
            a.bias = L.b; a.scale = L.scale; a.shift = L.shift; a.mask_out = ws->mask_mr + (size_t)e * R * 2;
            if (resid) { a.accumulate = 2; a.addend = resid; a.ld_add = F; }
            if ((rc = launch_gemm<2, 2, EPI_RELU_AFFINE, false>(a, st))) return rc;
        }
        if (ws->keep) {   // psg_gcn_debug_keep: this block's [P | Q] (mr: the gathered cat) before the next block overwrites it
            const size_t w = mr ? 2 * (size_t)P.C : 2 * GC;
            PSG_CHECK_HIP(hipMemcpyAsync(ws->k_pq + (size_t)e * R * ws->pq_w, mr ? ws->pq : ((e & 1) ? ws->pq2 : ws->pq), R * w * 4,
                                         hipMemcpyDeviceToDevice, st));
        }
    }
    EvScope prof_head(&ws->prof, GT_HEAD, 2.0 * R * ((double)F * 1024 + (double)F * 512 + 512.0 * 256 + 256.0 * NCLS), st);
    // fusion: Conv(F -> 1024) + ReLU + BN, global max over the room
    {
        GemmArgs a = gemm_args(ws->feats, F, m->wf, F, ws->fused, 1024, (int)R, F, 1024);
        a.bias = m->bf; a.scale = m->sf; a.shift = m->tf; a.mask_out = ws->mask_f;
        if ((rc = launch_gemm<2, 2, EPI_RELU_AFFINE, false>(a, st))) return rc;
        if ((rc = psg_global_max(ws->fused, B, N, 1024, ws->fkeys, ws->fmax, ws->farg, stream))) return rc;
    }
    // prediction.0 on cat(fusion broadcast, feats): the broadcast half is a per-room bias W1a . fmax
    hipLaunchKernelGGL(matvec_kernel, dim3(ceil_div(512, 4), B), dim3(256), 0, st, m->wp1, 1024 + F, ws->fmax, 1024, 512,
                       ws->gb1);
    PSG_LAUNCH_CHECK();
    {
        GemmArgs a = gemm_args(ws->feats, F, m->wp1 + 1024, 1024 + F, ws->h1, 512, (int)R, F, 512);
        a.bias = m->bp1; a.gbias = ws->gb1; a.group_rows = N; a.scale = m->s1; a.shift = m->t1; a.mask_out = ws->mask1;
        if ((rc = launch_gemm<2, 2, EPI_RELU_AFFINE, false>(a, st))) return rc;
    }
    {
        GemmArgs a = gemm_args(ws->h1, 512, m->wp2, 512, ws->h2, 256, (int)R, 512, 256);
        a.bias = m->bp2; a.scale = m->s2; a.shift = m->t2; a.mask_out = ws->mask2;
        if ((rc = launch_gemm<2, 2, EPI_RELU_AFFINE, false>(a, st))) return rc;
    }
    {
        GemmArgs a = gemm_args(ws->h2, 256, m->wp3, 256, ws->logits, NCLS, (int)R, 256, NCLS);
        a.bias = m->bp3;
        if ((rc = launch_gemm<4, 1, EPI_LINEAR, false>(a, st))) return rc;
    }
    if (logits_out != ws->logits)
        PSG_CHECK_HIP(hipMemcpyAsync(logits_out, ws->logits, R * NCLS * 4, hipMemcpyDeviceToDevice, st));
    ws->have_fwd = true;
    return PSG_OK;
}

// Backbone backward of the alternative blocks / convolutions.  dfeats[:, slice e] holds d loss / d y_e from the fusion
// and prediction layers; walking e downwards, every block adds its input gradient into the slice(s) it read, so a
// slice is complete when its block is reached:
//   res:    d x_{e-1} += d x_e + conv_e^T(d x_e)        plain:  d y_{e-1} += conv_e^T(d y_e)
//   dense:  d y_j     += conv_e^T(d y_e)[:, y_j]  for every j < e
static int backward_alt(psg_gcn_model *m, psg_gcn_ws *ws, float *dx0_out, hipStream_t st)
{
    const int N = ws->N, F = ws->fdim;
    const size_t R = (size_t)ws->B * N;
    const int g256 = ceil_div((int)(R * GC), 256);
    const bool mr = m->cfg.conv == PSG_GCN_CONV_MR;
    int rc;
    for (int e = m->cfg.n_blocks - 1; e >= 0; --e) {
        const EdgeLayer &L = m->edge[e];
        const GcnBlock P = gcn_block(m->cfg, e);
        const float *dy = ws->dfeats + (size_t)e * GC;                       // rows of F floats
        float *tgt = e == 0 ? dx0_out : ws->dfeats + P.tgt_off;
        const int ld_t = P.ld;
        const int32_t *nbr = ws->nbr + (size_t)e * R * KNB;
        if (!mr) {
            if ((rc = launch_edge_max_bwd(dy, F, nbr, ws->arg + (size_t)e * R * GC, L.scale, ws->dpq, N, R, st))) return rc;
            PSG_LAUNCH_CHECK();
            GemmArgs a = gemm_args(ws->dpq, 2 * GC, L.wcat_t, 2 * GC, tgt, ld_t, (int)R, 2 * GC, P.C);
            if (e > 0) {
                a.accumulate = 1;
                if (P.resid) { a.addend = dy; a.ld_add = F; }
            }
            if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
        } else {
            hipLaunchKernelGGL(mr_dz_kernel, dim3(g256), dim3(256), 0, st, dy, F, ws->mask_mr + (size_t)e * R * 2, L.scale,
                               ws->gcur, R * GC);
            PSG_LAUNCH_CHECK();
            GemmArgs a = gemm_args(ws->gcur, GC, L.w_t, GC, ws->dpq, 2 * P.C, (int)R, GC, 2 * P.C);
            if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
            const size_t tot = R * (size_t)P.C;
            const unsigned grid = (unsigned)((tot + 255) / 256);
            hipLaunchKernelGGL(mr_bwd_self_kernel, dim3(grid), dim3(256), 0, st, ws->dpq, P.C, tgt, ld_t,
                               P.resid ? dy : nullptr, F, e == 0 ? 1 : 0, tot);
            PSG_LAUNCH_CHECK();
            hipLaunchKernelGGL(mr_bwd_scatter_kernel, dim3(grid), dim3(256), 0, st, ws->dpq, P.C, nbr,
                               ws->arg_mr + P.arg_off * R, tgt, ld_t, N, tot);
            PSG_LAUNCH_CHECK();
        }
        if (ws->keep) {   // psg_gcn_debug_keep: [dP | dQ] (mr: gz and dcat), then the whole dfeats, then dx0 after block 0
            if (mr) PSG_CHECK_HIP(hipMemcpyAsync(ws->k_gz + (size_t)e * R * GC, ws->gcur, R * GC * 4, hipMemcpyDeviceToDevice, st));
            PSG_CHECK_HIP(hipMemcpyAsync(ws->k_dpq + (size_t)e * R * ws->pq_w, ws->dpq, R * (mr ? 2 * (size_t)P.C : 2 * GC) * 4,
                                         hipMemcpyDeviceToDevice, st));
            PSG_CHECK_HIP(hipMemcpyAsync(ws->k_state + (size_t)e * R * F, ws->dfeats, R * F * 4, hipMemcpyDeviceToDevice, st));
            if (e == 0) PSG_CHECK_HIP(hipMemcpyAsync(ws->k_dx0, dx0_out, R * 9 * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    return PSG_OK;
}

// ---- the test taps: psg_gcn_debug_ptr (read-only: pointer, rows, columns of a named buffer; the codes are listed in
// include/psg.h) and psg_gcn_debug_keep (per-block copies of what the loops overwrite, in an arena of their own)
extern "C" const void *psg_gcn_debug_ptr(const psg_gcn_ws *ws, int what, int block, int *rows_out, int *cols_out)
{
    if (!ws) { set_error("psg_gcn_debug_ptr: null workspace"); return nullptr; }
    if (block < 0 || block >= ws->cfg.n_blocks) {
        set_error("psg_gcn_debug_ptr: block %d out of range [0, %d)", block, ws->cfg.n_blocks);
        return nullptr;
    }
    const int B = ws->B, R = ws->B * ws->N, F = ws->fdim, e = block;
    const bool mr = ws->cfg.conv == PSG_GCN_CONV_MR, alt = mr || ws->cfg.block != PSG_GCN_BLOCK_RES;
    const GcnBlock P = gcn_block(ws->cfg, e);
    const int wpq = mr ? 2 * P.C : 2 * GC;
    const void *p = nullptr;
    int r = 0, c = 0;
    bool known = true, need_mr = false, need_keep = false;
    auto put = [&](const void *ptr, int rows, int cols) { p = ptr; r = rows; c = cols; };
    switch (what) {
    case 0: put(ws->xyz, R, 3); break;
    case 1: put(ws->feats, R, F); break;
    case 2: put(ws->nbr + (size_t)e * R * KNB, R, KNB); break;
    case 3: put(ws->arg + (size_t)e * R * GC, R, GC); break;
    case 4: need_mr = true; if (mr) put(ws->arg_mr + P.arg_off * R, R, P.C); break;
    case 5: need_mr = true; if (mr) put(ws->mask_mr + (size_t)e * R * 2, R, 2); break;
    case 6: put(ws->sq, R, 1); break;
    case 7: put(ws->xp, R, GC); break;
    case 8: put(ws->fused, R, 1024); break;
    case 9: put(ws->mask_f, R, 32); break;
    case 10: put(ws->fmax, B, 1024); break;
    case 11: put(ws->farg, B, 1024); break;
    case 12: put(ws->gb1, B, 512); break;
    case 13: put(ws->h1, R, 512); break;
    case 14: put(ws->mask1, R, 16); break;
    case 15: put(ws->h2, R, 256); break;
    case 16: put(ws->mask2, R, 8); break;
    case 17: put(ws->logits, R, NCLS); break;
    case 30: put(ws->g2, R, 256); break;
    case 31: put(ws->g1, R, 512); break;
    case 32: put(ws->g1part, B * ceil_div(ws->N, 64), 512); break;
    case 33: put(ws->g1sum, B, 512); break;
    case 34: put(ws->gfvec, B, 1024); break;
    case 35: put(ws->dfeats, R, F); break;
    case 36: put(ws->gcur, R, GC); break;
    case 50: need_keep = true; if (ws->keep) put(ws->k_pq + (size_t)e * R * ws->pq_w, R, wpq); break;
    case 51: need_keep = true; if (ws->keep) put(ws->k_dfh, R, F); break;
    case 52: need_keep = true; if (ws->keep) put(ws->k_dff, R, F); break;
    case 53: need_keep = true; if (ws->keep) put(ws->k_dpq + (size_t)e * R * ws->pq_w, R, wpq); break;
    case 54: need_keep = need_mr = true; if (ws->keep && mr) put(ws->k_gz + (size_t)e * R * GC, R, GC); break;
    case 55: need_keep = true; if (ws->keep) put(ws->k_state + (size_t)e * R * F, R, alt ? F : GC); break;
    case 56: need_keep = true; if (ws->keep) put(ws->k_dx0, R, 9); break;
    default: known = false;
    }
    if (!known) { set_error("psg_gcn_debug_ptr: unknown buffer code what=%d", what); return nullptr; }
    if (!p) {
        set_error("psg_gcn_debug_ptr: buffer code %d needs %s", what, need_keep && !ws->keep ? "psg_gcn_debug_keep on" : "conv = mr");
        return nullptr;
    }
    (void)need_mr;
    if (rows_out) *rows_out = r;
    if (cols_out) *cols_out = c;
    return p;
}

extern "C" int psg_gcn_debug_keep(psg_gcn_ws *ws, int on)
{
    PSG_REQUIRE(ws, "psg_gcn_debug_keep: null workspace");
    if (!on) {
        if (ws->keep) PSG_CHECK_HIP(hipFree(ws->keep));
        ws->keep = nullptr;
        return PSG_OK;
    }
    if (ws->keep) return PSG_OK;
    PSG_CHECK_HIP(hipSetDevice(ws->ctx->device));
    const size_t R = (size_t)ws->B * ws->N, nb = ws->cfg.n_blocks, F = ws->fdim;
    size_t bytes = 0;
    const int rc = carve_arena(&ws->keep, &bytes, "psg_gcn_debug_keep", [&](Bump &bp) {
        ws->k_pq = bp.take<float>(nb * R * ws->pq_w); ws->k_dpq = bp.take<float>(nb * R * ws->pq_w);
        ws->k_gz = bp.take<float>(nb * R * GC); ws->k_state = bp.take<float>(nb * R * F);
        ws->k_dfh = bp.take<float>(R * F); ws->k_dff = bp.take<float>(R * F); ws->k_dx0 = bp.take<float>(R * 9);
    });
    if (rc) ws->keep = nullptr;
    return rc;
}

int gcn_keep_refuses(const psg_gcn_ws *ws, const char *who)
{
    if (!ws->keep) return PSG_OK;
    set_error("%s: psg_gcn_debug_keep is on for this workspace (a replayed graph would not make the per-block copies)", who);
    return PSG_ERR_STATE;
}

extern "C" int psg_gcn_backward(psg_gcn_model *m, psg_gcn_ws *ws, const float *dlogits, float *dx0_out,
                                psg_stream stream)
{
    PSG_REQUIRE(m && ws && dlogits && dx0_out, "psg_gcn_backward: null argument");
    if (!ws->have_fwd) { set_error("psg_gcn_backward: no forward is resident in the workspace"); return PSG_ERR_STATE; }
    PSG_REQUIRE(gcn_same_cfg(m, ws), "psg_gcn_backward: model / workspace configuration mismatch");
    hipStream_t st = (hipStream_t)stream;
    const int B = ws->B, N = ws->N, F = ws->fdim;
    const size_t R = (size_t)B * N;
    int rc;
    EvScope prof(&ws->prof, GT_BACKWARD, 0.0, st);
    // prediction.3^T, then through ReLU/BN of prediction.1 (mask2; its scale s2 is folded into wp2_st)
    {
        GemmArgs a = gemm_args(dlogits, NCLS, m->wp3_t, NCLS, ws->g2, 256, (int)R, NCLS, 256);
        a.mask_in = ws->mask2;
        if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
    }
    {
        GemmArgs a = gemm_args(ws->g2, 256, m->wp2_st, 256, ws->g1, 512, (int)R, 256, 512);
        a.mask_in = ws->mask1;
        if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
    }
    // feats half of prediction.0^T
    {
        GemmArgs a = gemm_args(ws->g1, 512, m->wp1b_st, 512, ws->dfeats, F, (int)R, 512, F);
        if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
    }
    if (ws->keep) PSG_CHECK_HIP(hipMemcpyAsync(ws->k_dfh, ws->dfeats, R * F * 4, hipMemcpyDeviceToDevice, st));   // psg_gcn_debug_keep
    // fusion half: gradient of the broadcast vector = (s1 * W1a)^T . (column sum of g1), then back through the
    // global max (one point per channel), ReLU/BN of the fusion block and its 1x1 conv: 1024 scaled row adds
    {
        const int chunks = ceil_div(N, 64);
        hipLaunchKernelGGL(colsum_kernel, dim3(512 / 64, chunks, B), dim3(256), 0, st, ws->g1, N, 512, 64, ws->g1part);
        PSG_LAUNCH_CHECK();
        hipLaunchKernelGGL(colsum_finish_kernel, dim3(ceil_div(B * 512, 256)), dim3(256), 0, st, ws->g1part, chunks, 512, (size_t)B * 512, ws->g1sum);
        PSG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(matvec_kernel, dim3(ceil_div(1024, 4), B), dim3(256), 0, st, m->wp1a_st, 512, ws->g1sum, 512, 1024,
                       ws->gfvec);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(fusion_bwd_kernel, dim3(1024, B, ceil_div(F, 256)), dim3(256), 0, st, ws->gfvec, ws->farg, ws->mask_f, m->sf, m->wf, F,
                       1024, N, ws->dfeats);
    PSG_LAUNCH_CHECK();
    if (ws->keep) PSG_CHECK_HIP(hipMemcpyAsync(ws->k_dff, ws->dfeats, R * F * 4, hipMemcpyDeviceToDevice, st));
    if (m->cfg.block != PSG_GCN_BLOCK_RES || m->cfg.conv != PSG_GCN_CONV_EDGE) return backward_alt(m, ws, dx0_out, st);
    // backbone in reverse: G_e = d/d x_e
    PSG_CHECK_HIP(hipMemcpy2DAsync(ws->gcur, GC * 4, ws->dfeats + (size_t)(m->cfg.n_blocks - 1) * GC, (size_t)F * 4, GC * 4, R,
                                   hipMemcpyDeviceToDevice, st));
    // [dP | dQ] buffers alternate between two blocks (block e's GEMM may still read its buffer while block e - 1's edge
    // pass writes the other); every row of both halves has exactly one writer in the gather kernel: nothing to zero
    float *pp[2] = {ws->dpq, ws->dpq2};
    for (int e = m->cfg.n_blocks - 1; e >= 0; --e) {
        const EdgeLayer &L = m->edge[e];
        const GcnBlock P = gcn_block(m->cfg, e);
        float *dpq = pp[e & 1];
        if ((rc = launch_edge_max_bwd(ws->gcur, GC, ws->nbr + (size_t)e * R * KNB, ws->arg + (size_t)e * R * GC, L.scale, dpq, N, R,
                                      st))) return rc;
        // x_e = EdgeConv_e(x_{e-1}) + x_{e-1}:  G_{e-1} = dfeats[e-1] + G_e + [dP | dQ] . [W1-W2 ; W2]
        // (the residual's gradient slice dfeats[e-1] is added inside the GEMM's accumulate epilogue); the head writes dx0
        GemmArgs a = gemm_args(dpq, 2 * GC, L.wcat_t, 2 * GC, e > 0 ? ws->gcur : dx0_out, e > 0 ? GC : P.ld, (int)R, 2 * GC, P.C);
        if (e > 0) { a.accumulate = 1; a.addend = ws->dfeats + P.tgt_off; a.ld_add = F; }
        if ((rc = launch_gemm<4, 1, EPI_LINEAR, false>(a, st))) return rc;
        if (ws->keep) {   // psg_gcn_debug_keep: this block's [dP | dQ], then gcur (G_{e-1}; unchanged by the head), then dx0
            PSG_CHECK_HIP(hipMemcpyAsync(ws->k_dpq + (size_t)e * R * ws->pq_w, dpq, R * 2 * GC * 4, hipMemcpyDeviceToDevice, st));
            PSG_CHECK_HIP(hipMemcpyAsync(ws->k_state + (size_t)e * R * F, ws->gcur, R * GC * 4, hipMemcpyDeviceToDevice, st));
            if (e == 0) PSG_CHECK_HIP(hipMemcpyAsync(ws->k_dx0, dx0_out, R * 9 * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    return PSG_OK;
}
