// Vanilla PointNet semantic-segmentation network on gfx950: forward, input-gradient backward and the fused NB colour
// attack.  Reference (paths relative to the reference's PointNet/ directory):
//   models/pointnet.py:10-130        STN3d, STNkd, PointNetEncoder (feature_transform=True, channel=6)
//   models/pointnet_sem_seg.py:8-38  get_model: encoder -> 1088->512->256->128->13 -> log_softmax
//   attacks/torchattacks/attacks/{nontarget,target}.py  NB_attack / tar_NB_attack
//
// Eval mode, BatchNorm folded into every conv / linear layer on the host (runtime.fold_pointnet_state_dict).
// Shape of the work: three 128->1024 per-point layers, each followed by a max over all N points
// of the room, a per-room 3x3 transform of xyz and a per-room 64x64 transform of the 64-d features.
//   * per-point layers: gemm_rows_kernel (psg_gemm.cuh), fp32 MFMA, fused bias / ReLU / ReLU-bit epilogues;
//   * the 128->1024 layers: pn_max_gemm_kernel below, the same MFMA tiling with a max-pool epilogue that leaves one
//     (max, first arg-max) per 128-point tile and channel; pn_max_reduce_kernel folds the tiles in ascending order.
//     The N x 1024 activations never reach HBM;
//   * the transforms are folded into the next layer's weights per room (W T^T), one GEMM over the B rooms each;
//   * the head's global columns become a per-room bias (GemmArgs::gbias);
//   * backward: dense transposes through the head and the encoder's 64-wide layers, and one SPARSE pass per max-pool:
//     dY[c] lands on the arg-max point of channel c only (1 point in N), so each arg-max point gathers
//     sum_c g_c W3[c,:] (ascending c) and runs conv2^T / conv1^T on its own row.
// No atomics: every reduction has a fixed order, so results are bit-reproducible and a batch of B rooms is
// bit-identical to B one-room calls (every per-room quantity is computed by per-room work).
#include <algorithm>
#include <vector>

#include "psg_common.h"
#include "psg_gemm.cuh"

using namespace psg;

namespace {

constexpr int NCLS = PSG_POINTNET_NUM_CLASSES;
constexpr int PT = PSG_POINTNET_POINT_TILE;   // points per max-pool tile
constexpr int GF = 1024;                      // width of the three pooled layers
constexpr int NL = PSG_POINTNET_NUM_LAYERS;

// (out, in) of the folded layers, in the order of psg_pointnet_model_create
enum {
    L_A1, L_A2, L_A3, L_F1, L_F2, L_F3,         // feat.stn: conv1..3, fc1..3
    L_C1,                                      // feat.conv1
    L_K1, L_K2, L_K3, L_FK1, L_FK2, L_FK3,     // feat.fstn
    L_C2, L_C3,                                // feat.conv2, feat.conv3
    L_H1, L_H2, L_H3, L_H4                     // conv1..conv4 of the head
};
constexpr int LDIM[NL][2] = {{64, 6}, {128, 64}, {1024, 128}, {512, 1024}, {256, 512}, {9, 256},
                             {64, 6},
                             {64, 64}, {128, 64}, {1024, 128}, {512, 1024}, {256, 512}, {4096, 256},
                             {128, 64}, {1024, 128},
                             {512, 1088}, {256, 512}, {128, 256}, {13, 128}};
static_assert(sizeof(LDIM) / sizeof(LDIM[0]) == NL, "layer table");

// 128 x 128 tiles, or 64 x 64 tiles for the per-room and per-batch GEMMs (psg_gemm.cuh)
template <int EPI>
int run_gemm(const GemmArgs &a, hipStream_t st)
{
    return launch_gemm<2, 2, EPI, false>(a, 384, st);
}

// ---- 128 -> 1024 layer with the max-pool epilogue.  in [rows][K] (rows = B*N, N a multiple of PT), w [M][K], bias [M].
// Workgroup = PT points x 128 channels, 4 waves of 2 x 2 MFMA tiles (gemm_rows_kernel's tiling and k8-block LDS layout).
// Epilogue: z = acc + bias (ReLU'd when relu), then per channel the largest z of the tile and its first (lowest) point:
// over the wave's two 32-point tiles, across the 32 lanes of a half-wave (xor shuffles), then across the two waves
// that share the channel.  part_val / part_idx [rows / PT][M]; the index is room-local.
constexpr int MX_BR = PT, MX_BN = 128;
constexpr int MX_BLK_R = MX_BR * 8 + 8, MX_BLK_N = MX_BN * 8 + 8;    // floats per 8-k block (+8: bank de-phasing)
static_assert(PT == 128, "pn_max_gemm_kernel: the point tile is 2 waves x 2 MFMA tiles x 32 points");
static_assert(MX_BLK_R % 4 == 0 && MX_BLK_N % 4 == 0, "ds_read_b128 / ds_write_b128 need 16-byte aligned LDS blocks");

__global__ __launch_bounds__(256) void pn_max_gemm_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                          const float *__restrict__ bias, int K, int M, int N, int relu,
                                                          float *__restrict__ part_val, int32_t *__restrict__ part_idx)
{
    __shared__ __attribute__((aligned(16))) float s_in[4 * MX_BLK_R];
    __shared__ __attribute__((aligned(16))) float s_w[4 * MX_BLK_N];
    __shared__ float s_v[2][MX_BN];
    __shared__ int s_i[2][MX_BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int row0 = blockIdx.x * MX_BR, col0 = blockIdx.y * MX_BN;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][q][r] = 0.0f;

    constexpr int NI = MX_BR * 8 / 256, NWL = MX_BN * 8 / 256;
    for (int k0 = 0; k0 < K; k0 += 32) {
        float4 vi[NI], vw[NWL];
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int t = tid + u * 256, r = t >> 3, q = t & 7;
            vi[u] = *(const float4 *)(in + (size_t)(row0 + r) * K + k0 + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < NWL; ++u) {
            const int t = tid + u * 256, r = t >> 3, q = t & 7;
            vw[u] = *(const float4 *)(w + (size_t)(col0 + r) * K + k0 + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int t = tid + u * 256, r = t >> 3, q = t & 7;
            *(float4 *)(s_in + (q >> 1) * MX_BLK_R + r * 8 + (q & 1) * 4) = vi[u];
        }
#pragma unroll
        for (int u = 0; u < NWL; ++u) {
            const int t = tid + u * 256, r = t >> 3, q = t & 7;
            *(float4 *)(s_w + (q >> 1) * MX_BLK_N + r * 8 + (q & 1) * 4) = vw[u];
        }
        __syncthreads();
#pragma unroll
        for (int k8 = 0; k8 < 4; ++k8) {
            float4 wa[2], xb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) wa[i] = *(const float4 *)(s_w + k8 * MX_BLK_N + (wc * 64 + i * 32 + j) * 8 + 4 * h);
#pragma unroll
            for (int q = 0; q < 2; ++q) xb[q] = *(const float4 *)(s_in + k8 * MX_BLK_R + (wr * 64 + q * 32 + j) * 8 + 4 * h);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[i][q] = mfma4<false>(wa[i], xb[q], acc[i][q]);
        }
        __syncthreads();
    }

    // lane (j, h) of tile (i, q) holds channels cbase + acc_row(r, h) of tile-local point wr*64 + q*32 + j
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cl0 = wc * 64 + i * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cl = cl0 + acc_row(r, h);
            const float b = bias[col0 + cl];
            float v0 = acc[i][0][r] + b, v1 = acc[i][1][r] + b;
            if (relu) {
                v0 = v0 > 0.0f ? v0 : 0.0f;
                v1 = v1 > 0.0f ? v1 : 0.0f;
            }
            float v = v0;
            int ix = wr * 64 + j;
            if (v1 > v) { v = v1; ix = wr * 64 + 32 + j; }
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(v, off);
                const int oi = __shfl_xor(ix, off);
                if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
            }
            if (j == 0) { s_v[wr][cl] = v; s_i[wr][cl] = ix; }
        }
    }
    __syncthreads();
    if (tid < MX_BN) {
        float v = s_v[0][tid];
        int ix = s_i[0][tid];
        if (s_v[1][tid] > v) { v = s_v[1][tid]; ix = s_i[1][tid]; }   // wave row 1 holds the later points
        const int local0 = row0 % N;
        part_val[(size_t)blockIdx.x * M + col0 + tid] = v;
        part_idx[(size_t)blockIdx.x * M + col0 + tid] = local0 + ix;
    }
}

// tiles of a room in ascending order; strict > keeps the first arg-max.  out_* [B][ld_out] (+ c)
__global__ void pn_max_reduce_kernel(const float *__restrict__ part_val, const int32_t *__restrict__ part_idx, int B, int tiles,
                                     int M, float *__restrict__ out_val, int32_t *__restrict__ out_idx, int ld_out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * M) return;
    const int b = t / M, c = t % M;
    size_t o = (size_t)b * tiles * M + c;
    float v = part_val[o];
    int ix = part_idx[o];
    for (int k = 1; k < tiles; ++k) {
        o += M;
        const float pv = part_val[o];
        if (pv > v) { v = pv; ix = part_idx[o]; }
    }
    out_val[(size_t)b * ld_out + c] = v;
    out_idx[(size_t)b * ld_out + c] = ix;
}

// ---- sparse max-pool backward.  Workgroup (s, b): if s is the lowest channel whose arg-max is point p = idx[b][s], it
// owns point p:  v = sum_{c : idx[c] = p} g_c W3[c,:] (ascending c),  u2 = v * [act2_p > 0],  y = W2^T u2,
// then either  out_p[0:64] += y  (act1 == null), or  u1 = y * [act1_p > 0],  z = W1^T u1 (* [out_mask_p > 0]),
// out_p[0:c_out] += z.  Each point is owned by one workgroup: no two workgroups write the same row.
struct PoolBwdArgs {
    const float *coef;      // [B][1024] dL / d(pooled value)
    const float *pool;      // [B][ld_pool] pooled values
    const int32_t *idx;     // [B][ld_pool] room-local arg-max points
    int ld_pool, relu_pool; // relu_pool: the pooled layer ended in a ReLU (gradient only where the max is > 0)
    const float *w3;        // [1024][128]
    const float *act2;      // [B*N][128] the pooled layer's input (post-ReLU)
    const float *w2;        // [128][64]
    const float *act1;      // [B*N][64] the input of w2's layer (post-ReLU), or null
    const float *w1;        // [64][c_out]
    const float *out_mask;  // [B*N][64] values whose sign gates z, or null
    float *out;
    int ld_out, c_out, N;
};

__global__ __launch_bounds__(128) void pn_pool_bwd_kernel(PoolBwdArgs a)
{
    __shared__ int s_idx[GF];
    __shared__ float s_g[GF];
    __shared__ float s_u2[128];
    __shared__ float s_u1[64];
    __shared__ int s_dup;
    const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    for (int c = tid; c < GF; c += 128) {
        const size_t o = (size_t)b * a.ld_pool + c;
        s_idx[c] = a.idx[o];
        float g = a.coef[(size_t)b * GF + c];
        if (a.relu_pool && !(a.pool[o] > 0.0f)) g = 0.0f;
        s_g[c] = g;
    }
    if (tid == 0) s_dup = 0;
    __syncthreads();
    const int p = s_idx[s];
    for (int c = tid; c < s; c += 128)
        if (s_idx[c] == p) s_dup = 1;
    __syncthreads();
    if (s_dup) return;
    const size_t row = (size_t)b * a.N + p;
    float v = 0.0f;
    for (int c = s; c < GF; ++c)
        if (s_idx[c] == p) v = fmaf(s_g[c], a.w3[(size_t)c * 128 + tid], v);
    s_u2[tid] = a.act2[row * 128 + tid] > 0.0f ? v : 0.0f;
    __syncthreads();
    float y = 0.0f;
    if (tid < 64)
        for (int o = 0; o < 128; ++o) y = fmaf(a.w2[o * 64 + tid], s_u2[o], y);
    if (!a.act1) {
        if (tid < 64) a.out[row * a.ld_out + tid] += y;
        return;
    }
    if (tid < 64) s_u1[tid] = a.act1[row * 64 + tid] > 0.0f ? y : 0.0f;
    __syncthreads();
    if (tid < a.c_out) {
        float z = 0.0f;
        for (int o = 0; o < 64; ++o) z = fmaf(a.w1[o * a.c_out + tid], s_u1[o], z);
        if (a.out_mask && !(a.out_mask[row * 64 + tid] > 0.0f)) z = 0.0f;
        a.out[row * a.ld_out + tid] += z;
    }
}

// out[b][m] = sum_p x[b*N + p][m]: four interleaved partial sums per column, added in a fixed order
__global__ __launch_bounds__(256) void pn_colsum_kernel(const float *__restrict__ x, int N, int M, float *__restrict__ out)
{
    __shared__ float red[4][64];
    const int tid = threadIdx.x, b = blockIdx.y, col = blockIdx.x * 64 + (tid & 63), part = tid >> 6;
    float s = 0.0f;
    if (col < M)
        for (int p = part; p < N; p += 4) s += x[((size_t)b * N + p) * M + col];
    red[part][tid & 63] = s;
    __syncthreads();
    if (part == 0 && col < M) out[(size_t)b * M + col] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// [B][N][C] -> [B][C][N]
__global__ void pn_transpose_kernel(const float *__restrict__ in, int N, int C, float *__restrict__ out)
{
    __shared__ float tile[32][33];
    const int b = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 32 x 8
    for (int y = ty; y < 32; y += 8) {
        const int p = p0 + y, c = c0 + tx;
        tile[y][tx] = (p < N && c < C) ? in[((size_t)b * N + p) * C + c] : 0.0f;
    }
    __syncthreads();
    for (int y = ty; y < 32; y += 8) {
        const int c = c0 + y, p = p0 + tx;
        if (p < N && c < C) out[((size_t)b * C + c) * N + p] = tile[tx][y];
    }
}

// per-room encoder conv1 weights: W1f[b][o][0:3] = (W[:, 0:3] trans_b^T)[o] (t1 [64][B*3]), [3:6] = W[o][3:6], [6:8] = 0
__global__ void pn_c1_assemble_kernel(const float *__restrict__ t1, const float *__restrict__ w, int B, float *__restrict__ w1f)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * 64 * 8) return;
    const int b = t / 512, o = (t / 8) % 64, i = t % 8;
    float v = 0.0f;
    if (i < 3) v = t1[(size_t)o * B * 3 + b * 3 + i];
    else if (i < 6) v = w[o * 6 + i];
    w1f[t] = v;
}

// log_softmax over NCLS logits per row (x - max - log(sum exp(x - max)))
__global__ void pn_log_softmax_kernel(const float *__restrict__ z, size_t rows, float *__restrict__ logp)
{
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float v[NCLS], m = -INFINITY;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) { v[c] = z[r * NCLS + c]; m = fmaxf(m, v[c]); }
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) s += expf(v[c] - m);
    const float ls = logf(s);
#pragma unroll
    for (int c = 0; c < NCLS; ++c) logp[r * NCLS + c] = (v[c] - m) - ls;
}

// d logits = dlogp - softmax * sum(dlogp)
__global__ void pn_log_softmax_bwd_kernel(const float *__restrict__ logp, const float *__restrict__ dlogp, size_t rows,
                                          float *__restrict__ dz)
{
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) s += dlogp[r * NCLS + c];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) dz[r * NCLS + c] = dlogp[r * NCLS + c] - expf(logp[r * NCLS + c]) * s;
}

// ---- The seam between forward and backward of one NU optimiser step in ONE kernel: logits -> dz, pred, f sums.  What
// pn_log_softmax_kernel, nu_f_loss_grad_kernel (psg_attack.hip) and pn_log_softmax_bwd_kernel compute through three
// [rows][13] arrays in HBM, with the same per-element operations in the same order, so dz and pred are bit-identical to
// that sequence.  The three parts keep the floating-point contraction mode of the translation units they come from (the
// f-loss is compiled without contraction, the two log-softmax kernels with it): the products of one part never fuse into
// the sums of the next.
// 256 rows per workgroup: their 256 x 13 logits are one contiguous piece, read as coalesced 16-byte words into LDS; a thread
// then owns one row (stride 13 dwords: conflict-free) with the classes in registers - every class loop is unrolled and the
// label's class is picked by compares, not by indexing -, writes dz back into its LDS row, and the piece leaves as 16-byte
// words again.  f sums as in nu_f_loss_grad_kernel: a wave's 64 values by xor shuffles, the workgroup's waves in ascending
// order, one float atomicAdd per workgroup (per wave where a workgroup spans two rooms) into the room's sum.
__global__ __launch_bounds__(256) void pn_nu_head_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels, int target,
                                                         int rows, float kappa, float tsign, float *__restrict__ dz,
                                                         float *__restrict__ f_sum, int32_t *__restrict__ pred, int rows_per_sum)
{
    __shared__ __attribute__((aligned(16))) float s_z[256 * NCLS];
    __shared__ float s_part[4];
    const int tid = threadIdx.x, r0 = blockIdx.x * 256, nr = min(256, rows - r0);      // nr is a multiple of 128
    const float4 *src = (const float4 *)(logits + (size_t)r0 * NCLS);
    for (int i = tid; i < nr * NCLS / 4; i += 256) ((float4 *)s_z)[i] = src[i];
    __syncthreads();
    const int r = r0 + tid;
    float fval = 0.0f;
    if (tid < nr) {
        float *row = s_z + tid * NCLS;
        float lp[NCLS], g[NCLS];
        {   // pn_log_softmax_kernel
            float v[NCLS], m = -INFINITY;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) { v[c] = row[c]; m = fmaxf(m, v[c]); }
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) s += expf(v[c] - m);
            const float ls = logf(s);
#pragma unroll
            for (int c = 0; c < NCLS; ++c) lp[c] = (v[c] - m) - ls;
        }
        {   // nu_f_loss_grad_kernel
#pragma clang fp contract(off)
            float p[NCLS];
            float m = -INFINITY;
            int am = 0;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) {
                p[c] = lp[c];
                if (p[c] > m) { m = p[c]; am = c; }
            }
            pred[r] = am;
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) { p[c] = expf(p[c] - m); s += p[c]; }
#pragma unroll
            for (int c = 0; c < NCLS; ++c) p[c] = p[c] / s;
            const int y = labels ? labels[r] : target;
            float oth = -1.0f, py = 0.0f, poi = 0.0f;
            int oi = 0;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) {
                if (c == y) py = p[c];
                if (c != y && p[c] > oth) { oth = p[c]; oi = c; }
            }
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
                if (c == oi) poi = p[c];
            if (oth < 0.0f) oth = 0.0f;
            const float val = tsign * (py - oth);
            const bool pass = val >= -kappa;
            fval = pass ? val : -kappa;
            const float gy = pass ? tsign : 0.0f, go = pass ? -tsign : 0.0f;
            const float dot = gy * py + go * poi;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) {
                const float gc = c == y ? gy : (c == oi ? go : 0.0f);
                g[c] = p[c] * (gc - dot);
            }
        }
        {   // pn_log_softmax_bwd_kernel
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) s += g[c];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) row[c] = g[c] - expf(lp[c]) * s;
        }
    }
    __syncthreads();
    float4 *dst = (float4 *)(dz + (size_t)r0 * NCLS);
    for (int i = tid; i < nr * NCLS / 4; i += 256) dst[i] = ((const float4 *)s_z)[i];
    for (int o = 32; o >= 1; o >>= 1) fval += __shfl_xor(fval, o);
    if (rows_per_sum == 0 || rows_per_sum % 256 == 0) {
        if ((tid & 63) == 0) s_part[tid >> 6] = fval;
        __syncthreads();
        if (tid == 0) {
            float tot = 0.0f;
            for (int w = 0; w < 4; ++w) tot += s_part[w];
            atomicAdd(f_sum + (rows_per_sum ? r0 / rows_per_sum : 0), tot);
        }
    } else if ((tid & 63) == 0 && r < rows) {
        atomicAdd(f_sum + r / rows_per_sum, fval);
    }
}

// Input transform backward, one workgroup per room.  dxu [B*N][8]: columns 0:3 = d(xyz . trans), 3:6 = d rgb.
//   dx0[p] = [trans . dxu_p[0:3], dxu_p[3:6], 0, 0, 0]   (channels 6:9 are not read by the network: x[:, :6])
//   dtrans[b][i][j] = sum_p xyz_p[i] dxu_p[j]             (per-thread partials, then a fixed-order tree)
__global__ __launch_bounds__(256) void pn_xyz_bwd_kernel(const float *__restrict__ x0, const float *__restrict__ dxu,
                                                         const float *__restrict__ trans, int N, float *__restrict__ dx0,
                                                         float *__restrict__ dtrans)
{
    __shared__ float red[256][9];
    const int tid = threadIdx.x, b = blockIdx.x;
    float T[9], acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { T[k] = trans[b * 9 + k]; acc[k] = 0.0f; }
    for (int p = tid; p < N; p += 256) {
        const size_t row = (size_t)b * N + p;
        const float d0 = dxu[row * 8 + 0], d1 = dxu[row * 8 + 1], d2 = dxu[row * 8 + 2];
        const float x[3] = {x0[row * 9 + 0], x0[row * 9 + 1], x0[row * 9 + 2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dx0[row * 9 + i] = fmaf(T[3 * i + 2], d2, fmaf(T[3 * i + 1], d1, T[3 * i] * d0));
            dx0[row * 9 + 3 + i] = dxu[row * 8 + 3 + i];
            dx0[row * 9 + 6 + i] = 0.0f;
            acc[3 * i + 0] = fmaf(x[i], d0, acc[3 * i + 0]);
            acc[3 * i + 1] = fmaf(x[i], d1, acc[3 * i + 1]);
            acc[3 * i + 2] = fmaf(x[i], d2, acc[3 * i + 2]);
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) red[tid][k] = acc[k];
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st)
#pragma unroll
            for (int k = 0; k < 9; ++k) red[tid][k] += red[tid + st][k];
        __syncthreads();
    }
    if (tid < 9) dtrans[b * 9 + tid] = red[0][tid];
}

__global__ void pn_extract_color_kernel(const float *__restrict__ x0, float *__restrict__ ori, size_t rows)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < rows * 3) ori[t] = x0[(t / 3) * 9 + 3 + (t % 3)];
}

inline unsigned grid1(size_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

struct psg_pointnet_model {
    psg_ctx *ctx;
    uint64_t gen = 0;      // psg::next_generation(): what a hipGraph key compares instead of the handle's address
    float *w[NL], *b[NL];
    // transposes for the backward: [in][out] of the named layer (H1p / H1g: the pointfeat / global column blocks of conv1)
    float *f3t, *f2t, *f1t, *fk3t, *fk2t, *fk1t, *h4t, *h3t, *h2t, *h1pt, *h1gt, *c1t;
    std::vector<void *> allocs;
};

struct psg_pointnet_ws {
    psg_ctx *ctx;
    uint64_t gen = 0;
    int B, N;
    void *arena = nullptr;
    size_t bytes = 0;
    // forward
    float *a1, *a2, *h, *k1, *k2, *e2, *z1, *z2, *z3, *logits, *logp;   // per point
    uint32_t *mh, *m1, *m2, *m3;                                         // ReLU bits [rows][ceil(M/32)]
    float *part_val; int32_t *part_idx;                                  // [B*N/PT][1024]
    float *pool; int32_t *pidx;                                          // [B][3][1024]: stn3d, stnkd, encoder
    float *f1, *f2, *trans, *fk1, *fk2, *tf;                             // per room
    uint32_t *mf1, *mf2, *mfk1, *mfk2;
    float *t1, *w1f, *c2f, *h1pf, *gb;                                   // per-room folded weights, head bias
    float *x0in;                                                         // the forward's input [B*N][9]
    // backward
    float *dz4, *dz3, *dz2, *dz1, *s1, *dg, *dpf, *ht, *dpft, *dtf, *dfk2, *dfk1, *dgk, *dh, *dxu, *dtrans, *df2, *df1, *dgs;
    // attack
    float *x0, *ori, *dlogp, *dx0;
    int32_t *labels;
    uint8_t *mask;
    bool have_fwd = false;
};

namespace {

// with_logp = false stops at the head's logits (ws->logits): the NU window's pn_nu_head_kernel takes them from there
int forward_impl(psg_pointnet_model *m, psg_pointnet_ws *ws, const float *x0, float *logp_out, hipStream_t st, bool with_logp = true)
{
    const int B = ws->B, N = ws->N, R = B * N, T = R / PT;
    int rc;
    auto W = [&](int l) { return m->w[l]; };
    auto Bi = [&](int l) { return m->b[l]; };
    if (x0 != ws->x0in) PSG_CHECK_HIP(hipMemcpyAsync(ws->x0in, x0, (size_t)R * 9 * sizeof(float), hipMemcpyDeviceToDevice, st));
    const float *x = ws->x0in;
    // pooled 128 -> 1024 layer: partial maxima per tile, then the tiles of each room in order
    auto pool_layer = [&](const float *in, int l, int relu, int which) -> int {
        hipLaunchKernelGGL(pn_max_gemm_kernel, dim3(T, GF / MX_BN), dim3(256), 0, st, in, W(l), Bi(l), 128, GF, N, relu,
                           ws->part_val, ws->part_idx);
        PSG_LAUNCH_CHECK();
        hipLaunchKernelGGL(pn_max_reduce_kernel, dim3(grid1((size_t)B * GF)), dim3(256), 0, st, ws->part_val, ws->part_idx, B, N / PT,
                           GF, ws->pool + which * GF, ws->pidx + which * GF, 3 * GF);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    };
    // fc1 -> fc2 -> fc3 (+ identity, folded into fc3's bias) of a transform net on the pooled vector
    auto tail = [&](int which, int lf1, float *f1, uint32_t *mf1, float *f2, uint32_t *mf2, float *out, int kk) -> int {
        GemmArgs a = gemm_args(ws->pool + which * GF, 3 * GF, W(lf1), GF, f1, 512, B, GF, 512);
        a.bias = Bi(lf1); a.mask_out = mf1;
        if (int r = run_gemm<EPI_RELU_AFFINE>(a, st)) return r;
        a = gemm_args(f1, 512, W(lf1 + 1), 512, f2, 256, B, 512, 256);
        a.bias = Bi(lf1 + 1); a.mask_out = mf2;
        if (int r = run_gemm<EPI_RELU_AFFINE>(a, st)) return r;
        a = gemm_args(f2, 256, W(lf1 + 2), 256, out, kk, B, 256, kk);
        a.bias = Bi(lf1 + 2);
        return run_gemm<EPI_LINEAR>(a, st);
    };

    // ---- STN3d on x[:, :6]
    {
        GemmArgs a = gemm_args(x, 9, W(L_A1), 6, ws->a1, 64, R, 6, 64);
        a.bias = Bi(L_A1);
        if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        a = gemm_args(ws->a1, 64, W(L_A2), 64, ws->a2, 128, R, 64, 128);
        a.bias = Bi(L_A2);
        if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        if ((rc = pool_layer(ws->a2, L_A3, 1, 0))) return rc;
        if ((rc = tail(0, L_F1, ws->f1, ws->mf1, ws->f2, ws->mf2, ws->trans, 9))) return rc;
    }
    // ---- encoder conv1 with trans folded in per room: W1f_b = [W[:, 0:3] trans_b^T | W[:, 3:6]]
    {
        GemmArgs a = gemm_args(W(L_C1), 6, ws->trans, 3, ws->t1, B * 3, 64, 3, B * 3);
        if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
        hipLaunchKernelGGL(pn_c1_assemble_kernel, dim3(grid1((size_t)B * 512)), dim3(256), 0, st, ws->t1, W(L_C1), B, ws->w1f);
        PSG_LAUNCH_CHECK();
        for (int b = 0; b < B; ++b) {
            a = gemm_args(x + (size_t)b * N * 9, 9, ws->w1f + b * 512, 8, ws->h + (size_t)b * N * 64, 64, N, 6, 64);
            a.bias = Bi(L_C1); a.mask_out = ws->mh + (size_t)b * N * 2;
            if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        }
    }
    // ---- STNkd on h
    {
        GemmArgs a = gemm_args(ws->h, 64, W(L_K1), 64, ws->k1, 64, R, 64, 64);
        a.bias = Bi(L_K1);
        if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        a = gemm_args(ws->k1, 64, W(L_K2), 64, ws->k2, 128, R, 64, 128);
        a.bias = Bi(L_K2);
        if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        if ((rc = pool_layer(ws->k2, L_K3, 1, 1))) return rc;
        if ((rc = tail(1, L_FK1, ws->fk1, ws->mfk1, ws->fk2, ws->mfk2, ws->tf, 4096))) return rc;
    }
    // ---- trans_feat folded into conv2 and into the head's pointfeat columns: (W T_b^T)[o][i] = sum_j W[o][j] T_b[i][j],
    // one GEMM for all rooms (the B transforms stacked as the [B*64][64] weight operand)
    {
        GemmArgs a = gemm_args(W(L_C2), 64, ws->tf, 64, ws->c2f, B * 64, 128, 64, B * 64);
        if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
        a = gemm_args(W(L_H1) + GF, 1088, ws->tf, 64, ws->h1pf, B * 64, 512, 64, B * 64);
        if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
        for (int b = 0; b < B; ++b) {
            a = gemm_args(ws->h + (size_t)b * N * 64, 64, ws->c2f + b * 64, B * 64, ws->e2 + (size_t)b * N * 128, 128, N, 64, 128);
            a.bias = Bi(L_C2);
            if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        }
        if ((rc = pool_layer(ws->e2, L_C3, 0, 2))) return rc;
    }
    // ---- head: conv1's global columns as a per-room bias, the pointfeat columns with trans_feat folded in
    {
        GemmArgs a = gemm_args(ws->pool + 2 * GF, 3 * GF, W(L_H1), 1088, ws->gb, 512, B, GF, 512);
        a.bias = Bi(L_H1);
        if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
        for (int b = 0; b < B; ++b) {
            a = gemm_args(ws->h + (size_t)b * N * 64, 64, ws->h1pf + b * 64, B * 64, ws->z1 + (size_t)b * N * 512, 512, N, 64, 512);
            a.gbias = ws->gb + b * 512; a.group_rows = N; a.mask_out = ws->m1 + (size_t)b * N * 16;
            if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        }
        a = gemm_args(ws->z1, 512, W(L_H2), 512, ws->z2, 256, R, 512, 256);
        a.bias = Bi(L_H2); a.mask_out = ws->m2;
        if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        a = gemm_args(ws->z2, 256, W(L_H3), 256, ws->z3, 128, R, 256, 128);
        a.bias = Bi(L_H3); a.mask_out = ws->m3;
        if ((rc = run_gemm<EPI_RELU_AFFINE>(a, st))) return rc;
        a = gemm_args(ws->z3, 128, W(L_H4), 128, ws->logits, NCLS, R, 128, NCLS);
        a.bias = Bi(L_H4);
        if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
        if (!with_logp) {
            ws->have_fwd = true;
            return PSG_OK;
        }
        hipLaunchKernelGGL(pn_log_softmax_kernel, dim3(grid1(R)), dim3(256), 0, st, ws->logits, (size_t)R, ws->logp);
        PSG_LAUNCH_CHECK();
        if (logp_out && logp_out != ws->logp)
            PSG_CHECK_HIP(hipMemcpyAsync(logp_out, ws->logp, (size_t)R * NCLS * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    ws->have_fwd = true;
    return PSG_OK;
}

// dlogp == null: ws->dz4 already holds the gradient of the logits (written by pn_nu_head_kernel)
int backward_impl(psg_pointnet_model *m, psg_pointnet_ws *ws, const float *dlogp, const float *dtf_up, float *dx0_out,
                  hipStream_t st)
{
    const int B = ws->B, N = ws->N, R = B * N;
    int rc;
    // ---- head transposes through the stored ReLU bits
    if (dlogp) {
        hipLaunchKernelGGL(pn_log_softmax_bwd_kernel, dim3(grid1(R)), dim3(256), 0, st, ws->logp, dlogp, (size_t)R, ws->dz4);
        PSG_LAUNCH_CHECK();
    }
    GemmArgs a = gemm_args(ws->dz4, NCLS, m->h4t, NCLS, ws->dz3, 128, R, NCLS, 128);
    a.mask_in = ws->m3;
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    a = gemm_args(ws->dz3, 128, m->h3t, 128, ws->dz2, 256, R, 128, 256);
    a.mask_in = ws->m2;
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    a = gemm_args(ws->dz2, 256, m->h2t, 256, ws->dz1, 512, R, 256, 512);
    a.mask_in = ws->m1;
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    // pointfeat gradient (dense part) and the global branch: column sum of dz1, then W1g^T
    a = gemm_args(ws->dz1, 512, m->h1pt, 512, ws->dpf, 64, R, 512, 64);
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    hipLaunchKernelGGL(pn_colsum_kernel, dim3(512 / 64, B), dim3(256), 0, st, ws->dz1, N, 512, ws->s1);
    PSG_LAUNCH_CHECK();
    a = gemm_args(ws->s1, 512, m->h1gt, 512, ws->dg, GF, B, 512, GF);
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    // encoder max-pool (no ReLU before it): arg-max rows through conv3^T and conv2^T into dpf
    PoolBwdArgs pa{};
    pa.coef = ws->dg; pa.pool = ws->pool + 2 * GF; pa.idx = ws->pidx + 2 * GF; pa.ld_pool = 3 * GF; pa.relu_pool = 0;
    pa.w3 = m->w[L_C3]; pa.act2 = ws->e2; pa.w2 = m->w[L_C2]; pa.act1 = nullptr; pa.w1 = nullptr; pa.out_mask = nullptr;
    pa.out = ws->dpf; pa.ld_out = 64; pa.c_out = 64; pa.N = N;
    hipLaunchKernelGGL(pn_pool_bwd_kernel, dim3(GF, B), dim3(128), 0, st, pa);
    PSG_LAUNCH_CHECK();
    // trans_feat: dT_b = h_b^T dpf_b (+ the upstream gradient of trans_feat); dh = (dpf T_b^T) * [h > 0]
    const dim3 tg(ceil_div(N, 32), 2, B);
    hipLaunchKernelGGL(pn_transpose_kernel, tg, dim3(256), 0, st, ws->h, N, 64, ws->ht);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(pn_transpose_kernel, tg, dim3(256), 0, st, ws->dpf, N, 64, ws->dpft);
    PSG_LAUNCH_CHECK();
    for (int b = 0; b < B; ++b) {
        a = gemm_args(ws->ht + (size_t)b * 64 * N, N, ws->dpft + (size_t)b * 64 * N, N, ws->dtf + (size_t)b * 4096, 64, 64, N, 64);
        if (dtf_up) { a.accumulate = 2; a.addend = dtf_up + (size_t)b * 4096; a.ld_add = 64; }
        if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
        a = gemm_args(ws->dpf + (size_t)b * N * 64, 64, ws->tf + (size_t)b * 4096, 64, ws->dh + (size_t)b * N * 64, 64, N, 64, 64);
        a.mask_in = ws->mh + (size_t)b * N * 2;
        if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    }
    // STNkd: fc3^T, fc2^T, fc1^T, then its max-pool sparsely through conv3^T, conv2^T, conv1^T into dh
    a = gemm_args(ws->dtf, 4096, m->fk3t, 4096, ws->dfk2, 256, B, 4096, 256);
    a.mask_in = ws->mfk2;
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    a = gemm_args(ws->dfk2, 256, m->fk2t, 256, ws->dfk1, 512, B, 256, 512);
    a.mask_in = ws->mfk1;
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    a = gemm_args(ws->dfk1, 512, m->fk1t, 512, ws->dgk, GF, B, 512, GF);
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    pa.coef = ws->dgk; pa.pool = ws->pool + GF; pa.idx = ws->pidx + GF; pa.relu_pool = 1;
    pa.w3 = m->w[L_K3]; pa.act2 = ws->k2; pa.w2 = m->w[L_K2]; pa.act1 = ws->k1; pa.w1 = m->w[L_K1]; pa.out_mask = ws->h;
    pa.out = ws->dh; pa.ld_out = 64; pa.c_out = 64;
    hipLaunchKernelGGL(pn_pool_bwd_kernel, dim3(GF, B), dim3(128), 0, st, pa);
    PSG_LAUNCH_CHECK();
    // encoder conv1^T (unfolded weights: d(xyz . trans) and d rgb), then the input transform
    a = gemm_args(ws->dh, 64, m->c1t, 64, ws->dxu, 8, R, 64, 6);
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    hipLaunchKernelGGL(pn_xyz_bwd_kernel, dim3(B), dim3(256), 0, st, ws->x0in, ws->dxu, ws->trans, N, dx0_out, ws->dtrans);
    PSG_LAUNCH_CHECK();
    // STN3d: fc3^T, fc2^T, fc1^T, then its max-pool sparsely through conv3^T, conv2^T, conv1^T into dx0[:, 0:6]
    a = gemm_args(ws->dtrans, 9, m->f3t, 9, ws->df2, 256, B, 9, 256);
    a.mask_in = ws->mf2;
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    a = gemm_args(ws->df2, 256, m->f2t, 256, ws->df1, 512, B, 256, 512);
    a.mask_in = ws->mf1;
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    a = gemm_args(ws->df1, 512, m->f1t, 512, ws->dgs, GF, B, 512, GF);
    if ((rc = run_gemm<EPI_LINEAR>(a, st))) return rc;
    pa.coef = ws->dgs; pa.pool = ws->pool; pa.idx = ws->pidx; pa.relu_pool = 1;
    pa.w3 = m->w[L_A3]; pa.act2 = ws->a2; pa.w2 = m->w[L_A2]; pa.act1 = ws->a1; pa.w1 = m->w[L_A1]; pa.out_mask = nullptr;
    pa.out = dx0_out; pa.ld_out = 9; pa.c_out = 6;
    hipLaunchKernelGGL(pn_pool_bwd_kernel, dim3(GF, B), dim3(128), 0, st, pa);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// [in][out] transpose of columns [c0, c0 + cols) of a row-major [rows][ld] matrix
std::vector<float> transpose_cols(const float *w, int rows, int ld, int c0, int cols)
{
    std::vector<float> t((size_t)cols * rows);
    for (int o = 0; o < rows; ++o)
        for (int i = 0; i < cols; ++i) t[(size_t)i * rows + o] = w[(size_t)o * ld + c0 + i];
    return t;
}

}  // namespace

extern "C" int psg_pointnet_model_create(psg_ctx *ctx, const float *const *weights, const float *const *biases,
                                         psg_pointnet_model **out)
{
    PSG_REQUIRE(ctx && weights && biases && out, "psg_pointnet_model_create: null argument");
    for (int l = 0; l < NL; ++l) PSG_REQUIRE(weights[l] && biases[l], "psg_pointnet_model_create: layer %d missing", l);
    PSG_CHECK_HIP(hipSetDevice(ctx->device));
    auto *m = new psg_pointnet_model();
    m->ctx = ctx;
    m->gen = next_generation();
    bool ok = true;
    for (int l = 0; l < NL && ok; ++l) {
        const int M = LDIM[l][0], K = LDIM[l][1];
        m->w[l] = upload(m->allocs, std::vector<float>(weights[l], weights[l] + (size_t)M * K));
        m->b[l] = upload(m->allocs, std::vector<float>(biases[l], biases[l] + M));
        ok = m->w[l] && m->b[l];
    }
    auto T = [&](int l, int c0, int cols) {
        float *p = upload(m->allocs, transpose_cols(weights[l], LDIM[l][0], LDIM[l][1], c0, cols));
        ok = ok && p;
        return p;
    };
    if (ok) {
        m->f3t = T(L_F3, 0, 256); m->f2t = T(L_F2, 0, 512); m->f1t = T(L_F1, 0, GF);
        m->fk3t = T(L_FK3, 0, 256); m->fk2t = T(L_FK2, 0, 512); m->fk1t = T(L_FK1, 0, GF);
        m->h4t = T(L_H4, 0, 128); m->h3t = T(L_H3, 0, 256); m->h2t = T(L_H2, 0, 512);
        m->h1pt = T(L_H1, GF, 64); m->h1gt = T(L_H1, 0, GF); m->c1t = T(L_C1, 0, 6);
    }
    if (!ok) {
        for (void *p : m->allocs) (void)hipFree(p);
        delete m;
        set_error("psg_pointnet_model_create: device allocation or upload failed");
        return PSG_ERR_HIP;
    }
    *out = m;
    return PSG_OK;
}

extern "C" int psg_pointnet_model_destroy(psg_pointnet_model *m)
{
    if (!m) return PSG_OK;
    for (void *p : m->allocs) (void)hipFree(p);
    delete m;
    return PSG_OK;
}

extern "C" int psg_pointnet_ws_create(psg_ctx *ctx, int batch, int n_point, psg_pointnet_ws **out)
{
    PSG_REQUIRE(ctx && out, "psg_pointnet_ws_create: null argument");
    PSG_REQUIRE(batch > 0 && batch <= 256, "psg_pointnet_ws_create: batch=%d out of range (1..256)", batch);
    PSG_REQUIRE(n_point > 0 && n_point % PT == 0 && n_point <= (1 << 20),
                "psg_pointnet_ws_create: n_point=%d must be a positive multiple of the point tile %d", n_point, PT);
    PSG_CHECK_HIP(hipSetDevice(ctx->device));
    auto *ws = new psg_pointnet_ws();
    ws->ctx = ctx; ws->B = batch; ws->N = n_point;
    ws->gen = next_generation();
    const size_t B = batch, R = (size_t)batch * n_point, T = R / PT;
    auto layout = [&](Bump &bp) {
        auto F = [&](float **p, size_t n) { *p = bp.take<float>(n); };
        auto I = [&](int32_t **p, size_t n) { *p = bp.take<int32_t>(n); };
        auto U = [&](uint32_t **p, size_t n) { *p = bp.take<uint32_t>(n); };
        F(&ws->a1, R * 64); F(&ws->a2, R * 128); F(&ws->h, R * 64); F(&ws->k1, R * 64); F(&ws->k2, R * 128); F(&ws->e2, R * 128);
        F(&ws->z1, R * 512); F(&ws->z2, R * 256); F(&ws->z3, R * 128); F(&ws->logits, R * NCLS); F(&ws->logp, R * NCLS);
        U(&ws->mh, R * 2); U(&ws->m1, R * 16); U(&ws->m2, R * 8); U(&ws->m3, R * 4);
        F(&ws->part_val, T * GF); I(&ws->part_idx, T * GF); F(&ws->pool, B * 3 * GF); I(&ws->pidx, B * 3 * GF);
        F(&ws->f1, B * 512); F(&ws->f2, B * 256); F(&ws->trans, B * 9); F(&ws->fk1, B * 512); F(&ws->fk2, B * 256); F(&ws->tf, B * 4096);
        U(&ws->mf1, B * 16); U(&ws->mf2, B * 8); U(&ws->mfk1, B * 16); U(&ws->mfk2, B * 8);
        F(&ws->t1, 64 * B * 3); F(&ws->w1f, B * 512); F(&ws->c2f, 128 * B * 64); F(&ws->h1pf, 512 * B * 64); F(&ws->gb, B * 512);
        F(&ws->x0in, R * 9);
        F(&ws->dz4, R * NCLS); F(&ws->dz3, R * 128); F(&ws->dz2, R * 256); F(&ws->dz1, R * 512); F(&ws->s1, B * 512); F(&ws->dg, B * GF);
        F(&ws->dpf, R * 64); F(&ws->ht, R * 64); F(&ws->dpft, R * 64); F(&ws->dtf, B * 4096); F(&ws->dfk2, B * 256);
        F(&ws->dfk1, B * 512); F(&ws->dgk, B * GF); F(&ws->dh, R * 64); F(&ws->dxu, R * 8); F(&ws->dtrans, B * 9);
        F(&ws->df2, B * 256); F(&ws->df1, B * 512); F(&ws->dgs, B * GF);
        F(&ws->x0, R * 9); F(&ws->ori, R * 3); F(&ws->dlogp, R * NCLS); F(&ws->dx0, R * 9);
        I(&ws->labels, R);
        ws->mask = bp.take<uint8_t>((size_t)n_point);
    };
    if (int rc = carve_arena(&ws->arena, &ws->bytes, "psg_pointnet_ws_create", layout)) {
        delete ws;
        return rc;
    }
    // the dense dxu columns 6:8 are never written by the GEMM (M = 6): keep them defined
    if (psg::memset_sync(ws->dxu, 0, R * 8 * sizeof(float)) != hipSuccess) {
        (void)hipFree(ws->arena);
        delete ws;
        set_error("psg_pointnet_ws_create: memset failed");
        return PSG_ERR_HIP;
    }
    *out = ws;
    return PSG_OK;
}

extern "C" int psg_pointnet_ws_destroy(psg_pointnet_ws *ws)
{
    if (!ws) return PSG_OK;
    if (ws->arena) (void)hipFree(ws->arena);
    delete ws;
    return PSG_OK;
}

extern "C" int psg_pointnet_forward(psg_pointnet_model *m, psg_pointnet_ws *ws, const float *x0, float *logp_out,
                                    float *trans_out, float *trans_feat_out, float *pool_out, int32_t *arg_out,
                                    psg_stream stream)
{
    PSG_REQUIRE(m && ws && x0, "psg_pointnet_forward: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = forward_impl(m, ws, x0, logp_out, st)) return rc;
    const size_t B = ws->B;
    if (trans_out) PSG_CHECK_HIP(hipMemcpyAsync(trans_out, ws->trans, B * 9 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (trans_feat_out) PSG_CHECK_HIP(hipMemcpyAsync(trans_feat_out, ws->tf, B * 4096 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (pool_out) PSG_CHECK_HIP(hipMemcpyAsync(pool_out, ws->pool, B * 3 * GF * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (arg_out) PSG_CHECK_HIP(hipMemcpyAsync(arg_out, ws->pidx, B * 3 * GF * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return PSG_OK;
}

// Read-only tap into the workspace (include/psg.h lists the codes and the two validity windows): a pointer, a row count
// and a column count; no launch, no allocation, no synchronisation.
extern "C" const void *psg_pointnet_debug_ptr(const psg_pointnet_ws *ws, int what, int *rows_out, int *cols_out)
{
    if (!ws) { set_error("psg_pointnet_debug_ptr: null workspace"); return nullptr; }
    const int B = ws->B, R = ws->B * ws->N, T = R / PT;
    const void *p = nullptr;
    int r = 0, c = 0;
    auto put = [&](const void *ptr, int rows, int cols) { p = ptr; r = rows; c = cols; };
    switch (what) {
    case 0: put(ws->a1, R, 64); break;
    case 1: put(ws->a2, R, 128); break;
    case 2: put(ws->h, R, 64); break;
    case 3: put(ws->k1, R, 64); break;
    case 4: put(ws->k2, R, 128); break;
    case 5: put(ws->e2, R, 128); break;
    case 6: put(ws->z1, R, 512); break;
    case 7: put(ws->z2, R, 256); break;
    case 8: put(ws->z3, R, 128); break;
    case 9: put(ws->logits, R, NCLS); break;
    case 10: put(ws->logp, R, NCLS); break;
    case 11: put(ws->x0in, R, 9); break;
    case 20: put(ws->mh, R, 2); break;                                // mask words: cols = 32-bit words per row
    case 21: put(ws->m1, R, 16); break;
    case 22: put(ws->m2, R, 8); break;
    case 23: put(ws->m3, R, 4); break;
    case 24: put(ws->mf1, B, 16); break;
    case 25: put(ws->mf2, B, 8); break;
    case 26: put(ws->mfk1, B, 16); break;
    case 27: put(ws->mfk2, B, 8); break;
    case 30: put(ws->pool, B, 3 * GF); break;
    case 31: put(ws->pidx, B, 3 * GF); break;                         // int32
    case 32: put(ws->part_val, T, GF); break;
    case 33: put(ws->part_idx, T, GF); break;                         // int32
    case 40: put(ws->f1, B, 512); break;
    case 41: put(ws->f2, B, 256); break;
    case 42: put(ws->trans, B, 9); break;
    case 43: put(ws->fk1, B, 512); break;
    case 44: put(ws->fk2, B, 256); break;
    case 45: put(ws->tf, B, 4096); break;
    case 46: put(ws->t1, 64, 3 * B); break;
    case 47: put(ws->w1f, B * 64, 8); break;
    case 48: put(ws->c2f, 128, 64 * B); break;
    case 49: put(ws->h1pf, 512, 64 * B); break;
    case 50: put(ws->gb, B, 512); break;
    case 60: put(ws->dz4, R, NCLS); break;
    case 61: put(ws->dz3, R, 128); break;
    case 62: put(ws->dz2, R, 256); break;
    case 63: put(ws->dz1, R, 512); break;
    case 64: put(ws->s1, B, 512); break;
    case 65: put(ws->dg, B, GF); break;
    case 66: put(ws->dpf, R, 64); break;
    case 67: put(ws->ht, B * 64, ws->N); break;
    case 68: put(ws->dpft, B * 64, ws->N); break;
    case 69: put(ws->dtf, B, 4096); break;
    case 70: put(ws->dfk2, B, 256); break;
    case 71: put(ws->dfk1, B, 512); break;
    case 72: put(ws->dgk, B, GF); break;
    case 73: put(ws->dh, R, 64); break;
    case 74: put(ws->dxu, R, 8); break;
    case 75: put(ws->dtrans, B, 9); break;
    case 76: put(ws->df2, B, 256); break;
    case 77: put(ws->df1, B, 512); break;
    case 78: put(ws->dgs, B, GF); break;
    default: set_error("psg_pointnet_debug_ptr: unknown buffer code what=%d", what); return nullptr;
    }
    if (rows_out) *rows_out = r;
    if (cols_out) *cols_out = c;
    return p;
}

extern "C" int psg_pointnet_backward(psg_pointnet_model *m, psg_pointnet_ws *ws, const float *dlogp, const float *dtrans_feat,
                                     float *dx0_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && dlogp && dx0_out, "psg_pointnet_backward: null argument");
    if (!ws->have_fwd) {
        set_error("psg_pointnet_backward: no forward has run in this workspace");
        return PSG_ERR_STATE;
    }
    return backward_impl(m, ws, dlogp, dtrans_feat, dx0_out, (hipStream_t)stream);
}

extern "C" int psg_pointnet_nb_attack(psg_pointnet_model *m, psg_pointnet_ws *ws, const float *images, const int32_t *labels,
                                      const uint8_t *mask, float eps, float alpha, int iters, int targeted, int target,
                                      float *adv_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && images && adv_out, "psg_pointnet_nb_attack: null argument");
    PSG_REQUIRE(targeted || labels, "psg_pointnet_nb_attack: labels required for the non-targeted attack");
    PSG_REQUIRE(iters > 0, "psg_pointnet_nb_attack: iters=%d must be positive", iters);
    hipStream_t st = (hipStream_t)stream;
    const int B = ws->B, N = ws->N, R = B * N;
    int rc;
    if ((rc = psg_to_point_major(images, B, 9, N, ws->x0, st))) return rc;
    if (!targeted) PSG_CHECK_HIP(hipMemcpyAsync(ws->labels, labels, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (mask) PSG_CHECK_HIP(hipMemcpyAsync(ws->mask, mask, (size_t)N, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(pn_extract_color_kernel, dim3(grid1((size_t)R * 3)), dim3(256), 0, st, ws->x0, ws->ori, (size_t)R);
    PSG_LAUNCH_CHECK();
    for (int it = 0; it < iters; ++it) {
        if ((rc = forward_impl(m, ws, ws->x0, nullptr, st))) return rc;
        // non-targeted: CE_sum over all rooms / N (nontarget.py:34); targeted: CE_mean of room 0 (target.py:36-39)
        if ((rc = psg_ce_logp_grad(ws->logp, targeted ? nullptr : ws->labels, target, R, targeted ? N : R, NCLS, 1.0f / (float)N,
                                   ws->dlogp, nullptr, st)))
            return rc;
        if ((rc = backward_impl(m, ws, ws->dlogp, nullptr, ws->dx0, st))) return rc;
        if ((rc = psg_pgd_step(ws->x0, ws->dx0, ws->ori, mask ? ws->mask : nullptr, B, N, alpha, eps, targeted ? -1.0f : 1.0f,
                               it == iters - 1, st)))
            return rc;
    }
    return psg_to_channel_major(ws->x0, B, 9, N, adv_out, st);
}

// The window's seam on its own (tests, tools): logits [B][N][13] -> dz, pred, f sums (one per room when per_room, else one).
// With both scratch arrays the three-kernel sequence the per-step entry points run, else pn_nu_head_kernel.
extern "C" int psg_pointnet_nu_head(const float *logits, const int32_t *labels, int target, int B, int N, int per_room, float kappa,
                                    float tsign, float *logp_scratch, float *dlogp_scratch, float *dz_out, float *f_sum,
                                    int32_t *pred_out, psg_stream stream)
{
    PSG_REQUIRE(logits && dz_out && f_sum && pred_out && B > 0 && N > 0, "psg_pointnet_nu_head: bad argument");
    PSG_REQUIRE(N % PT == 0, "psg_pointnet_nu_head: N=%d must be a multiple of the point tile %d", N, PT);
    PSG_REQUIRE(labels || (target >= 0 && target < NCLS), "psg_pointnet_nu_head: target class %d out of range", target);
    PSG_REQUIRE(!logp_scratch == !dlogp_scratch, "psg_pointnet_nu_head: give both scratch arrays or neither");
    PSG_REQUIRE(((uintptr_t)logits | (uintptr_t)dz_out) % 16 == 0, "psg_pointnet_nu_head: logits and dz_out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t R = (size_t)B * N;
    if (!logp_scratch) {
        hipLaunchKernelGGL(pn_nu_head_kernel, dim3(grid1(R)), dim3(256), 0, st, logits, labels, target, (int)R, kappa, tsign, dz_out, f_sum,
                           pred_out, per_room ? N : 0);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    hipLaunchKernelGGL(pn_log_softmax_kernel, dim3(grid1(R)), dim3(256), 0, st, logits, R, logp_scratch);
    PSG_LAUNCH_CHECK();
    if (int rc = per_room ? psg_nu_f_loss_grad_rooms(logp_scratch, labels, target, B, N, NCLS, kappa, tsign, dlogp_scratch, f_sum, pred_out, stream)
                          : psg_nu_f_loss_grad(logp_scratch, labels, target, (int)R, NCLS, kappa, tsign, dlogp_scratch, f_sum, pred_out, stream))
        return rc;
    hipLaunchKernelGGL(pn_log_softmax_bwd_kernel, dim3(grid1(R)), dim3(256), 0, st, logp_scratch, dlogp_scratch, R, dz_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// ---- NU_attack / tar_NU_attack windows on this network (include/psg.h: psg_pointnet_nu_window_args) ----------------------
// One step sequence of a window, shared by the eager and the captured path; dconsts_rows: the window's device rows or null.
// Everything in it is a launch or an asynchronous device-to-device copy on `stream`: the forward and the backward take all
// their buffers from the workspace arena (psg_pointnet_ws_create), so a window can be captured as a single chain.
static int pn_nu_window_steps(const psg_pointnet_nu_window_args *a, const float *dconsts_rows, psg_stream stream)
{
    hipStream_t st = (hipStream_t)stream;
    const bool rooms = a->G > 1;
    const int B = a->G * a->rows, N = a->N, G = a->G;
    int rc = PSG_OK;
    for (int i = 0; i < a->n_steps && rc == PSG_OK; ++i) {
        const int step = a->step0 + i, adam_t = a->adam_t0 + i + 1;
        const int32_t *f_labels = a->use_target ? nullptr : a->labels;
        const int f_target = a->use_target ? a->target : 0;
        if ((rc = rooms ? psg_nu_tanh_color_rooms(a->w, a->mask, B, N, a->x0, stream) : psg_nu_tanh_color(a->w, a->mask, B, N, a->x0, stream)))
            break;
        if (a->fused_head) {
            if ((rc = forward_impl(a->model, a->ws, a->x0, nullptr, st, false))) break;
            hipLaunchKernelGGL(pn_nu_head_kernel, dim3(grid1((size_t)B * N)), dim3(256), 0, st, a->ws->logits, f_labels, f_target, B * N,
                               a->kappa, a->tsign, a->ws->dz4, a->scal, a->pred, rooms ? N : 0);
            PSG_LAUNCH_CHECK();
            if ((rc = backward_impl(a->model, a->ws, nullptr, nullptr, a->dx0, st))) break;
        } else {
            if ((rc = forward_impl(a->model, a->ws, a->x0, a->logp, st))) break;
            if ((rc = rooms ? psg_nu_f_loss_grad_rooms(a->ws->logp, f_labels, f_target, B, N, NCLS, a->kappa, a->tsign, a->dlogp, a->scal,
                                                       a->pred, stream)
                            : psg_nu_f_loss_grad(a->ws->logp, f_labels, f_target, B * N, NCLS, a->kappa, a->tsign, a->dlogp, a->scal, a->pred,
                                                 stream)))
                break;
            if ((rc = backward_impl(a->model, a->ws, a->dlogp, nullptr, a->dx0, st))) break;
        }
        if ((rc = psg_smooth_knn_rooms(a->x0 + 3, 9, (size_t)N * 9, a->ori, 3, (size_t)N * 3, G, N, a->neighbour, a->scal + G, a->sgrad,
                                       a->nn_state, (i > 0 || a->warm_first) ? 1 : 0, stream)))
            break;
        psg::NuStepConsts consts(dconsts_rows ? dconsts_rows + 4 * i : nullptr);
        rc = psg::nu_colour_adam(a, a->c_smooth, a->c_l2, a->rows, adam_t, stream);
        if (rc == PSG_OK) rc = psg::nu_latch(a, a->rows, a->hist + (size_t)i * 5 * G, step, stream);
    }
    return rc;
}

extern "C" int psg_pointnet_nu_window(const psg_pointnet_nu_window_args *a, psg_nu_graph *graph, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->w && a->m && a->v && a->x0 && a->ori && a->labels && a->dx0 && a->sgrad && a->pred &&
                    a->scal && a->nn_state && a->hist && a->out && a->active && a->exit_step,
                "psg_pointnet_nu_window: null argument");
    PSG_REQUIRE(a->fused_head || a->dlogp, "psg_pointnet_nu_window: the three-kernel head needs the dlogp scratch");
    PSG_REQUIRE(a->n_steps > 0 && a->G > 0 && a->rows > 0 && (a->G == 1 || a->rows == 1),
                "psg_pointnet_nu_window: (G, rows) must be (1, B) or (R, 1)");
    PSG_REQUIRE(a->G * a->rows == a->ws->B && a->N == a->ws->N, "psg_pointnet_nu_window: the workspace is for %d x %d points, not %d x %d",
                a->ws->B, a->ws->N, a->G * a->rows, a->N);
    PSG_REQUIRE(a->mode == 0 || (a->mask && a->n_mask), "psg_pointnet_nu_window: modes 1 and 2 need mask and n_mask");
    PSG_REQUIRE(a->use_target ? (a->target >= 0 && a->target < NCLS) : 1, "psg_pointnet_nu_window: target class %d out of range", a->target);
    psg_pointnet_nu_window_args key = *a;
    key.step0 = 0; key.adam_t0 = 0; key.lr = 0.0f;      // what the device row carries
    return nu_graph_window(graph, &key, sizeof(key), a->model->gen, a->ws->gen, a->n_steps, a->step0, a->adam_t0, a->lr, a->beta1,
                           a->beta2, (hipStream_t)stream, [&](const float *rows) { return pn_nu_window_steps(a, rows, stream); });
}
