// ResGCN-28 (dense DeepGCN) semantic-segmentation network on gfx950: forward, input-gradient backward
// and the NB colour attack loop.  Reference (paths relative to /root/reference/ResGCN):
//   gcn_lib/dense/torch_edge.py:32-79   pairwise_distance, dense_knn_matrix, DenseDilated(KnnGraph)
//   gcn_lib/dense/torch_nn.py:55-98     BasicConv (Conv -> ReLU -> BatchNorm), batched_index_select
//   gcn_lib/dense/torch_vertex.py:23-100 EdgeConv2d, DynConv2d, ResDynBlock2d
//   sem_seg_dense/architecture.py:58-68  DenseDeepGCN.forward
//   sem_seg_dense/attacks/torchattacks/attacks/colper.py:17-39  NB_attack
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
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "psg_common.h"
#include "psg_gemm.cuh"
#include "psg_knn.h"
#include "psg_knn_ops.cuh"
#include "psg_wave.cuh"

using namespace psg;

namespace {

constexpr int GC = 64;      // n_filters
constexpr int NCLS = 13;
constexpr int KNB = 16;     // k

// (PSG_GEMM_SMALL_BELOW: the workgroup count below which launch_gemm takes 64 x 64 tiles, for A/B runs)
template <int WM, int WN, int EPI, bool ASC>
int launch_gemm(const GemmArgs &a, hipStream_t st)
{
    static const size_t small_below = (size_t)psg::env_int("PSG_GEMM_SMALL_BELOW", 384);
    return psg::launch_gemm<WM, WN, EPI, ASC>(a, small_below, st);
}

// ---- squared norms with the reference's summation order (SURVEY 8a'): for C = 64 torch.sum(x*x, -1) uses
// 8 lanes x 4 accumulators (two passes of 32), lane-wise ((a0+a1)+a2)+a3, then the 8 lanes left to right.
__global__ void sumsq_rows_kernel(const float *__restrict__ x, int ld, int C, size_t rows, float *__restrict__ out)
{
    // (this file is compiled with -ffp-contract=off: hipcc's __fmul_rn / __fadd_rn are plain operators, and with the
    // default contraction they were fused into v_pk_fma_f32 - norms one ulp off torch's for some rows, which showed as
    // 1-4 different neighbour rows per 4096-point graph)
    size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float *p = x + r * ld;
    float s;
    if (C == 64) {
        float acc[4][8];
#pragma unroll
        for (int jq = 0; jq < 4; ++jq)
#pragma unroll
            for (int l = 0; l < 8; ++l) acc[jq][l] = 0.0f;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass)
#pragma unroll
            for (int jq = 0; jq < 4; ++jq)
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    const float v = p[32 * pass + 8 * jq + l];
                    acc[jq][l] = __fadd_rn(acc[jq][l], __fmul_rn(v, v));
                }
        s = 0.0f;
        bool first = true;
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const float t = __fadd_rn(__fadd_rn(__fadd_rn(acc[0][l], acc[1][l]), acc[2][l]), acc[3][l]);
            s = first ? t : __fadd_rn(s, t);
            first = false;
        }
    } else {
        s = __fmul_rn(p[0], p[0]);
        for (int c = 1; c < C; ++c) s = __fadd_rn(s, __fmul_rn(p[c], p[c]));
    }
    out[r] = s;
}

// ---- dilated kNN selection: ONE WAVE per query row, no workgroup barriers and no atomics.  Only the KK = (k-1)*d+1
// (<= 406) smallest of the N <= 4096 distances matter, so instead of sorting the row:
//   1. every lane keeps 64 order-preserving 32-bit distance keys in registers (element q*64 + lane);
//   2. a threshold t with KK <= #(keys <= t) <= M (M = the power of two the final sort runs on) is found by
//      bisection on the DISTANCE value (arithmetic mean of the two bounds: the bit patterns between a ~0 self
//      distance and the populated binades would cost ~10 extra halvings), started from a bracket read off a
//      64-key sample (sample[i] has about (i+1)*N/64 keys below it).  Counts are per-lane compares + a DPP wave
//      sum: no LDS round trips in the loop;
//   3. the selected keys are compacted in index order into LDS as composite keys (distance << 12 | index: ascending
//      distance, lowest index on ties; torch.topk leaves tie order unspecified) and bitonic-sorted by the wave.  If
//      more than M keys tie at the threshold, the lowest-index ones are taken, which is exactly that order;
//   4. ranks 0, d, 2d, ... are emitted (torch.topk(-dist, k*d)[..., ::d], torch_edge.py:56,29).
constexpr int KS_WAVES = 4;          // rows per workgroup (independent waves)
constexpr int KS_PER_LANE = 64;      // N <= 4096
constexpr int KS_MAX_SEL = 512;


__global__ __launch_bounds__(KS_WAVES * 64) void knn_select_kernel(const float *__restrict__ dist, int N, size_t rows,
                                                                  int k, int d, int32_t *__restrict__ out)
{
    __shared__ unsigned long long cand_all[KS_WAVES][KS_MAX_SEL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row = (size_t)blockIdx.x * KS_WAVES + wave;
    if (row >= rows) return;
    unsigned long long *cand = cand_all[wave];
    const float *drow = dist + row * (size_t)N;
    const unsigned KK = (unsigned)((k - 1) * d + 1);
    unsigned M = 64;
    while (M < KK) M <<= 1;          // sort size; any count in [KK, M] is acceptable

    unsigned key[KS_PER_LANE];       // keys of elements q*64 + lane; padding = 0xFFFFFFFF sorts last
#pragma unroll
    for (int q = 0; q < KS_PER_LANE; ++q) {
        const int i = q * 64 + lane;
        key[q] = i < N ? key_of(drow[i]) : 0xFFFFFFFFu;
    }
    // invariant of the search: #(keys <= lo) = c_lo < KK <= #(keys <= hi); lo starts just below the row minimum
    unsigned kmin = key[0], kmax = 0u;
#pragma unroll
    for (int q = 0; q < KS_PER_LANE; ++q) {
        kmin = key[q] < kmin ? key[q] : kmin;
        kmax = (key[q] != 0xFFFFFFFFu && key[q] > kmax) ? key[q] : kmax;   // padding excluded
    }
    kmin = ~wave_max_u32(~kmin);
    kmax = wave_max_u32(kmax);
    unsigned lo = kmin ? kmin - 1u : 0u, hi = kmax;
    unsigned c_lo = 0, cnt = (unsigned)N;
    {   // bracket from the 64-key sample of elements 0..63: rank of every sample key among the samples
        const unsigned sv = key[0];
        unsigned rank = 0;
        for (int l = 0; l < 64; ++l) {
            const unsigned o = (unsigned)__builtin_amdgcn_readlane((int)sv, l);
            rank += (o < sv || (o == sv && l < lane)) ? 1u : 0u;
        }
        const int i0 = (int)((KK * 64u) / (unsigned)N);
        const int ilo = i0 - 2 - (i0 >> 3), ihi = i0 + 2 + (i0 >> 3);
        unsigned blo = lo, bhi = hi;
        if (ilo >= 0 && ilo < 64) blo = (unsigned)__builtin_amdgcn_readlane((int)sv, __builtin_ctzll(__ballot(rank == (unsigned)ilo)));
        if (ihi < 64) bhi = (unsigned)__builtin_amdgcn_readlane((int)sv, __builtin_ctzll(__ballot(rank == (unsigned)ihi)));
        unsigned a = 0, b = 0;
#pragma unroll
        for (int q = 0; q < KS_PER_LANE; ++q) {
            a += key[q] <= blo ? 1u : 0u;
            b += key[q] <= bhi ? 1u : 0u;
        }
        a = wave_sum_u32(a);
        b = wave_sum_u32(b);
        if (b >= KK) {
            hi = bhi; cnt = b;
            if (a < KK && blo > lo) { lo = blo; c_lo = a; }
        } else {
            lo = bhi; c_lo = b;
        }
    }
    while (cnt > M && hi - lo > 1u) {
        unsigned mid = key_of(0.5f * dist_of(lo) + 0.5f * dist_of(hi));
        if (!(mid > lo && mid < hi)) mid = lo + ((hi - lo) >> 1);
        unsigned c = 0;
#pragma unroll
        for (int q = 0; q < KS_PER_LANE; ++q) c += key[q] <= mid ? 1u : 0u;
        c = wave_sum_u32(c);
        if (c < KK) { lo = mid; c_lo = c; }
        else { hi = mid; cnt = c; }
    }
    // compact the selected keys into LDS as composite keys (distance << 12 | index)
    for (unsigned t = lane; t < M; t += 64) cand[t] = ~0ull;
    wave_lds_fence();
    const unsigned thr = hi;
    const bool cut = cnt > M;          // more than M keys <= thr: thr = lo + 1 and the keys equal to thr are rationed
    if (!cut) {
        // usual case: everything <= thr is taken and the order in LDS is irrelevant (the sort follows).  Every lane
        // counts its own hits, one DPP scan gives it a private range of slots, and it fills that range by itself.
        unsigned mine = 0;
#pragma unroll
        for (int q = 0; q < KS_PER_LANE; ++q) mine += key[q] <= thr ? 1u : 0u;
        unsigned incl = mine;
        incl += dpp_get<0x111, 0xF>(incl);   // row_shr:1 (lanes shifted in from outside the row read 0)
        incl += dpp_get<0x112, 0xF>(incl);   // row_shr:2
        incl += dpp_get<0x114, 0xF>(incl);   // row_shr:4
        incl += dpp_get<0x118, 0xF>(incl);   // row_shr:8: inclusive scan inside each row of 16 lanes
        incl += dpp_get<0x142, 0xA>(incl);   // row_bcast15: rows 1, 3 += total of the row before
        incl += dpp_get<0x143, 0xC>(incl);   // row_bcast31: rows 2, 3 += total of rows 0..1
        unsigned slot = incl - mine;
        uint2 *cand2 = (uint2 *)cand;
#pragma unroll
        for (int q = 0; q < KS_PER_LANE; ++q) {
            if (key[q] <= thr) {
                // composite key built right here (volatile asm: left to itself the compiler pre-computes all 64
                // composite keys up front, which costs 128 VGPRs and half the occupancy)
                unsigned lo32, hi32;
                asm volatile("v_lshl_or_b32 %0, %2, 12, %3\n\tv_or_b32 %0, %4, %0\n\tv_lshrrev_b32 %1, 20, %2"
                             : "=&v"(lo32), "=&v"(hi32) : "v"(key[q]), "v"(lane), "n"(q * 64));
                cand2[slot] = make_uint2(lo32, hi32);
                ++slot;
            }
        }
    } else {
        // tie cut (rare: more than M - KK equal distances): index order matters, so this path walks the row in index
        // order with ballots; it re-reads the distances instead of indexing the register copy (a rolled loop over
        // key[] would force the whole array into scratch, an unrolled one doubles the kernel's registers)
        const unsigned long long lt_mask = (1ull << lane) - 1ull;
        unsigned base_a = 0, base_b = 0;   // class a: keys below thr (slots from 0); class b: tied keys (slots from c_lo)
#pragma unroll 1
        for (int q = 0; q < KS_PER_LANE; ++q) {
            const int i = q * 64 + lane;
            const unsigned kq = i < N ? key_of(drow[i]) : 0xFFFFFFFFu;
            const bool pa = kq < thr, pb = kq == thr;
            const unsigned long long ma = __ballot(pa), mb = __ballot(pb);
            const unsigned long long ck = ((unsigned long long)kq << 12) | (unsigned)i;
            if (pa) cand[base_a + __popcll(ma & lt_mask)] = ck;
            if (pb) {
                const unsigned s2 = c_lo + base_b + __popcll(mb & lt_mask);
                if (s2 < M) cand[s2] = ck;
            }
            base_a += __popcll(ma);
            base_b += __popcll(mb);
        }
    }
    wave_lds_fence();
    switch (M) {
    case 64: wave_sort_keys<1>(cand, lane); break;
    case 128: wave_sort_keys<2>(cand, lane); break;
    case 256: wave_sort_keys<4>(cand, lane); break;
    default: wave_sort_keys<8>(cand, lane); break;
    }
    wave_lds_fence();
    if (lane < k) out[row * k + lane] = (int32_t)(cand[(size_t)lane * d] & 0xFFFull);
}

// ---- EdgeConv edge pass (forward): y[i][c] = max_k ( s_c * relu(P[i][c] + Q[nbr(i,k)][c]) + t_c ) (+ residual)
// One thread per (vertex, channel), channel fastest: the 64 lanes of a wave read one 256-byte Q row.
__global__ void edge_max_fwd_kernel(const float *__restrict__ pq, const int32_t *__restrict__ nbr,
                                    const float *__restrict__ scale, const float *__restrict__ shift,
                                    const float *__restrict__ resid, int ld_res, float *__restrict__ out, int ld_out,
                                    uint8_t *__restrict__ arg, int N, size_t total, float *__restrict__ sq_out,
                                    float *__restrict__ xp_out, unsigned short *__restrict__ bp_out)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % GC);
    const size_t v = t / GC;                 // global vertex (room * N + i)
    const size_t room_base = (v / N) * N;
    const float p = pq[v * 2 * GC + c];
    const float s = scale[c], sh = shift[c];
    float best = -INFINITY;
    int bk = 0;
    bool bact = false;
    const int32_t *nb = nbr + v * KNB;
    // all sixteen neighbour rows in flight at once (the indices are wave-uniform: one 64-byte scalar-side read), then the
    // max pass in edge order: the kernel is a chain of L2 round trips, four rounds of four cost twice the time of one of sixteen
    int nbk[KNB];
#pragma unroll
    for (int k = 0; k < KNB; ++k) nbk[k] = nb[k];
    float q[KNB];
#pragma unroll
    for (int k = 0; k < KNB; ++k) q[k] = pq[(room_base + nbk[k]) * 2 * GC + GC + c];
#pragma unroll
    for (int k = 0; k < KNB; ++k) {
        const float z = p + q[k];
        const bool act = z > 0.0f;
        const float y = (act ? z : 0.0f) * s + sh;
        if (y > best) { best = y; bk = k; bact = act; }
    }
    if (resid) best += resid[v * ld_res + c];
    out[v * ld_out + c] = best;
    arg[t] = (uint8_t)(bk | (bact ? 0x80 : 0));
    if (xp_out) {   // the next block's kNN reads the features in MFMA operand order (psg_knn_ops.cuh)
        knn_store_xp(xp_out, v, c, best);
        if (bp_out) knn_store_bp(bp_out, v, c, best);
    }
    if (sq_out) {
        // squared norm of the vertex's 64 new features for the next block's kNN, in torch.sum's order for 64
        // contiguous floats (sumsq_rows_kernel).  One wave holds exactly one vertex (lane = channel).
        const float sacc = knn_wave_sumsq(best, threadIdx.x & 63);
        if (c == 0) {
            sq_out[v] = sacc;
            if (bp_out) knn_store_aug((uint4 *)bp_out, v, sacc);
        }
    }
}

// ---- The same pass for 32 vertices per workgroup, followed by the NEXT block's per-vertex product on the matrix cores:
// the 32 x 64 tile of new features is kept in LDS (k8-block layout of psg_gemm.cuh) and four waves compute
// [P | Q]_next = y . [W1 - W2 ; W2]_next^T + [b, 0] for those vertices (one 32 x 32 tile each, 32 MFMAs, weights read from L2
// in operand order) - the [R, 64] x [64, 128] GEMM launch between two blocks and its re-read of the features are gone.
// The arithmetic of both halves is that of the separate kernels (same lane = channel max pass; same k order and the same
// mfma4 chain as gemm_rows_kernel's plain path), so features and products are bit-identical to the unfused sequence.
// 1024 threads = 16 waves, two vertices per wave in the first phase (occupancy hides the 16 gathered Q rows per vertex).
constexpr int EMF_V = 32, EMF_T = 1024, EMF_BLK = EMF_V * 8 + 8;
__global__ __launch_bounds__(EMF_T) void edge_max_pq_fwd_kernel(const float *__restrict__ pq, const int32_t *__restrict__ nbr,
                                                                 const float *__restrict__ scale, const float *__restrict__ shift,
                                                                 const float *__restrict__ resid, int ld_res, float *__restrict__ out,
                                                                 int ld_out, uint8_t *__restrict__ arg, int N, float *__restrict__ sq_out,
                                                                 float *__restrict__ xp_out, unsigned short *__restrict__ bp_out,
                                                                 const float *__restrict__ wk8_next, const float *__restrict__ bias_next,
                                                                 float *__restrict__ pq_next)
{
    __shared__ float s_x[8 * EMF_BLK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t v0 = (size_t)blockIdx.x * EMF_V;
    const int c = lane;
    const float s = scale[c], sh = shift[c];
#pragma unroll
    for (int pass = 0; pass < EMF_V / 16; ++pass) {
        const int vl = wave + 16 * pass;
        const size_t v = v0 + vl;
        const size_t t = v * GC + c;
        const size_t room_base = (v / N) * N;
        const float p = pq[v * 2 * GC + c];
        float best = -INFINITY;
        int bk = 0;
        bool bact = false;
        const int32_t *nb = nbr + v * KNB;
#pragma unroll 4
        for (int k = 0; k < KNB; ++k) {
            const float z = p + pq[(room_base + nb[k]) * 2 * GC + GC + c];
            const bool act = z > 0.0f;
            const float y = (act ? z : 0.0f) * s + sh;
            if (y > best) { best = y; bk = k; bact = act; }
        }
        if (resid) best += resid[v * ld_res + c];
        out[v * ld_out + c] = best;
        arg[t] = (uint8_t)(bk | (bact ? 0x80 : 0));
        s_x[(c >> 3) * EMF_BLK + vl * 8 + (c & 7)] = best;
        if (xp_out) {
            knn_store_xp(xp_out, v, c, best);
            if (bp_out) knn_store_bp(bp_out, v, c, best);
        }
        if (sq_out) {
            const float sacc = knn_wave_sumsq(best, lane);
            if (c == 0) {
                sq_out[v] = sacc;
                if (bp_out) knn_store_aug((uint4 *)bp_out, v, sacc);
            }
        }
    }
    __syncthreads();
    if (wave >= 4) return;
    const int j = lane & 31, h = lane >> 5;
    const int cbase = 32 * wave;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int k8 = 0; k8 < GC / 8; ++k8) {
        const float4 wa = *(const float4 *)(wk8_next + ((size_t)k8 * 2 * GC + cbase + j) * 8 + 4 * h);
        const float4 xb = *(const float4 *)(s_x + k8 * EMF_BLK + j * 8 + 4 * h);
        acc = mfma4<false>(wa, xb, acc);
    }
    // lane (j, h) holds channels cbase + 8 g + 4 h + (0..3) of vertex v0 + j (gemm_rows_kernel's epilogue, EPI_LINEAR)
    float *o = pq_next + (v0 + j) * 2 * GC + cbase + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 b4 = *(const float4 *)(bias_next + cbase + 8 * g + 4 * h);
        *(float4 *)(o + 8 * g) = make_float4(acc[4 * g] + b4.x, acc[4 * g + 1] + b4.y, acc[4 * g + 2] + b4.z, acc[4 * g + 3] + b4.w);
    }
}

// ---- EdgeConv edge pass (backward): g = dY * s_c where the winning edge was active;  dP[i][c] = g,
// dQ[nbr(i,k*)][c] += g.  dpq must be zeroed (Q half) before the launch.
__global__ void edge_max_bwd_kernel(const float *__restrict__ dy, int ld_dy, const int32_t *__restrict__ nbr,
                                    const uint8_t *__restrict__ arg, const float *__restrict__ scale,
                                    float *__restrict__ dpq, int N, size_t total, float *__restrict__ zero_q = nullptr)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % GC);
    const size_t v = t / GC;
    const uint8_t a = arg[t];
    float g = 0.0f;
    if (a & 0x80) g = dy[v * ld_dy + c] * scale[c];
    dpq[v * 2 * GC + c] = g;
    if (zero_q) zero_q[v * 2 * GC + GC + c] = 0.0f;     // the Q half of the NEXT launch's buffer (ping-pong: no memset per block)
    if (g != 0.0f) {
        const size_t j = (v / N) * N + nbr[v * KNB + (a & 0x7F)];
        atomicAdd(dpq + j * 2 * GC + GC + c, g);
    }
}

// ---- The same pass WITHOUT atomics (round 4; default): the transpose of the neighbour gather as a gather through the
// inverse graph, built on the fly, in ONE launch.  A workgroup owns 64 destination vertices j of one room.
// (1) Its 16 waves scan the room's N x 16 edge table once (256 KB from L2, all 16 loads of a thread in flight together) and
//     mark every edge v -> j that lands in the range in an LDS bitmap [64][N bits] (LDS atomicOr: the result does not
//     depend on the order).
// (2) Popcounts + DPP wave scans turn the bitmap rows into ONE flat list of source vertices, destination-major, ascending
//     v per destination (the in-edges of the 64 destinations: ~1024 entries), staged in LDS.
// (3) The flat list is cut into 64 EQUAL slices, one per quarter-wave (16 lanes x 4 channels) - in-degrees of a kNN graph
//     are heavy-tailed (median 15, maximum 77 in the network's graphs), and a quarter that walks one whole list waits for
//     the longest.  Per edge v -> j a lane loads v's neighbour entry `ql` (a ballot over the quarter gives j's slot in v's
//     row), the four arg bytes and the four output gradients of its channels, and adds dY * s_c where the arg byte names
//     that slot as the active winner: four edges per instruction, no per-edge records in memory.  A slice that crosses a
//     destination boundary closes a PIECE (partial row in LDS) and goes on with the next destination.
// (4) Quarter d adds the pieces of destination d in slice order and writes the dQ row; the dP row (the vertex's own term)
//     is written by the same lanes.
// What bounds this pass is instruction issue and dependent-instruction latency of the walking waves, not bandwidth
// (tools/edge_bwd_probe.py with the stamp build: a ds_bpermute scan instead of the DPP one alone cost 12k cycles per wave;
// one edge per wave-instruction with scalar addressing 250 cycles per edge) - hence few, wide, independent instructions per
// edge (raw buffer loads: one 32-bit offset per row instead of 64-bit address arithmetic) and equal work per wave.
// One writer per row and a summation order that depends on the graph only (ascending v inside a piece, pieces in order):
// no memset, no float atomics, and the ResGCN input gradient is bit-reproducible run to run.  Lists of any length are
// served: more than EBG_CAP in-edges per workgroup run as several passes over the flat list.
#ifndef EBG_UNROLL_N
#define EBG_UNROLL_N 4
#endif
constexpr int EBG_D = 64, EBG_T = 1024, EBG_WORDS = 128, EBG_CAP = 8192, EBG_UNROLL = EBG_UNROLL_N, EBG_Q = EBG_D / (EBG_T / 64);
static_assert(EBG_Q == 4, "a wave owns four bitmap rows and has four quarters");

// inclusive scan over the 64 lanes on the DPP network (row_shr 1 / 2 / 4 / 8, then row_bcast15 / row_bcast31), no LDS
__device__ __forceinline__ unsigned wave_incl_scan_u32(unsigned v)
{
    v += dpp_get<0x111, 0xF>(v);
    v += dpp_get<0x112, 0xF>(v);
    v += dpp_get<0x114, 0xF>(v);
    v += dpp_get<0x118, 0xF>(v);
    v += dpp_get<0x142, 0xA>(v);
    v += dpp_get<0x143, 0xC>(v);
    return v;
}

#ifdef EBG_STAMP   // diagnostic variant (tools/build_variant.sh): s_memtime at the phase boundaries of every wave
__device__ unsigned long long ebg_stamps[256 * 16 * 8];
#define EBG_MARK(k) do { if (lane == 0 && blockIdx.x < 256) ebg_stamps[(blockIdx.x * 16 + wave) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define EBG_MARK(k) do { } while (0)
#endif

__device__ __forceinline__ __amdgpu_buffer_rsrc_t ebg_rsrc(const void *p, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, (int)bytes, 0x00020000);   // raw buffer: offsets past `bytes` read 0
}

__global__ __launch_bounds__(EBG_T) void edge_max_bwd_gather_kernel(const float *__restrict__ dy, int ld_dy,
                                                                     const int32_t *__restrict__ nbr,
                                                                     const uint8_t *__restrict__ arg,
                                                                     const float *__restrict__ scale, float *__restrict__ dpq,
                                                                     int N, int chunks)
{
    __shared__ unsigned s_bm[EBG_D * EBG_WORDS];
    __shared__ unsigned short s_stage[EBG_CAP];                  // the flat list (one pass of it): source vertices
    __shared__ float s_part[2 * EBG_D][GC];                      // piece (destination d, slice k) -> row d + k
    __shared__ int s_cnt[EBG_D], s_offend[EBG_D + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    if ((gridDim.x & 7) == 0) b = (b & 7) * (gridDim.x >> 3) + (b >> 3);   // an XCD serves consecutive chunks: one room's tables per L2
    const int room = b / chunks, j0 = (b % chunks) * EBG_D;
    const size_t rb = (size_t)room * N;
    const int quarter = lane >> 4, ql = lane & 15, qw = EBG_Q * wave + quarter;   // qw: this quarter-wave, 0..63
    // one room's tables as raw buffers; this lane's piece of a row: neighbour entry ql / arg bytes and gradients 4 ql .. 4 ql + 3
    const __amdgpu_buffer_rsrc_t r_nb = ebg_rsrc(nbr + rb * KNB, (size_t)N * KNB * 4);
    const __amdgpu_buffer_rsrc_t r_arg = ebg_rsrc(arg + rb * GC, (size_t)N * GC);
    const __amdgpu_buffer_rsrc_t r_dy = ebg_rsrc(dy + rb * ld_dy, (size_t)N * ld_dy * 4);
    const unsigned ld_bytes = (unsigned)ld_dy * 4u;
    const float4 sc = *(const float4 *)(scale + 4 * ql);
    const int shift = 16 * quarter;
    EBG_MARK(0);
    for (int i = tid; i < EBG_D * EBG_WORDS / 4; i += EBG_T) ((uint4 *)s_bm)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    {
        const int4 *nb4 = (const int4 *)(nbr + rb * KNB);
        const int n4 = N * (KNB / 4);
        for (int base = tid; base < n4; base += 16 * EBG_T) {
            int4 q[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int i = base + u * EBG_T;
                q[u] = nb4[i < n4 ? i : base];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int i = base + u * EBG_T;
                if (i < n4) {
                    const int v = i >> 2;
                    const unsigned bit = 1u << (v & 31);
                    // word of destination x = s_bm + (x - j0) * 128 + (v >> 5): one shift-add per entry on a per-load base
                    unsigned *wbase = s_bm + (v >> 5) - j0 * EBG_WORDS;
                    if ((unsigned)(q[u].x - j0) < (unsigned)EBG_D) atomicOr(wbase + q[u].x * EBG_WORDS, bit);
                    if ((unsigned)(q[u].y - j0) < (unsigned)EBG_D) atomicOr(wbase + q[u].y * EBG_WORDS, bit);
                    if ((unsigned)(q[u].z - j0) < (unsigned)EBG_D) atomicOr(wbase + q[u].z * EBG_WORDS, bit);
                    if ((unsigned)(q[u].w - j0) < (unsigned)EBG_D) atomicOr(wbase + q[u].w * EBG_WORDS, bit);
                }
            }
        }
    }
    EBG_MARK(1);
    __syncthreads();
    EBG_MARK(2);
    // the vertex's own term (quarter-wave qw <-> vertex j0 + qw): dP[j][c] = dY[j][c] * s_c where the winning edge was active
    const int jq = j0 + qw;
    unsigned a_self = 0u;
    float4 y_self = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jq < N) {
        a_self = __builtin_amdgcn_raw_buffer_load_b32(r_arg, (unsigned)jq * (unsigned)GC + 4u * ql, 0, 0);
        y_self = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r_dy, (unsigned)jq * ld_bytes + 16u * ql, 0, 0));
    }
    // list lengths of the wave's four bitmap rows (two DPP scans of two 16-bit counts each: a list has at most N <= 4096
    // entries); per lane the rank of its first bit in each row
    uint2 w2[EBG_Q];
    unsigned first[EBG_Q];
    {
        unsigned cnt[EBG_Q];
#pragma unroll
        for (int q = 0; q < EBG_Q; ++q) {
            w2[q] = *(const uint2 *)&s_bm[(EBG_Q * wave + q) * EBG_WORDS + 2 * lane];
            cnt[q] = __popc(w2[q].x) + __popc(w2[q].y);
        }
        const unsigned inc01 = wave_incl_scan_u32(cnt[0] | cnt[1] << 16), inc23 = wave_incl_scan_u32(cnt[2] | cnt[3] << 16);
#pragma unroll
        for (int q = 0; q < EBG_Q; ++q) {
            const unsigned inc = ((q < 2 ? inc01 : inc23) >> (16 * (q & 1))) & 0xFFFFu;
            first[q] = inc - cnt[q];
            if (lane == 63) s_cnt[EBG_Q * wave + q] = (int)inc;
        }
    }
    __syncthreads();
    // flat offsets: lane d holds the rank where destination d's list ends (every wave computes them for itself)
    const int offend = (int)wave_incl_scan_u32((unsigned)s_cnt[lane]);
    const int total = __builtin_amdgcn_readlane(offend, 63);
    if (wave == 0) { s_offend[lane] = offend; if (lane == 0) s_offend[EBG_D] = 0x7FFFFFFF; }
    int base_q[EBG_Q];                                           // flat rank where the wave's q-th row starts
#pragma unroll
    for (int q = 0; q < EBG_Q; ++q)
        base_q[q] = EBG_Q * wave + q == 0 ? 0 : __builtin_amdgcn_readlane(offend, (EBG_Q * wave + q + 63) & 63);
    EBG_MARK(3);
    float accd[4] = {0.0f, 0.0f, 0.0f, 0.0f};                    // dQ[j0 + qw][4 ql ..], summed over pieces (and passes)
    for (int c0 = 0; c0 < total; c0 += EBG_CAP) {
        const int cend = total - c0 < EBG_CAP ? total : c0 + EBG_CAP;
        const int S = (cend - c0 + EBG_D - 1) / EBG_D;           // slice length of this pass
        // ---- stage the pass's part of the flat list
#pragma unroll
        for (int q = 0; q < EBG_Q; ++q) {
            unsigned long long bits = ((unsigned long long)w2[q].y << 32) | w2[q].x;
            int r = base_q[q] + (int)first[q] - c0;
            while (bits) {
                if ((unsigned)r < (unsigned)EBG_CAP) s_stage[r] = (unsigned short)(64 * lane + __ffsll(bits) - 1);
                ++r;
                bits &= bits - 1;
            }
        }
        __syncthreads();
        EBG_MARK(4);
        // ---- walk this quarter-wave's slice [e, eend)
        {
            int e = c0 + qw * S;
            const int eend = e + S < cend ? e + S : cend;
            const bool any = e < eend;
            // the destination that holds rank e: the number of lists that end at or before it
            int d = 0;
#pragma unroll
            for (int q = 0; q < EBG_Q; ++q) {
                const int x = c0 + (EBG_Q * wave + q) * S;
                const int dq = __popcll(__ballot(offend <= x));
                d = quarter == q ? dq : d;
            }
            d = d < EBG_D ? d : EBG_D - 1;
            int rend = any ? s_offend[d] : 0x7FFFFFFF;
            int j = j0 + d;
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int i0 = 0; i0 < S; i0 += EBG_UNROLL) {
                float4 y[EBG_UNROLL];
                unsigned a[EBG_UNROLL];
                int nb[EBG_UNROLL];
#pragma unroll
                for (int u = 0; u < EBG_UNROLL; ++u) {
                    const int ee = e + u;
                    const int ec = ee < eend ? ee : (any ? eend - 1 : c0);   // past the end: a staged entry again, masked below
                    const unsigned v = s_stage[ec - c0];
                    const unsigned o = v * (unsigned)GC + 4u * ql;       // a neighbour row and an arg row are both 64 bytes
                    nb[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(r_nb, o, 0, 0);
                    a[u] = __builtin_amdgcn_raw_buffer_load_b32(r_arg, o, 0, 0);
                    y[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r_dy, v * ld_bytes + 16u * ql, 0, 0));
                }
#pragma unroll
                for (int u = 0; u < EBG_UNROLL; ++u) {
                    const int ee = e + u;
                    if (ee < eend && ee >= rend) {                      // the slice crosses into the next destination(s): close the piece
                        *(float4 *)&s_part[d + qw][4 * ql] = make_float4(acc[0], acc[1], acc[2], acc[3]);
                        acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
                        do { ++d; rend = s_offend[d]; } while (rend <= ee);
                        j = j0 + d;
                    }
                    const int jm = ee < eend ? j : -2;                  // (a neighbour index is >= 0)
                    const unsigned mq = (unsigned)(__ballot(nb[u] == jm) >> shift) & 0xFFFFu;
                    const unsigned key = 0x80u | (mq ? (unsigned)__ffs(mq) - 1u : 0x7Fu);   // j's (first) slot in v's row; none: no byte matches
                    acc[0] += (a[u] & 0xFFu) == key ? y[u].x * sc.x : 0.0f;
                    acc[1] += ((a[u] >> 8) & 0xFFu) == key ? y[u].y * sc.y : 0.0f;
                    acc[2] += ((a[u] >> 16) & 0xFFu) == key ? y[u].z * sc.z : 0.0f;
                    acc[3] += (a[u] >> 24) == key ? y[u].w * sc.w : 0.0f;
                }
                e += EBG_UNROLL;
            }
            if (any) *(float4 *)&s_part[d + qw][4 * ql] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
        EBG_MARK(5);
        __syncthreads();
        // ---- destination qw: its pieces of this pass, in slice order
        {
            const int my_lo = qw == 0 ? 0 : s_offend[qw - 1], my_hi = s_offend[qw];   // destination qw's flat range
            const int lo = my_lo > c0 ? my_lo : c0, hi = my_hi < cend ? my_hi : cend;
            if (lo < hi) {
                const int k2 = (hi - 1 - c0) / S;
                for (int k = (lo - c0) / S; k <= k2; ++k) {
                    const float4 p = *(const float4 *)&s_part[qw + k][4 * ql];
                    accd[0] += p.x; accd[1] += p.y; accd[2] += p.z; accd[3] += p.w;
                }
            }
        }
        if (cend < total) __syncthreads();                       // (another pass re-uses the stage and the piece rows)
    }
#ifdef EBG_STAMP
    if (lane == 0 && blockIdx.x < 256) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        ebg_stamps[(blockIdx.x * 16 + wave) * 8 + 6] = ((unsigned long long)xcc << 32) | hw;
        ebg_stamps[(blockIdx.x * 16 + wave) * 8 + 7] = (unsigned long long)total;
    }
#endif
    if (jq < N) {
        float *row = dpq + (rb + jq) * 2 * GC + 4 * ql;
        *(float4 *)row = make_float4((a_self & 0x80u) ? y_self.x * sc.x : 0.0f, (a_self & 0x8000u) ? y_self.y * sc.y : 0.0f,
                                     (a_self & 0x800000u) ? y_self.z * sc.z : 0.0f, (a_self & 0x80000000u) ? y_self.w * sc.w : 0.0f);
        *(float4 *)(row + GC) = make_float4(accd[0], accd[1], accd[2], accd[3]);
    }
}

#ifdef EBG_STAMP
extern "C" int psg_debug_ebg_stamps(unsigned long long *host, int n_words)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(ebg_stamps), (size_t)n_words * 8) == hipSuccess ? 0 : -2;
}
#endif

// [dP | dQ] of one EdgeConv max pass: the gather kernel above (N <= 4096, any number of rooms, ld_dy a multiple of 4), or
// the atomic scatter (larger rooms, or PSG_GCN_EDGE_BWD=atomic for A/B runs: it needs dpq's Q half zeroed, done here).
int launch_edge_max_bwd(const float *dy, int ld_dy, const int32_t *nbr, const uint8_t *arg, const float *scale, float *dpq,
                        int N, size_t R, hipStream_t st)
{
    static const bool atomic = []() { const char *v = psg::env_str("PSG_GCN_EDGE_BWD"); return v && std::string(v) == "atomic"; }();
    if (!atomic && N <= 32 * EBG_WORDS && ld_dy % 4 == 0 && ((uintptr_t)dy & 15) == 0) {
        const int chunks = ceil_div(N, EBG_D);
        hipLaunchKernelGGL(edge_max_bwd_gather_kernel, dim3((unsigned)((R / N) * chunks)), dim3(EBG_T), 0, st, dy, ld_dy, nbr, arg,
                           scale, dpq, N, chunks);
        PSG_LAUNCH_CHECK();
    } else {
        PSG_CHECK_HIP(hipMemsetAsync(dpq, 0, R * 2 * GC * 4, st));
        hipLaunchKernelGGL(edge_max_bwd_kernel, dim3(ceil_div((int)(R * GC), 256)), dim3(256), 0, st, dy, ld_dy, nbr, arg, scale, dpq,
                           N, R * GC, (float *)nullptr);
        PSG_LAUNCH_CHECK();
    }
    return PSG_OK;
}

__global__ void add_slice_kernel(float *__restrict__ g, const float *__restrict__ src, int ld_src, size_t rows)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < rows * GC) g[t] += src[(t / GC) * ld_src + (t % GC)];
}

// ---- global max over the N points of a room, per channel (torch.max_pool2d over [N,1], architecture.py:64).
// Row chunks reduce in parallel into one 64-bit atomicMax per (room, channel): key = ordered value bits << 32 |
// ~row, so the maximum value wins and equal values resolve to the lowest row.  `keys` must be zeroed.
__global__ __launch_bounds__(256) void colmax_partial_kernel(const float *__restrict__ x, int N, int C, int rows_per_chunk,
                                                             unsigned long long *__restrict__ keys)
{
    const int cc = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cc;
    const size_t room = blockIdx.z;
    const int r0 = blockIdx.y * rows_per_chunk, r1 = min(N, r0 + rows_per_chunk);
    unsigned long long best = 0ull;
    for (int i = r0 + part; i < r1; i += 4) {
        unsigned u = __float_as_uint(x[(room * N + i) * C + c]);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        const unsigned long long key = ((unsigned long long)u << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)i);
        best = key > best ? key : best;
    }
    atomicMax(keys + room * C + c, best);
}

__global__ void colmax_decode_kernel(const unsigned long long *__restrict__ keys, size_t n, float *__restrict__ mx,
                                     int32_t *__restrict__ arg)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned long long key = keys[t];
    unsigned u = (unsigned)(key >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    mx[t] = __uint_as_float(u);
    arg[t] = (int32_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
}

// out[room][m] = sum_k w[m][k] * v[room][k]   (small mat-vec; one wave per output, lanes stride over k: coalesced)
__global__ __launch_bounds__(256) void matvec_kernel(const float *__restrict__ w, int ld_w, const float *__restrict__ v, int K,
                                                     int M, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t room = blockIdx.y;
    if (m >= M) return;
    float acc = 0.0f;
    for (int k = lane; k < K; k += 64) acc += w[(size_t)m * ld_w + k] * v[room * K + k];
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[room * M + m] = acc;
}

// column sums over the N rows of each room: out[room][c] = sum_i x[room*N+i][c]; row chunks in parallel, every chunk's
// partial sums written to part[room][chunk][c], added up in chunk order by colsum_finish_kernel (round 5: rounds 1-4 added
// the chunks with float atomics, the last order-dependent sum of the ResGCN input gradient).
__global__ __launch_bounds__(256) void colsum_kernel(const float *__restrict__ x, int N, int C, int rows_per_chunk,
                                                     float *__restrict__ part)
{
    __shared__ float s_v[4][64];
    const int cc = threadIdx.x & 63, prt = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cc;
    const size_t room = blockIdx.z;
    const int r0 = blockIdx.y * rows_per_chunk, r1 = min(N, r0 + rows_per_chunk);
    float acc = 0.0f;
    for (int i = r0 + prt; i < r1; i += 4) acc += x[(room * N + i) * C + c];
    s_v[prt][cc] = acc;
    __syncthreads();
    if (prt == 0) part[(room * gridDim.y + blockIdx.y) * C + c] = ((s_v[0][cc] + s_v[1][cc]) + s_v[2][cc]) + s_v[3][cc];
}
__global__ void colsum_finish_kernel(const float *__restrict__ part, int chunks, int C, size_t total, float *__restrict__ out)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       // (room, channel)
    if (t >= total) return;
    const size_t room = t / C;
    const int c = (int)(t - room * C);
    float acc = 0.0f;
    for (int k = 0; k < chunks; ++k) acc += part[(room * chunks + k) * C + c];
    out[t] = acc;
}

// fusion backward: dfeats[argmax point of channel c][:] += gvec[c] * s_c[active] * Wf[c][:]
__global__ void fusion_bwd_kernel(const float *__restrict__ gvec, const int32_t *__restrict__ arg,
                                  const uint32_t *__restrict__ mask, const float *__restrict__ scale,
                                  const float *__restrict__ wf, int Cin, int Cout, int N, float *__restrict__ dfeats)
{
    // grid (Cout, rooms), block 256 threads over the Cin input channels.  Several channels can have their maximum at the same
    // point; rounds 1-4 let every channel's block add its row with float atomics.  Round 5: the block of the LOWEST channel
    // of a point is the point's only writer - it adds the rows of all the point's channels in ascending channel order and
    // stores once; the other blocks leave.  Fixed order, no atomics: the ResGCN input gradient is bit-reproducible.
    __shared__ int s_arg[1024];
    const int c = blockIdx.x;
    const size_t room = blockIdx.y;
    for (int t = threadIdx.x; t < Cout; t += blockDim.x) s_arg[t] = arg[room * Cout + t];
    __syncthreads();
    const int i = s_arg[c];
    int earlier = 0;
    for (int t = threadIdx.x; t < c; t += blockDim.x) earlier |= s_arg[t] == i;
    if (__syncthreads_or(earlier)) return;
    const size_t row = room * N + i;
    // the point's channels, ascending: wave 0 scans the table 64 channels at a time (ballot order = channel order)
    __shared__ int s_list[1024];
    __shared__ int s_n;
    if (threadIdx.x < 64) {
        int n = 0;
        for (int c0 = c & ~63; c0 < Cout; c0 += 64) {
            const int cc = c0 + (int)threadIdx.x;
            const bool hit = cc >= c && s_arg[cc] == i;
            const unsigned long long bl = __ballot(hit);
            if (hit) s_list[n + __popcll(bl & ((1ull << threadIdx.x) - 1ull))] = cc;
            n += __popcll(bl);
        }
        if (threadIdx.x == 0) s_n = n;
    }
    __syncthreads();
    const int n_list = s_n;
    // the channels' factors first, all at once (a hub point can be the maximum of hundreds of channels: computed inside the
    // accumulation loop, each was a dependent chain of three global loads in front of the row it scales - 305 us per launch)
    __shared__ float s_g[1024];
    for (int q = threadIdx.x; q < n_list; q += blockDim.x) {
        const int cc = s_list[q];
        const bool act = (mask[row * (Cout / 32) + (cc >> 5)] >> (cc & 31)) & 1u;
        s_g[q] = act ? gvec[room * Cout + cc] * scale[cc] : 0.0f;
    }
    __syncthreads();
    // one input channel per thread, blockIdx.z = the 256-channel slice: the point's only writer is a ROW of blocks, so that a
    // hub's few hundred rows are streamed by Cin / 256 blocks side by side
    const int k = threadIdx.x + 256 * blockIdx.z;
    if (k >= Cin) return;
    float acc = 0.0f;
#pragma unroll 8
    for (int q = 0; q < n_list; ++q) {
        const float g = s_g[q];
        acc += g * wf[(size_t)s_list[q] * Cin + k];         // (g = 0 for a channel whose ReLU was off: adds +-0)
    }
    dfeats[row * Cin + k] += acc;
}

__global__ void scale_rows_kernel(const float *__restrict__ w, int M, int K, const float *__restrict__ s_by_k,
                                  float *__restrict__ out)
{
    // out[m][k] = w[m][k] * s_by_k[k]
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (size_t)M * K) out[t] = w[t] * s_by_k[t % K];
}

// ---- MRConv2d vertex pass (torch_vertex.py:8-20): cat[v] = [x_v | max_k (x_nbr(v,k) - x_v)], first index on ties
// like torch.max; arg = winning k.  One thread per (vertex, channel); C = 9, 64 or a multiple of 64.
__global__ void mr_gather_fwd_kernel(const float *__restrict__ x, int ld, int C, const int32_t *__restrict__ nbr,
                                     float *__restrict__ cat, uint8_t *__restrict__ arg, int N, size_t total)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C);
    const size_t v = t / C;
    const size_t room_base = (v / N) * N;
    const float xv = x[v * ld + c];
    const int32_t *nb = nbr + v * KNB;
    float best = -INFINITY;
    int bk = 0;
#pragma unroll 4
    for (int k = 0; k < KNB; ++k) {
        const float r = x[(room_base + nb[k]) * ld + c] - xv;
        if (r > best) { best = r; bk = k; }
    }
    cat[v * 2 * C + c] = xv;
    cat[v * 2 * C + C + c] = best;
    arg[t] = (uint8_t)bk;
}

// gz[v][o] = dy[v][o] * s_o where the conv output was positive (backward through BatchNorm and ReLU of a BasicConv)
__global__ void mr_dz_kernel(const float *__restrict__ dy, int ld_dy, const uint32_t *__restrict__ mask,
                             const float *__restrict__ scale, float *__restrict__ gz, size_t total)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int o = (int)(t % GC);
    const size_t v = t / GC;
    const bool act = (mask[v * 2 + (o >> 5)] >> (o & 31)) & 1u;
    gz[t] = act ? dy[v * ld_dy + o] * scale[o] : 0.0f;
}

// d cat -> d x, own-vertex part: tgt[v][c] (+)= dcat[v][c] - dcat[v][C + c] (+ extra[v][c]);  `assign` overwrites.
__global__ void mr_bwd_self_kernel(const float *__restrict__ dcat, int C, float *__restrict__ tgt, int ld_t,
                                   const float *__restrict__ extra, int ld_e, int assign, size_t total)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C);
    const size_t v = t / C;
    float g = dcat[v * 2 * C + c] - dcat[v * 2 * C + C + c];
    if (extra) g += extra[v * ld_e + c];
    float *o = tgt + v * ld_t + c;
    *o = assign ? g : *o + g;
}

// neighbour part: tgt[nbr(v, k*)][c] += dcat[v][C + c]  (launched after mr_bwd_self_kernel has finished)
__global__ void mr_bwd_scatter_kernel(const float *__restrict__ dcat, int C, const int32_t *__restrict__ nbr,
                                      const uint8_t *__restrict__ arg, float *__restrict__ tgt, int ld_t, int N, size_t total)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C);
    const size_t v = t / C;
    const float g = dcat[v * 2 * C + C + c];
    if (g != 0.0f) {
        const size_t j = (v / N) * N + nbr[v * KNB + arg[t]];
        atomicAdd(tgt + j * ld_t + c, g);
    }
}

struct EdgeLayer {
    float *wcat;    // [128][C]: rows 0..63 = W1 - W2, rows 64..127 = W2
    float *bcat;    // [128] = [b, 0]
    float *wcat_t;  // [C][128] (transpose, for the input gradient)
    float *wcat_k8 = nullptr;   // C == 64: wcat as MFMA operand blocks [k / 8][128][8] (edge_max_pq_fwd_kernel)
    float *scale, *shift;  // eval BatchNorm after the ReLU
    float *w = nullptr, *b = nullptr;   // conv = mr: plain [64][2C] weight and [64] bias of the BasicConv
    float *w_t = nullptr;               // conv = mr: [2C][64] transpose (input gradient)
    int C;
    size_t arg_off = 0;                 // conv = mr: offset of this layer's arg-max bytes per vertex block (sum of C before it)
};

}  // namespace

struct psg_gcn_model {
    uint64_t gen = psg::next_generation();   // never re-used (psg_common.h): what the replayed NB iteration is keyed on
    psg_ctx *ctx;
    int n_blocks;
    int block = PSG_GCN_BLOCK_RES, conv = PSG_GCN_CONV_EDGE;   // architecture.py:26-39, torch_vertex.py:44-49
    size_t arg_total = 0;                 // conv = mr: arg-max bytes per vertex over all layers
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
    std::vector<void *> allocs;
};

struct psg_gcn_ws {
    uint64_t gen = psg::next_generation();   // never re-used: what the replayed NU windows are keyed on (psg_common.h)
    psg_ctx *ctx;
    int B, N, NP2, n_blocks, fdim;
    int block = PSG_GCN_BLOCK_RES, conv = PSG_GCN_CONV_EDGE;
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
    int knn_mode = 2;          // 1 = exact fused kernel only (PSG_GCN_KNN=f32), 2 = bf16 prefilter up to knn_bf_max_d, 0 = round-1 path (=matrix)
    int knn_bf_max_d = 27;     // the prefilter kernel serves dilations up to this (PSG_GCN_KNN_BF_MAXD), the exact kernel the rest
    unsigned long long *knn_stats = nullptr;   // PSG_GCN_KNN_STATS=1: device counters of the prefilter kernel
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
    bool have_fwd = false;
    bool fixed_graphs = false;  // psg_gcn_set_graphs: forward uses the supplied neighbour tables
    bool head_graph_frozen = false;  // inside an attack loop: xyz never changes, the head's xyz kNN graph is kept
    // hipGraph of one interior PGD iteration (forward, CE, backward, step): ~300 short launches replayed as one
    // graph launch; valid for (model, eps, alpha) below, rebuilt when they change
    int32_t *nb_labels;        // [B*N] the attack's labels, copied so that the captured kernels' arguments never change
    psg::GraphSlot nb;
    uint64_t nb_model_gen = 0;       // the model's generation number, not its address (psg_common.h)
    float nb_eps = 0.f, nb_alpha = 0.f;
    bool nb_fixed = false;
    // psg_gcn_nb_attack_field: the clean coordinates, and the hipGraph of one interior iteration of the coordinate-field loop
    // with what it is valid for (a holder of its own: the colour loop's graph above survives a field call and vice versa)
    float *ori_xyz;            // [B*N][3]
    psg::GraphSlot nbf;
    uint64_t nbf_model_gen = 0;
    int nbf_field = 0;
    float nbf_eps = 0.f, nbf_alpha = 0.f, nbf_ceps = 0.f, nbf_calpha = 0.f;
    bool nbf_fixed = false;
    EvLog prof;              // psg_gcn_prof_enable
};

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

__global__ void extract3_kernel(const float *__restrict__ x0, float *__restrict__ xyz, size_t rows)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < rows * 3) xyz[t] = x0[(t / 3) * 9 + (t % 3)];
}

__global__ void extract_color3_kernel(const float *__restrict__ x0, float *__restrict__ ori, size_t rows)
{
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < rows * 3) ori[t] = x0[(t / 3) * 9 + 3 + (t % 3)];
}

enum GcnTag { GT_KNN = 0, GT_KNN_OTHER, GT_VERTEX_GEMM, GT_EDGE_MAX, GT_HEAD, GT_BACKWARD, GT_COUNT };

// which kernel builds the dilated graph of C-wide features: the bf16-prefilter kernel (default), the exact fused kernel
// (PSG_GCN_KNN=f32, and sizes the prefilter does not take), or -1 = the round-1 path (distance matrix in HBM + selection
// kernel: the xyz graph of the head, dense blocks, PSG_GCN_KNN=matrix)
int knn_path(const psg_gcn_ws *ws, int C, int d)
{
    if (ws->knn_mode == 0 || C != 64) return -1;
    if (ws->knn_mode == 2 && d <= ws->knn_bf_max_d && knn_shape_ok(ws->N, KNB, d, KNN_PATH_BF16)) return KNN_PATH_BF16;
    return knn_shape_ok(ws->N, KNB, d, KNN_PATH_F32) ? KNN_PATH_F32 : -1;
}

KnnBuffers knn_buffers(const psg_gcn_ws *ws)
{
    KnnBuffers b;
    b.xp = ws->xp; b.bp = ws->bp; b.sq = ws->sq; b.stats = ws->knn_stats;
    return b;
}

// have_sq: ws->sq (and, on the fused paths, ws->xp / ws->bp) already hold the norms / operand copies of x (the forward
// pass gets them from the producing edge_max_fwd kernel)
int knn_graph(psg_gcn_ws *ws, const float *x, int ld, int C, int d, int32_t *out, hipStream_t st, bool have_sq = false)
{
    const size_t rows = (size_t)ws->B * ws->N;
    const int path = knn_path(ws, C, d);
    if (path >= 0) {
        KnnBuffers buf = knn_buffers(ws);
        buf.x = x; buf.ld = ld;
        if (!have_sq) PSG_CHECK_HIP(knn_prep_launch(x, ld, rows, buf, path == KNN_PATH_BF16, st));
        EvScope prof(&ws->prof, GT_KNN, 2.0 * ws->B * (double)ws->N * ws->N * 64.0, st);
        PSG_CHECK_HIP(knn_launch(buf, ws->B, ws->N, KNB, d, out, (KnnPath)path, st));
        return PSG_OK;
    }
    EvScope prof(&ws->prof, GT_KNN_OTHER, 2.0 * ws->B * (double)ws->N * ws->N * C, st);   // round-1 path, xyz graph
    if (!have_sq) {
        hipLaunchKernelGGL(sumsq_rows_kernel, dim3(ceil_div((int)rows, 256)), dim3(256), 0, st, x, ld, C, rows, ws->sq);
        PSG_LAUNCH_CHECK();
    }
    for (int b = 0; b < ws->B; ++b) {  // distances never cross rooms
        GemmArgs a = gemm_args(x + (size_t)b * ws->N * ld, ld, x + (size_t)b * ws->N * ld, ld,
                               ws->dist + (size_t)b * ws->N * ws->N, ws->N, ws->N, C, ws->N);
        a.sq = ws->sq + (size_t)b * ws->N;
        int rc = launch_gemm<2, 2, EPI_KNN_DIST, true>(a, st);
        if (rc) return rc;
    }
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
    m->ctx = ctx; m->n_blocks = n_blocks; m->fdim = GC * n_blocks;
    m->block = block; m->conv = conv;
    bool ok = true;
    auto dev_upload = [&](const std::vector<float> &h) {
        float *p = upload(m->allocs, h);
        ok = ok && p;
        return p;
    };
    int ti = 0;
    for (int e = 0; e < n_blocks; ++e) {
        const int C = e == 0 ? 9 : (block == PSG_GCN_BLOCK_DENSE ? GC * e : GC);
        const float *W = tensors[ti], *b = tensors[ti + 1];
        std::vector<float> s, t;
        bn_affine(tensors[ti + 2], tensors[ti + 3], tensors[ti + 4], tensors[ti + 5], GC, s, t);
        ti += 6;
        std::vector<float> wcat((size_t)2 * GC * C), wt((size_t)C * 2 * GC), bcat(2 * GC, 0.0f);
        for (int o = 0; o < GC; ++o) {
            bcat[o] = b[o];
            for (int c = 0; c < C; ++c) {
                const float w1 = W[(size_t)o * 2 * C + c], w2 = W[(size_t)o * 2 * C + C + c];
                wcat[(size_t)o * C + c] = w1 - w2;
                wcat[(size_t)(GC + o) * C + c] = w2;
            }
        }
        for (int r = 0; r < 2 * GC; ++r)
            for (int c = 0; c < C; ++c) wt[(size_t)c * 2 * GC + r] = wcat[(size_t)r * C + c];
        EdgeLayer L;
        L.C = C;
        L.wcat = dev_upload(wcat); L.bcat = dev_upload(bcat); L.wcat_t = dev_upload(wt);
        if (C == GC) {
            std::vector<float> wk((size_t)2 * GC * C);
            for (int r = 0; r < 2 * GC; ++r)
                for (int c = 0; c < C; ++c) wk[((size_t)(c >> 3) * 2 * GC + r) * 8 + (c & 7)] = wcat[(size_t)r * C + c];
            L.wcat_k8 = dev_upload(wk);
        }
        L.scale = dev_upload(s); L.shift = dev_upload(t);
        if (conv == PSG_GCN_CONV_MR) {
            std::vector<float> wplain(W, W + (size_t)GC * 2 * C), wtr((size_t)2 * C * GC);
            for (int o = 0; o < GC; ++o)
                for (int k = 0; k < 2 * C; ++k) wtr[(size_t)k * GC + o] = W[(size_t)o * 2 * C + k];
            L.w = dev_upload(wplain); L.w_t = dev_upload(wtr);
            L.b = dev_upload(std::vector<float>(b, b + GC));
            L.arg_off = m->arg_total;
            m->arg_total += (size_t)C;
        }
        m->edge.push_back(L);
    }
    const int F = m->fdim;
    auto up = [&](const float *p, size_t n) { return dev_upload(std::vector<float>(p, p + n)); };
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
    std::vector<float> s, t;
    m->wf = up(fold_dense(tensors[ti], 1024, 0), (size_t)1024 * F); m->bf = up(tensors[ti + 1], 1024);
    bn_affine(tensors[ti + 2], tensors[ti + 3], tensors[ti + 4], tensors[ti + 5], 1024, s, t);
    m->sf = dev_upload(s); m->tf = dev_upload(t); ti += 6;
    const float *W1 = fold_dense(tensors[ti], 512, 1024);
    m->wp1 = up(W1, (size_t)512 * (1024 + F)); m->bp1 = up(tensors[ti + 1], 512);
    std::vector<float> s1v, t1v;
    bn_affine(tensors[ti + 2], tensors[ti + 3], tensors[ti + 4], tensors[ti + 5], 512, s1v, t1v);
    m->s1 = dev_upload(s1v); m->t1 = dev_upload(t1v); ti += 6;
    const float *W2 = tensors[ti];
    m->wp2 = up(W2, (size_t)256 * 512); m->bp2 = up(tensors[ti + 1], 256);
    std::vector<float> s2v, t2v;
    bn_affine(tensors[ti + 2], tensors[ti + 3], tensors[ti + 4], tensors[ti + 5], 256, s2v, t2v);
    m->s2 = dev_upload(s2v); m->t2 = dev_upload(t2v); ti += 6;
    const float *W3 = tensors[ti];
    m->wp3 = up(W3, (size_t)NCLS * 256); m->bp3 = up(tensors[ti + 1], NCLS);
    // transposes for the input-gradient pass, BatchNorm scales folded in
    std::vector<float> w3t((size_t)256 * NCLS), w2st((size_t)512 * 256), w1bst((size_t)F * 512), w1ast((size_t)1024 * 512);
    for (int o = 0; o < NCLS; ++o)
        for (int k = 0; k < 256; ++k) w3t[(size_t)k * NCLS + o] = W3[(size_t)o * 256 + k];
    for (int o = 0; o < 256; ++o)
        for (int k = 0; k < 512; ++k) w2st[(size_t)k * 256 + o] = W2[(size_t)o * 512 + k] * s2v[o];
    for (int o = 0; o < 512; ++o) {
        for (int k = 0; k < F; ++k) w1bst[(size_t)k * 512 + o] = W1[(size_t)o * (1024 + F) + 1024 + k] * s1v[o];
        for (int k = 0; k < 1024; ++k) w1ast[(size_t)k * 512 + o] = W1[(size_t)o * (1024 + F) + k] * s1v[o];
    }
    m->wp3_t = dev_upload(w3t); m->wp2_st = dev_upload(w2st); m->wp1b_st = dev_upload(w1bst);
    m->wp1a_st = dev_upload(w1ast);
    if (!ok) {
        psg_gcn_model_destroy(m);
        set_error("psg_gcn_model_create: device allocation or upload failed");
        return PSG_ERR_HIP;
    }
    *out = m;
    return PSG_OK;
}

extern "C" int psg_gcn_model_create(psg_ctx *ctx, const float *const *tensors, int n_tensors, int n_blocks,
                                    psg_gcn_model **out)
{
    return psg_gcn_model_create_cfg(ctx, tensors, n_tensors, n_blocks, PSG_GCN_BLOCK_RES, PSG_GCN_CONV_EDGE, out);
}

extern "C" int psg_gcn_model_destroy(psg_gcn_model *m)
{
    if (!m) return PSG_OK;
    for (void *p : m->allocs) (void)hipFree(p);
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
    ws->ctx = ctx; ws->B = batch; ws->N = n_point; ws->n_blocks = n_blocks; ws->fdim = GC * n_blocks;
    ws->block = block; ws->conv = conv;
    {
        const char *kv = psg::env_str("PSG_GCN_KNN");
        const std::string mode = kv ? kv : "";
        // default: the bf16-prefilter kernel for every dilation of the network (1..27): since round 6 (2048-bin final ranking,
        // DESIGN.md section 2) it is the faster one on the network's own features up to d = 27 (148-153 us against 178-184 us
        // per 4-room call at d = 21..27, no tile on the exact path; rounds 4-5 split at 20, where rows of more than 256
        // finalists started to fall back); the exact fused kernel stays as the in-launch fallback and for PSG_GCN_KNN=f32; both
        // give the same graph bit for bit.  PSG_GCN_KNN=f32 / =bf16 force one kernel for every dilation, =matrix the round-1 path
        ws->knn_mode = mode == "matrix" ? 0 : (mode == "f32" ? 1 : 2);
        ws->knn_bf_max_d = mode == "bf16" ? 1 << 30 : 27;
        if (const char *md = psg::env_str("PSG_GCN_KNN_BF_MAXD")) ws->knn_bf_max_d = atoi(md);
        // the fused kNN kernels need 129 KB of dynamic LDS (raised once, outside any stream capture); a device that does
        // not grant it keeps the round-1 path (distance matrix in HBM + selection kernel)
        if (ws->knn_mode && knn_setup() != hipSuccess) { (void)hipGetLastError(); ws->knn_mode = 0; }
    }
    // widest conv input (dense: all earlier outputs) and the total arg-max bytes per vertex of the mr layers
    const int c_max = block == PSG_GCN_BLOCK_DENSE ? std::max(GC, GC * (n_blocks - 1)) : GC;
    size_t arg_total = 9;
    for (int e = 1; e < n_blocks; ++e) arg_total += block == PSG_GCN_BLOCK_DENSE ? (size_t)GC * e : (size_t)GC;
    ws->pq_w = conv == PSG_GCN_CONV_MR ? std::max(128, 2 * c_max) : 128;
    ws->NP2 = 1;
    while (ws->NP2 < n_point) ws->NP2 <<= 1;
    const size_t R = (size_t)batch * n_point;
    auto layout = [&](Bump &bp) {
        ws->feats = bp.take<float>(R * ws->fdim);
        ws->dfeats = bp.take<float>(R * ws->fdim);
        ws->dist = bp.take<float>(R * n_point);
        ws->sq = bp.take<float>(R);
        ws->xp = (float *)bp.take<char>(knn_xp_bytes(R));
        ws->bp = bp.take<char>(knn_bp_bytes(R));
        ws->knn_stats = psg::env_str("PSG_GCN_KNN_STATS") ? bp.take<unsigned long long>(8) : nullptr;
        ws->pq = bp.take<float>(R * ws->pq_w);
        ws->pq2 = bp.take<float>(R * 2 * GC);
        ws->dpq = bp.take<float>(R * ws->pq_w);
        ws->dpq2 = bp.take<float>(R * 2 * GC);
        if (conv == PSG_GCN_CONV_MR) {
            ws->arg_mr = bp.take<uint8_t>(R * arg_total);
            ws->mask_mr = bp.take<uint32_t>((size_t)n_blocks * R * 2);
        }
        ws->nbr = bp.take<int32_t>((size_t)n_blocks * R * KNB);
        ws->arg = bp.take<uint8_t>((size_t)n_blocks * R * GC);
        ws->fused = bp.take<float>(R * 1024);
        ws->mask_f = bp.take<uint32_t>(R * 32);
        ws->mask1 = bp.take<uint32_t>(R * 16);
        ws->mask2 = bp.take<uint32_t>(R * 8);
        ws->fmax = bp.take<float>((size_t)batch * 1024);
        ws->farg = bp.take<int32_t>((size_t)batch * 1024);
        ws->fkeys = bp.take<unsigned long long>((size_t)batch * 1024);
        ws->gb1 = bp.take<float>((size_t)batch * 512);
        ws->h1 = bp.take<float>(R * 512);
        ws->h2 = bp.take<float>(R * 256);
        ws->g2 = bp.take<float>(R * 256);
        ws->g1 = bp.take<float>(R * 512);
        ws->g1sum = bp.take<float>((size_t)batch * 512);
        ws->g1part = bp.take<float>((size_t)batch * ceil_div(n_point, 64) * 512);
        ws->gfvec = bp.take<float>((size_t)batch * 1024);
        ws->gcur = bp.take<float>(R * GC);
        ws->logits = bp.take<float>(R * NCLS);
        ws->dlogits = bp.take<float>(R * NCLS);
        ws->x0 = bp.take<float>(R * 9);
        ws->ori = bp.take<float>(R * 3);
        ws->dx0 = bp.take<float>(R * 9);
        ws->xyz = bp.take<float>(R * 3);
        ws->nb_labels = bp.take<int32_t>(R);
        ws->ori_xyz = bp.take<float>(R * 3);
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
    ws->nb.destroy();
    ws->nbf.destroy();
    if (ws->arena) (void)hipFree(ws->arena);
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
    if (!ws || block < 0 || block >= ws->n_blocks) return nullptr;
    return ws->nbr + (size_t)block * ws->B * ws->N * KNB;
}

extern "C" int psg_gcn_set_graphs(psg_gcn_ws *ws, const int32_t *nbr, psg_stream stream)
{
    PSG_REQUIRE(ws, "psg_gcn_set_graphs: null workspace");
    if (!nbr) { ws->fixed_graphs = false; return PSG_OK; }
    PSG_CHECK_HIP(hipMemcpyAsync(ws->nbr, nbr, (size_t)ws->n_blocks * ws->B * ws->N * KNB * 4, hipMemcpyDeviceToDevice,
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

// pairwise_distance, torch_edge.py:32-42: x [B][N][C] -> out [B][N][N] = (|x_i|^2 + (-2 x_i.x_j)) + |x_j|^2 with the
// reference's fp32 order (norms in torch.sum's order, dot products as the ascending-k fmaf chain); sq: scratch [B*N]
extern "C" int psg_gcn_pairwise_distance(const float *x, int B, int N, int C, float *sq, float *out, psg_stream stream)
{
    PSG_REQUIRE(x && sq && out && B > 0 && N > 0 && C > 0, "psg_gcn_pairwise_distance: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)B * N;
    hipLaunchKernelGGL(sumsq_rows_kernel, dim3(ceil_div((int)rows, 256)), dim3(256), 0, st, x, C, C, rows, sq);
    PSG_LAUNCH_CHECK();
    for (int b = 0; b < B; ++b) {
        GemmArgs a = gemm_args(x + (size_t)b * N * C, C, x + (size_t)b * N * C, C, out + (size_t)b * N * N, N, N, C, N);
        a.sq = sq + (size_t)b * N;
        int rc = launch_gemm<2, 2, EPI_KNN_DIST, true>(a, st);
        if (rc) return rc;
    }
    return PSG_OK;
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
extern "C" int psg_gcn_forward(psg_gcn_model *m, psg_gcn_ws *ws, const float *x0, float *logits_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && x0 && logits_out, "psg_gcn_forward: null argument");
    PSG_REQUIRE(m->n_blocks == ws->n_blocks && m->block == ws->block && m->conv == ws->conv,
                "psg_gcn_forward: model / workspace configuration mismatch");
    hipStream_t st = (hipStream_t)stream;
    const int B = ws->B, N = ws->N, F = ws->fdim;
    const size_t R = (size_t)B * N;
    const int g256 = ceil_div((int)(R * GC), 256);
    int rc;
    hipLaunchKernelGGL(extract3_kernel, dim3(ceil_div((int)(R * 3), 256)), dim3(256), 0, st, x0, ws->xyz, R);
    PSG_LAUNCH_CHECK();
    const bool dense = m->block == PSG_GCN_BLOCK_DENSE, res = m->block == PSG_GCN_BLOCK_RES, mr = m->conv == PSG_GCN_CONV_MR;
    // PSG_GCN_PQ_FUSION=1: a block's edge pass also computes the next block's per-vertex product (edge_max_pq_fwd_kernel).
    // Measured on MI355X: 0.21 ms less kernel time per 4-room iteration (8.09 -> 7.89) and +2 % with one launch in flight
    // (10.18 -> 10.39 rooms/s), but -0.7 % at the bench's three launches in flight (12.05 -> 11.96): the small GEMM launches
    // it removes were running inside the idle slots of another launch's kNN kernel.  Off by default for that reason.
    static const bool fuse_pq = (psg::env_int("PSG_GCN_PQ_FUSION", 0) != 0);
    bool pq_ready = false;     // this block's [P | Q] was written by the previous block's edge pass
    for (int e = 0; e < m->n_blocks; ++e) {
        const EdgeLayer &L = m->edge[e];
        int32_t *nbr = ws->nbr + (size_t)e * R * KNB;
        // input of block e: the previous block's output (res / plain) or all earlier outputs (dense: a prefix of the rows)
        const float *xin = e == 0 ? x0 : (dense ? ws->feats : ws->feats + (size_t)(e - 1) * GC);
        const int ld = e == 0 ? 9 : F;
        // graph: xyz kNN for the head (architecture.py:59); feature-space kNN for block e with dilation e (res, dense:
        // architecture.py:23,28) or 1 (plain, :36).  The norms of a 64-wide EdgeConv output come out of its max kernel.
        const int dil = e == 0 || m->block == PSG_GCN_BLOCK_PLAIN ? 1 : e;
        const bool have_sq = e > 0 && !mr && !dense;
        if (!ws->fixed_graphs && !(e == 0 && ws->head_graph_frozen) &&
            (rc = knn_graph(ws, e == 0 ? ws->xyz : xin, e == 0 ? 3 : ld, e == 0 ? 3 : L.C, dil, nbr, st, have_sq)))
            return rc;
        float *yout = ws->feats + (size_t)e * GC;
        if (!mr) {
            // [P | Q] = x . [W1 - W2 ; W2]^T + [b, 0]: a GEMM launch, unless the previous block's edge pass has produced it
            float *pq_cur = (e & 1) ? ws->pq2 : ws->pq, *pq_nxt = (e & 1) ? ws->pq : ws->pq2;
            if (!pq_ready) {
                GemmArgs a = gemm_args(xin, ld, L.wcat, L.C, pq_cur, 2 * GC, (int)R, L.C, 2 * GC);
                a.bias = L.bcat;
                EvScope prof(&ws->prof, GT_VERTEX_GEMM, 2.0 * R * L.C * 2.0 * GC, st);
                if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
            }
            // the next block's kNN kernel decides which operand copies this kernel writes beside the features
            const int next_path = (!ws->fixed_graphs && !dense && e + 1 < m->n_blocks)
                                      ? knn_path(ws, GC, m->block == PSG_GCN_BLOCK_PLAIN ? 1 : e + 1) : -1;
            // fused with the next block's per-vertex product when that block reads exactly this block's 64 outputs
            const bool fuse_next = fuse_pq && !dense && e + 1 < m->n_blocks && m->edge[e + 1].wcat_k8 && R % EMF_V == 0;
            EvScope prof(&ws->prof, GT_EDGE_MAX, fuse_next ? 2.0 * R * GC * 2.0 * GC : 0.0, st);
            const float *resid = (e == 0 || !res) ? nullptr : xin;
            float *sq_o = (ws->fixed_graphs || dense) ? nullptr : ws->sq;
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
            const size_t tot = R * (size_t)L.C;
            hipLaunchKernelGGL(mr_gather_fwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, xin, ld, L.C, nbr,
                               ws->pq, ws->arg_mr + L.arg_off * R, N, tot);
            PSG_LAUNCH_CHECK();
            GemmArgs a = gemm_args(ws->pq, 2 * L.C, L.w, 2 * L.C, yout, F, (int)R, 2 * L.C, GC);
            a.bias = L.b; a.scale = L.scale; a.shift = L.shift; a.mask_out = ws->mask_mr + (size_t)e * R * 2;
            if (res && e > 0) { a.accumulate = 2; a.addend = xin; a.ld_add = F; }
            if ((rc = launch_gemm<2, 2, EPI_RELU_AFFINE, false>(a, st))) return rc;
        }
    }
    EvScope prof_head(&ws->prof, GT_HEAD, 2.0 * R * ((double)F * 1024 + (double)F * 512 + 512.0 * 256 + 256.0 * NCLS), st);
    // fusion: Conv(F -> 1024) + ReLU + BN, global max over the room
    {
        GemmArgs a = gemm_args(ws->feats, F, m->wf, F, ws->fused, 1024, (int)R, F, 1024);
        a.bias = m->bf; a.scale = m->sf; a.shift = m->tf; a.mask_out = ws->mask_f;
        if ((rc = launch_gemm<2, 2, EPI_RELU_AFFINE, false>(a, st))) return rc;
        PSG_CHECK_HIP(hipMemsetAsync(ws->fkeys, 0, (size_t)B * 1024 * 8, st));
        hipLaunchKernelGGL(colmax_partial_kernel, dim3(1024 / 64, ceil_div(N, 64), B), dim3(256), 0, st, ws->fused, N, 1024, 64,
                           ws->fkeys);
        PSG_LAUNCH_CHECK();
        hipLaunchKernelGGL(colmax_decode_kernel, dim3(ceil_div(B * 1024, 256)), dim3(256), 0, st, ws->fkeys, (size_t)B * 1024,
                           ws->fmax, ws->farg);
        PSG_LAUNCH_CHECK();
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
    const bool dense = m->block == PSG_GCN_BLOCK_DENSE, res = m->block == PSG_GCN_BLOCK_RES, mr = m->conv == PSG_GCN_CONV_MR;
    int rc;
    for (int e = m->n_blocks - 1; e >= 0; --e) {
        const EdgeLayer &L = m->edge[e];
        const float *dy = ws->dfeats + (size_t)e * GC;                       // rows of F floats
        float *tgt = e == 0 ? dx0_out : (dense ? ws->dfeats : ws->dfeats + (size_t)(e - 1) * GC);
        const int ld_t = e == 0 ? 9 : F;
        const int32_t *nbr = ws->nbr + (size_t)e * R * KNB;
        if (!mr) {
            if ((rc = launch_edge_max_bwd(dy, F, nbr, ws->arg + (size_t)e * R * GC, L.scale, ws->dpq, N, R, st))) return rc;
            PSG_LAUNCH_CHECK();
            GemmArgs a = gemm_args(ws->dpq, 2 * GC, L.wcat_t, 2 * GC, tgt, ld_t, (int)R, 2 * GC, L.C);
            if (e > 0) {
                a.accumulate = 1;
                if (res) { a.addend = dy; a.ld_add = F; }
            }
            if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
        } else {
            hipLaunchKernelGGL(mr_dz_kernel, dim3(g256), dim3(256), 0, st, dy, F, ws->mask_mr + (size_t)e * R * 2, L.scale,
                               ws->gcur, R * GC);
            PSG_LAUNCH_CHECK();
            GemmArgs a = gemm_args(ws->gcur, GC, L.w_t, GC, ws->dpq, 2 * L.C, (int)R, GC, 2 * L.C);
            if ((rc = launch_gemm<2, 2, EPI_LINEAR, false>(a, st))) return rc;
            const size_t tot = R * (size_t)L.C;
            const unsigned grid = (unsigned)((tot + 255) / 256);
            hipLaunchKernelGGL(mr_bwd_self_kernel, dim3(grid), dim3(256), 0, st, ws->dpq, L.C, tgt, ld_t,
                               (res && e > 0) ? dy : nullptr, F, e == 0 ? 1 : 0, tot);
            PSG_LAUNCH_CHECK();
            hipLaunchKernelGGL(mr_bwd_scatter_kernel, dim3(grid), dim3(256), 0, st, ws->dpq, L.C, nbr,
                               ws->arg_mr + L.arg_off * R, tgt, ld_t, N, tot);
            PSG_LAUNCH_CHECK();
        }
    }
    return PSG_OK;
}

extern "C" int psg_gcn_backward(psg_gcn_model *m, psg_gcn_ws *ws, const float *dlogits, float *dx0_out,
                                psg_stream stream)
{
    PSG_REQUIRE(m && ws && dlogits && dx0_out, "psg_gcn_backward: null argument");
    if (!ws->have_fwd) { set_error("psg_gcn_backward: no forward is resident in the workspace"); return PSG_ERR_STATE; }
    PSG_REQUIRE(m->n_blocks == ws->n_blocks && m->block == ws->block && m->conv == ws->conv,
                "psg_gcn_backward: model / workspace configuration mismatch");
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
    if (m->block != PSG_GCN_BLOCK_RES || m->conv != PSG_GCN_CONV_EDGE) return backward_alt(m, ws, dx0_out, st);
    // backbone in reverse: G_e = d/d x_e
    PSG_CHECK_HIP(hipMemcpy2DAsync(ws->gcur, GC * 4, ws->dfeats + (size_t)(m->n_blocks - 1) * GC, (size_t)F * 4, GC * 4, R,
                                   hipMemcpyDeviceToDevice, st));
    // [dP | dQ] buffers alternate between two blocks (block e's GEMM may still read its buffer while block e - 1's edge
    // pass writes the other); every row of both halves has exactly one writer in the gather kernel: nothing to zero
    float *pp[2] = {ws->dpq, ws->dpq2};
    for (int e = m->n_blocks - 1; e >= 0; --e) {
        const EdgeLayer &L = m->edge[e];
        float *dpq = pp[e & 1];
        if ((rc = launch_edge_max_bwd(ws->gcur, GC, ws->nbr + (size_t)e * R * KNB, ws->arg + (size_t)e * R * GC, L.scale, dpq, N, R,
                                      st))) return rc;
        if (e > 0) {
            // x_e = EdgeConv_e(x_{e-1}) + x_{e-1}:  G_{e-1} = dfeats[e-1] + G_e + [dP | dQ] . [W1-W2 ; W2]
            // (the residual's gradient slice dfeats[e-1] is added inside the GEMM's accumulate epilogue)
            GemmArgs a = gemm_args(dpq, 2 * GC, L.wcat_t, 2 * GC, ws->gcur, GC, (int)R, 2 * GC, GC);
            a.accumulate = 1;
            a.addend = ws->dfeats + (size_t)(e - 1) * GC;
            a.ld_add = F;
            if ((rc = launch_gemm<4, 1, EPI_LINEAR, false>(a, st))) return rc;
        } else {
            GemmArgs a = gemm_args(dpq, 2 * GC, L.wcat_t, 2 * GC, dx0_out, 9, (int)R, 2 * GC, 9);
            if ((rc = launch_gemm<4, 1, EPI_LINEAR, false>(a, st))) return rc;
        }
    }
    return PSG_OK;
}

// ====================================================================================== NB attack
// The `iters` iterations of an NB attack (psg_gcn_nb_attack, psg_gcn_nb_attack_field).  The first iteration runs eagerly (it
// also sets kernel attributes outside any capture).  The interior iterations 1 .. iters-2 enqueue exactly the same ~300 short
// launches with the same arguments: where the caller allows (`may_capture`) and at least two of them are left, they are
// captured once into `slot` (kept in the workspace with its key: `same_key()` compares it, `store_key()` records it) and
// replayed, which removes most of the per-launch cost that bounds a single-room ResGCN iteration; a capture that fails - it
// is not possible on the legacy default stream - leaves them eager, counted.  The last iteration differs (it returns the
// un-projected step) and is eager again.
template <typename Iteration, typename SameKey, typename StoreKey>
static int nb_iterations(psg::GraphSlot &slot, hipStream_t st, int iters, bool may_capture, Iteration &&iteration, SameKey &&same_key,
                         StoreKey &&store_key)
{
    int rc;
    if ((rc = iteration(iters == 1))) return rc;
    int it = 1;
    if (may_capture && iters - 1 - it >= 2) {
        if (!same_key()) PSG_CHECK_HIP(slot.forget(st));
        if (!slot.exec && !slot.capture_failed) {
            slot.capture(st, [&] { return iteration(false); });
            store_key();
        }
        if (slot.exec) {
            PSG_CHECK_HIP(slot.replay(st, iters - 1 - it));
            it = iters - 1;
        } else {
            slot.note_eager(iters - 1 - it);
        }
    }
    for (; it < iters; ++it)
        if ((rc = iteration(it == iters - 1))) return rc;
    return PSG_OK;
}

// colper.NB_attack (ResGCN/sem_seg_dense/attacks/torchattacks/attacks/colper.py:17-39): CrossEntropyLoss()
// (mean over all B*N points) on the logits, sign ascent on the colour channels, L-inf projection; the
// returned colours are the un-projected last step (the projection is not written back after the loop).
extern "C" int psg_gcn_nb_attack(psg_gcn_model *m, psg_gcn_ws *ws, const float *images, const int32_t *labels,
                                 float eps, float alpha, int iters, float *adv_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && images && labels && adv_out, "psg_gcn_nb_attack: null argument");
    PSG_REQUIRE(iters > 0, "psg_gcn_nb_attack: iters must be positive");
    hipStream_t st = (hipStream_t)stream;
    const int B = ws->B, N = ws->N;
    const size_t R = (size_t)B * N;
    int rc;
    if ((rc = psg_to_point_major(images, B, 9, N, ws->x0, st))) return rc;
    hipLaunchKernelGGL(extract_color3_kernel, dim3(ceil_div((int)(R * 3), 256)), dim3(256), 0, st, ws->x0, ws->ori, R);
    PSG_LAUNCH_CHECK();
    PSG_CHECK_HIP(hipMemcpyAsync(ws->nb_labels, labels, R * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    // the attack moves colours only: the head's kNN graph on xyz (architecture.py:59) is the same in every iteration, so the
    // first forward builds it and the later ones keep it
    struct Unfreeze { psg_gcn_ws *w; ~Unfreeze() { w->head_graph_frozen = false; } } unfreeze{ws};
    ws->head_graph_frozen = false;
    auto iteration = [&](bool last) -> int {
        int r;
        if ((r = psg_gcn_forward(m, ws, ws->x0, ws->logits, st))) return r;
        ws->head_graph_frozen = true;
        if ((r = psg_ce_logp_grad(ws->logits, ws->nb_labels, 0, (int)R, (int)R, NCLS, 1.0f / (float)R, ws->dlogits, nullptr, st)))
            return r;
        if ((r = psg_gcn_backward(m, ws, ws->dlogits, ws->dx0, st))) return r;
        return psg_pgd_step(ws->x0, ws->dx0, ws->ori, nullptr, B, N, alpha, eps, 1.0f, last ? 1 : 0, st);
    };
    static const bool use_graph = !((psg::env_int("PSG_GCN_NO_GRAPH", 0) != 0)) && !trace_sync_enabled();   // (the tracer synchronises after every launch)
    if ((rc = nb_iterations(
             ws->nb, st, iters, use_graph && !ws->prof.on, iteration,
             [&] { return ws->nb_model_gen == m->gen && ws->nb_eps == eps && ws->nb_alpha == alpha && ws->nb_fixed == ws->fixed_graphs; },
             [&] { ws->nb_model_gen = m->gen; ws->nb_eps = eps; ws->nb_alpha = alpha; ws->nb_fixed = ws->fixed_graphs; })))
        return rc;
    return psg_to_channel_major(ws->x0, B, 9, N, adv_out, st);
}

// ====================================================================================== NU attack windows
// colper.NU_attack / tcolper.tar_NU_attack (ResGCN/sem_seg_dense/attacks/torchattacks/attacks/colper.py:62-95,
// tcolper.py:85-132) for G one-room attacks in lockstep: one step sequence of a window, shared by the eager and the captured
// path; dconsts_rows: the window's device rows or null.  Everything in it is a launch or an asynchronous device-to-device
// copy on `stream` (the forward and backward are the ones psg_gcn_nb_attack captures), so a window is a single chain.
// The head's xyz graph is rebuilt by every forward: freezing it inside a window has not been measured, and a restart's
// clamp moves xyz between windows.
static int gcn_nu_window_steps(const psg_gcn_nu_window_args *a, const float *dconsts_rows, psg_stream stream)
{
    const int G = a->G, N = a->N;
    int rc = PSG_OK;
    for (int i = 0; i < a->n_steps && rc == PSG_OK; ++i) {
        const int step = a->step0 + i, adam_t = a->adam_t0 + i + 1;
        const int f_target = a->use_target ? a->target : 0;
        if ((rc = psg_nu_tanh_color_rooms(a->w, a->mask, G, N, a->x0, stream))) break;
        if ((rc = psg_gcn_forward(a->model, a->ws, a->x0, a->logits, stream))) break;
        if ((rc = psg_gcn_f_loss_grad_rooms(a->logits, a->labels, f_target, a->mask, a->mode, G, N, NCLS, a->kappa, a->tsign, a->c_f,
                                            a->dlogits, a->scal, a->pred, stream)))
            break;
        if ((rc = psg_gcn_backward(a->model, a->ws, a->dlogits, a->dx0, stream))) break;
        if ((rc = psg_smooth_knn_sym_rooms(a->x0 + 3, 9, (size_t)N * 9, G, N, a->neighbour, a->scal + G, a->sgrad, a->active,
                                           a->nn_state, stream)))
            break;
        psg::NuStepConsts consts(dconsts_rows ? dconsts_rows + 4 * i : nullptr);
        rc = psg::nu_colour_adam(a, a->c_smooth, a->c_l2, 1, adam_t, stream);
        if (rc == PSG_OK) rc = psg::nu_latch(a, 1, a->hist + (size_t)i * 5 * G, step, stream);
    }
    return rc;
}

extern "C" int psg_gcn_nu_window(const psg_gcn_nu_window_args *a, psg_nu_graph *graph, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->w && a->m && a->v && a->x0 && a->ori && a->labels && a->logits && a->dlogits && a->dx0 &&
                    a->sgrad && a->pred && a->scal && a->nn_state && a->hist && a->out && a->active && a->exit_step,
                "psg_gcn_nu_window: null argument");
    PSG_REQUIRE(a->n_steps > 0 && a->G > 0 && a->N > 0, "psg_gcn_nu_window: n_steps=%d G=%d N=%d out of range", a->n_steps, a->G, a->N);
    PSG_REQUIRE(a->G == a->ws->B && a->N == a->ws->N,
                "psg_gcn_nu_window: rooms form only - the workspace is for %d rooms of %d points, the window for %d of %d", a->ws->B,
                a->ws->N, a->G, a->N);
    PSG_REQUIRE(a->model->n_blocks == a->ws->n_blocks && a->model->block == a->ws->block && a->model->conv == a->ws->conv,
                "psg_gcn_nu_window: model / workspace configuration mismatch");
    PSG_REQUIRE(a->mode >= 0 && a->mode <= 2, "psg_gcn_nu_window: mode %d out of range", a->mode);
    PSG_REQUIRE(a->mode == 0 || (a->mask && a->n_mask), "psg_gcn_nu_window: modes 1 and 2 need mask and n_mask");
    PSG_REQUIRE((a->mode == 2) == (a->use_target != 0), "psg_gcn_nu_window: mode 2 is the one that takes a target class");
    PSG_REQUIRE(!a->use_target || (a->target >= 0 && a->target < NCLS), "psg_gcn_nu_window: target class %d out of range", a->target);
    PSG_REQUIRE(a->neighbour > 0 && a->neighbour <= 16 && a->N <= 8192, "psg_gcn_nu_window: neighbour=%d (1..16) / N=%d (<= 8192) out of range",
                a->neighbour, a->N);
    // what a captured window is valid for: the argument block without what the device rows carry, and whether the forward
    // builds its graphs or takes the ones psg_gcn_set_graphs supplied (the two enqueue different launches)
    struct Key { psg_gcn_nu_window_args a; int fixed_graphs; } key;
    memset(&key, 0, sizeof(key));
    key.a = *a;
    key.a.step0 = 0; key.a.adam_t0 = 0; key.a.lr = 0.0f;
    key.fixed_graphs = a->ws->fixed_graphs ? 1 : 0;
    return nu_graph_window(a->ws->prof.on ? nullptr : graph, &key, sizeof(key), a->model->gen, a->ws->gen, a->n_steps, a->step0,
                           a->adam_t0, a->lr, a->beta1, a->beta2, (hipStream_t)stream,
                           [&](const float *rows) { return gcn_nu_window_steps(a, rows, stream); });
}

// ====================================================================================== coordinate-field attacks
// An extension of the reference API: the reference's colper.py:17-37 branches on `atype` and ships the
// colour branch only.  The kNN graphs are constants of the derivative (topk under no_grad), so psg_gcn_backward's dx0[0:3]
// IS the coordinate gradient; what changes is that the head's xyz graph follows the moved points - it is never frozen here.

// NB_attack with field = coord | both: iters x (forward, CE, backward, psg_pgd_step_field on channels 0:3 - sign step, eta
// clamped to +-coord_eps, no [0, 1] clamp - and, both, on 3:6); the un-projected last step is returned, as on colours.
extern "C" int psg_gcn_nb_attack_field(psg_gcn_model *m, psg_gcn_ws *ws, const float *images, const int32_t *labels, int field,
                                       float eps, float alpha, float coord_eps, float coord_alpha, int iters, float *adv_out,
                                       psg_stream stream)
{
    PSG_REQUIRE(m && ws && images && labels && adv_out, "psg_gcn_nb_attack_field: null argument");
    PSG_REQUIRE(iters > 0, "psg_gcn_nb_attack_field: iters must be positive");
    PSG_REQUIRE(field == PSG_NU_FIELD_COORD || field == PSG_NU_FIELD_BOTH,
                "psg_gcn_nb_attack_field: field %d is neither coord (%d) nor both (%d); colours alone are psg_gcn_nb_attack", field,
                PSG_NU_FIELD_COORD, PSG_NU_FIELD_BOTH);
    PSG_REQUIRE(m->n_blocks == ws->n_blocks && m->block == ws->block && m->conv == ws->conv,
                "psg_gcn_nb_attack_field: model / workspace configuration mismatch");
    hipStream_t st = (hipStream_t)stream;
    const int B = ws->B, N = ws->N;
    const size_t R = (size_t)B * N;
    const bool both = field == PSG_NU_FIELD_BOTH;
    int rc;
    if ((rc = psg_to_point_major(images, B, 9, N, ws->x0, st))) return rc;
    hipLaunchKernelGGL(extract_color3_kernel, dim3(ceil_div((int)(R * 3), 256)), dim3(256), 0, st, ws->x0, ws->ori, R);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(extract3_kernel, dim3(ceil_div((int)(R * 3), 256)), dim3(256), 0, st, ws->x0, ws->ori_xyz, R);
    PSG_LAUNCH_CHECK();
    PSG_CHECK_HIP(hipMemcpyAsync(ws->nb_labels, labels, R * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    ws->head_graph_frozen = false;            // the points move: every forward rebuilds the head's xyz graph
    auto iteration = [&](bool last) -> int {
        int r;
        if ((r = psg_gcn_forward(m, ws, ws->x0, ws->logits, st))) return r;
        if ((r = psg_ce_logp_grad(ws->logits, ws->nb_labels, 0, (int)R, (int)R, NCLS, 1.0f / (float)R, ws->dlogits, nullptr, st)))
            return r;
        if ((r = psg_gcn_backward(m, ws, ws->dlogits, ws->dx0, st))) return r;
        if ((r = psg_pgd_step_field(ws->x0, ws->dx0, ws->ori_xyz, nullptr, B, N, 0, coord_alpha, coord_eps, 1.0f, last ? 1 : 0, st)))
            return r;
        return both ? psg_pgd_step_field(ws->x0, ws->dx0, ws->ori, nullptr, B, N, 3, alpha, eps, 1.0f, last ? 1 : 0, st) : PSG_OK;
    };
    // the interior iterations are captured into ws->nbf (a single chain on `st`).  On the legacy default stream (no capture
    // there), under the launch tracer and while the workspace is profiling, the loop stays eager.
    static const bool use_graph = !((psg::env_int("PSG_GCN_NO_GRAPH", 0) != 0)) && !trace_sync_enabled();
    if ((rc = nb_iterations(
             ws->nbf, st, iters, use_graph && st && !ws->prof.on, iteration,
             [&] {
                 return ws->nbf_model_gen == m->gen && ws->nbf_field == field && ws->nbf_eps == eps && ws->nbf_alpha == alpha &&
                        ws->nbf_ceps == coord_eps && ws->nbf_calpha == coord_alpha && ws->nbf_fixed == ws->fixed_graphs;
             },
             [&] {
                 ws->nbf_model_gen = m->gen; ws->nbf_field = field; ws->nbf_eps = eps; ws->nbf_alpha = alpha;
                 ws->nbf_ceps = coord_eps; ws->nbf_calpha = coord_alpha; ws->nbf_fixed = ws->fixed_graphs;
             })))
        return rc;
    return psg_to_channel_major(ws->x0, B, 9, N, adv_out, st);
}

// NU_attack / tar_NU_attack with field = coord | both for G one-room attacks in lockstep: the step sequence of
// gcn_nu_window_steps with delta applied first and the coordinate Smooth term and Adam step added - apply, forward,
// f-loss, backward, Smooth term(s), Adam step(s), latch, then the two coordinate sums into rows 5, 6 of the history row.
// Everything is a launch or an asynchronous device-to-device copy on `stream`: a window is a single chain, and - this
// network has no FPS plan and draws nothing inside a step - it is captured and replayed like the colour windows.
static int gcn_nu_field_window_steps(const psg_gcn_nu_field_window_args *a, const float *dconsts_rows, psg_stream stream)
{
    const int G = a->G, N = a->N;
    const bool both = a->field == PSG_NU_FIELD_BOTH;
    int rc = PSG_OK;
    for (int i = 0; i < a->n_steps && rc == PSG_OK; ++i) {
        const int step = a->step0 + i, adam_t = a->adam_t0 + i + 1;
        const int f_target = a->use_target ? a->target : 0;
        float *hist = a->hist + (size_t)i * 7 * G;
        if ((rc = psg_nu_coord_apply_rooms(a->delta, a->ori_xyz, a->mask, G, N, a->active, a->x0, stream))) break;
        if (both && (rc = psg_nu_tanh_color_rooms(a->w, a->mask, G, N, a->x0, stream))) break;
        if ((rc = psg_gcn_forward(a->model, a->ws, a->x0, a->logits, stream))) break;
        if ((rc = psg_gcn_f_loss_grad_rooms(a->logits, a->labels, f_target, a->mask, a->mode, G, N, NCLS, a->kappa, a->tsign, a->c_f,
                                            a->dlogits, a->scal, a->pred, stream)))
            break;
        if ((rc = psg_gcn_backward(a->model, a->ws, a->dlogits, a->dx0, stream))) break;
        if (both && (rc = psg_smooth_knn_sym_rooms(a->x0 + 3, 9, (size_t)N * 9, G, N, a->neighbour, a->scal + G, a->sgrad, a->active,
                                                   a->nn_state, stream)))
            break;
        if ((rc = psg_smooth_knn_xyz_sym_rooms(a->x0, 9, (size_t)N * 9, G, N, a->neighbour, a->scal + 3 * G, a->sgrad_xyz, a->active,
                                               a->nn_xyz, stream)))
            break;
        {
            psg::NuStepConsts consts(dconsts_rows ? dconsts_rows + 4 * i : nullptr);
            if (both) rc = psg::nu_colour_adam(a, a->c_smooth, a->c_l2, 1, adam_t, stream);
            if (rc == PSG_OK)
                rc = psg_nu_coord_adam_step_rooms_w(a->delta, a->mx, a->vx, a->mask, a->dx0, a->sgrad_xyz, a->c_smooth_xyz, a->c_l2_xyz,
                                                    a->coord_lr, a->beta1, a->beta2, a->eps, adam_t, G, N, a->active, a->scal + 4 * G, stream);
            if (rc == PSG_OK) rc = psg::nu_latch(a, 1, hist, step, stream);
        }
        if (rc == PSG_OK) rc = psg::nu_field_hist_tail(a->scal, hist, G, (hipStream_t)stream);
    }
    return rc;
}

extern "C" int psg_gcn_nu_field_window(const psg_gcn_nu_field_window_args *a, psg_nu_graph *graph, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->delta && a->mx && a->vx && a->ori_xyz && a->sgrad_xyz && a->nn_xyz && a->x0 && a->labels &&
                    a->logits && a->dlogits && a->dx0 && a->pred && a->scal && a->hist && a->out && a->active && a->exit_step,
                "psg_gcn_nu_field_window: null argument");
    PSG_REQUIRE(a->field == PSG_NU_FIELD_COORD || a->field == PSG_NU_FIELD_BOTH,
                "psg_gcn_nu_field_window: field %d is neither coord (%d) nor both (%d); colours alone are psg_gcn_nu_window", a->field,
                PSG_NU_FIELD_COORD, PSG_NU_FIELD_BOTH);
    PSG_REQUIRE(a->field != PSG_NU_FIELD_BOTH || (a->w && a->m && a->v && a->ori && a->sgrad && a->nn_state),
                "psg_gcn_nu_field_window: field both needs the colour state");
    PSG_REQUIRE(a->n_steps > 0 && a->G > 0 && a->N > 0, "psg_gcn_nu_field_window: n_steps=%d G=%d N=%d out of range", a->n_steps, a->G, a->N);
    PSG_REQUIRE(a->G == a->ws->B && a->N == a->ws->N,
                "psg_gcn_nu_field_window: rooms form only - the workspace is for %d rooms of %d points, the window for %d of %d", a->ws->B,
                a->ws->N, a->G, a->N);
    PSG_REQUIRE(a->model->n_blocks == a->ws->n_blocks && a->model->block == a->ws->block && a->model->conv == a->ws->conv,
                "psg_gcn_nu_field_window: model / workspace configuration mismatch");
    PSG_REQUIRE(a->mode >= 0 && a->mode <= 2, "psg_gcn_nu_field_window: mode %d out of range", a->mode);
    PSG_REQUIRE(a->mode == 0 || (a->mask && a->n_mask), "psg_gcn_nu_field_window: modes 1 and 2 need mask and n_mask");
    PSG_REQUIRE((a->mode == 2) == (a->use_target != 0), "psg_gcn_nu_field_window: mode 2 is the one that takes a target class");
    PSG_REQUIRE(!a->use_target || (a->target >= 0 && a->target < NCLS), "psg_gcn_nu_field_window: target class %d out of range", a->target);
    PSG_REQUIRE(a->neighbour > 0 && a->neighbour <= 16 && a->N <= 8192,
                "psg_gcn_nu_field_window: neighbour=%d (1..16) / N=%d (<= 8192) out of range", a->neighbour, a->N);
    // what a captured window is valid for: the argument block without what the device rows carry (step, both step sizes)
    struct Key { psg_gcn_nu_field_window_args a; int fixed_graphs; } key;
    memset(&key, 0, sizeof(key));
    key.a = *a;
    key.a.step0 = 0; key.a.adam_t0 = 0; key.a.lr = 0.0f; key.a.coord_lr = 0.0f;
    key.fixed_graphs = a->ws->fixed_graphs ? 1 : 0;
    // slot 3 of the device rows: the coordinate variable's step size coord_lr / (1 - beta1^t), as
    // psg_nu_coord_adam_step_rooms_w computes it from its arguments
    float slot3[PSG_NU_GRAPH_MAX_STEPS];
    for (int i = 0; i < a->n_steps && i < PSG_NU_GRAPH_MAX_STEPS; ++i)
        slot3[i] = (float)((double)a->coord_lr / (1.0 - pow((double)a->beta1, (double)(a->adam_t0 + i + 1))));
    return nu_graph_window(a->ws->prof.on ? nullptr : graph, &key, sizeof(key), a->model->gen, a->ws->gen, a->n_steps, a->step0,
                           a->adam_t0, a->lr, a->beta1, a->beta2, (hipStream_t)stream,
                           [&](const float *rows) { return gcn_nu_field_window_steps(a, rows, stream); }, slot3);
}
