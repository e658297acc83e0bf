// Every kernel of the ResGCN unit, with the two launch helpers that belong to them (launch_gemm with the unit's tile
// threshold, launch_edge_max_bwd).  Included by psg_resgcn.hip ONLY, behind its using-directives: each kernel is compiled once.
#pragma once
#include "psg_gemm.cuh"
#include "psg_knn.h"
#include "psg_knn_ops.cuh"
#include "psg_resgcn.h"
#include "psg_wave.cuh"

namespace {

template <int WM, int WN, int EPI, bool ASC> int launch_gemm(const GemmArgs &a, hipStream_t st)
{
    return psg::launch_gemm<WM, WN, EPI, ASC>(a, (size_t)gcn_switches().gemm_small_below, st);
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
    if (!gcn_switches().edge_bwd_atomic && N <= 32 * EBG_WORDS && ld_dy % 4 == 0 && ((uintptr_t)dy & 15) == 0) {
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

}  // namespace
