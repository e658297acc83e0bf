// Geometry kernels of the PointNet++ hot path for gfx950: farthest-point sampling, ball query,
// 3-NN + inverse-distance weights, row gather.  All of them are integer-output (or feed integer
// decisions), so the fp32 evaluation order is the one pinned in SURVEY.md section 8(a') and every
// multiply/add below is written with explicit rounding intrinsics (this file is also compiled with
// -ffp-contract=off).  VALU fp32 on purpose: MFMA accumulation order would break bit-exact grouping.
//
// Reference semantics (paths relative to /root/reference):
//   farthest_point_sample  PointNet/models/pointnet_util.py:63-84
//   query_ball_point       PointNet/models/pointnet_util.py:87-107  (square_distance :19-40)
//   3-NN interpolation     PointNet/models/pointnet_util.py:301-307
//   index_points           PointNet/models/pointnet_util.py:43-60
//
// Batching: every kernel runs P independent "problems" (= rooms x attack iterations).  A problem p
// reads cloud (p % n_clouds) of a [n_clouds][N][3] array, so the level-0 xyz of a room is shared by
// all attack iterations while deeper levels have one cloud per problem.
#include "psg_common.h"
#include "psg_sqdist.cuh"

namespace {

using psg::sqdist;   // square_distance for one pair, the pinned fp32 order (psg_sqdist.cuh)
using psg::sumsq3;

typedef float v2f __attribute__((ext_vector_type(2)));   // operand of the packed-fp32 pipe (v_pk_*_f32)

// ---- wave-level max with DPP (no LDS round trips) --------------------------------------------
// `old` is 0, the identity of an unsigned max: a lane the row mask leaves out gets 0 and keeps its own v, exactly as with
// old = v, and the compiler folds the whole stage into ONE v_max_u32_dpp (with old = v it is v_mov, s_nop, v_mov_dpp, v_max).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_max_u32(unsigned v)
{
    unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
    return o > v ? o : v;
}
// max over each row of 16 lanes, result in every lane of the row
__device__ __forceinline__ unsigned row_max_u32(unsigned v)
{
    v = dpp_max_u32<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
    v = dpp_max_u32<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
    v = dpp_max_u32<0x141, 0xF>(v);  // row_half_mirror
    v = dpp_max_u32<0x140, 0xF>(v);  // row_mirror
    return v;
}
// max over the 64 lanes of the wave, returned wave-uniform
__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
    v = row_max_u32(v);
    v = dpp_max_u32<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
    v = dpp_max_u32<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// max of N keys as a tree of three-input maxima (v_max3_u32), depth ceil(log3 N)
template <int N>
__device__ __forceinline__ unsigned max_of(const unsigned (&k)[N])
{
    constexpr int G = (N + 2) / 3;
    unsigned t[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        unsigned a = k[3 * g];
        if (3 * g + 1 < N) a = max(a, k[3 * g + 1]);
        if (3 * g + 2 < N) a = max(a, k[3 * g + 2]);
        t[g] = a;
    }
    if constexpr (G == 1) return t[0];
    else return max_of<G>(t);
}

// ---------------------------------------------------------------------------------------------
// FPS: one workgroup per problem; thread t owns the PPT consecutive points PPT*t .. PPT*t+PPT-1
// (so a lower lane / lower wave always means a lower point index).  The points stay in registers for the
// distance update; the centroid of a step is broadcast from the cloud in LDS (LDSC) or, in the form that
// keeps LDS free for more resident problems, read from the cloud in global memory by scalar loads at
// the wave-uniform index.  Per step:
//   distance update  ->  per-lane max of the keys  ->  wave max by DPP  ->  ballot picks the lowest lane
//   holding it, one compare per key against the wave max gives the lanes holding it at point j, and the
//   lowest j whose mask has the winning lane's bit is picked on the scalar side  ->  one LDS slot per
//   wave, ONE barrier (slots double-buffered)  ->  16-lane DPP max over the wave partials, ballot picks
//   the lowest wave.
// Distances are non-negative floats, kept and compared as their bit patterns (exact same order): the
// update `d < dist ? d : dist` is an unsigned min on the bits - d is +0 or above, NaN or +inf, never
// -0, and the bits of a NaN (either sign) or of +inf lie above those of every distance the array can
// hold (<= 1e10f), so they keep the old distance as `<` does.  A padding point (index >= N) starts at
// 0, stays at 0 under min, and a key of 0 never beats a real point: at equal keys the lower index
// wins, and index 0 is real.  Ties resolve to the lowest index like torch.max on CPU.  When every key is 0
// (all points taken, or S above the number of distinct positions) every lane of every wave ties at 0,
// the lowest lane's lowest point is picked in wave 0, and the result is index 0.
// ---------------------------------------------------------------------------------------------
template <int NT, int PPT, bool LDSC>
__global__ __launch_bounds__(NT) void fps_kernel(const float *__restrict__ xyz, int n_clouds, int N, int S,
                                                 const int32_t *__restrict__ start, int32_t *__restrict__ out)
{
    constexpr int NW = NT / 64;
    extern __shared__ float smem[];
    float *s_xyz = smem;                                           // LDSC: [NT*PPT*3] (padded cloud)
    uint2 *s_part = (uint2 *)(smem + (LDSC ? NT * PPT * 3 : 0));   // [2][NW] (value bits, index)

    const int p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *src = xyz + (size_t)(p % n_clouds) * N * 3;
    if (LDSC) {
        for (int i = tid; i < NT * PPT * 3; i += NT) s_xyz[i] = i < N * 3 ? src[i] : 0.0f;
        __syncthreads();
    }

    // points in registers as pairs: the distance update runs on the packed-fp32 pipe (two points per instruction,
    // every lane result bit-identical to the scalar sub / mul / add sequence of sumsq3); PPT = 1 has one point in
    // both halves of its pair and a single key
    constexpr int PP = (PPT + 1) / 2;
    v2f px[PP], py[PP], pz[PP];
    unsigned dist[PPT];
#pragma unroll
    for (int q = 0; q < PP; ++q) {
        const int i = tid * PPT + 2 * q, i1 = (2 * q + 1 < PPT) ? i + 1 : i;
        if (LDSC) {
            px[q] = v2f{s_xyz[3 * i], s_xyz[3 * i1]};
            py[q] = v2f{s_xyz[3 * i + 1], s_xyz[3 * i1 + 1]};
            pz[q] = v2f{s_xyz[3 * i + 2], s_xyz[3 * i1 + 2]};
        } else {
            // a thread's PPT points are 12 * PPT consecutive bytes of the cloud; padding points are zeros, as in the LDS image
            const bool in0 = i < N, in1 = i1 < N;
            px[q] = v2f{in0 ? src[3 * i] : 0.0f, in1 ? src[3 * i1] : 0.0f};
            py[q] = v2f{in0 ? src[3 * i + 1] : 0.0f, in1 ? src[3 * i1 + 1] : 0.0f};
            pz[q] = v2f{in0 ? src[3 * i + 2] : 0.0f, in1 ? src[3 * i1 + 2] : 0.0f};
        }
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) dist[j] = (tid * PPT + j) < N ? __float_as_uint(1e10f) : 0u;

    int far = start[p];
    int32_t *o = out + (size_t)p * S;
    for (int s = 0; s < S; ++s) {
        if (tid == 0) o[s] = far;
        float cx, cy, cz;
        if (LDSC) {
            cx = s_xyz[3 * far], cy = s_xyz[3 * far + 1], cz = s_xyz[3 * far + 2];
        } else {
            const float *c = src + 3 * (size_t)far;   // far is wave-uniform and < N: three scalar loads, served by L2
            cx = c[0], cy = c[1], cz = c[2];
        }
        const v2f cx2 = {cx, cx}, cy2 = {cy, cy}, cz2 = {cz, cz};
#pragma unroll
        for (int q = 0; q < PP; ++q) {
            const v2f dx = px[q] - cx2, dy = py[q] - cy2, dz = pz[q] - cz2;
            const v2f d = ((dx * dx) + (dy * dy)) + (dz * dz);
            dist[2 * q] = min(dist[2 * q], __float_as_uint(d[0]));
            if (2 * q + 1 < PPT) dist[2 * q + 1] = min(dist[2 * q + 1], __float_as_uint(d[1]));
        }
        const unsigned best = max_of<PPT>(dist);
        const unsigned wmax = wave_max_u32(best);
        const unsigned long long hit = __ballot(best == wmax);
        const int src_lane = __builtin_ctzll(hit);
        // the winning lane holds wmax at one point at least: the lowest such point, from the lane masks of the keys
        int bq = PPT - 1;
#pragma unroll
        for (int j = PPT - 2; j >= 0; --j)
            if ((__ballot(dist[j] == wmax) >> src_lane) & 1ull) bq = j;
        int widx = (wave * 64 + src_lane) * PPT + bq;
        if (NW > 1) {
            uint2 *slot = s_part + (s & 1) * NW;
            if (lane == 0) slot[wave] = make_uint2(wmax, (unsigned)widx);
            __syncthreads();
            const uint2 part = slot[lane & (NW - 1)];
            const unsigned gmax = row_max_u32(part.x);
            const unsigned long long hw = __ballot(part.x == gmax) & ((1ull << NW) - 1ull);
            widx = __builtin_amdgcn_readlane((int)part.y, __builtin_ctzll(hw));
        }
        far = __builtin_amdgcn_readfirstlane(widx);
    }
}

// out[p][s][:] = points[p % n_clouds][idx[p][s]][:]
__global__ void gather_rows_kernel(const float *__restrict__ pts, int n_clouds, int N, int C,
                                   const int32_t *__restrict__ idx, int S, float *__restrict__ out, int P)
{
    size_t total = (size_t)P * S * C;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        int c = (int)(t % C);
        size_t r = t / C;
        int s = (int)(r % S);
        int p = (int)(r / S);
        out[t] = pts[((size_t)(p % n_clouds) * N + idx[(size_t)p * S + s]) * C + c];
    }
}

// ---------------------------------------------------------------------------------------------
// Ball query: the cloud (x,y,z,|p|^2) is staged once per workgroup in LDS; one wave per centroid
// scans it 64 points at a time in index order, compacting hits with ballot + prefix popcount and
// stopping at K.  No [S,N] matrix, no sort (the reference materialises both).
// ---------------------------------------------------------------------------------------------
constexpr int BQ_THREADS = 1024;
constexpr int BQ_CPB = 128;  // centroids per workgroup (8 per wave)
constexpr int BQ_UNROLL = 4; // 64-point chunks in flight per wave (hides the LDS latency of the scan)

__global__ __launch_bounds__(BQ_THREADS) void ball_query_kernel(const float *__restrict__ xyz, int n_clouds,
                                                                const float *__restrict__ new_xyz, int N, int S,
                                                                float r2, int K, int32_t *__restrict__ out)
{
    // structure-of-arrays staging: a lane's points j and j + 64 of one plane come back from ONE ds_read2_b32 in
    // adjacent registers, i.e. directly as an operand of the packed-fp32 pipe (two distances per instruction)
    extern __shared__ float s_soa[];   // x[NP] y[NP] z[NP] |p|^2[NP], NP = N rounded up to 256
    const int NP = (N + 255) & ~255;
    float *s_x = s_soa, *s_y = s_soa + NP, *s_z = s_soa + 2 * NP, *s_q = s_soa + 3 * NP;
    const int p = blockIdx.y;
    const float *src = xyz + (size_t)(p % n_clouds) * N * 3;
    for (int i = threadIdx.x; i < NP; i += BQ_THREADS) {
        float x = 0.f, y = 0.f, z = 0.f, q = INFINITY;       // padding points are infinitely far away
        if (i < N) { x = src[3 * i]; y = src[3 * i + 1]; z = src[3 * i + 2]; q = sumsq3(x, y, z); }
        s_x[i] = x; s_y[i] = y; s_z[i] = z; s_q[i] = q;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int c_end = min(S, (int)(blockIdx.x + 1) * BQ_CPB);
    for (int c = blockIdx.x * BQ_CPB + wave; c < c_end; c += BQ_THREADS / 64) {
        const float *cp = new_xyz + ((size_t)p * S + c) * 3;
        const float cx = cp[0], cy = cp[1], cz = cp[2];
        const float csq = sumsq3(cx, cy, cz);
        const v2f cx2 = {cx, cx}, cy2 = {cy, cy}, cz2 = {cz, cz}, cs2 = {csq, csq}, m2 = {-2.0f, -2.0f};
        int32_t *o = out + ((size_t)p * S + c) * K;
        int cnt = 0, first = N;
        for (int base = 0; base < N && cnt < K; base += 64 * BQ_UNROLL) {
            bool in[BQ_UNROLL];
#pragma unroll
            for (int u = 0; u < BQ_UNROLL; u += 2) {
                const int j = base + u * 64 + lane;             // and j + 64
                const v2f qx = {s_x[j], s_x[j + 64]}, qy = {s_y[j], s_y[j + 64]}, qz = {s_z[j], s_z[j + 64]},
                          qs = {s_q[j], s_q[j + 64]};
                // square_distance order: ((-2 * fma chain) + |centroid|^2) + |point|^2, as sqdist()
                v2f dot = cx2 * qx;
                dot = __builtin_elementwise_fma(cy2, qy, dot);
                dot = __builtin_elementwise_fma(cz2, qz, dot);
                const v2f dd = ((m2 * dot) + cs2) + qs;
                in[u] = !(dd[0] > r2);                          // padding: +inf > r2
                in[u + 1] = !(dd[1] > r2);
            }
#pragma unroll
            for (int u = 0; u < BQ_UNROLL; ++u) {
                unsigned long long m = __ballot(in[u]);
                if (m) {
                    if (cnt == 0) first = base + u * 64 + __builtin_ctzll(m);
                    int pos = cnt + __popcll(m & lt_mask);
                    if (in[u] && pos < K) o[pos] = base + u * 64 + lane;
                    cnt += __popcll(m);
                }
            }
        }
        // pad with the first hit (pointnet_util.py:104-106); an empty ball emits N (reference would fault)
        for (int pos = min(cnt, K) + lane; pos < K; pos += 64) o[pos] = first;
    }
}

// ---------------------------------------------------------------------------------------------
// Ball query through a uniform grid (round 4), for clouds of 2048 to 4096 points (SA level 0).  The scan above tests every centroid
// against every point (1024 x 4096 pairs per problem at level 0: the kernel sat at ~45 % of the vector peak and was 3 %
// of an attack); a ball of radius r holds a few dozen points.  Per workgroup: the cloud is staged as before, its
// bounding box is reduced, points are binned into cells of edge >= 1.05 r (LDS counting sort: histogram, scan,
// scatter; the order inside a cell is arbitrary), and a wave then serves a centroid from the 27 cells around it
// (9 contiguous runs of the sorted index list): the candidates - typically 40 to 150 instead of 4096 - get the SAME
// distance arithmetic as the scan (sqdist: the reference's expansion, whose rounding decides membership at the ball
// boundary), hits set their bit in a per-wave bitmap over the N points, and the first K set bits ARE the reference's
// "first nsample indices in ascending order" (pointnet_util.py:100-106).  Pruning can only drop points that the exact
// test would reject: the expansion's rounding error is below 2.4e-7 (|c| + |p|)^2 <= 3e-6 max|coordinate|^2, so a point
// that passes the test has a true squared distance below r^2 + 1e-5 max|coordinate|^2 - and the cell edge is 1.05 x the
// root of exactly that, i.e. the point is less than one cell edge away per axis - and both cell indices come from the same
// monotone formula (a centroid outside the cloud's box is clamped to the border cell: what it can reach lies in the border
// cells).  A cloud with non-finite coordinates is one cell, i.e. the full scan.  The argument above is about centroids that
// can REACH the cloud: psg_ball_query is a public entry that takes arbitrary new_xyz, so a centroid that is non-finite
// (every `dd > r2` is false for a NaN: the scan returns 0 .. K-1) or lies more than one cell edge outside the cloud's box
// (far enough away, cancellation in the expansion passes points no cell walk would visit) takes ALL N points as its
// candidates - the scan, inside this kernel (advisor, round 4; tests/test_gpu_ball_grid.py).  Same indices, bit for bit
// (tests/test_gpu_parity.py: reference fixtures; test_unit_geometry_vs_oracle; tests/test_gpu_edge.py).
// ---------------------------------------------------------------------------------------------
constexpr int BQG_CELLS = 4096;     // cells per cloud at most (the edge grows by 1.25x until the box fits)
constexpr int BQG_CPB = 1024;       // centroids per workgroup (64 per wave): the grid build is shared by all queries of a level-0 problem

// inclusive prefix sum over the 64 lanes on the DPP network (row_shr 1 / 2 / 4 / 8, then row_bcast15 / row_bcast31); lanes
// shifted in from outside a row read 0.  (A __shfl_up scan is six dependent LDS round trips: three of them per centroid
// were most of this kernel's first version.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned bq_dpp0(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ unsigned bq_wave_incl_scan(unsigned v)
{
    v += bq_dpp0<0x111, 0xF>(v);
    v += bq_dpp0<0x112, 0xF>(v);
    v += bq_dpp0<0x114, 0xF>(v);
    v += bq_dpp0<0x118, 0xF>(v);
    v += bq_dpp0<0x142, 0xA>(v);
    v += bq_dpp0<0x143, 0xC>(v);
    return v;
}

__global__ __launch_bounds__(BQ_THREADS) void ball_query_grid_kernel(const float *__restrict__ xyz, int n_clouds,
                                                                     const float *__restrict__ new_xyz, int N, int S,
                                                                     float r2, int K, int32_t *__restrict__ out)
{
    extern __shared__ float s_soa[];   // x[NP] y[NP] z[NP] |p|^2[NP] | cell starts [CELLS + 1] | cursors [CELLS] = bitmaps | sorted [NP] u16
    const int NP = (N + 255) & ~255;
    float *s_x = s_soa, *s_y = s_soa + NP, *s_z = s_soa + 2 * NP, *s_q = s_soa + 3 * NP;
    int *s_start = (int *)(s_soa + 4 * NP);
    int *s_cur = s_start + BQG_CELLS + 1;
    unsigned short *s_sorted = (unsigned short *)(s_cur + BQG_CELLS);
    __shared__ float s_red[BQ_THREADS / 64][6];
    __shared__ float s_box[8];          // min x, y, z, 1 / cell edge; max x, y, z, cell edge
    __shared__ int s_dim[4];            // nx, ny, nz, cells
    __shared__ int s_wsum[BQ_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.y;
    const float *src = xyz + (size_t)(p % n_clouds) * N * 3;
    float mn0 = INFINITY, mn1 = INFINITY, mn2 = INFINITY, mx0 = -INFINITY, mx1 = -INFINITY, mx2 = -INFINITY;
    for (int i = tid; i < NP; i += BQ_THREADS) {
        float x = 0.f, y = 0.f, z = 0.f, q = INFINITY;
        if (i < N) {
            x = src[3 * i]; y = src[3 * i + 1]; z = src[3 * i + 2]; q = sumsq3(x, y, z);
            mn0 = fminf(mn0, x); mn1 = fminf(mn1, y); mn2 = fminf(mn2, z);
            mx0 = fmaxf(mx0, x); mx1 = fmaxf(mx1, y); mx2 = fmaxf(mx2, z);
        }
        s_x[i] = x; s_y[i] = y; s_z[i] = z; s_q[i] = q;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn0 = fminf(mn0, __shfl_xor(mn0, o)); mn1 = fminf(mn1, __shfl_xor(mn1, o)); mn2 = fminf(mn2, __shfl_xor(mn2, o));
        mx0 = fmaxf(mx0, __shfl_xor(mx0, o)); mx1 = fmaxf(mx1, __shfl_xor(mx1, o)); mx2 = fmaxf(mx2, __shfl_xor(mx2, o));
    }
    if (lane == 0) { s_red[wave][0] = mn0; s_red[wave][1] = mn1; s_red[wave][2] = mn2; s_red[wave][3] = mx0; s_red[wave][4] = mx1; s_red[wave][5] = mx2; }
    __syncthreads();
    if (tid == 0) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int w = 0; w < BQ_THREADS / 64; ++w)
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], s_red[w][a]); hi[a] = fmaxf(hi[a], s_red[w][3 + a]); }
        float maxabs = 0.0f;
        for (int a = 0; a < 3; ++a) maxabs = fmaxf(maxabs, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
        maxabs += sqrtf(r2);                                           // (a centroid that reaches the cloud is at most r outside its box)
        float edge = 1.05f * sqrtf(r2 + 1e-5f * maxabs * maxabs);
        const bool finite = maxabs < 1e18f;                            // (false for NaN and infinities)
        int nx, ny, nz;
        for (;;) {
            if (!finite) { nx = ny = nz = 1; edge = 1.0f; break; }
            nx = (int)((hi[0] - lo[0]) / edge) + 1; ny = (int)((hi[1] - lo[1]) / edge) + 1; nz = (int)((hi[2] - lo[2]) / edge) + 1;
            if ((long long)nx * ny * nz <= BQG_CELLS) break;
            edge *= 1.25f;
        }
        s_box[0] = lo[0]; s_box[1] = lo[1]; s_box[2] = lo[2]; s_box[3] = 1.0f / edge;
        s_box[4] = hi[0]; s_box[5] = hi[1]; s_box[6] = hi[2]; s_box[7] = edge;
        s_dim[0] = nx; s_dim[1] = ny; s_dim[2] = nz; s_dim[3] = nx * ny * nz;
    }
    __syncthreads();
    const float bx = s_box[0], by = s_box[1], bz = s_box[2], inv = s_box[3];
    const float hx = s_box[4], hy = s_box[5], hz = s_box[6], edge1 = s_box[7];
    const int nx = s_dim[0], ny = s_dim[1], nz = s_dim[2], ncell = s_dim[3];
    auto cell1 = [&](float v, float b, int n) {
        if (n == 1) return 0;
        const int c = (int)((v - b) * inv);
        return c < 0 ? 0 : (c >= n ? n - 1 : c);
    };
    for (int c = tid; c <= ncell; c += BQ_THREADS) s_start[c] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += BQ_THREADS)
        atomicAdd(&s_start[(cell1(s_z[i], bz, nz) * ny + cell1(s_y[i], by, ny)) * nx + cell1(s_x[i], bx, nx) + 1], 1);
    __syncthreads();
    {   // inclusive scan of s_start[1 .. ncell] in place (s_start[c + 1] = end of cell c): four cells per thread
        const int c0 = 1 + 4 * tid;
        int v[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) { v[u] = c0 + u <= ncell ? s_start[c0 + u] : 0; sum += v[u]; v[u] = sum; }
        const int inc = (int)bq_wave_incl_scan((unsigned)sum);
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        int base = inc - sum;
        for (int w = 0; w < wave; ++w) base += s_wsum[w];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c0 + u <= ncell) s_start[c0 + u] = base + v[u];
    }
    __syncthreads();
    for (int c = tid; c < ncell; c += BQ_THREADS) s_cur[c] = s_start[c];
    __syncthreads();
    for (int i = tid; i < N; i += BQ_THREADS) {
        const int cell = (cell1(s_z[i], bz, nz) * ny + cell1(s_y[i], by, ny)) * nx + cell1(s_x[i], bx, nx);
        s_sorted[atomicAdd(&s_cur[cell], 1)] = (unsigned short)i;
    }
    __syncthreads();
    // ---- queries: one wave per centroid; the cursors are dead, their memory holds the per-wave bitmaps
    const int words = NP >> 5;
    unsigned *bm = (unsigned *)s_cur + wave * words;
    const int c_end = min(S, (int)(blockIdx.x + 1) * BQG_CPB);
    for (int c = blockIdx.x * BQG_CPB + wave; c < c_end; c += BQ_THREADS / 64) {
        for (int w = lane; w < words; w += 64) bm[w] = 0u;
        const float *cp = new_xyz + ((size_t)p * S + c) * 3;
        const float cx = cp[0], cy = cp[1], cz = cp[2];
        const float csq = sumsq3(cx, cy, cz);
        const int ix = cell1(cx, bx, nx), iy = cell1(cy, by, ny), iz = cell1(cz, bz, nz);
        // the 9 runs of the sorted list: rows (iz + dz, iy + dy), cells ix - 1 .. ix + 1 (contiguous: x runs fastest)
        int start = 0, len = 0;
        // (written so that a NaN coordinate makes it true)
        const bool off_cloud = !(cx >= bx - edge1 && cx <= hx + edge1 && cy >= by - edge1 && cy <= hy + edge1 && cz >= bz - edge1 &&
                                 cz <= hz + edge1);
        if (off_cloud) {
            len = lane == 0 ? N : 0;      // one run: the whole sorted list = every point of the cloud
        } else if (lane < 9) {
            const int z = iz + lane / 3 - 1, y = iy + lane % 3 - 1;
            if (z >= 0 && z < nz && y >= 0 && y < ny) {
                const int x0 = ix > 0 ? ix - 1 : 0, x1 = ix + 1 < nx ? ix + 1 : nx - 1;
                const int lin = (z * ny + y) * nx + x0;
                start = s_start[lin];
                len = s_start[lin + (x1 - x0) + 1] - start;
            }
        }
        const int incl = (int)bq_wave_incl_scan((unsigned)len);
        const int T = __builtin_amdgcn_readlane(incl, 8);
        const int off = incl - len;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int i0 = 0; i0 < T; i0 += 64) {
            const int i = i0 + lane;
            int pos = -1;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int o = __builtin_amdgcn_readlane(off, r), l = __builtin_amdgcn_readlane(len, r),
                          st = __builtin_amdgcn_readlane(start, r);
                pos = (i >= o && i < o + l) ? st + (i - o) : pos;
            }
            if (pos >= 0) {
                const int j = s_sorted[pos];
                const float dd = sqdist(cx, cy, cz, csq, s_x[j], s_y[j], s_z[j], s_q[j]);
                if (!(dd > r2)) atomicOr(&bm[j >> 5], 1u << (j & 31));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the first K set bits, ascending; pad with the first hit (pointnet_util.py:104-106); an empty ball emits N
        int32_t *o = out + ((size_t)p * S + c) * K;
        int cnt = 0, first = N;
        for (int w0 = 0; w0 < words && cnt < K; w0 += 64) {
            unsigned word = w0 + lane < words ? bm[w0 + lane] : 0u;
            const int pc = __popc(word);
            const int inc = (int)bq_wave_incl_scan((unsigned)pc);
            const int tot = __builtin_amdgcn_readlane(inc, 63);
            if (tot == 0) continue;
            if (cnt == 0) {
                const int fl = __builtin_ctzll(__ballot(word != 0u));
                first = (w0 + fl) * 32 + __builtin_ctz((unsigned)__builtin_amdgcn_readlane((int)word, fl));
            }
            int rank = cnt + inc - pc;
            while (word && rank < K) {
                o[rank++] = (w0 + lane) * 32 + __builtin_ctz(word);
                word &= word - 1u;
            }
            cnt += tot;
        }
        for (int pos = min(cnt, K) + lane; pos < K; pos += 64) o[pos] = first;
        __builtin_amdgcn_wave_barrier();
    }
}
// ---------------------------------------------------------------------------------------------
// 3-NN: one thread per fine point, coarse cloud broadcast from LDS, top-3 kept in registers with
// strict '<' so equal distances keep the lower index first (stable ascending order).
// ---------------------------------------------------------------------------------------------
constexpr int NN_THREADS = 256;

// Two coarse points per step on the packed-fp32 pipe (v_pk_mul/fma/add_f32: two IEEE fp32 results per lane per
// instruction, each bit-identical to the scalar op): the coarse cloud is staged in LDS as pairs
// {x0,x1,y0,y1} {z0,z1,|p0|^2,|p1|^2}; an odd tail is padded with a point at infinite distance.
__global__ __launch_bounds__(NN_THREADS) void three_nn_kernel(const float *__restrict__ xyz1, int n_clouds1,
                                                              const float *__restrict__ xyz2, int N, int S,
                                                              int32_t *__restrict__ idx, float *__restrict__ w)
{
    extern __shared__ float4 s_pair[];  // [2 * ceil(S/2)]
    const int p = blockIdx.y;
    const float *c2 = xyz2 + (size_t)p * S * 3;
    const int S2 = (S + 1) >> 1;
    for (int i = threadIdx.x; i < S2; i += NN_THREADS) {
        const int a = 2 * i, b = 2 * i + 1;
        const float xa = c2[3 * a], ya = c2[3 * a + 1], za = c2[3 * a + 2];
        float xb = 0.f, yb = 0.f, zb = 0.f, sb = INFINITY;
        if (b < S) { xb = c2[3 * b]; yb = c2[3 * b + 1]; zb = c2[3 * b + 2]; sb = sumsq3(xb, yb, zb); }
        s_pair[2 * i] = make_float4(xa, xb, ya, yb);
        s_pair[2 * i + 1] = make_float4(za, zb, sumsq3(xa, ya, za), sb);
    }
    __syncthreads();
    const int i = blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= N) return;
    const float *fp = xyz1 + ((size_t)(p % n_clouds1) * N + i) * 3;
    const float fx = fp[0], fy = fp[1], fz = fp[2];
    const float fsq = sumsq3(fx, fy, fz);
    const v2f fx2 = {fx, fx}, fy2 = {fy, fy}, fz2 = {fz, fz}, fs2 = {fsq, fsq}, m2 = {-2.0f, -2.0f};
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int jj = 0; jj < S2; ++jj) {
        const float4 q0 = s_pair[2 * jj], q1 = s_pair[2 * jj + 1];
        const v2f qx = {q0.x, q0.y}, qy = {q0.z, q0.w}, qz = {q1.x, q1.y}, qs = {q1.z, q1.w};
        // square_distance order: ((-2 * (fma chain over x, y, z)) + |fine|^2) + |coarse|^2
        v2f dot = fx2 * qx;
        dot = __builtin_elementwise_fma(fy2, qy, dot);
        dot = __builtin_elementwise_fma(fz2, qz, dot);
        const v2f dd = ((m2 * dot) + fs2) + qs;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float d = dd[u];
            const int j = 2 * jj + u;
            if (d < d2) {
                if (d < d1) {
                    d2 = d1; i2 = i1;
                    if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = j; }
                    else { d1 = d; i1 = j; }
                } else { d2 = d; i2 = j; }
            }
        }
    }
    float r0 = __fdiv_rn(1.0f, __fadd_rn(d0, 1e-8f));
    float r1 = __fdiv_rn(1.0f, __fadd_rn(d1, 1e-8f));
    float r2 = __fdiv_rn(1.0f, __fadd_rn(d2, 1e-8f));
    float norm = __fadd_rn(__fadd_rn(r0, r1), r2);
    size_t o = ((size_t)p * N + i) * 3;
    idx[o] = i0; idx[o + 1] = i1; idx[o + 2] = i2;
    w[o] = __fdiv_rn(r0, norm); w[o + 1] = __fdiv_rn(r1, norm); w[o + 2] = __fdiv_rn(r2, norm);
}

// ---------------------------------------------------------------------------------------------
// 3-NN through a uniform grid over the COARSE cloud (round 29), for the level-0 shape (4096 fine points against 1024
// coarse ones: the scan above tests every pair, 10.7 G of them per plan of 2560 problems, and is vector-issue-bound).  The
// three nearest of the ~evenly spread FPS samples lie a few centimetres away: a few dozen candidates instead of S.
// Per workgroup: the coarse cloud is staged with |p|^2, its bounding box reduced, the points binned by an LDS counting
// sort as in ball_query_grid_kernel (the sorted copy holds {x, y, z, |p|^2} so that a run of cells is a contiguous read);
// there is no radius here, so the cell edge is free: cbrt(NNG_PPC x box volume / S), i.e. about NNG_PPC points per cell
// of a volume-filling cloud (a flat axis counts as 1/64 of the longest), grown by 1.25 x until the box fits NNG_CELLS.
// One LANE per fine point then looks outward from its own cell - the 3 x 3 x 3 block first, then the shell around it, and so
// on - keeping its best three as keys (d, j):
//   * d is three_nn_kernel's arithmetic, operation for operation (sqdist: fma chain, (-2 dot + |fine|^2) + |coarse|^2);
//   * the order is d ascending, then j ascending - what the scan's strict `<` over ascending j produces; the grid meets
//     candidates in cell order, so the tie rule is explicit; the slots start as (inf, 0) and a candidate whose d is +inf or NaN
//     never enters, as in the scan;
//   * after a block / shell: L = distance from the query to the nearest face of what is not yet visited (faces beyond the
//     border cells do not count: there is nothing behind them), less NNG_SLACK x max|coordinate| for the rounding of the
//     cell index and of the face position.  An unvisited point is at least L away, and its COMPUTED d is at least
//     L^2 - err, err = 1e-5 max|coordinate|^2 (the expansion's rounding is below 2.4e-7 (|f| + |c|)^2 <= 3e-6
//     max|coordinate|^2, query included: the ball grid's bound and its factor).  The walk stops only when L^2 - err is
//     STRICTLY above the third-best d: a candidate that would tie the third best with a lower j is never skipped.  A
//     walk that reaches every cell is the scan;
//   * a query that is non-finite or further outside the coarse box than the grid is long, and every query of a problem
//     whose coarse cloud holds a non-finite coordinate (no grid is built), takes all S candidates in ascending j through
//     the scan's own compare chain.
// Schedule.  Lanes that walk by themselves pay for each other: per candidate the wave runs the run-advance and the insert of
// its slowest lane, ~100 instructions against the scan's 8, and the first version of this kernel (one lane, one walk, queries
// in file order) was SLOWER than the scan (3.42 against 2.07 ms per 2560 problems).  So the workgroup also sorts its queries by
// cell of the same grid (a second counting sort, inside the launch, from the buffers passed in: nothing is kept across
// calls), a wave takes 64 queries that are neighbours in that order, and the first step is taken TOGETHER: every cell of the
// box around the wave's blocks - a superset of each lane's own block, which is as good for the stop rule - with wave-uniform
// run bounds and candidates (LDS broadcasts, scalar loop control, four candidates per step, the index read only when d can
// enter): ~146 candidates per query instead of 37, at a tenth of the cost each.  A lane whose stop rule fails after that step
// (0.1 % of the lanes of a room) starts over and walks by itself, block and shells, as described above.
// Same idx and w as three_nn_kernel, byte for byte (tests/test_gpu_three_nn_grid.py; the walk, the schedule and the stop rule
// restated in numpy: tests/three_nn_grid_ref.py, tests/test_three_nn_grid_host.py).
// ---------------------------------------------------------------------------------------------
constexpr int NNG_THREADS = 512;         // 8 waves: three workgroups per CU at 7 waves per SIMD and 51 KiB of LDS each
constexpr int NNG_CELLS = 2 * NNG_THREADS;   // cells per coarse cloud at most (the scan of the cell counts takes two per thread)
constexpr int NNG_MAX_S = 1024;        // LDS: 34 B per coarse point, 8 KiB of cell tables, 2 B per query: 50 KiB at level 0
constexpr float NNG_PPC = 2.0f;        // coarse points per cell the edge aims at (tools/three_nn_probe.py; DESIGN round 29)
constexpr float NNG_ERR = 1e-5f;       // x max|coordinate|^2: rounding of the expansion
constexpr float NNG_SLACK = 4e-6f;     // x max|coordinate|: rounding of cell index and face position

__device__ __forceinline__ int nn_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float nn_uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ bool nn_before(float d, int j, float bd, int bj) { return d < bd || (d == bd && j < bj); }

__global__ __launch_bounds__(NNG_THREADS) void three_nn_grid_kernel(const float *__restrict__ xyz1, int n_clouds1,
                                                                    const float *__restrict__ xyz2, int N, int S, int qpb,
                                                                    int32_t *__restrict__ idx, float *__restrict__ w)
{
    // file order [S] | cell order [S] | cell starts [CELLS + 1] | cursors [CELLS + 1] | j in cell order [S] u16 | queries in cell order [qpb] u16
    extern __shared__ float4 s_pt[];
    float4 *s_sp = s_pt + S;
    int *s_start = (int *)(s_sp + S);
    int *s_cur = s_start + NNG_CELLS + 1;
    unsigned short *s_sj = (unsigned short *)(s_cur + NNG_CELLS + 1);
    unsigned short *s_qs = s_sj + S;
    __shared__ float s_red[NNG_THREADS / 64][6];
    __shared__ float s_box[8];          // min x, y, z, 1 / cell edge; max x, y, z, cell edge
    __shared__ int s_dim[4];            // nx, ny, nz, cells
    __shared__ int s_wsum[NNG_THREADS / 64];
    __shared__ int s_bad;               // the coarse cloud holds a non-finite coordinate
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.y;
    const float *c2 = xyz2 + (size_t)p * S * 3;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    float mn0 = INFINITY, mn1 = INFINITY, mn2 = INFINITY, mx0 = -INFINITY, mx1 = -INFINITY, mx2 = -INFINITY;
    bool bad = false;
    for (int i = tid; i < S; i += NNG_THREADS) {
        const float x = c2[3 * i], y = c2[3 * i + 1], z = c2[3 * i + 2];
        s_pt[i] = make_float4(x, y, z, sumsq3(x, y, z));
        mn0 = fminf(mn0, x); mn1 = fminf(mn1, y); mn2 = fminf(mn2, z);
        mx0 = fmaxf(mx0, x); mx1 = fmaxf(mx1, y); mx2 = fmaxf(mx2, z);
        bad = bad || !(fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z)) < 1e18f) || x != x || y != y || z != z;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn0 = fminf(mn0, __shfl_xor(mn0, o)); mn1 = fminf(mn1, __shfl_xor(mn1, o)); mn2 = fminf(mn2, __shfl_xor(mn2, o));
        mx0 = fmaxf(mx0, __shfl_xor(mx0, o)); mx1 = fmaxf(mx1, __shfl_xor(mx1, o)); mx2 = fmaxf(mx2, __shfl_xor(mx2, o));
    }
    if (lane == 0) { s_red[wave][0] = mn0; s_red[wave][1] = mn1; s_red[wave][2] = mn2; s_red[wave][3] = mx0; s_red[wave][4] = mx1; s_red[wave][5] = mx2; }
    if (bad) s_bad = 1;
    __syncthreads();
    const bool scan_all = nn_uni(s_bad) != 0;   // (uniform over the workgroup)
    float bx = 0.f, by = 0.f, bz = 0.f, inv = 1.f, hx = 0.f, hy = 0.f, hz = 0.f, edge = 1.f;
    int nx = 1, ny = 1, nz = 1;
    if (!scan_all) {
        if (tid == 0) {
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int wv = 0; wv < NNG_THREADS / 64; ++wv) {
#pragma unroll
                for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], s_red[wv][a]); hi[a] = fmaxf(hi[a], s_red[wv][3 + a]); }
            }
            const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
            const float emax = fmaxf(ex, fmaxf(ey, ez));
            float e = 1.0f;
            int dx = 1, dy = 1, dz = 1;
            if (emax > 0.0f) {                                         // (all points identical: one cell)
                const float fl = emax * (1.0f / 64.0f);
                e = cbrtf(fmaxf(ex, fl) * fmaxf(ey, fl) * fmaxf(ez, fl) * (NNG_PPC / (float)S));
                for (;;) {
                    dx = (int)(ex / e) + 1; dy = (int)(ey / e) + 1; dz = (int)(ez / e) + 1;
                    if ((long long)dx * dy * dz <= NNG_CELLS) break;
                    e *= 1.25f;
                }
            }
            s_box[0] = lo[0]; s_box[1] = lo[1]; s_box[2] = lo[2]; s_box[3] = 1.0f / e;
            s_box[4] = hi[0]; s_box[5] = hi[1]; s_box[6] = hi[2]; s_box[7] = e;
            s_dim[0] = dx; s_dim[1] = dy; s_dim[2] = dz; s_dim[3] = dx * dy * dz;
        }
        __syncthreads();
        // (workgroup-uniform: kept in scalar registers)
        bx = nn_uni(s_box[0]); by = nn_uni(s_box[1]); bz = nn_uni(s_box[2]); inv = nn_uni(s_box[3]);
        hx = nn_uni(s_box[4]); hy = nn_uni(s_box[5]); hz = nn_uni(s_box[6]); edge = nn_uni(s_box[7]);
        nx = nn_uni(s_dim[0]); ny = nn_uni(s_dim[1]); nz = nn_uni(s_dim[2]);
    }
    const int ncell = nx * ny * nz;
    // the cell of a coordinate: clamped in float (a NaN becomes 0), then truncated - monotone in v
    auto cell1 = [&](float v, float b, int n) { return (int)fminf(fmaxf((v - b) * inv, 0.0f), (float)(n - 1)); };
    // inclusive scan of a[1 .. ncell] in place over the workgroup (counts -> a[c] = start of cell c, a[0] = 0): two cells per thread
    auto scan_counts = [&](int *a) {
        const int c0 = 1 + 2 * tid;
        const int v0 = c0 <= ncell ? a[c0] : 0, v1 = c0 + 1 <= ncell ? a[c0 + 1] : 0;
        const int inc = (int)bq_wave_incl_scan((unsigned)(v0 + v1));
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        int base = inc;
        for (int wv = 0; wv < wave; ++wv) base += s_wsum[wv];
        if (c0 <= ncell) a[c0] = base - v1;
        if (c0 + 1 <= ncell) a[c0 + 1] = base;
        __syncthreads();
    };
    const float *f1 = xyz1 + (size_t)(p % n_clouds1) * N * 3;
    const int q_begin = blockIdx.x * qpb, nq = min(N, q_begin + qpb) - q_begin;
    auto cell_of = [&](float x, float y, float z) { return (cell1(z, bz, nz) * ny + cell1(y, by, ny)) * nx + cell1(x, bx, nx); };
    if (!scan_all) {
        for (int c = tid; c <= ncell; c += NNG_THREADS) s_start[c] = 0;
        __syncthreads();
        for (int i = tid; i < S; i += NNG_THREADS) {
            const float4 q = s_pt[i];
            atomicAdd(&s_start[cell_of(q.x, q.y, q.z) + 1], 1);
        }
        __syncthreads();
        scan_counts(s_start);
        for (int c = tid; c <= ncell; c += NNG_THREADS) s_cur[c] = c < ncell ? s_start[c] : 0;
        __syncthreads();
        for (int i = tid; i < S; i += NNG_THREADS) {
            const float4 q = s_pt[i];
            const int pos = atomicAdd(&s_cur[cell_of(q.x, q.y, q.z)], 1);
            s_sp[pos] = q;
            s_sj[pos] = (unsigned short)i;
        }
        __syncthreads();
        // the workgroup's queries in cell order of the same grid (a query outside the box goes to the border cell, a NaN to 0)
        for (int c = tid; c <= ncell; c += NNG_THREADS) s_cur[c] = 0;
        __syncthreads();
        for (int t = tid; t < nq; t += NNG_THREADS) {
            const float *fp = f1 + (size_t)(q_begin + t) * 3;
            atomicAdd(&s_cur[cell_of(fp[0], fp[1], fp[2]) + 1], 1);
        }
        __syncthreads();
        scan_counts(s_cur);
        for (int t = tid; t < nq; t += NNG_THREADS) {
            const float *fp = f1 + (size_t)(q_begin + t) * 3;
            s_qs[atomicAdd(&s_cur[cell_of(fp[0], fp[1], fp[2])], 1)] = (unsigned short)t;
        }
    }
    __syncthreads();
    const float span = (float)max(nx, max(ny, nz)) * edge;
    const float box_abs = fmaxf(fmaxf(fmaxf(fabsf(bx), fabsf(by)), fabsf(bz)), fmaxf(fmaxf(fabsf(hx), fabsf(hy)), fabsf(hz)));
    // a wave serves 64 queries that are neighbours in cell order
    for (int g = wave; g * 64 < nq; g += NNG_THREADS / 64) {
        const int t = g * 64 + lane;
        const bool live = t < nq;
        const int i = q_begin + (live ? (scan_all ? t : (int)s_qs[t]) : 0);
        const float *fp = f1 + (size_t)i * 3;
        const float fx = fp[0], fy = fp[1], fz = fp[2];
        const float fsq = sumsq3(fx, fy, fz);
        float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
        int i0 = 0, i1 = 0, i2 = 0;
        auto take = [&](float d, int j) {       // (d, j) into the best three, which stay ordered by d, then j
            if (nn_before(d, j, d2, i2)) {      // (selects, not nested branches: before slot 0 implies before slot 1)
                const bool b1 = nn_before(d, j, d1, i1), b0 = nn_before(d, j, d0, i0);
                d2 = b1 ? d1 : d; i2 = b1 ? i1 : j;
                d1 = b0 ? d0 : (b1 ? d : d1); i1 = b0 ? i0 : (b1 ? j : i1);
                d0 = b0 ? d : d0; i0 = b0 ? j : i0;
            }
        };
        auto cand = [&](int pos) {
            const float4 q = s_sp[pos];
            take(sqdist(fx, fy, fz, fsq, q.x, q.y, q.z, q.w), (int)s_sj[pos]);
        };
        // (written so that a NaN coordinate makes it true)
        const bool far = scan_all || !(fx >= bx - span && fx <= hx + span && fy >= by - span && fy <= hy + span &&
                                       fz >= bz - span && fz <= hz + span);
        const bool walks = live && !far;
        const int cx = cell1(fx, bx, nx), cy = cell1(fy, by, ny), cz = cell1(fz, bz, nz);
        const float maxabs = fmaxf(box_abs, fmaxf(fmaxf(fabsf(fx), fabsf(fy)), fabsf(fz)));
        const float err = NNG_ERR * (maxabs * maxabs), slack = NNG_SLACK * maxabs;
        // after the cells [c - k, c + k]^3: may the walk stop?
        auto done = [&](int k) {
            float L = INFINITY;                 // nearest face of what is not visited
            if (cx - k > 0) L = fminf(L, fx - (bx + (float)(cx - k) * edge));
            if (cx + k < nx - 1) L = fminf(L, (bx + (float)(cx + k + 1) * edge) - fx);
            if (cy - k > 0) L = fminf(L, fy - (by + (float)(cy - k) * edge));
            if (cy + k < ny - 1) L = fminf(L, (by + (float)(cy + k + 1) * edge) - fy);
            if (cz - k > 0) L = fminf(L, fz - (bz + (float)(cz - k) * edge));
            if (cz + k < nz - 1) L = fminf(L, (bz + (float)(cz + k + 1) * edge) - fz);
            if (L == INFINITY) return true;     // every cell visited
            const float Ls = L - slack;
            return Ls > 0.0f && Ls * Ls - err > d2;
        };
        bool alone = false;                     // this lane's walk goes on beyond what the wave visited together
        if (__any(walks)) {
            // together: every cell of the box around the wave's 3 x 3 x 3 blocks, a superset of each lane's own block; the run
            // bounds and the candidates are wave-uniform (LDS broadcasts), a candidate costs what it costs in the scan
            int x0 = walks ? cx : nx, x1 = walks ? cx : -1, y0 = walks ? cy : ny, y1 = walks ? cy : -1, z0 = walks ? cz : nz, z1 = walks ? cz : -1;
            for (int o = 32; o > 0; o >>= 1) {
                x0 = min(x0, __shfl_xor(x0, o)); y0 = min(y0, __shfl_xor(y0, o)); z0 = min(z0, __shfl_xor(z0, o));
                x1 = max(x1, __shfl_xor(x1, o)); y1 = max(y1, __shfl_xor(y1, o)); z1 = max(z1, __shfl_xor(z1, o));
            }
            x0 = max(__builtin_amdgcn_readfirstlane(x0) - 1, 0); x1 = min(__builtin_amdgcn_readfirstlane(x1) + 1, nx - 1);
            y0 = max(__builtin_amdgcn_readfirstlane(y0) - 1, 0); y1 = min(__builtin_amdgcn_readfirstlane(y1) + 1, ny - 1);
            z0 = max(__builtin_amdgcn_readfirstlane(z0) - 1, 0); z1 = min(__builtin_amdgcn_readfirstlane(z1) + 1, nz - 1);
            // rows that follow each other in the sorted list (the box spans all of x, or all of x and y) are one run; four
            // candidates per step, and the index of a candidate is read only when its d can enter the best three
            const bool all_x = x0 == 0 && x1 == nx - 1;
            const int ys = all_x ? y1 - y0 + 1 : 1;
            const int zs = all_x && ys == ny ? z1 - z0 + 1 : 1;
            if (walks) {
                for (int z = z0; z <= z1; z += zs)
                    for (int y = y0; y <= y1; y += ys) {
                        const int end = nn_uni(s_start[((z + zs - 1) * ny + (y + ys - 1)) * nx + x1 + 1]);
                        for (int pos = nn_uni(s_start[(z * ny + y) * nx + x0]); pos < end; pos += 4) {
                            float d[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const float4 q = s_sp[min(pos + u, S - 1)];
                                d[u] = sqdist(fx, fy, fz, fsq, q.x, q.y, q.z, q.w);
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (pos + u < end && d[u] <= d2) take(d[u], (int)s_sj[pos + u]);
                        }
                    }
            }
            alone = walks && !done(1);
        }
        if (alone) {
            // rare (the third best lies beyond this lane's own block): the lane starts over and walks by itself, its own block
            // as one loop over the candidates of its 9 runs, then shell by shell
            d0 = d1 = d2 = INFINITY; i0 = i1 = i2 = 0;
            {
                const int x0 = max(cx - 1, 0), xn = min(cx + 1, nx - 1) - x0 + 1;
                int r = 0, pos = 0, end = 0;
                for (;;) {
                    while (pos >= end && r < 9) {
                        const int rz = (r * 11) >> 5;                  // r / 3 for r < 9
                        const int z = cz + rz - 1, y = cy + (r - 3 * rz) - 1;
                        if (z >= 0 && z < nz && y >= 0 && y < ny) {
                            const int lin = (z * ny + y) * nx + x0;
                            pos = s_start[lin]; end = s_start[lin + xn];
                        }
                        ++r;
                    }
                    if (pos >= end) break;
                    cand(pos++);
                }
            }
            for (int k = 1; !done(k); ++k) {
                // shell k + 1: full x runs in its top / bottom / front / back rows, the two end cells in the others
                const int kk = k + 1;
                for (int z = max(cz - kk, 0); z <= min(cz + kk, nz - 1); ++z)
                    for (int y = max(cy - kk, 0); y <= min(cy + kk, ny - 1); ++y) {
                        const int row = (z * ny + y) * nx;
                        const bool rim = z - cz == kk || cz - z == kk || y - cy == kk || cy - y == kk;
                        if (rim) {
                            const int end = s_start[row + min(cx + kk, nx - 1) + 1];
                            for (int pos = s_start[row + max(cx - kk, 0)]; pos < end; ++pos) cand(pos);
                        } else {
                            if (cx - kk >= 0) { const int end = s_start[row + cx - kk + 1]; for (int pos = s_start[row + cx - kk]; pos < end; ++pos) cand(pos); }
                            if (cx + kk < nx) { const int end = s_start[row + cx + kk + 1]; for (int pos = s_start[row + cx + kk]; pos < end; ++pos) cand(pos); }
                        }
                    }
            }
        }
        if (live && far) {
            for (int j = 0; j < S; ++j) {       // the scan: ascending j, strict `<`
                const float4 q = s_pt[j];
                const float d = sqdist(fx, fy, fz, fsq, q.x, q.y, q.z, q.w);
                if (d < d2) {
                    if (d < d1) {
                        d2 = d1; i2 = i1;
                        if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = j; }
                        else { d1 = d; i1 = j; }
                    } else { d2 = d; i2 = j; }
                }
            }
        }
        if (live) {
            float r0 = __fdiv_rn(1.0f, __fadd_rn(d0, 1e-8f));
            float r1 = __fdiv_rn(1.0f, __fadd_rn(d1, 1e-8f));
            float r2 = __fdiv_rn(1.0f, __fadd_rn(d2, 1e-8f));
            float norm = __fadd_rn(__fadd_rn(r0, r1), r2);
            size_t o = ((size_t)p * N + i) * 3;
            idx[o] = i0; idx[o + 1] = i1; idx[o + 2] = i2;
            w[o] = __fdiv_rn(r0, norm); w[o + 1] = __fdiv_rn(r1, norm); w[o + 2] = __fdiv_rn(r2, norm);
        }
    }
}

// square_distance(src, dst) materialised (public helper of pointnet_util; not on the attack path)
__global__ void square_distance_kernel(const float *__restrict__ src, const float *__restrict__ dst, int N, int M,
                                       float *__restrict__ out)
{
    const int b = blockIdx.z;
    const int i = blockIdx.y;
    const float *s = src + ((size_t)b * N + i) * 3;
    const float sx = s[0], sy = s[1], sz = s[2];
    const float ssq = sumsq3(sx, sy, sz);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < M; j += gridDim.x * blockDim.x) {
        const float *d = dst + ((size_t)b * M + j) * 3;
        out[((size_t)b * N + i) * M + j] = sqdist(sx, sy, sz, ssq, d[0], d[1], d[2], sumsq3(d[0], d[1], d[2]));
    }
}

template <int NT, int PPT, bool LDSC = true>
int launch_fps(const float *xyz, int n_clouds, int P, int N, int S, const int32_t *start, int32_t *out,
               hipStream_t st)
{
    size_t lds = (LDSC ? (size_t)NT * PPT * 3 * 4 : 0) + 2 * (NT / 64) * 8;
    if (lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)fps_kernel<NT, PPT, LDSC>));
    hipLaunchKernelGGL((fps_kernel<NT, PPT, LDSC>), dim3(P), dim3(NT), lds, st, xyz, n_clouds, N, S, start, out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

}  // namespace

extern "C" int psg_fps(psg_ctx *ctx, const float *xyz, int n_clouds, int P, int N, int S, const int32_t *start,
                       int32_t *out_idx, psg_stream stream)
{
    PSG_REQUIRE(ctx && xyz && start && out_idx, "psg_fps: null argument");
    PSG_REQUIRE(P > 0 && n_clouds > 0 && N > 0 && S > 0 && S <= N, "psg_fps: bad sizes P=%d N=%d S=%d", P, N, S);
    PSG_REQUIRE(N <= 8192, "psg_fps: N=%d exceeds the LDS-resident limit 8192", N);
    hipStream_t st = (hipStream_t)stream;
    if (N <= 64) return launch_fps<64, 1>(xyz, n_clouds, P, N, S, start, out_idx, st);
    if (N <= 256) return launch_fps<64, 4>(xyz, n_clouds, P, N, S, start, out_idx, st);
    if (N <= 1024) return launch_fps<256, 4>(xyz, n_clouds, P, N, S, start, out_idx, st);
    // few problems (up to one per CU): the latency of a step is what counts, and 512 threads x 8 points has it.  More (a whole
    // attack plan: iterations x rooms): throughput counts; 256 threads x 16 points needs a 4-wave instead of an 8- or 16-wave
    // reduction per step, and without the 48 KiB cloud in LDS (the centroid of a step comes from global memory by scalar loads;
    // the level-0 cloud of a room is shared by all its forwards and sits in L2) seven problems instead of three are resident per
    // CU.  tools/fps_cfg_probe.py on MI355X, microseconds per 4096 -> 1024 call,
    //                 1024 x 4   512 x 8   256 x 16   256 x 16, no LDS cloud   512 x 8, no LDS cloud
    //    1 problem       548        547       580             638                     575
    //  128               573        557       579             627                     589
    //  256               597        578       596             649                     608
    //  320               875        814       769             754                     821
    //  640              1307       1086      1051            1048                    1116
    // 1280              2077       1913      1690            1570                    1754
    // 2560              3869       3185      3054            2756                    3148
    // (with the step loop of before - compare + select per point, in-lane index tracking - the first three columns were
    // 693 / 680 / 737 at 1 problem, 1193 / 1023 / 989 at 320 and 5353 / 4126 / 3804 at 2560)
    // measurement switch: 1 = 1024 x 4, 2 = 512 x 8, 3 = 256 x 16, 4 = 256 x 16 and 5 = 512 x 8 without the cloud in LDS
    static const int cfg = psg::env_int("PSG_FPS_CFG", 0);
    if (N <= 4096 && cfg == 1) return launch_fps<1024, 4>(xyz, n_clouds, P, N, S, start, out_idx, st);
    if (N <= 4096 && cfg == 3) return launch_fps<256, 16>(xyz, n_clouds, P, N, S, start, out_idx, st);
    if (N <= 4096 && cfg == 5) return launch_fps<512, 8, false>(xyz, n_clouds, P, N, S, start, out_idx, st);
    if (N <= 4096 && (cfg == 4 || (cfg == 0 && P > 256))) return launch_fps<256, 16, false>(xyz, n_clouds, P, N, S, start, out_idx, st);
    if (N <= 4096) return launch_fps<512, 8>(xyz, n_clouds, P, N, S, start, out_idx, st);
    return launch_fps<1024, 8>(xyz, n_clouds, P, N, S, start, out_idx, st);
}

extern "C" int psg_square_distance(psg_ctx *ctx, const float *src, const float *dst, int B, int N, int M, float *out,
                                   psg_stream stream)
{
    PSG_REQUIRE(ctx && src && dst && out, "psg_square_distance: null argument");
    PSG_REQUIRE(B > 0 && N > 0 && M > 0 && N <= 65535 && B <= 65535, "psg_square_distance: bad sizes");
    hipLaunchKernelGGL(square_distance_kernel, dim3(std::min(64, psg::ceil_div(M, 256)), N, B), dim3(256), 0,
                       (hipStream_t)stream, src, dst, N, M, out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_gather_points(psg_ctx *ctx, const float *points, int n_clouds, int P, int N, int C,
                                 const int32_t *idx, int S, float *out, psg_stream stream)
{
    PSG_REQUIRE(ctx && points && idx && out, "psg_gather_points: null argument");
    PSG_REQUIRE(P > 0 && n_clouds > 0 && N > 0 && C > 0 && S > 0, "psg_gather_points: bad sizes");
    size_t total = (size_t)P * S * C;
    int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, points, n_clouds, N, C,
                       idx, S, out, P);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_ball_query(psg_ctx *ctx, const float *xyz, int n_clouds, const float *new_xyz, int P, int N,
                              int S, float r2, int K, int32_t *out_idx, psg_stream stream)
{
    PSG_REQUIRE(ctx && xyz && new_xyz && out_idx, "psg_ball_query: null argument");
    PSG_REQUIRE(P > 0 && n_clouds > 0 && N > 0 && S > 0 && K > 0, "psg_ball_query: bad sizes");
    PSG_REQUIRE(N <= 8192, "psg_ball_query: N=%d exceeds the LDS-resident limit 8192", N);
    // Clouds of 2048 .. 4096 points: the grid kernel (same indices; see its header).  Measured per launch of 2560 problems
    // (tools/ball_query_probe.py): N = 4096, S = 1024: 1.44 ms against 2.87 ms for the scan; N = 1024, S = 256: 0.29 against
    // 0.27 (the build is not repaid), so smaller clouds keep the scan.  PSG_BALL_QUERY=scan forces the scan (A/B runs).
    static const bool scan_only = []() { const char *v = psg::env_str("PSG_BALL_QUERY"); return v && std::string(v) == "scan"; }();
    const size_t soa = (size_t)((N + 255) & ~255) * 4 * sizeof(float);
    if (!scan_only && N >= 2048 && N <= 4096 && r2 > 0.0f && r2 < 1e30f) {
        const size_t lds = soa + (size_t)(2 * BQG_CELLS + 1) * 4 + (size_t)((N + 255) & ~255) * 2;
        if (lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)ball_query_grid_kernel));
        hipLaunchKernelGGL(ball_query_grid_kernel, dim3(psg::ceil_div(S, BQG_CPB), P), dim3(BQ_THREADS), lds, (hipStream_t)stream, xyz,
                           n_clouds, new_xyz, N, S, r2, K, out_idx);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    if (soa > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)ball_query_kernel));
    hipLaunchKernelGGL(ball_query_kernel, dim3(psg::ceil_div(S, BQ_CPB), P), dim3(BQ_THREADS), soa,
                       (hipStream_t)stream, xyz, n_clouds, new_xyz, N, S, r2, K, out_idx);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_three_nn(psg_ctx *ctx, const float *xyz1, int n_clouds1, const float *xyz2, int P, int N, int S,
                            int32_t *out_idx, float *out_w, psg_stream stream)
{
    PSG_REQUIRE(ctx && xyz1 && xyz2 && out_idx && out_w, "psg_three_nn: null argument");
    PSG_REQUIRE(P > 0 && n_clouds1 > 0 && N > 0 && S >= 3, "psg_three_nn: bad sizes (need S >= 3)");
    PSG_REQUIRE(S <= 8192, "psg_three_nn: S=%d exceeds the LDS-resident limit 8192", S);
    // PSG_THREE_NN=scan forces the scan, =grid the grid kernel wherever its LDS layout fits (A/B runs, tests); unset: the grid
    // kernel at the level-0 shape of a plan.  tools/three_nn_probe.py on MI355X, ms per launch, scan / grid:
    //                  2560 problems    320 problems    8 problems
    //   4096 x 1024    2.07 / 1.08      0.32 / 0.26     0.078 / 0.098
    //   1024 x  256    0.22 / 0.25      0.039 / 0.080   0.027 / 0.058
    //    256 x   64    0.024 / 0.107    0.010 / 0.042   0.009 / 0.036
    // (the build and the sort of the queries cost a workgroup ~30 us before its first candidate: not repaid below level 0, and
    // not with eight problems; between 8 and 320 problems nothing was measured, so the scan stays there)
    static const int mode = []() {
        const char *v = psg::env_str("PSG_THREE_NN");
        return !v ? 0 : std::string(v) == "scan" ? 1 : std::string(v) == "grid" ? 2 : 0;
    }();
    if (S <= NNG_MAX_S && (mode == 2 || (mode == 0 && N >= 2048 && S >= 512 && P >= 320))) {
        // a workgroup serves all queries of a problem (one grid build per problem) once there are problems enough to fill the
        // device, else 1024 of them
        const int qpb = (size_t)P * psg::ceil_div(N, 1024) > 2048 ? 4096 : 1024;
        const size_t glds = (size_t)S * (2 * sizeof(float4) + 2) + (size_t)(2 * NNG_CELLS + 2) * 4 + (size_t)qpb * 2;
        if (glds + 1024 > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)three_nn_grid_kernel));
        hipLaunchKernelGGL(three_nn_grid_kernel, dim3(psg::ceil_div(N, qpb), P), dim3(NNG_THREADS), glds, (hipStream_t)stream,
                           xyz1, n_clouds1, xyz2, N, S, qpb, out_idx, out_w);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    size_t lds = (size_t)2 * ((S + 1) / 2) * sizeof(float4);
    if (lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)three_nn_kernel));
    hipLaunchKernelGGL(three_nn_kernel, dim3(psg::ceil_div(N, NN_THREADS), P), dim3(NN_THREADS), lds,
                       (hipStream_t)stream, xyz1, n_clouds1, xyz2, N, S, out_idx, out_w);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}
