// Grid sub-sampling and sub-cloud projection of the RandLA-Net data preparation on the device.
//
// A. Reference: DataProcessing.grid_sub_sampling (RandLA-Net/helper_tool.py:197-216) over utils/cpp_wrappers/cpp_subsampling
// (grid_subsampling.cpp:5-106): a raw cloud of N points is binned into cubic cells of edge dl; every occupied cell gives one
// output point, the barycentre of its members, with their mean feature and their most frequent label.  The reference fills an
// unordered_map cell -> running sums in ONE pass over the points, so a cell's sums are sequential fp32 additions in input
// order, and that order decides the output's bits.  Here:
//   minmax_kernel   min / max corner (integer atomics on order-preserving bit patterns: exact) and a non-finite flag
//   (host)          origin = floor(min * (1 / dl)) * dl and the grid's NX, NY, NZ in fp32, after ONE read-back of 28 bytes;
//                   the refusals (non-finite coordinates, more than 2^20 cells along an axis) are made here, before any result
//   keys_kernel     key = iX + NX * iY + NX * NY * iZ (64 bits), i = floor((p - origin) / dl) clamped at 0
//   hipcub radix sort of (key, point index) over the bits of NX * NY * NZ: stable, so a cell's members stay in input order
//   heads_kernel + hipcub inclusive scan   rank of every sorted position's cell among the occupied cells = its output row
//   segments_kernel seg_start [M + 1] and voxel_of_point [N]; M is read back here (the second and last read-back: it sizes
//                   the caller's outputs)
//   sums_kernel     one thread per (cell, channel): a sequential fp32 accumulator over the cell's members in input order;
//                   barycentre = sum * (float)(1.0 / count), mean feature = sum / (float)count.  No float atomics, no tree.
//   label_keys_kernel + radix sort of (rank << 32 | label with the sign bit flipped) + vote_kernel   per label dimension: run
//                   lengths over the cell's sorted labels, the first longest run wins = the smallest label among the most
//                   frequent ones.  Linear in a cell's population.
// Output order: ascending key.  (The reference's order is the iteration order of its hash map, its label ties go to whichever
// maximum that order meets first, and a cell index of -1 - origin can exceed the minimum by a rounding - is undefined there.)
//
// B. proj_idx of utils/data_prepare_s3dis.py (KDTree(sub_xyz).query(xyz, k = 1)): the nearest sub-point of every raw point,
// with psg_knn_points' arithmetic and tie rule, through a cell table in place of a scan of all M sub-points.  The sub-points
// are binned by THEIR OWN coordinates with A's key formula (a barycentre may round to just outside the cell it was averaged
// in; the cell edge is grid_size, doubled while the grid has more than 64 cells per sub-point) and sorted by key; a row of cells
// iX0..iX1 at fixed (iY, iZ) is one contiguous key interval, found by one binary search.
// A query searches the Chebyshev rings around its (clamped) cell until its best squared distance is provably below that of
// every point outside the searched block; DESIGN.md (the grid section) derives the bound and its fp32 margin.
#include <hipcub/hipcub.hpp>

#include "psg_common.h"

using namespace psg;

typedef unsigned long long u64;

namespace {

constexpr int GRID_MAX_AXIS = 1 << 20;      // cells along one axis: three axes fit a 60-bit key
constexpr int GRID_CELLS_PER_POINT = 64;    // B: the table's grid has at most this many cells per sub-point (psg_grid_index)

struct GridDims {
    float o[3];       // origin corner
    float dl;
    int n[3];         // cells along x, y, z
};

}  // namespace

struct psg_grid {
    psg_ctx *ctx;
    int cap;                          // points the buffers hold
    u64 *keys, *keys_sorted;          // [cap]
    int32_t *iota, *order;            // [cap]  order = point indices ascending by (key, index)
    int32_t *head, *rank1;            // [cap]  rank1 = 1 + output row of the sorted position
    int32_t *seg_start;               // [cap + 1]
    float4 *cell_pts;                 // [cap]  B: the sub-points in key order, w = the sub-point's index (bits)
    unsigned *mm;                     // [8]    min xyz, max xyz (ordered bits), non-finite flag
    void *tmp;
    size_t tmp_bytes;
    int n_assigned, n_voxels;         // A: state of the last psg_grid_assign (0: none)
    int n_indexed;                    // B: sub-points of the last psg_grid_index (0: none)
    GridDims index_dims;
};

namespace {

// order-preserving map float -> unsigned (finite values and infinities)
__device__ __forceinline__ unsigned ordered_bits(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
float from_ordered_bits(unsigned u)
{
    const unsigned b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

__global__ void minmax_kernel(const float *__restrict__ pts, int n, unsigned *__restrict__ mm)
{
    unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    int bad = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[(size_t)i * 3 + a];
            bad |= !isfinite(v);
            const unsigned b = ordered_bits(v);
            lo[a] = min(lo[a], b);
            hi[a] = max(hi[a], b);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], o));
            hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], o));
        }
        bad |= __shfl_xor(bad, o);
    }
    // one set of global atomics per workgroup, not per wave: thousands of atomics on the same seven words serialise in L2
    // (measured: 0.29 ms of a 4 M-point cloud's 0.62 ms)
    __shared__ unsigned s_lo[4][3], s_hi[4][3];
    __shared__ int s_bad[4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_lo[w][a] = lo[a]; s_hi[w][a] = hi[a]; }
        s_bad[w] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        atomicMin(mm + a, min(min(s_lo[0][a], s_lo[1][a]), min(s_lo[2][a], s_lo[3][a])));
        atomicMax(mm + 3 + a, max(max(s_hi[0][a], s_hi[1][a]), max(s_hi[2][a], s_hi[3][a])));
    } else if (threadIdx.x == 3 && (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3])) {
        atomicOr(mm + 6, 1u);
    }
}

// cell index along one axis: floor((p - origin) / dl) in fp32, IEEE division, clamped at 0
__device__ __forceinline__ float cell_f(float p, float o, float dl) { return fmaxf(floorf(__fdiv_rn(__fsub_rn(p, o), dl)), 0.0f); }

__global__ void keys_kernel(const float *__restrict__ pts, int n, GridDims gd, u64 *__restrict__ keys, int32_t *__restrict__ iota)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = pts + (size_t)i * 3;
    // (the cell formula is monotonic in the coordinate, so no index exceeds the maximum corner's, n - 1)
    const u64 ix = (u64)cell_f(p[0], gd.o[0], gd.dl), iy = (u64)cell_f(p[1], gd.o[1], gd.dl), iz = (u64)cell_f(p[2], gd.o[2], gd.dl);
    keys[i] = ix + (u64)gd.n[0] * iy + (u64)gd.n[0] * (u64)gd.n[1] * iz;
    iota[i] = i;
}

__global__ void heads_kernel(const u64 *__restrict__ ks, int n, int32_t *__restrict__ head)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) head[j] = (j == 0 || ks[j] != ks[j - 1]) ? 1 : 0;
}

__global__ void segments_kernel(const int32_t *__restrict__ head, const int32_t *__restrict__ rank1, const int32_t *__restrict__ order, int n,
                                int32_t *__restrict__ seg_start, int32_t *__restrict__ voxel_of_point)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int r = rank1[j] - 1;
    if (head[j]) seg_start[r] = j;
    if (j == n - 1) seg_start[r + 1] = n;
    if (voxel_of_point) voxel_of_point[order[j]] = r;
}

// thread = (cell, channel): channels 0..2 the coordinates, 3.. the features
__global__ void sums_kernel(const float *__restrict__ pts, const float *__restrict__ feat, int d, const int32_t *__restrict__ order,
                            const int32_t *__restrict__ seg_start, int m, float *__restrict__ sub_pts, float *__restrict__ sub_feat)
{
    const int C = 3 + d;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)m * C) return;
    const int v = (int)(t / C), c = (int)(t % C);
    const int s = seg_start[v], e = seg_start[v + 1];
    float acc = 0.0f;
    if (c < 3)
        for (int j = s; j < e; ++j) acc = __fadd_rn(acc, pts[(size_t)order[j] * 3 + c]);
    else
        for (int j = s; j < e; ++j) acc = __fadd_rn(acc, feat[(size_t)order[j] * d + (c - 3)]);
    const int count = e - s;
    if (c < 3)
        sub_pts[(size_t)v * 3 + c] = __fmul_rn(acc, (float)(1.0 / (double)count));
    else
        sub_feat[(size_t)v * d + (c - 3)] = __fdiv_rn(acc, (float)count);
}

__global__ void label_keys_kernel(const int32_t *__restrict__ labels, int l, int c, const int32_t *__restrict__ order,
                                  const int32_t *__restrict__ rank1, int n, u64 *__restrict__ keys)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned lab = (unsigned)labels[(size_t)order[j] * l + c] ^ 0x80000000u;      // signed order as unsigned order
    keys[j] = ((u64)(unsigned)(rank1[j] - 1) << 32) | lab;
}

// thread = cell: the first longest run of its sorted labels
__global__ void vote_kernel(const u64 *__restrict__ ks, const int32_t *__restrict__ seg_start, int m, int l, int c,
                            int32_t *__restrict__ sub_labels)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m) return;
    const int s = seg_start[v], e = seg_start[v + 1];
    unsigned best = (unsigned)ks[s], cur = best;
    int best_n = 0, cur_n = 0;
    for (int j = s; j < e; ++j) {
        const unsigned k = (unsigned)ks[j];
        if (k != cur) { cur = k; cur_n = 0; }
        ++cur_n;
        if (cur_n > best_n) { best_n = cur_n; best = cur; }
    }
    sub_labels[(size_t)v * l + c] = (int32_t)(best ^ 0x80000000u);
}

__global__ void cell_points_kernel(const float *__restrict__ pts, const int32_t *__restrict__ order, int m, float4 *__restrict__ out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int i = order[j];
    out[j] = make_float4(pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2], __int_as_float(i));
}

// One lane per query.  Ring r = the cells at Chebyshev distance r from the query's cell c (the query's own cell, clamped into the
// grid), inside the grid.  Per (iY, iZ) row of the ring: rows on the ring's y / z faces are searched over iX = c.x - r .. c.x + r
// in one key interval, the other rows only at their two end cells.  After ring r the block [c - r, c + r]^3 is searched.  A
// point outside it has, along some axis a, a cell index >= c[a] + r + 1 or <= c[a] - r - 1, and therefore lies
// beyond the face o[a] + k * dl less a margin of at most 3 * 2^-24 * k * dl, k <= n[a]; `gap` is the distance from the query
// to the nearest such face over the sides that still have cells, less the margin, in double.  The search ends when
// best < gap^2 * (1 - 2^-20) - strictly, so that no outside point can even tie (a tie goes to the lower index, wherever it
// is) - or when the block covers the grid.
__global__ void nearest_kernel(const u64 *__restrict__ keys, const float4 *__restrict__ cpts, int m, GridDims gd,
                               const float *__restrict__ query, int nq, int32_t *__restrict__ out)
{
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const float q[3] = {query[(size_t)qi * 3], query[(size_t)qi * 3 + 1], query[(size_t)qi * 3 + 2]};
    int c[3], rmax = 0;
    double margin[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = (int)fminf(cell_f(q[a], gd.o[a], gd.dl), (float)(gd.n[a] - 1));      // (a NaN becomes cell 0)
        rmax = max(rmax, max(c[a], gd.n[a] - 1 - c[a]));
        const double ext = (double)(gd.n[a] + 1) * (double)gd.dl;
        margin[a] = ext * 0x1p-21 + (fabs((double)gd.o[a]) + fabs((double)q[a]) + ext) * 0x1p-50;
    }
    float best = INFINITY;
    int best_i = 0x7FFFFFFF;
    auto scan = [&](u64 lo, u64 hi) {
        int a = 0, b = m;                                   // first position with key >= lo
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (keys[mid] < lo) a = mid + 1; else b = mid;
        }
        for (; a < m && keys[a] <= hi; ++a) {
            const float4 p = cpts[a];
            const float dx = __fsub_rn(q[0], p.x), dy = __fsub_rn(q[1], p.y), dz = __fsub_rn(q[2], p.z);
            const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            const int i = __float_as_int(p.w);
            if (d < best || (d == best && i < best_i)) { best = d; best_i = i; }
        }
    };
    for (int r = 0;; ++r) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, gd.n[0] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, gd.n[1] - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, gd.n[2] - 1);
        for (int iz = z0; iz <= z1; ++iz)
            for (int iy = y0; iy <= y1; ++iy) {
                const u64 base = (u64)gd.n[0] * ((u64)iy + (u64)gd.n[1] * (u64)iz);
                if (iz == c[2] - r || iz == c[2] + r || iy == c[1] - r || iy == c[1] + r) {
                    scan(base + x0, base + x1);
                } else {
                    if (c[0] - r >= 0) scan(base + (c[0] - r), base + (c[0] - r));
                    if (c[0] + r <= gd.n[0] - 1) scan(base + (c[0] + r), base + (c[0] + r));
                }
            }
        if (r >= rmax) break;
        double gap = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int kup = c[a] + r + 1, klo = c[a] - r;
            if (kup <= gd.n[a] - 1) gap = fmin(gap, ((double)gd.o[a] + (double)kup * (double)gd.dl) - (double)q[a] - margin[a]);
            if (klo >= 1) gap = fmin(gap, (double)q[a] - ((double)gd.o[a] + (double)klo * (double)gd.dl) - margin[a]);
        }
        if (gap > 1e-18 && (double)best < gap * gap * (1.0 - 0x1p-20)) break;
    }
    out[qi] = best_i == 0x7FFFFFFF ? 0 : best_i;
}

int bits_for(u64 count)      // bits that hold 0 .. count - 1, at least 1
{
    int b = 1;
    while (b < 64 && ((u64)1 << b) < count) ++b;
    return b;
}

// min / max corner of pts [n][3] -> corners [6] on the host.  Synchronises the stream.  Non-finite coordinates are refused here.
int read_corners(psg_grid *g, const float *pts, int n, hipStream_t st, const char *who, float *corners)
{
    PSG_CHECK_HIP(hipMemsetAsync(g->mm, 0xFF, 12, st));
    PSG_CHECK_HIP(hipMemsetAsync(g->mm + 3, 0, 20, st));
    const int blocks = std::min(ceil_div(n, 256), 512);      // minmax_kernel: 256 threads = the four waves its LDS step expects
    hipLaunchKernelGGL(minmax_kernel, dim3(blocks), dim3(256), 0, st, pts, n, g->mm);
    PSG_LAUNCH_CHECK();
    unsigned h[8];
    PSG_CHECK_HIP(hipMemcpyAsync(h, g->mm, sizeof(h), hipMemcpyDeviceToHost, st));
    PSG_CHECK_HIP(hipStreamSynchronize(st));
    PSG_REQUIRE(h[6] == 0, "%s: non-finite coordinates (NaN or infinity) in the points", who);
    for (int i = 0; i < 6; ++i) corners[i] = from_ordered_bits(h[i]);
    return PSG_OK;
}

// The reference's origin and grid size (grid_subsampling.cpp:25-31) from the corners, on the host in fp32 (volatile: every
// intermediate rounded to float, as the reference's own host code has it).  -1: fits; else the first axis with more than 2^20 cells.
int grid_dims(const float *corners, float dl, GridDims *gd)
{
    gd->dl = dl;
    volatile float inv = 1.0f / dl;      // rounded to fp32 first (grid_subsampling.cpp:27)
    for (int a = 0; a < 3; ++a) {
        volatile float scaled = corners[a] * inv;
        volatile float o = floorf(scaled) * dl;
        volatile float ext = corners[3 + a] - o;
        volatile float cells = floorf(ext / dl);
        if (!(std::isfinite((float)o) && (float)cells < (float)GRID_MAX_AXIS)) return a;
        gd->o[a] = o;
        gd->n[a] = (int)std::max((float)cells, 0.0f) + 1;
    }
    return -1;
}

int sort_by_key(psg_grid *g, const float *pts, int n, const GridDims &gd, hipStream_t st)
{
    hipLaunchKernelGGL(keys_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, pts, n, gd, g->keys, g->iota);
    PSG_LAUNCH_CHECK();
    size_t tb = g->tmp_bytes;
    const int end_bit = bits_for((u64)gd.n[0] * (u64)gd.n[1] * (u64)gd.n[2]);
    PSG_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(g->tmp, tb, g->keys, g->keys_sorted, g->iota, g->order, n, 0, end_bit, st));
    return PSG_OK;
}

}  // namespace

extern "C" int psg_grid_destroy(psg_grid *g)
{
    if (!g) return PSG_OK;
    void *all[] = {g->keys, g->keys_sorted, g->iota, g->order, g->head, g->rank1, g->seg_start, g->cell_pts, g->mm, g->tmp};
    for (void *p : all) (void)hipFree(p);
    delete g;
    return PSG_OK;
}

extern "C" int psg_grid_create(psg_ctx *ctx, int max_points, psg_grid **out)
{
    PSG_REQUIRE(ctx && out, "psg_grid_create: null argument");
    PSG_REQUIRE(max_points >= 1 && max_points <= (1 << 30), "psg_grid_create: max_points=%d outside [1, 2^30]", max_points);
    PSG_CHECK_HIP(hipSetDevice(ctx->device));
    psg_grid *g = new psg_grid();
    g->ctx = ctx; g->cap = max_points;
    const size_t P = (size_t)max_points;
    size_t t1 = 0, t2 = 0, t3 = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t1, (u64 *)nullptr, (u64 *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, max_points,
                                             0, 64, (hipStream_t)0);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t2, (u64 *)nullptr, (u64 *)nullptr, max_points, 0, 64, (hipStream_t)0);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, t3, (int32_t *)nullptr, (int32_t *)nullptr, max_points, (hipStream_t)0);
    g->tmp_bytes = std::max(std::max(t1, t2), std::max(t3, (size_t)16));
    void **slots[] = {(void **)&g->keys, (void **)&g->keys_sorted, (void **)&g->iota, (void **)&g->order, (void **)&g->head,
                      (void **)&g->rank1, (void **)&g->seg_start, (void **)&g->cell_pts, (void **)&g->mm, &g->tmp};
    const size_t sizes[] = {P * 8, P * 8, P * 4, P * 4, P * 4, P * 4, (P + 1) * 4, P * 16, 32, g->tmp_bytes};
    for (int i = 0; i < 10; ++i) {
        if (hipMalloc(slots[i], sizes[i]) != hipSuccess) {
            set_error("psg_grid_create: hipMalloc(%zu) failed", sizes[i]);
            *slots[i] = nullptr;
            (void)psg_grid_destroy(g);
            return PSG_ERR_HIP;
        }
    }
    *out = g;
    return PSG_OK;
}

extern "C" int psg_grid_assign(psg_grid *g, const float *points, int n, float grid_size, int32_t *voxel_of_point, int *n_voxels_out,
                               psg_stream stream)
{
    PSG_REQUIRE(g && points && n_voxels_out, "psg_grid_assign: null argument");
    PSG_REQUIRE(n >= 1 && n <= g->cap, "psg_grid_assign: n=%d outside [1, max_points=%d]", n, g->cap);
    PSG_REQUIRE(std::isfinite(grid_size) && grid_size > 0.0f, "psg_grid_assign: grid_size=%g is not a positive finite number", (double)grid_size);
    PSG_CHECK_HIP(hipSetDevice(g->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    g->n_assigned = 0; g->n_indexed = 0;
    GridDims gd;
    float corners[6];
    int rc = read_corners(g, points, n, st, "psg_grid_assign", corners);
    if (rc != PSG_OK) return rc;
    const int wide = grid_dims(corners, grid_size, &gd);
    PSG_REQUIRE(wide < 0, "psg_grid_assign: the grid has more than 2^20 cells along axis %d (extent %g at grid_size %g)", wide,
                (double)corners[3 + wide] - (double)corners[wide], (double)grid_size);
    rc = sort_by_key(g, points, n, gd, st);
    if (rc != PSG_OK) return rc;
    const dim3 grid(ceil_div(n, 256)), block(256);
    hipLaunchKernelGGL(heads_kernel, grid, block, 0, st, g->keys_sorted, n, g->head);
    PSG_LAUNCH_CHECK();
    size_t tb = g->tmp_bytes;
    PSG_CHECK_HIP(hipcub::DeviceScan::InclusiveSum(g->tmp, tb, g->head, g->rank1, n, st));
    hipLaunchKernelGGL(segments_kernel, grid, block, 0, st, g->head, g->rank1, g->order, n, g->seg_start, voxel_of_point);
    PSG_LAUNCH_CHECK();
    int32_t m = 0;
    PSG_CHECK_HIP(hipMemcpyAsync(&m, g->rank1 + (n - 1), 4, hipMemcpyDeviceToHost, st));
    PSG_CHECK_HIP(hipStreamSynchronize(st));
    PSG_REQUIRE(m >= 1 && m <= n, "psg_grid_assign: internal error: %d voxels for %d points", m, n);
    g->n_assigned = n; g->n_voxels = m;
    *n_voxels_out = m;
    return PSG_OK;
}

extern "C" int psg_grid_reduce(psg_grid *g, const float *points, const float *features, int d, const int32_t *labels, int l,
                               float *sub_points, float *sub_features, int32_t *sub_labels, psg_stream stream)
{
    PSG_REQUIRE(g && points && sub_points, "psg_grid_reduce: null argument");
    PSG_REQUIRE(g->n_assigned > 0, "psg_grid_reduce: no psg_grid_assign before it");
    PSG_REQUIRE(d >= 0 && d <= 4096 && (d == 0) == (features == nullptr) && (d == 0) == (sub_features == nullptr),
                "psg_grid_reduce: d=%d and the feature pointers do not agree", d);
    PSG_REQUIRE(l >= 0 && l <= 4096 && (l == 0) == (labels == nullptr) && (l == 0) == (sub_labels == nullptr),
                "psg_grid_reduce: l=%d and the label pointers do not agree", l);
    PSG_CHECK_HIP(hipSetDevice(g->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int n = g->n_assigned, m = g->n_voxels;
    const size_t threads = (size_t)m * (3 + d);
    PSG_REQUIRE((threads + 255) / 256 <= 0x7FFFFFFFull, "psg_grid_reduce: %d voxels x %d channels is too large", m, 3 + d);
    hipLaunchKernelGGL(sums_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, points, features, d, g->order, g->seg_start, m,
                       sub_points, sub_features);
    PSG_LAUNCH_CHECK();
    const int end_bit = 32 + bits_for((u64)m);
    for (int c = 0; c < l; ++c) {
        // (the cell keys of psg_grid_assign are not needed any more: their two buffers hold the label keys)
        hipLaunchKernelGGL(label_keys_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, labels, l, c, g->order, g->rank1, n, g->keys);
        PSG_LAUNCH_CHECK();
        size_t tb = g->tmp_bytes;
        PSG_CHECK_HIP(hipcub::DeviceRadixSort::SortKeys(g->tmp, tb, g->keys, g->keys_sorted, n, 0, end_bit, st));
        hipLaunchKernelGGL(vote_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, g->keys_sorted, g->seg_start, m, l, c, sub_labels);
        PSG_LAUNCH_CHECK();
    }
    return PSG_OK;
}

extern "C" int psg_grid_index(psg_grid *g, const float *sub_points, int m, float grid_size, psg_stream stream)
{
    PSG_REQUIRE(g && sub_points, "psg_grid_index: null argument");
    PSG_REQUIRE(m >= 1 && m <= g->cap, "psg_grid_index: m=%d outside [1, max_points=%d]", m, g->cap);
    PSG_REQUIRE(std::isfinite(grid_size) && grid_size > 0.0f, "psg_grid_index: grid_size=%g is not a positive finite number", (double)grid_size);
    PSG_CHECK_HIP(hipSetDevice(g->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    g->n_assigned = 0; g->n_indexed = 0;
    float corners[6];
    int rc = read_corners(g, sub_points, m, st, "psg_grid_index", corners);
    if (rc != PSG_OK) return rc;
    // The answer does not depend on the cell size, the work does: a query in an empty region walks ring after ring of binary
    // searches.  So grid_size is the SMALLEST cell the table uses: it is doubled until the grid has at most GRID_CELLS_PER_POINT
    // cells per sub-point (and at most 2^20 along an axis), which bounds a query's work by a multiple of the scan's.
    float dl = grid_size;
    for (int tries = 0;; ++tries) {
        PSG_REQUIRE(tries < 300 && std::isfinite(dl), "psg_grid_index: no cell size from grid_size=%g fits the cloud", (double)grid_size);
        const GridDims &gd = g->index_dims;
        if (grid_dims(corners, dl, &g->index_dims) < 0 && (double)gd.n[0] * gd.n[1] * gd.n[2] <= (double)GRID_CELLS_PER_POINT * m) break;
        dl *= 2.0f;
    }
    rc = sort_by_key(g, sub_points, m, g->index_dims, st);
    if (rc != PSG_OK) return rc;
    hipLaunchKernelGGL(cell_points_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, sub_points, g->order, m, g->cell_pts);
    PSG_LAUNCH_CHECK();
    g->n_indexed = m;
    return PSG_OK;
}

extern "C" int psg_grid_nearest(psg_grid *g, const float *query, int n_query, int32_t *out_idx, psg_stream stream)
{
    PSG_REQUIRE(g && query && out_idx, "psg_grid_nearest: null argument");
    PSG_REQUIRE(g->n_indexed > 0, "psg_grid_nearest: no psg_grid_index before it");
    PSG_REQUIRE(n_query >= 1, "psg_grid_nearest: n_query=%d", n_query);
    PSG_CHECK_HIP(hipSetDevice(g->ctx->device));
    hipLaunchKernelGGL(nearest_kernel, dim3(ceil_div(n_query, 64)), dim3(64), 0, (hipStream_t)stream, g->keys_sorted, g->cell_pts,
                       g->n_indexed, g->index_dims, query, n_query, out_idx);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}
