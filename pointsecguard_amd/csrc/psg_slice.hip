// The whole-scene block slicer on the device: ScannetDatasetWholeScene.__getitem__
// (PointNet/data_utils/S3DISDataLoader.py:124-175) without its per-cell host loop.
//
// The reference cuts a room into grid cells (block_size x block_size columns, `stride` apart); per non-empty cell it takes
// inside = np.where(the point lies in the padded window)[0], pads it to a multiple of block_points with np.random.choice,
// shuffles, and forms nine float64 channels per slot.  Both random draws depend on the cell's member COUNT only, so the work
// splits: the device counts and lists the members, the host draws the plan (harness.slice_plan) from the counts, the device
// gathers.
//   slice_count_kernel    tile = 256 consecutive points, owned by ONE wave (four 64-point rows, x / y loaded once into
//                         registers); workgroup = four tiles; the cell windows sit in LDS.  Per cell: four IEEE double
//                         compares per point (>=, <=; the bounds come from the host, the device never recomputes one),
//                         ballot + popcount -> tile_cnt [cell][tile]
//   slice_scan_kernel     one workgroup: exclusive scan of tile_cnt in (cell, tile) order, in place = where every tile's
//                         members of every cell start in `inside`; cell_off [n_cells + 1] and counts [n_cells] from it
//   slice_members_kernel  the same tiles, the same compares: position = tile offset + members of the wave's earlier rows +
//                         members in lower lanes.  Ascending point index per cell (np.where's order); no atomics, every
//                         position has one writer, two runs give the same bytes
//   slice_gather_kernel   one thread per output slot: p = inside[cell_off[cell] + src_pos[slot]]; every value is formed in
//                         double by the reference's single operation and rounded once to float32 (astype(np.float32) of
//                         the host's float64 block).  Compiled with -ffp-contract=off.
#include "psg_common.h"

using namespace psg;

namespace {

constexpr int SLICE_MAX_CELLS = PSG_SLICE_MAX_CELLS;      // windows in LDS: 4 doubles per cell = 32 KiB
constexpr int SLICE_TILE = PSG_SLICE_TILE;                // points of one wave: 4 rows of 64
constexpr int SLICE_ROWS = SLICE_TILE / 64;
constexpr int SLICE_WG_TILES = 4;                         // waves of a workgroup
constexpr int SLICE_SCAN_THREADS = 1024;
constexpr int SLICE_MAX_ITEMS = 1 << 30;                  // n_cells * n_tiles

// The points of one wave's tile: x, y of its four rows and whether the row's point exists.
struct TilePoints {
    double x[SLICE_ROWS], y[SLICE_ROWS];
    bool ok[SLICE_ROWS];
};

__device__ __forceinline__ void load_tile(const double *__restrict__ xy, int stride, int n, int tile, int lane, TilePoints &t)
{
#pragma unroll
    for (int r = 0; r < SLICE_ROWS; ++r) {
        const int p = tile * SLICE_TILE + r * 64 + lane;
        t.ok[r] = p < n;
        const double *q = xy + (size_t)(t.ok[r] ? p : 0) * stride;
        t.x[r] = q[0];
        t.y[r] = q[1];
    }
}

// s_x - pad <= x <= e_x + pad and s_y - pad <= y <= e_y + pad: the reference's four compares (a NaN is in no cell)
__device__ __forceinline__ bool in_window(double x, double y, const double *w) { return x >= w[0] && x <= w[1] && y >= w[2] && y <= w[3]; }

__device__ __forceinline__ void load_windows(const double *__restrict__ windows, int n_cells, double *s_win)
{
    for (int i = threadIdx.x; i < n_cells * 4; i += blockDim.x) s_win[i] = windows[i];
    __syncthreads();
}

__global__ __launch_bounds__(64 * SLICE_WG_TILES) void slice_count_kernel(const double *__restrict__ xy, int stride, int n,
                                                                          const double *__restrict__ windows, int n_cells, int n_tiles,
                                                                          int32_t *__restrict__ tile_cnt)
{
    __shared__ double s_win[SLICE_MAX_CELLS * 4];
    load_windows(windows, n_cells, s_win);
    const int lane = threadIdx.x & 63, tile = blockIdx.x * SLICE_WG_TILES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;      // (whole waves, after the kernel's only barrier)
    TilePoints t;
    load_tile(xy, stride, n, tile, lane, t);
    for (int c = 0; c < n_cells; ++c) {
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < SLICE_ROWS; ++r) cnt += __popcll(__ballot(t.ok[r] && in_window(t.x[r], t.y[r], s_win + 4 * c)));
        if (lane == 0) tile_cnt[(size_t)c * n_tiles + tile] = cnt;
    }
}

// In place: t [L] counts -> exclusive prefix sums, t[L] = the total.  Every thread owns a contiguous span; the sums are
// carried in 64 bits and stored modulo 2^32 (a count is a difference of two neighbours and at most n, so counts [] is exact
// whatever the total; the caller refuses a total beyond INT_MAX before it uses an offset).
__global__ __launch_bounds__(SLICE_SCAN_THREADS) void slice_scan_kernel(int32_t *__restrict__ t, int L, int n_cells, int n_tiles,
                                                                        int32_t *__restrict__ counts, int32_t *__restrict__ cell_off)
{
    __shared__ long long s[SLICE_SCAN_THREADS];
    const int tid = threadIdx.x, span = (L + SLICE_SCAN_THREADS - 1) / SLICE_SCAN_THREADS;
    const int lo = (int)min((long long)tid * span, (long long)L), hi = (int)min((long long)(tid + 1) * span, (long long)L);
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += t[i];
    s[tid] = sum;
    __syncthreads();
    for (int o = 1; o < SLICE_SCAN_THREADS; o <<= 1) {
        const long long v = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    long long run = s[tid] - sum;
    for (int i = lo; i < hi; ++i) {
        const int32_t v = t[i];
        t[i] = (int32_t)(unsigned)(unsigned long long)run;
        run += v;
    }
    if (tid == SLICE_SCAN_THREADS - 1) t[L] = (int32_t)(unsigned)(unsigned long long)s[tid];
    __syncthreads();
    for (int c = tid; c <= n_cells; c += SLICE_SCAN_THREADS) {
        const unsigned a = (unsigned)t[(size_t)c * n_tiles];
        cell_off[c] = (int32_t)a;
        if (c < n_cells) counts[c] = (int32_t)((unsigned)t[(size_t)(c + 1) * n_tiles] - a);
    }
}

__global__ __launch_bounds__(64 * SLICE_WG_TILES) void slice_members_kernel(const double *__restrict__ xy, int stride, int n,
                                                                            const double *__restrict__ windows, int n_cells, int n_tiles,
                                                                            const int32_t *__restrict__ tile_off, int32_t *__restrict__ inside,
                                                                            int inside_len)
{
    __shared__ double s_win[SLICE_MAX_CELLS * 4];
    load_windows(windows, n_cells, s_win);
    const int lane = threadIdx.x & 63, tile = blockIdx.x * SLICE_WG_TILES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    TilePoints t;
    load_tile(xy, stride, n, tile, lane, t);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c = 0; c < n_cells; ++c) {
        int pos = tile_off[(size_t)c * n_tiles + tile];
#pragma unroll
        for (int r = 0; r < SLICE_ROWS; ++r) {
            const bool in = t.ok[r] && in_window(t.x[r], t.y[r], s_win + 4 * c);
            const unsigned long long b = __ballot(in);
            const int mine = pos + __popcll(b & below);
            if (in && mine >= 0 && mine < inside_len) inside[mine] = tile * SLICE_TILE + r * 64 + lane;
            pos += __popcll(b);
        }
    }
}

struct SliceCmax { double v[3]; };

__global__ void slice_gather_kernel(const double *__restrict__ xyz, int xyz_stride, const double *__restrict__ rgb, int rgb_stride,
                                    const int32_t *__restrict__ labels, int n, const int32_t *__restrict__ inside, int inside_len,
                                    const int32_t *__restrict__ cell_off, const int32_t *__restrict__ block_cell,
                                    const double *__restrict__ centres, int n_cells, const int32_t *__restrict__ src_pos, int nb, int bp,
                                    SliceCmax cmax, const float *__restrict__ labelweights, float *__restrict__ data,
                                    int32_t *__restrict__ label, float *__restrict__ smpw, int32_t *__restrict__ index)
{
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (size_t)nb * bp) return;
    const int cell = block_cell[slot / bp];
    int p = -1;
    if (cell >= 0 && cell < n_cells) {
        const int off = cell_off[cell], cnt = cell_off[cell + 1] - off, sp = src_pos[slot];
        if (sp >= 0 && sp < cnt && off >= 0 && off + sp < inside_len) p = inside[off + sp];
    }
    float *d = data + slot * 9;
    if (p < 0 || p >= n) {      // a plan that does not belong to these lists: nothing is read through it
        for (int k = 0; k < 9; ++k) d[k] = 0.0f;
        label[slot] = 0; smpw[slot] = 0.0f; index[slot] = -1;
        return;
    }
    const double *q = xyz + (size_t)p * xyz_stride, *c = rgb + (size_t)p * rgb_stride;
    const double x = q[0], y = q[1], z = q[2];
    d[0] = (float)(x - centres[2 * cell]);            // block[:, 0] - (s_x + bs / 2.0)
    d[1] = (float)(y - centres[2 * cell + 1]);
    d[2] = (float)z;
    d[3] = (float)(c[0] / 255.0);                      // block[:, 3:6] /= 255.0
    d[4] = (float)(c[1] / 255.0);
    d[5] = (float)(c[2] / 255.0);
    d[6] = (float)(x / cmax.v[0]);                     // block[:, :3] / cmax: a division, not a multiply by a reciprocal
    d[7] = (float)(y / cmax.v[1]);
    d[8] = (float)(z / cmax.v[2]);
    const int lab = labels[p];
    label[slot] = lab;
    smpw[slot] = (lab >= 0 && lab < PSG_SLICE_CLASSES) ? labelweights[lab] : 0.0f;
    index[slot] = p;
}

int check_scene_args(const char *who, const void *xy, int stride, int n, const void *windows, int n_cells, long long tile_items, int *n_tiles)
{
    PSG_REQUIRE(xy && windows, "%s: null argument", who);
    PSG_REQUIRE(n >= 1 && n <= (1 << 30) && stride >= 2, "%s: n=%d outside [1, 2^30] or stride=%d below the two columns of a point", who, n,
                stride);
    PSG_REQUIRE(n_cells >= 1 && n_cells <= SLICE_MAX_CELLS,
                "%s: the grid has %d cells, the device slicer holds 1 .. %d (their windows sit in LDS)", who, n_cells, SLICE_MAX_CELLS);
    *n_tiles = ceil_div(n, SLICE_TILE);
    PSG_REQUIRE((long long)*n_tiles * n_cells <= SLICE_MAX_ITEMS, "%s: %d cells x %d tiles of points is too large", who, n_cells, *n_tiles);
    PSG_REQUIRE(tile_items >= (long long)*n_tiles * n_cells + 1, "%s: tile_off holds %lld items, %d cells x %d tiles need one more than their product",
                who, tile_items, n_cells, *n_tiles);
    return PSG_OK;
}

}  // namespace

extern "C" int psg_slice_count(const double *xy, int stride, int n, const double *windows, int n_cells, int32_t *tile_off,
                               long long tile_items, int32_t *counts, int32_t *cell_off, psg_stream stream)
{
    int n_tiles = 0;
    const int rc = check_scene_args("psg_slice_count", xy, stride, n, windows, n_cells, tile_items, &n_tiles);
    if (rc != PSG_OK) return rc;
    PSG_REQUIRE(tile_off && counts && cell_off, "psg_slice_count: null argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(slice_count_kernel, dim3(ceil_div(n_tiles, SLICE_WG_TILES)), dim3(64 * SLICE_WG_TILES), 0, st, xy, stride, n, windows,
                       n_cells, n_tiles, tile_off);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(slice_scan_kernel, dim3(1), dim3(SLICE_SCAN_THREADS), 0, st, tile_off, n_tiles * n_cells, n_cells, n_tiles, counts,
                       cell_off);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_slice_members(const double *xy, int stride, int n, const double *windows, int n_cells, const int32_t *tile_off,
                                 long long tile_items, int32_t *inside, int inside_len, psg_stream stream)
{
    int n_tiles = 0;
    const int rc = check_scene_args("psg_slice_members", xy, stride, n, windows, n_cells, tile_items, &n_tiles);
    if (rc != PSG_OK) return rc;
    PSG_REQUIRE(tile_off && inside && inside_len >= 1, "psg_slice_members: null argument or inside_len=%d", inside_len);
    hipLaunchKernelGGL(slice_members_kernel, dim3(ceil_div(n_tiles, SLICE_WG_TILES)), dim3(64 * SLICE_WG_TILES), 0, (hipStream_t)stream, xy,
                       stride, n, windows, n_cells, n_tiles, tile_off, inside, inside_len);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_slice_gather(const double *xyz, int xyz_stride, const double *rgb, int rgb_stride, const int32_t *labels, int n,
                                const int32_t *inside, int inside_len, const int32_t *cell_off, const int32_t *block_cell,
                                const double *centres, int n_cells, const int32_t *src_pos, int nb, int bp, double cmax_x, double cmax_y,
                                double cmax_z, const float *labelweights, float *data, int32_t *label, float *smpw, int32_t *index,
                                psg_stream stream)
{
    PSG_REQUIRE(xyz && rgb && labels && inside && cell_off && block_cell && centres && src_pos && labelweights && data && label && smpw &&
                index, "psg_slice_gather: null argument");
    PSG_REQUIRE(n >= 1 && xyz_stride >= 3 && rgb_stride >= 3 && inside_len >= 1, "psg_slice_gather: n=%d, strides %d / %d, inside_len=%d", n,
                xyz_stride, rgb_stride, inside_len);
    PSG_REQUIRE(n_cells >= 1 && n_cells <= SLICE_MAX_CELLS, "psg_slice_gather: n_cells=%d outside [1, %d]", n_cells, SLICE_MAX_CELLS);
    PSG_REQUIRE(nb >= 1 && bp >= 1 && (long long)nb * bp <= 0x7FFFFFFFll / 9, "psg_slice_gather: %d blocks x %d points outside 1 .. INT_MAX / 9",
                nb, bp);
    const long long slots = (long long)nb * bp;
    SliceCmax cm = {{cmax_x, cmax_y, cmax_z}};
    hipLaunchKernelGGL(slice_gather_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xyz, xyz_stride, rgb,
                       rgb_stride, labels, n, inside, inside_len, cell_off, block_cell, centres, n_cells, src_pos, nb, bp, cm, labelweights,
                       data, label, smpw, index);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}
