// Whole-scene NB attack: ONE colour per scene point across all the overlapping blocks that hold it.
//   psg_scene_occ_build         occurrence lists of every scene point over the block slots, entries ascending
//   psg_scene_colour_to_blocks  scene colours -> channels 3:6 of every block row
//   psg_scene_rows_mask         zero the dlogp rows of slots whose scene point is not under the scene mask
//   psg_scene_pgd_step          gradient summed over a point's occurrences in ascending slot order, then psg_pgd_step's
//                               arithmetic (psg_attack.hip: pgd_step_kernel) on the scene's colours
// and the coordinate field of the same attack: ONE displacement delta [n_scene][3] per scene point
//   psg_scene_delta_to_blocks   channels 0:3 of every block row <- fl32(clean coordinate of the row + delta of its point)
//   psg_scene_field_step        the same ordered sum over channels 0:3 of the block gradients, a sign step on delta and the
//                               clamp to [-eps, +eps] (no box: coordinates have none)
// Compiled with -ffp-contract=off: the summation order and the step's evaluation order decide bits.  No float atomics
// anywhere; every output element has one writer.  The only atomics are integer ones (histogram, list cursors, the bad-index
// flag), whose results do not depend on the order they land in; the order INSIDE a list, which an atomic cursor would leave
// to scheduling, is fixed afterwards by ranking every entry among its list.  The readers of the lists - the two step kernels
// here, scene_nu_step_kernel in psg_scene_nu.hip - all go through for_each_slot (psg_scene_lists.cuh).
#include <climits>

#include "psg_common.h"
#include "psg_scene_lists.cuh"

using namespace psg;

namespace {

constexpr int SCAN_THREADS = 1024;

// cnt[p] += 1 for every row with a valid index (cnt zeroed by the caller); an index outside [0, n_scene) raises the flag
__global__ void occ_count_kernel(const int32_t *__restrict__ point_idx, int rows, int n_scene, int32_t *__restrict__ cnt,
                                 int32_t *__restrict__ bad)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)rows) return;
    const int p = point_idx[e];
    if (p < 0 || p >= n_scene) { atomicOr(bad, 1); return; }
    atomicAdd(&cnt[p], 1);
}

// In-place exclusive scan of v[0 .. n) by ONE workgroup: every thread owns a contiguous segment (serial sum, LDS scan of the
// 1024 segment sums, serial write-back).  Built once per scene: n = n_scene + 1, a few hundred thousand entries.
__global__ __launch_bounds__(SCAN_THREADS) void occ_scan_kernel(int32_t *__restrict__ v, size_t n, int32_t *__restrict__ cursor)
{
    __shared__ int32_t s_sum[SCAN_THREADS];
    const size_t seg = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const size_t lo = min((size_t)threadIdx.x * seg, n), hi = min(lo + seg, n);
    int32_t acc = 0;
    for (size_t i = lo; i < hi; ++i) acc += v[i];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {          // Hillis-Steele inclusive scan
        const int32_t add = (int)threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += add;
        __syncthreads();
    }
    int32_t run = s_sum[threadIdx.x] - acc;               // exclusive prefix of this segment
    for (size_t i = lo; i < hi; ++i) {
        const int32_t c = v[i];
        v[i] = run;
        if (i + 1 < n) cursor[i] = run;                   // (the list cursors: one per scene point, not for the end marker)
        run += c;
    }
}

// unordered fill: slot e goes to the next free place of its point's list (which place is left to scheduling - see occ_rank)
__global__ void occ_fill_kernel(const int32_t *__restrict__ point_idx, int rows, int n_scene, int32_t *__restrict__ cursor,
                                int32_t *__restrict__ unordered)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)rows) return;
    const int p = point_idx[e];
    if (p < 0 || p >= n_scene) return;
    const int at = atomicAdd(&cursor[p], 1);
    if (at >= 0 && at < rows) unordered[at] = (int32_t)e;
}

// ordered lists: slot e's place in its point's list is the number of the list's entries below e - a function of the index
// array alone, whatever order the fill left.  sum over lists of length^2 reads; a list is at most a block's worth of
// repeats per block that holds the point (padding by sampling with replacement), and its readers share cache lines.
__global__ void occ_rank_kernel(const int32_t *__restrict__ point_idx, int rows, int n_scene, const int32_t *__restrict__ occ_off,
                                const int32_t *__restrict__ unordered, int32_t *__restrict__ occ_ent)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)rows) return;
    const int p = point_idx[e];
    if (p < 0 || p >= n_scene) return;
    const int lo = occ_off[p], hi = occ_off[p + 1];
    if (lo < 0 || hi > rows || lo > hi) return;
    int rank = 0;
    for (int i = lo; i < hi; ++i) rank += unordered[i] < (int32_t)e ? 1 : 0;
    if (lo + rank < hi) occ_ent[lo + rank] = (int32_t)e;
}

// x[row][3 + ch] = scene_rgb[point_idx[row]][ch]; the other six floats of a row are not touched
__global__ void colour_to_blocks_kernel(const float *__restrict__ scene_rgb, const int32_t *__restrict__ point_idx, size_t total,
                                        int n_scene, float *__restrict__ x, int32_t *__restrict__ bad)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over rows * 3
    if (t >= total) return;
    const size_t row = t / 3;
    const int ch = (int)(t % 3);
    const int p = point_idx[row];
    if (p < 0 || p >= n_scene) { atomicOr(bad, 1); return; }
    x[row * 9 + 3 + ch] = scene_rgb[(size_t)p * 3 + ch];
}

// dlogp[row][:] = +0.0 where the row's scene point is not under the mask (an index out of range counts as unmasked)
__global__ void rows_mask_kernel(float *__restrict__ dlogp, const int32_t *__restrict__ point_idx, const uint8_t *__restrict__ scene_mask,
                                 size_t total, int n_cls, int n_scene)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over rows * n_cls
    if (t >= total) return;
    const int p = point_idx[t / n_cls];
    const bool on = p >= 0 && p < n_scene && scene_mask[p];
    if (!on) dlogp[t] = 0.0f;
}

// one thread per (scene point, colour channel): g = ((0 + d[e0]) + d[e1]) + ... over the point's slots in list order, then
// pgd_step_kernel's arithmetic with the scene's clean colour as `ori`.  `step` = dir * alpha already rounded to fp32.
__global__ void scene_pgd_step_kernel(float *__restrict__ scene_rgb, const float *__restrict__ scene_ori, const uint8_t *__restrict__ scene_mask,
                                      const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ_ent,
                                      const float *__restrict__ dx0, int rows, size_t total, float step, float eps, int last,
                                      float *__restrict__ gsum_out)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over n_scene * 3
    if (t >= total) return;
    const size_t p = t / 3;
    const int ch = (int)(t % 3);
    float g = 0.0f;
    bool any = false;
    if (!scene_mask || scene_mask[p])
        any = for_each_slot(occ_off, occ_ent, p, rows, [&](int e) { g = __fadd_rn(g, dx0[(size_t)e * 9 + 3 + ch]); });
    if (gsum_out) gsum_out[t] = g;
    if (!any) return;                                  // no occurrence (or not under the mask): the point does not move
    const float sg = g > 0.0f ? 1.0f : (g < 0.0f ? -1.0f : 0.0f);
    const float stepped = __fadd_rn(scene_rgb[t], __fmul_rn(step, sg));
    const float o = scene_ori[t];
    const float eta = fminf(fmaxf(__fsub_rn(stepped, o), -eps), eps);
    const float proj = fminf(fmaxf(__fadd_rn(o, eta), 0.0f), 1.0f);
    scene_rgb[t] = last ? stepped : proj;
}

// x[row][ch] = fl32(x_clean[row][ch] + delta[point_idx[row]][ch]) for ch in 0:3 - one fp32 add onto the CLEAN coordinate of
// the slot (never onto the previously moved one); the other six floats of a row are not touched
__global__ void delta_to_blocks_kernel(const float *__restrict__ delta, const int32_t *__restrict__ point_idx,
                                       const float *__restrict__ x_clean, size_t total, int n_scene, float *__restrict__ x,
                                       int32_t *__restrict__ bad)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over rows * 3
    if (t >= total) return;
    const size_t row = t / 3;
    const int ch = (int)(t % 3);
    const int p = point_idx[row];
    if (p < 0 || p >= n_scene) { atomicOr(bad, 1); return; }
    x[row * 9 + ch] = __fadd_rn(x_clean[row * 9 + ch], delta[(size_t)p * 3 + ch]);
}

// one thread per (scene point, coordinate): scene_pgd_step_kernel's ordered sum over channels 0:3, then
// stepped = delta + step * sign(g); delta = last ? stepped : clamp(stepped, -eps, +eps)
__global__ void scene_field_step_kernel(float *__restrict__ delta, const uint8_t *__restrict__ scene_mask,
                                        const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ_ent,
                                        const float *__restrict__ dx0, int rows, size_t total, float step, float eps, int last,
                                        float *__restrict__ gsum_out)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over n_scene * 3
    if (t >= total) return;
    const size_t p = t / 3;
    const int ch = (int)(t % 3);
    float g = 0.0f;
    bool any = false;
    if (!scene_mask || scene_mask[p])
        any = for_each_slot(occ_off, occ_ent, p, rows, [&](int e) { g = __fadd_rn(g, dx0[(size_t)e * 9 + ch]); });
    if (gsum_out) gsum_out[t] = g;
    if (!any) return;                                  // no occurrence (or not under the mask): the point does not move
    const float sg = g > 0.0f ? 1.0f : (g < 0.0f ? -1.0f : 0.0f);
    const float stepped = __fadd_rn(delta[t], __fmul_rn(step, sg));
    delta[t] = last ? stepped : fminf(fmaxf(stepped, -eps), eps);
}

}  // namespace

extern "C" int psg_scene_occ_build(const int32_t *point_idx, int rows, int n_scene, int32_t *occ_off, int32_t *occ_ent,
                                   int32_t *scratch, int32_t *bad_flag, psg_stream stream)
{
    PSG_REQUIRE(point_idx && occ_off && occ_ent && scratch && bad_flag && n_scene > 0 && n_scene < INT_MAX,
                "psg_scene_occ_build: bad argument");
    PSG_REQUIRE(rows_ok(rows), "psg_scene_occ_build: rows=%d outside 1 .. INT_MAX / 9 (slot numbers address [rows][9] floats)", rows);
    hipStream_t st = (hipStream_t)stream;
    int32_t *cursor = scratch;                         // [n_scene]
    int32_t *unordered = scratch + (size_t)n_scene;    // [rows]
    PSG_CHECK_HIP(hipMemsetAsync(occ_off, 0, ((size_t)n_scene + 1) * sizeof(int32_t), st));
    // (entries of rows with a bad index are never written: -1 keeps such a tail out of every reader's range check)
    PSG_CHECK_HIP(hipMemsetAsync(occ_ent, 0xFF, (size_t)rows * sizeof(int32_t), st));
    PSG_CHECK_HIP(hipMemsetAsync(unordered, 0xFF, (size_t)rows * sizeof(int32_t), st));
    hipLaunchKernelGGL(occ_count_kernel, dim3(blocks_for((size_t)rows)), dim3(256), 0, st, point_idx, rows, n_scene, occ_off, bad_flag);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, occ_off, (size_t)n_scene + 1, cursor);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(occ_fill_kernel, dim3(blocks_for((size_t)rows)), dim3(256), 0, st, point_idx, rows, n_scene, cursor, unordered);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(occ_rank_kernel, dim3(blocks_for((size_t)rows)), dim3(256), 0, st, point_idx, rows, n_scene, occ_off, unordered,
                       occ_ent);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_colour_to_blocks(const float *scene_rgb, const int32_t *point_idx, int rows, int n_scene, float *x,
                                          int32_t *bad_flag, psg_stream stream)
{
    PSG_REQUIRE(scene_rgb && point_idx && x && bad_flag && n_scene > 0, "psg_scene_colour_to_blocks: bad argument");
    PSG_REQUIRE(rows_ok(rows), "psg_scene_colour_to_blocks: rows=%d outside 1 .. INT_MAX / 9", rows);
    const size_t total = (size_t)rows * 3;
    hipLaunchKernelGGL(colour_to_blocks_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, scene_rgb, point_idx, total,
                       n_scene, x, bad_flag);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_rows_mask(float *dlogp, const int32_t *point_idx, const uint8_t *scene_mask, int rows, int n_cls,
                                   int n_scene, psg_stream stream)
{
    PSG_REQUIRE(dlogp && point_idx && scene_mask && n_scene > 0, "psg_scene_rows_mask: bad argument");
    PSG_REQUIRE(n_cls > 0 && n_cls <= 32, "psg_scene_rows_mask: n_cls=%d out of range (1..32)", n_cls);
    PSG_REQUIRE(rows_ok(rows), "psg_scene_rows_mask: rows=%d outside 1 .. INT_MAX / 9", rows);
    const size_t total = (size_t)rows * (size_t)n_cls;
    hipLaunchKernelGGL(rows_mask_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, dlogp, point_idx, scene_mask,
                       total, n_cls, n_scene);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_pgd_step(float *scene_rgb, const float *scene_ori, const uint8_t *scene_mask, const int32_t *occ_off,
                                  const int32_t *occ_ent, const float *dx0, int rows, int n_scene, float alpha, float eps, float dir,
                                  int last, float *gsum_out, psg_stream stream)
{
    PSG_REQUIRE(scene_rgb && scene_ori && occ_off && occ_ent && dx0 && n_scene > 0, "psg_scene_pgd_step: bad argument");
    PSG_REQUIRE(rows_ok(rows), "psg_scene_pgd_step: rows=%d outside 1 .. INT_MAX / 9 (slot numbers address [rows][9] floats)", rows);
    const size_t total = (size_t)n_scene * 3;
    hipLaunchKernelGGL(scene_pgd_step_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, scene_rgb, scene_ori,
                       scene_mask, occ_off, occ_ent, dx0, rows, total, dir * alpha, eps, last, gsum_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_delta_to_blocks(const float *delta, const int32_t *point_idx, const float *x_clean, int rows, int n_scene,
                                         float *x, int32_t *bad_flag, psg_stream stream)
{
    PSG_REQUIRE(delta && point_idx && x_clean && x && bad_flag && n_scene > 0, "psg_scene_delta_to_blocks: bad argument");
    PSG_REQUIRE(rows_ok(rows), "psg_scene_delta_to_blocks: rows=%d outside 1 .. INT_MAX / 9", rows);
    const size_t total = (size_t)rows * 3;
    hipLaunchKernelGGL(delta_to_blocks_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, delta, point_idx, x_clean,
                       total, n_scene, x, bad_flag);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_field_step(float *delta, const uint8_t *scene_mask, const int32_t *occ_off, const int32_t *occ_ent,
                                    const float *dx0, int rows, int n_scene, float alpha, float eps, float dir, int last,
                                    float *gsum_out, psg_stream stream)
{
    PSG_REQUIRE(delta && occ_off && occ_ent && dx0 && n_scene > 0, "psg_scene_field_step: bad argument");
    PSG_REQUIRE(rows_ok(rows), "psg_scene_field_step: rows=%d outside 1 .. INT_MAX / 9 (slot numbers address [rows][9] floats)", rows);
    const size_t total = (size_t)n_scene * 3;
    hipLaunchKernelGGL(scene_field_step_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, delta, scene_mask,
                       occ_off, occ_ent, dx0, rows, total, dir * alpha, eps, last, gsum_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}
