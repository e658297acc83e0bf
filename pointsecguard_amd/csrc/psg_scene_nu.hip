// Whole-scene NU attack: Adam in tanh space on ONE colour per scene point across all the overlapping
// blocks that hold it.  The lists are psg_scene_occ_build's (psg_scene.hip), read through for_each_slot
// (psg_scene_lists.cuh); the arithmetic is psg_attack.hip's NU kernels (nu_inverse_tanh_kernel, nu_tanh_color_kernel,
// nu_adam_step_kernel), operation for operation, the Adam update being the one both call (psg_adam.cuh).
//   psg_scene_nu_init    w = inverse_tanh_space(c0) for every scene point
//   psg_scene_nu_colour  c = 1/2 (tanh w + 1) on the moving points while the attack is active
//   psg_scene_nu_step    f-loss and Smooth gradients summed over a point's slots in ascending slot order, the L2 term once
//                        per point, the chain through tanh_space, torch's single-tensor Adam on w / m / v
//   psg_scene_nu_field_step  the coordinate field (section 5z): the same two ordered sums over channels 0:3 and the per-slot
//                        Smooth_xyz gradients, nu_coord_adam_kernel's assembly, Adam on the displacement delta / m / v
//   psg_scene_nu_latch   integer exit test over all slots: two counters, the decision by one thread in a launch of its own,
//                        the snapshot of the colours the step's forward saw
// Compiled with -ffp-contract=off: the summation order and the step's evaluation order decide bits.  No float atomics; every
// output element has one writer.  The only atomics are the integer ones of the latch's two counters.  `active` is one int32
// word on the device: while it is 0 the colour, step and latch launches leave every byte alone.
#include <algorithm>

#include "psg_adam.cuh"
#include "psg_common.h"
#include "psg_scene_lists.cuh"

using namespace psg;

namespace {

constexpr int LATCH_THREADS = 1024;
constexpr unsigned COUNT_BLOCKS = 1024;

// w = atanh(2 c0 - 1) written the reference's way, 0.5 * log((1 + x) / (1 - x)): nu_inverse_tanh_kernel on [n_scene][3]
__global__ void scene_nu_init_kernel(const float *__restrict__ c0, float *__restrict__ w, size_t total)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over n_scene * 3
    if (t >= total) return;
    const float x = __fsub_rn(__fmul_rn(c0[t], 2.0f), 1.0f);
    w[t] = __fmul_rn(0.5f, logf(__fdiv_rn(__fadd_rn(1.0f, x), __fsub_rn(1.0f, x))));
}

// c = 1/2 (tanh(w) + 1) (nu_tanh_color_kernel) for the points that move: under the mask, with at least one slot
__global__ void scene_nu_colour_kernel(const float *__restrict__ w, const uint8_t *__restrict__ scene_mask,
                                       const int32_t *__restrict__ occ_off, const int32_t *__restrict__ active, size_t total,
                                       float *__restrict__ c)
{
    if (!active[0]) return;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over n_scene * 3
    if (t >= total) return;
    const size_t p = t / 3;
    if (scene_mask && !scene_mask[p]) return;
    if (occ_off[p + 1] <= occ_off[p]) return;
    c[t] = __fmul_rn(0.5f, __fadd_rn(tanhf(w[t]), 1.0f));
}

// one thread per (scene point, colour channel): the ordered sums over dx0[e][3 + ch] and over sgrad[e][ch] in one walk of the
// point's slots, then nu_adam_step_kernel's gradient assembly and Adam update with the L2 term of the POINT (once, not once
// per slot)
__global__ void scene_nu_step_kernel(float *__restrict__ w, float *__restrict__ m, float *__restrict__ v, const float *__restrict__ c,
                                     const float *__restrict__ c0, const uint8_t *__restrict__ scene_mask,
                                     const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ_ent,
                                     const float *__restrict__ dx0, const float *__restrict__ sgrad, int rows, size_t total, float cw,
                                     float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                                     const int32_t *__restrict__ active, float *__restrict__ gsum_f_out, float *__restrict__ gsum_s_out)
{
    if (!active[0]) return;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over n_scene * 3
    if (t >= total) return;
    const size_t p = t / 3;
    const int ch = (int)(t % 3);
    float gf = 0.0f, gs = 0.0f;
    bool any = false;
    if (!scene_mask || scene_mask[p])
        any = for_each_slot(occ_off, occ_ent, p, rows, [&](int e) {
            gf = __fadd_rn(gf, dx0[(size_t)e * 9 + 3 + ch]);
            gs = __fadd_rn(gs, sgrad[(size_t)e * 3 + ch]);
        });
    if (gsum_f_out) gsum_f_out[t] = gf;
    if (gsum_s_out) gsum_s_out[t] = gs;
    if (!any) return;                                  // no occurrence (or not under the mask): the point does not move
    const float diff = __fsub_rn(c[t], c0[t]);
    float g = __fadd_rn(gf, __fmul_rn(__fmul_rn(cw, 2.0f), diff));
    g = __fadd_rn(g, __fmul_rn(cw, gs));
    const float th = tanhf(w[t]);
    g = __fmul_rn(__fmul_rn(g, 0.5f), __fsub_rn(1.0f, __fmul_rn(th, th)));
    w[t] = adam_update(w[t], m[t], v[t], g, beta1, beta2, eps, step_size, bc2_sqrt);
}

// the coordinate field, one thread per (scene point, coordinate): the ordered sums over dx0[e][ch] and
// over sgrad_xyz[e][ch] in one walk of the point's slots, then nu_coord_adam_kernel's gradient assembly (psg_nu_field.cuh) and
// the Adam update on the displacement itself - no tanh space, coordinates have no box - with the L2 term of the POINT
__global__ void scene_nu_field_step_kernel(float *__restrict__ delta, float *__restrict__ m, float *__restrict__ v,
                                           const uint8_t *__restrict__ scene_mask, const int32_t *__restrict__ occ_off,
                                           const int32_t *__restrict__ occ_ent, const float *__restrict__ dx0,
                                           const float *__restrict__ sgrad_xyz, int rows, size_t total, float coord_c, float beta1,
                                           float beta2, float eps, float step_size, float bc2_sqrt, const int32_t *__restrict__ active,
                                           float *__restrict__ gsum_x_out, float *__restrict__ gsum_s_out)
{
    if (!active[0]) return;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over n_scene * 3
    if (t >= total) return;
    const size_t p = t / 3;
    const int ch = (int)(t % 3);
    float gx = 0.0f, gs = 0.0f;
    bool any = false;
    if (!scene_mask || scene_mask[p])
        any = for_each_slot(occ_off, occ_ent, p, rows, [&](int e) {
            gx = __fadd_rn(gx, dx0[(size_t)e * 9 + ch]);
            gs = __fadd_rn(gs, sgrad_xyz[(size_t)e * 3 + ch]);
        });
    if (gsum_x_out) gsum_x_out[t] = gx;
    if (gsum_s_out) gsum_s_out[t] = gs;
    if (!any) return;                                  // no occurrence (or not under the mask): the point does not move
    const float d = delta[t];
    float g = __fadd_rn(gx, __fmul_rn(__fmul_rn(coord_c, 2.0f), d));
    g = __fadd_rn(g, __fmul_rn(coord_c, gs));
    delta[t] = adam_update(d, m[t], v[t], g, beta1, beta2, eps, step_size, bc2_sqrt);
}

// counters[0] += slots that hit, counters[1] += slots that count (both zero on entry).  Non-targeted (scene_mask == NULL):
// every slot counts, a hit is pred == label.  Targeted: the slots of points under the mask count (an index out of range
// counts as unmasked), a hit is pred == target.  A grid-stride loop over at most COUNT_BLOCKS workgroups, one integer atomic
// per workgroup and counter: with one per wave the 19 000 waves of a 300 000-point room queued on the two addresses (434 us
// per launch).
__global__ __launch_bounds__(256) void scene_nu_count_kernel(const int32_t *__restrict__ pred, const int32_t *__restrict__ labels,
                                                              int target, const int32_t *__restrict__ point_idx,
                                                              const uint8_t *__restrict__ scene_mask, int rows, int n_scene,
                                                              const int32_t *__restrict__ active, int32_t *__restrict__ counters)
{
    if (!active[0]) return;
    int hit = 0, counted = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)rows; e += (size_t)gridDim.x * blockDim.x) {
        if (scene_mask) {
            const int p = point_idx[e];
            const bool on = p >= 0 && p < n_scene && scene_mask[p];
            counted += on ? 1 : 0;
            hit += (on && pred[e] == target) ? 1 : 0;
        } else {
            counted += 1;
            hit += pred[e] == labels[e] ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        hit += __shfl_down(hit, o);
        counted += __shfl_down(counted, o);
    }
    __shared__ int s_hit[4], s_counted[4];             // (256 threads) the four waves' sums: two atomics per workgroup
    if ((threadIdx.x & 63) == 0) {
        s_hit[threadIdx.x >> 6] = hit;
        s_counted[threadIdx.x >> 6] = counted;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        hit = (s_hit[0] + s_hit[1]) + (s_hit[2] + s_hit[3]);
        counted = (s_counted[0] + s_counted[1]) + (s_counted[2] + s_counted[3]);
        if (hit) atomicAdd(&counters[0], hit);
        if (counted) atomicAdd(&counters[1], counted);
    }
}

// ONE workgroup, launched after the counts have landed: thread 0 reads the counters, files the history row, takes the
// integer decision (64-bit products) and zeroes the counters for the next step; a firing step's colours are copied by the
// whole workgroup (once per attack), then thread 0 records the step and clears `active`.
__global__ __launch_bounds__(LATCH_THREADS) void scene_nu_decide_kernel(int32_t *__restrict__ counters, int targeted, long long num,
                                                                         long long den, int step, const float *__restrict__ c,
                                                                         float *__restrict__ snap, size_t total,
                                                                         long long *__restrict__ hist_row,
                                                                         int32_t *__restrict__ exit_step, int32_t *__restrict__ active)
{
    __shared__ int s_fire;
    if (threadIdx.x == 0) {
        int fire = 0;
        if (active[0]) {
            const long long n_hits = counters[0], n_counted = counters[1];
            counters[0] = 0;
            counters[1] = 0;
            hist_row[0] = n_hits;
            hist_row[1] = n_counted;
            fire = targeted ? (n_hits * den > num * n_counted) : (n_hits * den < num * n_counted);
        }
        s_fire = fire;
    }
    __syncthreads();
    if (!s_fire) return;
    for (size_t t = threadIdx.x; t < total; t += LATCH_THREADS) snap[t] = c[t];
    if (threadIdx.x == 0) {
        exit_step[0] = step;
        active[0] = 0;
    }
}

}  // namespace

extern "C" int psg_scene_nu_init(const float *c0, int n_scene, float *w_out, psg_stream stream)
{
    PSG_REQUIRE(c0 && w_out && n_scene > 0, "psg_scene_nu_init: bad argument");
    const size_t total = (size_t)n_scene * 3;
    hipLaunchKernelGGL(scene_nu_init_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, c0, w_out, total);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_nu_colour(const float *w, const uint8_t *scene_mask, const int32_t *occ_off, int n_scene,
                                   const int32_t *active, float *c, psg_stream stream)
{
    PSG_REQUIRE(w && occ_off && active && c && n_scene > 0, "psg_scene_nu_colour: bad argument");
    const size_t total = (size_t)n_scene * 3;
    hipLaunchKernelGGL(scene_nu_colour_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, w, scene_mask, occ_off,
                       active, total, c);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_nu_step(float *w, float *m, float *v, const float *c, const float *c0, const uint8_t *scene_mask,
                                 const int32_t *occ_off, const int32_t *occ_ent, const float *dx0, const float *sgrad, int rows,
                                 int n_scene, float cw, float lr, float beta1, float beta2, float eps, int step,
                                 const int32_t *active, float *gsum_f_out, float *gsum_s_out, psg_stream stream)
{
    PSG_REQUIRE(w && m && v && c && c0 && occ_off && occ_ent && dx0 && sgrad && active && n_scene > 0 && step >= 1,
                "psg_scene_nu_step: bad argument");
    PSG_REQUIRE(rows_ok(rows), "psg_scene_nu_step: rows=%d outside 1 .. INT_MAX / 9 (slot numbers address [rows][9] floats)", rows);
    const AdamConsts k = adam_consts(lr, beta1, beta2, step);
    const size_t total = (size_t)n_scene * 3;
    hipLaunchKernelGGL(scene_nu_step_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, w, m, v, c, c0, scene_mask,
                       occ_off, occ_ent, dx0, sgrad, rows, total, cw, beta1, beta2, eps, k.step_size, k.bc2_sqrt, active, gsum_f_out,
                       gsum_s_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_nu_field_step(float *delta, float *m, float *v, const uint8_t *scene_mask, const int32_t *occ_off,
                                       const int32_t *occ_ent, const float *dx0, const float *sgrad_xyz, int rows, int n_scene,
                                       float coord_c, float coord_lr, float beta1, float beta2, float eps, int step,
                                       const int32_t *active, float *gsum_x_out, float *gsum_s_out, psg_stream stream)
{
    PSG_REQUIRE(delta && m && v && occ_off && occ_ent && dx0 && sgrad_xyz && active && n_scene > 0 && step >= 1,
                "psg_scene_nu_field_step: bad argument");
    PSG_REQUIRE(rows_ok(rows), "psg_scene_nu_field_step: rows=%d outside 1 .. INT_MAX / 9 (slot numbers address [rows][9] floats)", rows);
    const AdamConsts k = adam_consts(coord_lr, beta1, beta2, step);
    const size_t total = (size_t)n_scene * 3;
    hipLaunchKernelGGL(scene_nu_field_step_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, delta, m, v, scene_mask,
                       occ_off, occ_ent, dx0, sgrad_xyz, rows, total, coord_c, beta1, beta2, eps, k.step_size, k.bc2_sqrt, active,
                       gsum_x_out, gsum_s_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_scene_nu_latch(const int32_t *pred, const int32_t *labels, int target, const int32_t *point_idx,
                                  const uint8_t *scene_mask, int rows, int n_scene, int num, int den, int step, const float *c,
                                  float *snap, int32_t *counters, long long *hist_row, int32_t *exit_step, int32_t *active,
                                  psg_stream stream)
{
    PSG_REQUIRE(pred && c && snap && counters && hist_row && exit_step && active && n_scene > 0 && step >= 0,
                "psg_scene_nu_latch: bad argument");
    PSG_REQUIRE(scene_mask ? point_idx != nullptr : labels != nullptr,
                "psg_scene_nu_latch: the non-targeted test needs labels, the targeted one (scene_mask given) point_idx");
    PSG_REQUIRE(num >= 0 && den > 0, "psg_scene_nu_latch: the exit ratio %d / %d needs num >= 0 and den > 0", num, den);
    PSG_REQUIRE(rows_ok(rows), "psg_scene_nu_latch: rows=%d outside 1 .. INT_MAX / 9", rows);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(scene_nu_count_kernel, dim3(std::min(blocks_for((size_t)rows), COUNT_BLOCKS)), dim3(256), 0, st, pred, labels, target, point_idx,
                       scene_mask, rows, n_scene, active, counters);
    PSG_LAUNCH_CHECK();
    // (the decision in a launch of its own: stream order puts it after every count; no grid-wide wait anywhere)
    hipLaunchKernelGGL(scene_nu_decide_kernel, dim3(1), dim3(LATCH_THREADS), 0, st, counters, scene_mask ? 1 : 0, (long long)num,
                       (long long)den, step, c, snap, (size_t)n_scene * 3, hist_row, exit_step, active);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}
