// Attack-loop arithmetic on gfx950: layout transposes, CE-on-log-probs gradient, the fused
// sign-step / L-inf projection update, and segmentation statistics.  All elementwise / tiny
// reductions: HBM-bound by construction (12-52 bytes per point), coalesced along the point index.
//
// Reference (paths relative to /root/reference):
//   PointNet/attacks/torchattacks/attacks/nontarget.py:26,34-39   NB_attack loss + update
//   PointNet/attacks/torchattacks/attacks/target.py:27,36-43      tar_NB_attack loss + update
//   PointNet/NB_nontarget_test_semseg.py:188-211                  acc / per-class I, U, seen
#include <string.h>

#include "psg_adam.cuh"
#include "psg_ce_row.cuh"
#include "psg_common.h"

namespace {

__global__ void to_point_major_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int N, size_t total)
{
    // one thread per (b, n): reads are coalesced along n for every channel
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        size_t b = t / N, n = t % N;
        for (int c = 0; c < C; ++c) dst[t * C + c] = src[(b * C + c) * N + n];
    }
}

__global__ void to_channel_major_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int N,
                                        size_t total)
{
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        size_t b = t / N, n = t % N;
        for (int c = 0; c < C; ++c) dst[(b * C + c) * N + n] = src[t * C + c];
    }
}

constexpr int MAXC = psg::CE_ROW_MAXC;

// 256 rows per workgroup staged through LDS: the rows of a block are one contiguous piece of logp / dlogp, so global
// accesses are whole cache lines (a thread per row reading its n_cls floats directly strides the lanes 52 bytes apart);
// the per-row arithmetic is unchanged.
__global__ __launch_bounds__(256) void ce_logp_grad_kernel(const float *__restrict__ logp, const int32_t *__restrict__ labels, int target,
                                                            int rows, int rows_active, int n_cls, float scale, float *__restrict__ dlogp,
                                                            float *__restrict__ cost)
{
    __shared__ float s_z[256 * MAXC];
    const int r0 = blockIdx.x * 256, nr = min(256, rows - r0);
    const float *src = logp + (size_t)r0 * n_cls;
    for (int i = threadIdx.x; i < nr * n_cls; i += 256) s_z[i] = src[i];
    __syncthreads();
    const int r = r0 + (int)threadIdx.x;
    float g[MAXC];
    if ((int)threadIdx.x < nr) {
        // (the row arithmetic: psg_ce_row.cuh, shared with the fused fp1 + head launch of the PointNet++ NB loop)
        const bool active = r < rows_active;
        const int y = !active ? -1 : labels ? labels[r] : target;
        const float term = psg::ce_row_grad(s_z + threadIdx.x * n_cls, n_cls, y, scale, active, g);   // (n_cls = 13: an odd stride, conflict-free)
        if (cost && active && y >= 0 && y < n_cls) atomicAdd(cost, term);
    }
    __syncthreads();
    if ((int)threadIdx.x < nr) {
        float *o = s_z + threadIdx.x * n_cls;
        for (int c = 0; c < n_cls; ++c) o[c] = g[c];
    }
    __syncthreads();
    float *dst = dlogp + (size_t)r0 * n_cls;
    for (int i = threadIdx.x; i < nr * n_cls; i += 256) dst[i] = s_z[i];
}

__global__ void pgd_step_kernel(float *__restrict__ x, const float *__restrict__ grad, const float *__restrict__ ori,
                                const uint8_t *__restrict__ mask, int N, size_t total, float step, float eps, int last)
{
    // one thread per (room, point, colour channel); `step` = dir*alpha already rounded to fp32
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total * 3; t += (size_t)gridDim.x * blockDim.x) {
        size_t pt = t / 3;
        int ch = (int)(t % 3);
        if (mask && !mask[pt % N]) continue;
        size_t xi = pt * 9 + 3 + ch;
        float g = grad[xi];
        float sg = g > 0.0f ? 1.0f : (g < 0.0f ? -1.0f : 0.0f);
        float stepped = __fadd_rn(x[xi], __fmul_rn(step, sg));
        float o = ori[t];
        float eta = fminf(fmaxf(__fsub_rn(stepped, o), -eps), eps);
        float proj = fminf(fmaxf(__fadd_rn(o, eta), 0.0f), 1.0f);
        x[xi] = last ? stepped : proj;
    }
}

// The same update on either three-channel field of the rooms: c0 = 3 colours (projection onto the eps ball and [0, 1]),
// c0 = 0 coordinates (eps ball only: metres, not colours)
__global__ void pgd_step_field_kernel(float *__restrict__ x, const float *__restrict__ grad, const float *__restrict__ ori,
                                      const uint8_t *__restrict__ mask, int N, size_t total, int c0, float step, float eps, int last)
{
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total * 3; t += (size_t)gridDim.x * blockDim.x) {
        size_t pt = t / 3;
        int ch = (int)(t % 3);
        if (mask && !mask[pt % N]) continue;
        size_t xi = pt * 9 + c0 + ch;
        float g = grad[xi];
        float sg = g > 0.0f ? 1.0f : (g < 0.0f ? -1.0f : 0.0f);
        float stepped = __fadd_rn(x[xi], __fmul_rn(step, sg));
        float o = ori[t];
        float eta = fminf(fmaxf(__fsub_rn(stepped, o), -eps), eps);
        float proj = __fadd_rn(o, eta);
        if (c0 == 3) proj = fminf(fmaxf(proj, 0.0f), 1.0f);
        x[xi] = last ? stepped : proj;
    }
}

__global__ void seg_stats_kernel(const float *__restrict__ logp, const int32_t *__restrict__ labels, int rows,
                                 int n_cls, unsigned long long *__restrict__ counters, int32_t *__restrict__ pred_out)
{
    __shared__ unsigned int h[3 * MAXC];
    for (int i = threadIdx.x; i < 3 * MAXC; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const float *lp = logp + (size_t)r * n_cls;
        float best = lp[0];
        int bi = 0;
        for (int c = 1; c < n_cls; ++c)
            if (lp[c] > best) { best = lp[c]; bi = c; }
        const int y = labels[r];
        if (pred_out) pred_out[r] = bi;
        atomicAdd(&h[y], 1u);                    // seen
        if (bi == y) {
            atomicAdd(&h[MAXC + y], 1u);         // intersection
            atomicAdd(&h[2 * MAXC + y], 1u);     // union
        } else {
            atomicAdd(&h[2 * MAXC + y], 1u);
            atomicAdd(&h[2 * MAXC + bi], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * n_cls; i += blockDim.x) {
        int k = i / n_cls, c = i % n_cls;
        unsigned v = h[k * MAXC + c];
        if (v) atomicAdd(&counters[k * n_cls + c], (unsigned long long)v);
    }
}

inline int grid_for(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 2048); }

}  // namespace

extern "C" int psg_to_point_major(const float *src_cn, int B, int C, int N, float *dst_nc, psg_stream stream)
{
    PSG_REQUIRE(src_cn && dst_nc && B > 0 && C > 0 && N > 0, "psg_to_point_major: bad argument");
    size_t total = (size_t)B * N;
    hipLaunchKernelGGL(to_point_major_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src_cn, dst_nc, C,
                       N, total);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_to_channel_major(const float *src_nc, int B, int C, int N, float *dst_cn, psg_stream stream)
{
    PSG_REQUIRE(src_nc && dst_cn && B > 0 && C > 0 && N > 0, "psg_to_channel_major: bad argument");
    size_t total = (size_t)B * N;
    hipLaunchKernelGGL(to_channel_major_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src_nc, dst_cn,
                       C, N, total);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_ce_logp_grad(const float *logp, const int32_t *labels, int target, int rows, int rows_active,
                                int n_cls, float scale, float *dlogp_out, float *cost_out, psg_stream stream)
{
    PSG_REQUIRE(logp && dlogp_out && rows > 0, "psg_ce_logp_grad: bad argument");
    PSG_REQUIRE(n_cls > 0 && n_cls <= MAXC, "psg_ce_logp_grad: n_cls=%d out of range (1..%d)", n_cls, MAXC);
    PSG_REQUIRE(labels || (target >= 0 && target < n_cls), "psg_ce_logp_grad: target class %d out of range", target);
    PSG_REQUIRE(rows_active >= 0 && rows_active <= rows, "psg_ce_logp_grad: rows_active out of range");
    hipLaunchKernelGGL(ce_logp_grad_kernel, dim3(psg::ceil_div(rows, 256)), dim3(256), 0, (hipStream_t)stream, logp,
                       labels, target, rows, rows_active, n_cls, scale, dlogp_out, cost_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_pgd_step(float *x, const float *grad, const float *ori, const uint8_t *mask, int B, int N,
                            float alpha, float eps, float dir, int last, psg_stream stream)
{
    PSG_REQUIRE(x && grad && ori && B > 0 && N > 0, "psg_pgd_step: bad argument");
    size_t total = (size_t)B * N;
    hipLaunchKernelGGL(pgd_step_kernel, dim3(grid_for(total * 3)), dim3(256), 0, (hipStream_t)stream, x, grad, ori, mask,
                       N, total, dir * alpha, eps, last);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_pgd_step_field(float *x, const float *grad, const float *ori, const uint8_t *mask, int B, int N, int c0,
                                  float alpha, float eps, float dir, int last, psg_stream stream)
{
    PSG_REQUIRE(x && grad && ori && B > 0 && N > 0, "psg_pgd_step_field: bad argument");
    PSG_REQUIRE(c0 == 0 || c0 == 3, "psg_pgd_step_field: channel offset %d is neither 0 (coordinates) nor 3 (colours)", c0);
    size_t total = (size_t)B * N;
    hipLaunchKernelGGL(pgd_step_field_kernel, dim3(grid_for(total * 3)), dim3(256), 0, (hipStream_t)stream, x, grad, ori, mask,
                       N, total, c0, dir * alpha, eps, last);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_seg_stats(const float *logp, const int32_t *labels, int rows, int n_cls, long long *counters,
                             int32_t *pred_out, psg_stream stream)
{
    PSG_REQUIRE(logp && labels && counters && rows > 0, "psg_seg_stats: bad argument");
    PSG_REQUIRE(n_cls > 0 && n_cls <= MAXC, "psg_seg_stats: n_cls=%d out of range (1..%d)", n_cls, MAXC);
    hipLaunchKernelGGL(seg_stats_kernel, dim3(std::min(256, psg::ceil_div(rows, 256))), dim3(256), 0,
                       (hipStream_t)stream, logp, labels, rows, n_cls, (unsigned long long *)counters, pred_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// =============================================================================================
// Whole-scene evaluation harness: vote pool, vote arg-max statistics, L2 distance.
// Reference: PointNet/NB_nontarget_test_semseg.py:55-62 (add_vote), :184 (torch.dist), :219-241 (per-scene IoU).
// =============================================================================================
namespace {

// pool[point_idx[r]][argmax logp[r]] += 1 where weight[r] != 0 (integer votes: the adds commute, result exact)
__global__ void vote_add_kernel(const float *__restrict__ logp, const int32_t *__restrict__ pred_in,
                                const int32_t *__restrict__ point_idx, const float *__restrict__ weight, int rows,
                                int n_cls, int n_points, int32_t *__restrict__ pool, int *__restrict__ bad)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        if (weight && weight[r] == 0.0f) continue;
        int bi;
        if (pred_in) bi = pred_in[r];
        else {
            const float *lp = logp + (size_t)r * n_cls;
            float best = lp[0];
            bi = 0;
            for (int c = 1; c < n_cls; ++c)
                if (lp[c] > best) { best = lp[c]; bi = c; }
        }
        const int p = point_idx[r];
        if (p < 0 || p >= n_points || bi < 0 || bi >= n_cls) { atomicOr(bad, 1); continue; }
        atomicAdd(&pool[(size_t)p * n_cls + bi], 1);
    }
}

// per scene: pred = argmax over the votes (first index on ties, np.argmax), then the seen / correct / union counters
__global__ void vote_stats_kernel(const int32_t *__restrict__ pool, const int32_t *__restrict__ labels, int n_points,
                                  int n_cls, unsigned long long *__restrict__ counters, int32_t *__restrict__ pred_out)
{
    __shared__ unsigned int h[3 * MAXC];
    for (int i = threadIdx.x; i < 3 * MAXC; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n_points; p += gridDim.x * blockDim.x) {
        const int32_t *v = pool + (size_t)p * n_cls;
        int best = v[0], bi = 0;
        for (int c = 1; c < n_cls; ++c)
            if (v[c] > best) { best = v[c]; bi = c; }
        const int y = labels[p];
        if (pred_out) pred_out[p] = bi;
        atomicAdd(&h[y], 1u);
        if (bi == y) {
            atomicAdd(&h[MAXC + y], 1u);
            atomicAdd(&h[2 * MAXC + y], 1u);
        } else {
            atomicAdd(&h[2 * MAXC + y], 1u);
            atomicAdd(&h[2 * MAXC + bi], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * n_cls; i += blockDim.x) {
        int k = i / n_cls, c = i % n_cls;
        unsigned v = h[k * MAXC + c];
        if (v) atomicAdd(&counters[k * n_cls + c], (unsigned long long)v);
    }
}

// sum of squared differences in double (one partial per workgroup, fixed tree inside the workgroup; the final sum
// over <= 256 partials runs on one thread in index order): deterministic
__global__ void sqdiff_partial_kernel(const float *__restrict__ a, const float *__restrict__ b, size_t n,
                                      double *__restrict__ part)
{
    __shared__ double sh[256];
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double d = (double)a[i] - (double)b[i];
        acc += d * d;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ void sqdiff_final_kernel(const double *__restrict__ part, int n_part, float *__restrict__ out)
{
    double acc = 0.0;
    for (int i = 0; i < n_part; ++i) acc += part[i];
    out[0] = (float)sqrt(acc);
}

}  // namespace

extern "C" int psg_vote_add(const float *logp, const int32_t *pred, const int32_t *point_idx, const float *weight,
                            int rows, int n_cls, int n_points, int32_t *pool, int32_t *bad_flag, psg_stream stream)
{
    PSG_REQUIRE((logp || pred) && point_idx && pool && bad_flag && rows > 0 && n_points > 0, "psg_vote_add: bad argument");
    PSG_REQUIRE(n_cls > 0 && n_cls <= MAXC, "psg_vote_add: n_cls=%d out of range (1..%d)", n_cls, MAXC);
    hipLaunchKernelGGL(vote_add_kernel, dim3(grid_for((size_t)rows)), dim3(256), 0, (hipStream_t)stream, logp, pred,
                       point_idx, weight, rows, n_cls, n_points, pool, bad_flag);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_vote_stats(const int32_t *pool, const int32_t *labels, int n_points, int n_cls, long long *counters,
                              int32_t *pred_out, psg_stream stream)
{
    PSG_REQUIRE(pool && labels && counters && n_points > 0, "psg_vote_stats: bad argument");
    PSG_REQUIRE(n_cls > 0 && n_cls <= MAXC, "psg_vote_stats: n_cls=%d out of range (1..%d)", n_cls, MAXC);
    hipLaunchKernelGGL(vote_stats_kernel, dim3(std::min(256, psg::ceil_div(n_points, 256))), dim3(256), 0,
                       (hipStream_t)stream, pool, labels, n_points, n_cls, (unsigned long long *)counters, pred_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_l2_dist(const float *a, const float *b, size_t n, double *scratch256, float *out, psg_stream stream)
{
    PSG_REQUIRE(a && b && scratch256 && out && n > 0, "psg_l2_dist: bad argument");
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 256);
    hipLaunchKernelGGL(sqdiff_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, b, n, scratch256);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(sqdiff_final_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, scratch256, blocks, out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// =============================================================================================
// NU (norm-unbounded, Adam in tanh space) attack arithmetic.
// Reference: PointNet/attacks/torchattacks/attacks/nontarget.py:52-135 (NU_attack),
//            PointNet/attacks/torchattacks/attacks/target.py:62-175 (tar_NU_attack).
// =============================================================================================
namespace {

// w = atanh(2c - 1) written the reference's way: 0.5*log((1+x)/(1-x))  (nontarget.py:110-116)
__global__ void nu_inverse_tanh_kernel(const float *__restrict__ x0, float *__restrict__ w, size_t rows)
{
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows * 3; t += (size_t)gridDim.x * blockDim.x) {
        float c = x0[(t / 3) * 9 + 3 + (t % 3)];
        float x = __fsub_rn(__fmul_rn(c, 2.0f), 1.0f);
        w[t] = __fmul_rn(0.5f, logf(__fdiv_rn(__fadd_rn(1.0f, x), __fsub_rn(1.0f, x))));
    }
}

// colour = 1/2 * (tanh(w) + 1)  (nontarget.py:107-108) written into channels 3:6 of x0, masked points only
__global__ void nu_tanh_color_kernel(const float *__restrict__ w, const uint8_t *__restrict__ mask, float *__restrict__ x0,
                                     int N, size_t rows, int mask_per_room)
{
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows * 3; t += (size_t)gridDim.x * blockDim.x) {
        size_t pt = t / 3;
        if (mask && !mask[mask_per_room ? pt : pt % N]) continue;
        x0[pt * 9 + 3 + (t % 3)] = __fmul_rn(0.5f, __fadd_rn(tanhf(w[t]), 1.0f));
    }
}

// f-loss of the paper on softmax(log-probs) + its gradient w.r.t. the log-probs (nontarget.py:119-128,
// target.py:148-168): f = clamp(tsign * (p_y - max_{k != y} p_k), min = -kappa), summed over points.
__global__ void nu_f_loss_grad_kernel(const float *__restrict__ logp, const int32_t *__restrict__ labels, int target,
                                      int rows, int n_cls, float kappa, float tsign, float *__restrict__ dlogp,
                                      float *__restrict__ f_sum, int32_t *__restrict__ pred, int rows_per_sum)
{
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    float fval = 0.0f;
    if (r < rows) {
        const float *lp = logp + (size_t)r * n_cls;
        float p[MAXC];
        float m = -INFINITY;
        int am = 0;
        for (int c = 0; c < n_cls; ++c) {
            p[c] = lp[c];
            if (p[c] > m) { m = p[c]; am = c; }
        }
        if (pred) pred[r] = am;
        float s = 0.0f;
        for (int c = 0; c < n_cls; ++c) { p[c] = expf(p[c] - m); s += p[c]; }
        for (int c = 0; c < n_cls; ++c) p[c] = p[c] / s;
        const int y = labels ? labels[r] : target;
        float oth = -1.0f;
        int oi = 0;
        for (int c = 0; c < n_cls; ++c)
            if (c != y && p[c] > oth) { oth = p[c]; oi = c; }
        if (oth < 0.0f) oth = 0.0f;  // (1 - onehot) * p is 0 at the true class: the max is never below 0
        const float val = tsign * (p[y] - oth);
        const bool pass = val >= -kappa;
        fval = pass ? val : -kappa;
        const float gy = pass ? tsign : 0.0f, go = pass ? -tsign : 0.0f;
        const float dot = gy * p[y] + go * p[oi];
        float *g = dlogp + (size_t)r * n_cls;
        for (int c = 0; c < n_cls; ++c) {
            float gc = c == y ? gy : (c == oi ? go : 0.0f);
            g[c] = p[c] * (gc - dot);
        }
    }
    // reduction of the f values (rows_per_sum > 0: one sum per room, a multiple of 64 rows each).  One atomic per
    // workgroup when all its rows belong to one sum, else one per wave: thousands of waves adding into a handful of
    // addresses serialise on them (the per-room launches spent most of their time there).
    for (int o = 32; o >= 1; o >>= 1) fval += __shfl_xor(fval, o);
    if (!f_sum) return;
    if (rows_per_sum == 0 || rows_per_sum % (int)blockDim.x == 0) {
        __shared__ float s_part[16];
        const int wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
        if ((threadIdx.x & 63) == 0) s_part[wv] = fval;
        __syncthreads();
        if (threadIdx.x == 0) {
            float tot = 0.0f;
            for (int w = 0; w < nw; ++w) tot += s_part[w];
            const int r0 = blockIdx.x * blockDim.x;
            if (r0 < rows) atomicAdd(f_sum + (rows_per_sum ? r0 / rows_per_sum : 0), tot);
        }
    } else if ((threadIdx.x & 63) == 0 && r < rows) {
        atomicAdd(f_sum + r / rows_per_sum, fval);
    }
}

// f-loss of the ResGCN NU attacks, on raw logits (ResGCN/.../attacks/colper.py:108-113, tcolper.py:145-163).
// The reference multiplies the logits by one-hot masks before torch.max, so a masked-out slot contributes a 0:
//   mode 0 (NU_attack.f):        j = max(z_y, 0),            i = max(max_{k!=y} z_k, 0),  f = clamp(t*(j - i), -kappa)
//   mode 1 (tar_NU non_f):       j = z_y,                    i = max(max_{k!=y} z_k, 0),  f = clamp(t*(j - i), -kappa)
//   mode 2 (tar_NU tar_f, y=T):  j = max(max_{k!=T} z_k, 0), i = z_T,                     f = clamp(t*(j - i), -kappa)
// Modes 1/2 only count batch row 0 under `mask` ([0][self.mask] in the reference).  Writes scale * d(sum f)/dz.
__global__ void gcn_f_loss_grad_kernel(const float *__restrict__ z, const int32_t *__restrict__ labels, int target,
                                       const uint8_t *__restrict__ mask, int mode, int rows, int N, int n_cls, float kappa,
                                       float tsign, float scale, float *__restrict__ dz, float *__restrict__ f_sum,
                                       int32_t *__restrict__ pred)
{
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    float fval = 0.0f;
#include "psg_gcn_f_loss_row.cuh"
    for (int o = 32; o >= 1; o >>= 1) fval += __shfl_xor(fval, o);
    if ((threadIdx.x & 63) == 0 && f_sum) atomicAdd(f_sum, fval);
}

// The same rows for G one-room attacks in lockstep (psg_gcn_f_loss_grad_rooms): blockIdx.y = room, every room under its own
// mask row - what the kernel above does for a batch of one.  One atomic per workgroup into the room's sum.
__global__ __launch_bounds__(256) void gcn_f_loss_grad_rooms_kernel(const float *__restrict__ z, const int32_t *__restrict__ labels,
                                                                     int target, const uint8_t *__restrict__ mask, int mode, int N,
                                                                     int n_cls, float kappa, float tsign, float scale,
                                                                     float *__restrict__ dz, float *__restrict__ f_sum,
                                                                     int32_t *__restrict__ pred)
{
    const size_t base = (size_t)blockIdx.y * N;
    z += base * n_cls; dz += base * n_cls;
    if (pred) pred += base;
    if (labels) labels += base;
    if (mask) mask += base;
    const int rows = N, r = blockIdx.x * blockDim.x + threadIdx.x;
    float fval = 0.0f;
#include "psg_gcn_f_loss_row.cuh"
    for (int o = 32; o >= 1; o >>= 1) fval += __shfl_xor(fval, o);
    __shared__ float s_part[4];
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = fval;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(f_sum + blockIdx.y, (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]));
}

// Smooth loss (nontarget.py:131-135): for every adversarial colour of a room the `nb` smallest Euclidean distances to the
// reference colours; returns their sum and d(sum)/d(adv colour).
// A workgroup of 1024 threads stages the room's reference colours (+ |r|^2) in LDS once and serves 256 queries, FOUR lanes per
// query: each scans every 4th reference keeping its own sorted top-NBT in registers (a sorted insertion with static
// indexing; after the first few hundred references almost every candidate fails the one compare against the list's last
// entry), then the four short lists are merged nb times through two DPP-sized shuffles by (distance, index) - the lower
// index wins a tie, as a sequential scan with a strict '<' would - and the winner shifts its list.  Two workgroups (32
// waves) share a CU, and a 32-room lockstep launch (psg_smooth_knn_rooms) is exactly one round of 512 workgroups.
// (Round 2's version gave 16 lanes and a 64-KB staging copy to every 16 queries and merged in one lane: 2 workgroups =
// 8 waves per CU, 122 us for one room and 2.2 ms for 32 - half of the GPU time of a lockstep tar_NU step.)
constexpr int SM_MAX_NB = 16;
constexpr int SM_T = 1024;
constexpr int SM_REFRESH = 64;              // scan iterations between two updates of the query's common threshold
// SUB = lanes per query (4: 256 queries per workgroup, for launches of 16+ rooms; 16: 64 queries per workgroup, so that a
// one-room call still spreads over 64 workgroups)

// one step of the SUB-way merge: the smallest head of the query's SUB sorted lists by (distance, index) is returned in
// every lane of the query and popped from the one list that holds it (reference indices are unique across the lists;
// exhausted lists show (inf, 0x7FFFFFFF) and may pop together, which changes nothing)
template <int NBT, int SM_SUB>
__device__ __forceinline__ void smooth_pop_min(float (&bd)[NBT], int (&bi)[NBT], float &best, int &bidx)
{
    best = bd[0];
    bidx = bi[0];
#pragma unroll
    for (int o = 1; o < SM_SUB; o <<= 1) {
        const float od = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        if (od < best || (od == best && oi < bidx)) { best = od; bidx = oi; }
    }
    if (bi[0] == bidx) {
#pragma unroll
        for (int u = 0; u + 1 < NBT; ++u) { bd[u] = bd[u + 1]; bi[u] = bi[u + 1]; }
        bd[NBT - 1] = INFINITY; bi[NBT - 1] = 0x7FFFFFFF;
    }
}

typedef float sm_v2f __attribute__((ext_vector_type(2)));   // operand of the packed-fp32 pipe (v_pk_*_f32)

template <int NBT, int SM_SUB>
__global__ __launch_bounds__(SM_T) void smooth_knn_kernel(const float *__restrict__ adv, int adv_stride,
                                                          const float *__restrict__ ref, int ref_stride, int N, int nb,
                                                          float *__restrict__ dist_sum, float *__restrict__ grad, int symmetric,
                                                          size_t adv_room_stride, size_t ref_room_stride,
                                                          int32_t *__restrict__ nn_io, int have_prev)
{
    // Equal distances INSIDE one lane's list: the insertion below moves a displaced entry past the entries of equal distance
    // behind it (the compare is strict for the carried entry too), so references at exactly the same distance from a query can
    // leave a lane in descending index order - and, with a full list, the lower index can be the one that falls out.  Between
    // lanes the merge is by (distance, index).  The results of the PointNet / PointNet++ NU loops and of the one-room ResGCN
    // loop are pinned with this behaviour, so it stays; smooth_knn_sym_own_kernel runs the same text with the stable insertion.
    constexpr bool SM_STABLE_TIES = false;
#include "psg_smooth_knn_body.cuh"
}

// ---- smooth(adv, adv) of the ResGCN NU attacks for G rooms in lockstep, WITHOUT float atomics on the gradient
// (psg_smooth_knn_sym_rooms; colper.py:115-120).  Two launches:
//   1. the scan above with the room's own colours as references, one-sided: grad[i] = sum over i's neighbours in ascending
//      rank of u(i, j) = (a_i - a_j) / d(i, j), the lists to nn, the distances to the room's sum.  A room that has left its
//      loop is skipped.
//   2. smooth_sym_incoming_kernel: grad[i] -= u(k, i) for every k that holds i among its neighbours, in ascending k.
// The second pass finds those k without inverse lists (at nb = 10, N = 4096 the flat lists alone are 160 KB: a room's would
// not fit beside anything in LDS, and in memory they need a counting pass, a scan and a sort): colour i is a neighbour of
// k exactly when (d(k, i), i) <= (d(k, j*), j*) for k's LAST neighbour j* - the selection is a total order by (distance,
// index) - so every workgroup stages each k's colour and that key (one gather per k) in 24-byte LDS slots, 2048 k at a
// time, and a colour's 16 lanes walk the k in ascending order 16 at a time, evaluating d(k, i) with k in the query's role
// exactly as pass 1 did (the expansion is not symmetric in fp32).  Hits are rare (nb per N), the wave branches on a ballot.
template <int NBT, int SM_SUB>
__global__ __launch_bounds__(SM_T) void smooth_knn_sym_own_kernel(const float *__restrict__ adv, int adv_stride, int N, int nb,
                                                                  float *__restrict__ dist_sum, float *__restrict__ grad,
                                                                  size_t adv_room_stride, int32_t *__restrict__ nn_io,
                                                                  const uint8_t *__restrict__ room_active)
{
    if (room_active && !room_active[blockIdx.y]) return;
    // one-sided, the room's own colours as references, no warm start; equal distances strictly by index (see above)
    constexpr bool SM_STABLE_TIES = true;
    const float *ref = adv;
    const int ref_stride = adv_stride, symmetric = 0, have_prev = 0;
    const size_t ref_room_stride = adv_room_stride;
#include "psg_smooth_knn_body.cuh"
}

constexpr int SI_T = 1024;                  // threads of the second pass
constexpr int SI_SUB = 16;                  // lanes per colour
constexpr int SI_TILE = 2048;               // k staged at a time: 2048 x (16 + 8) bytes = 48 KB

__global__ __launch_bounds__(SI_T) void smooth_sym_incoming_kernel(const float *__restrict__ adv, int adv_stride, size_t adv_room_stride,
                                                                   int N, int nb, const int32_t *__restrict__ nn,
                                                                   float *__restrict__ grad, const uint8_t *__restrict__ room_active)
{
    if (room_active && !room_active[blockIdx.y]) return;
    adv += blockIdx.y * adv_room_stride;
    nn += (size_t)blockIdx.y * N * nb;
    grad += (size_t)blockIdx.y * N * 3;
    __shared__ float4 s_k[SI_TILE];         // {-2 x, -2 y, -2 z, |a|^2} of colour k, as the query of pass 1 holds them
    __shared__ float2 s_key[SI_TILE];       // k's last neighbour: {clamped d^2, index bits}; d^2 = -1: no such k
    const int sub = threadIdx.x % SI_SUB;
    const int i = blockIdx.x * (SI_T / SI_SUB) + threadIdx.x / SI_SUB;
    const int last = (nb < N ? nb : N) - 1;                     // rank of the last neighbour every colour holds
    float rx = 0.f, ry = 0.f, rz = 0.f, rq = 0.f;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (i < N) {
        rx = adv[(size_t)i * adv_stride]; ry = adv[(size_t)i * adv_stride + 1]; rz = adv[(size_t)i * adv_stride + 2];
        rq = rx * rx + ry * ry + rz * rz;                       // |r|^2 as pass 1 stages it
        gx = grad[(size_t)i * 3]; gy = grad[(size_t)i * 3 + 1]; gz = grad[(size_t)i * 3 + 2];   // own terms (pass 1)
    }
    for (int k0 = 0; k0 < N; k0 += SI_TILE) {
        if (k0) __syncthreads();
        for (int t = threadIdx.x; t < SI_TILE; t += SI_T) {
            const int k = k0 + t;
            float4 q = {0.f, 0.f, 0.f, 0.f};
            float2 key = {-1.0f, 0.0f};
            if (k < N) {
                const float ax = adv[(size_t)k * adv_stride], ay = adv[(size_t)k * adv_stride + 1], az = adv[(size_t)k * adv_stride + 2];
                q = float4{-2.0f * ax, -2.0f * ay, -2.0f * az, ax * ax + ay * ay + az * az};
                const int j = nn[(size_t)k * nb + last];
                if (j >= 0 && j < N) {
                    const float jx = adv[(size_t)j * adv_stride], jy = adv[(size_t)j * adv_stride + 1], jz = adv[(size_t)j * adv_stride + 2];
                    float d2 = __fmaf_rn(q.z, jz, __fmaf_rn(q.y, jy, __fmul_rn(q.x, jx)));
                    d2 = __fadd_rn(__fadd_rn(d2, q.w), jx * jx + jy * jy + jz * jz);
                    key = float2{fmaxf(d2, 0.0f), __int_as_float(j)};
                }
            }
            s_k[t] = q;
            s_key[t] = key;
        }
        __syncthreads();
        const int nt = min(SI_TILE, N - k0);
        for (int t = sub; t < nt + sub; t += SI_SUB) {          // (the 16 lanes of a colour stay together: t - sub < nt)
            const bool in = t < nt && i < N;
            const float4 q = s_k[in ? t : 0];
            const float2 key = s_key[in ? t : 0];
            float d2 = __fmaf_rn(q.z, rz, __fmaf_rn(q.y, ry, __fmul_rn(q.x, rx)));
            d2 = fmaxf(__fadd_rn(__fadd_rn(d2, q.w), rq), 0.0f);
            const bool hit = in && (d2 < key.x || (d2 == key.x && i <= __float_as_int(key.y)));
            const unsigned long long bal = __ballot(hit);
            if (bal == 0ull) continue;                           // (uniform over the wave)
            float ux = 0.f, uy = 0.f, uz = 0.f;
            if (hit) {
                const float d = sqrtf(d2);
                if (d > 0.0f) { ux = (-0.5f * q.x - rx) / d; uy = (-0.5f * q.y - ry) / d; uz = (-0.5f * q.z - rz) / d; }
            }
            // the hits of this colour's 16 lanes, in lane (= ascending k) order; the lanes of a colour see the same bits
            unsigned mine = (unsigned)(bal >> (threadIdx.x & 48)) & 0xFFFFu;
            while (mine) {
                const int s = __ffs(mine) - 1;
                mine &= mine - 1;
                gx -= __shfl(ux, s, SI_SUB); gy -= __shfl(uy, s, SI_SUB); gz -= __shfl(uz, s, SI_SUB);
            }
        }
    }
    if (sub == 0 && i < N) { grad[(size_t)i * 3] = gx; grad[(size_t)i * 3 + 1] = gy; grad[(size_t)i * 3 + 2] = gz; }
}

// Gradient assembly + torch.optim.Adam single-tensor update on w (fp32, torch's operation order).
// Set by psg_pn2_nu_window while it enqueues the steps of a window that is (or will be) replayed as a hipGraph: the Adam
// step and the latch of step i then read {step, lr / (1 - beta1^t), sqrt(1 - beta2^t)} from this device row instead of their
// arguments.  Null everywhere else.
static thread_local const float *g_nu_dconsts = nullptr;

__global__ void nu_adam_step_kernel(float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                    const uint8_t *__restrict__ mask, const float *__restrict__ dx0,
                                    const float *__restrict__ x0, const float *__restrict__ ori,
                                    const float *__restrict__ smooth_grad, float c_smooth, float c_l2, float beta1,
                                    float beta2, float eps, float step_size, float bc2_sqrt, int N, size_t rows,
                                    float *__restrict__ l2_sum, const uint8_t *__restrict__ room_active,
                                    const float *__restrict__ dconsts)
{
    // (a replayed hipGraph cannot change kernel arguments: the step-dependent constants of a captured window come from memory)
    if (dconsts) { step_size = dconsts[1]; bc2_sqrt = dconsts[2]; }
    // gridDim.y > 1: slice y is one room of a lockstep batch (rows = N) with its own mask row, smoothness gradient and
    // L2 sum; a room that has left its loop (room_active[y] == 0) is not touched.  gridDim.y == 1: the reference's batch
    // call (rows = B N, one mask, the smoothness gradient on batch row 0 only, one sum).
    if (gridDim.y > 1) {
        const size_t y = blockIdx.y, o3 = y * rows * 3;
        if (room_active && !room_active[y]) return;
        w += o3; m += o3; v += o3; ori += o3;
        dx0 += y * rows * 9; x0 += y * rows * 9;
        if (mask) mask += y * rows;
        if (smooth_grad) smooth_grad += o3;
        if (l2_sum) l2_sum += y;
    }
    float l2 = 0.0f;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows * 3; t += (size_t)gridDim.x * blockDim.x) {
        const size_t pt = t / 3;
        const int ch = (int)(t % 3);
        if (mask && !mask[pt % N]) continue;
        const float color = x0[pt * 9 + 3 + ch];
        const float diff = color - ori[t];
        l2 += diff * diff;
        float g = dx0[pt * 9 + 3 + ch] + c_l2 * 2.0f * diff;
        if (smooth_grad && pt < (size_t)N) g += c_smooth * smooth_grad[t];
        const float th = tanhf(w[t]);
        g = g * 0.5f * (1.0f - th * th);
        w[t] = psg::adam_update(w[t], m[t], v[t], g, beta1, beta2, eps, step_size, bc2_sqrt);
    }
    for (int o = 32; o >= 1; o >>= 1) l2 += __shfl_xor(l2, o);
    if (!l2_sum) return;
    __shared__ float s_l2[4];                                  // (256 threads) one atomic per workgroup
    if ((threadIdx.x & 63) == 0) s_l2[threadIdx.x >> 6] = l2;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(l2_sum, (s_l2[0] + s_l2[1]) + (s_l2[2] + s_l2[3]));
}

}  // namespace

__device__ __forceinline__ unsigned wave_reduce_add_u32(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_down((int)v, o);
    return v;            // lane 0 holds the sum
}

// ---- Per-step statistics and EXIT LATCH of the NU attacks on the device (round 4): what the reference evaluates on the
// host after every optimiser step (nontarget.py:87,95-96 `correct / 4096 < 1 / 13`; target.py:105-121 `target_acc`
// against 0.9 or 1 / 13) and what made the host loop wait for a read-back per step.  One workgroup per attack (a group of
// `rows` batch rows: rows = B for one call on a batch, rows = 1 for the lockstep rooms).  It counts the correct points and
// the target hits, files them with the step's f / Smooth / L2 sums (scal [3][G], zeroed here for the next step) into the
// history row hist_step [5][G], and evaluates the exit test in double precision exactly as the host did; the FIRST step
// whose test fires snapshots the group's image (x0 point-major -> out channel-major), records the step and clears the
// group's active byte (the lockstep optimiser skips inactive rooms).  The host then only reads the history where the
// reference itself has to touch the host: after step 0, after every 10th step (restart test + noise draw, lr halving)
// and at the end; a group that exits at step s returns its step-s image, at most 9 later steps are speculation.
__global__ __launch_bounds__(256) void nu_step_latch_kernel(const int32_t *__restrict__ pred, const int32_t *__restrict__ labels,
                                                             int target, const uint8_t *__restrict__ mask,
                                                             const int32_t *__restrict__ n_mask, int rows, int N, int mode,
                                                             float *__restrict__ scal, float *__restrict__ hist_step,
                                                             const float *__restrict__ x0, float *__restrict__ out,
                                                             uint8_t *__restrict__ active, int32_t *__restrict__ exit_step, int step,
                                                             int G, const float *__restrict__ dconsts)
{
    if (dconsts) step = __float_as_int(dconsts[0]);
    __shared__ unsigned s_cnt[2];
    __shared__ int s_exit;
    const int g = blockIdx.x, tid = threadIdx.x;
    if (tid < 2) s_cnt[tid] = 0u;
    __syncthreads();
    const size_t base = (size_t)g * rows * N;
    unsigned nc = 0, nt = 0;
    for (size_t i = tid; i < (size_t)rows * N; i += blockDim.x) {
        const int p = pred[base + i];
        const bool ok = p == labels[base + i];
        const bool in_mask = mask ? mask[(size_t)g * N + i % N] != 0 : true;
        nc += ok ? 1u : 0u;
        // mode 0: the non-targeted attack (hits = correct); 1: the targeted class's untargeted goal (correct, on the mask);
        // 2: targeted (predicted == target, on the mask)
        nt += (mode == 2 ? p == target : ok) && (mode == 0 || in_mask) ? 1u : 0u;
    }
    nc = wave_reduce_add_u32(nc);
    nt = wave_reduce_add_u32(nt);
    if ((tid & 63) == 0) { atomicAdd(&s_cnt[0], nc); atomicAdd(&s_cnt[1], nt); }
    __syncthreads();
    if (tid == 0) {
        const unsigned n_correct = s_cnt[0], n_tgt = s_cnt[1];
        hist_step[0 * G + g] = (float)n_correct;
        hist_step[1 * G + g] = (float)n_tgt;
#pragma unroll
        for (int k = 0; k < 3; ++k) { hist_step[(2 + k) * G + g] = scal[k * G + g]; scal[k * G + g] = 0.0f; }
        bool fire;
        if (mode == 0) fire = (double)n_correct / 4096.0 < 1.0 / 13.0;                       // nontarget.py:87,95
        else {
            const double acc = (double)n_tgt / (double)n_mask[g];                            // target.py:105,113 (0 / 0 = NaN: never fires)
            fire = mode == 2 ? acc > 0.9 : acc < 1.0 / 13.0;                                 // target.py:116-121
        }
        s_exit = fire && active[g] && exit_step[g] < 0 ? 1 : 0;
    }
    __syncthreads();
    if (!s_exit) return;
    if (rows == 1) {                       // (a batch of rows is copied by nu_latch_snapshot_kernel, a full grid)
        const float *src = x0 + base * 9;
        float *dst = out + base * 9;
        for (int i = tid; i < N * 9; i += blockDim.x) dst[(i % 9) * N + i / 9] = src[i];
    }
    if (tid == 0) { exit_step[g] = step; active[g] = 0; }
}

// the snapshot of a group of several batch rows whose exit test has just fired (exit_step[g] == step): x0 -> out, transposed
__global__ void nu_latch_snapshot_kernel(const float *__restrict__ x0, float *__restrict__ out, const int32_t *__restrict__ exit_step,
                                         int step, int rows, int N, size_t total, const float *__restrict__ dconsts)
{
    if (dconsts) step = __float_as_int(dconsts[0]);
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t per_group = (size_t)rows * N * 9;
    if (exit_step[t / per_group] != step) return;
    const size_t row = t / ((size_t)N * 9), i = t % ((size_t)N * 9);       // destination element i = c * N + n of this row
    out[t] = x0[row * N * 9 + (i % N) * 9 + i / N];
}

extern "C" int psg_nu_inverse_tanh(const float *x0, int B, int N, float *w_out, psg_stream stream)
{
    PSG_REQUIRE(x0 && w_out && B > 0 && N > 0, "psg_nu_inverse_tanh: bad argument");
    size_t rows = (size_t)B * N;
    hipLaunchKernelGGL(nu_inverse_tanh_kernel, dim3(grid_for(rows * 3)), dim3(256), 0, (hipStream_t)stream, x0, w_out, rows);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_nu_tanh_color(const float *w, const uint8_t *mask, int B, int N, float *x0, psg_stream stream)
{
    PSG_REQUIRE(w && x0 && B > 0 && N > 0, "psg_nu_tanh_color: bad argument");
    size_t rows = (size_t)B * N;
    hipLaunchKernelGGL(nu_tanh_color_kernel, dim3(grid_for(rows * 3)), dim3(256), 0, (hipStream_t)stream, w, mask, x0, N,
                       rows, 0);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// The "_rooms" entry points serve B INDEPENDENT one-room attacks advanced in lockstep (the reference's tar_NU / NU attack
// called once per room, target.py:62-133 at B = 1; pointsecguard_amd/attacks/torchattacks/attacks/nu.py: nu_attack_rooms):
// every room has its own mask row, its own smoothness term and its own loss sums; a room that has left the loop is frozen.
extern "C" int psg_nu_tanh_color_rooms(const float *w, const uint8_t *mask_rooms, int B, int N, float *x0, psg_stream stream)
{
    PSG_REQUIRE(w && x0 && B > 0 && N > 0, "psg_nu_tanh_color_rooms: bad argument");
    size_t rows = (size_t)B * N;
    hipLaunchKernelGGL(nu_tanh_color_kernel, dim3(grid_for(rows * 3)), dim3(256), 0, (hipStream_t)stream, w, mask_rooms, x0, N,
                       rows, 1);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_nu_f_loss_grad(const float *logp, const int32_t *labels, int target, int rows, int n_cls, float kappa,
                                  float tsign, float *dlogp_out, float *f_sum, int32_t *pred_out, psg_stream stream)
{
    PSG_REQUIRE(logp && dlogp_out && rows > 0, "psg_nu_f_loss_grad: bad argument");
    PSG_REQUIRE(n_cls > 1 && n_cls <= MAXC, "psg_nu_f_loss_grad: n_cls=%d out of range", n_cls);
    PSG_REQUIRE(labels || (target >= 0 && target < n_cls), "psg_nu_f_loss_grad: target class %d out of range", target);
    hipLaunchKernelGGL(nu_f_loss_grad_kernel, dim3(psg::ceil_div(rows, 256)), dim3(256), 0, (hipStream_t)stream, logp,
                       labels, target, rows, n_cls, kappa, tsign, dlogp_out, f_sum, pred_out, 0);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_nu_f_loss_grad_rooms(const float *logp, const int32_t *labels, int target, int B, int N, int n_cls, float kappa,
                                        float tsign, float *dlogp_out, float *f_sum_rooms, int32_t *pred_out, psg_stream stream)
{
    PSG_REQUIRE(logp && dlogp_out && f_sum_rooms && B > 0 && N > 0, "psg_nu_f_loss_grad_rooms: bad argument");
    PSG_REQUIRE(N % 64 == 0, "psg_nu_f_loss_grad_rooms: N=%d must be a multiple of 64 (one wave never spans two rooms)", N);
    PSG_REQUIRE(n_cls > 1 && n_cls <= MAXC, "psg_nu_f_loss_grad_rooms: n_cls=%d out of range", n_cls);
    PSG_REQUIRE(labels || (target >= 0 && target < n_cls), "psg_nu_f_loss_grad_rooms: target class %d out of range", target);
    const int rows = B * N;
    hipLaunchKernelGGL(nu_f_loss_grad_kernel, dim3(psg::ceil_div(rows, 256)), dim3(256), 0, (hipStream_t)stream, logp,
                       labels, target, rows, n_cls, kappa, tsign, dlogp_out, f_sum_rooms, pred_out, N);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_gcn_f_loss_grad(const float *logits, const int32_t *labels, int target, const uint8_t *mask, int mode,
                                   int rows, int n_point, int n_cls, float kappa, float tsign, float scale,
                                   float *dlogits_out, float *f_sum, int32_t *pred_out, psg_stream stream)
{
    PSG_REQUIRE(logits && dlogits_out && rows > 0 && n_point > 0, "psg_gcn_f_loss_grad: bad argument");
    PSG_REQUIRE(mode >= 0 && mode <= 2, "psg_gcn_f_loss_grad: mode %d out of range", mode);
    PSG_REQUIRE(n_cls > 1 && n_cls <= MAXC, "psg_gcn_f_loss_grad: n_cls=%d out of range", n_cls);
    PSG_REQUIRE((mode != 2 && labels) || (target >= 0 && target < n_cls), "psg_gcn_f_loss_grad: labels / target missing");
    hipLaunchKernelGGL(gcn_f_loss_grad_kernel, dim3(psg::ceil_div(rows, 256)), dim3(256), 0, (hipStream_t)stream, logits,
                       labels, target, mask, mode, rows, n_point, n_cls, kappa, tsign, scale, dlogits_out, f_sum, pred_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_gcn_f_loss_grad_rooms(const float *logits, const int32_t *labels, int target, const uint8_t *mask_rooms, int mode,
                                         int G, int N, int n_cls, float kappa, float tsign, float scale, float *dlogits_out,
                                         float *f_sum_rooms, int32_t *pred_out, psg_stream stream)
{
    PSG_REQUIRE(logits && dlogits_out && f_sum_rooms && G > 0 && G <= 65535 && N > 0, "psg_gcn_f_loss_grad_rooms: bad argument");
    PSG_REQUIRE(mode >= 0 && mode <= 2, "psg_gcn_f_loss_grad_rooms: mode %d out of range", mode);
    PSG_REQUIRE(n_cls > 1 && n_cls <= MAXC, "psg_gcn_f_loss_grad_rooms: n_cls=%d out of range", n_cls);
    PSG_REQUIRE((mode != 2 && labels) || (target >= 0 && target < n_cls), "psg_gcn_f_loss_grad_rooms: labels / target missing");
    hipLaunchKernelGGL(gcn_f_loss_grad_rooms_kernel, dim3(psg::ceil_div(N, 256), G), dim3(256), 0, (hipStream_t)stream, logits, labels,
                       target, mask_rooms, mode, N, n_cls, kappa, tsign, scale, dlogits_out, f_sum_rooms, pred_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

static int smooth_knn_launch(const float *adv_color, int adv_stride, size_t adv_room_stride, const float *ref_color, int ref_stride,
                             size_t ref_room_stride, int B, int N, int nb, float *dist_sum, float *grad_out, psg_stream stream,
                             int32_t *nn_io = nullptr, int have_prev = 0)
{
    PSG_REQUIRE(adv_color && ref_color && grad_out && N > 0 && B > 0 && B <= 65535, "psg_smooth_knn: bad argument");
    PSG_REQUIRE(nb > 0 && nb <= SM_MAX_NB, "psg_smooth_knn: neighbour count %d out of range (1..%d)", nb, SM_MAX_NB);
    PSG_REQUIRE(N <= 8192, "psg_smooth_knn: N=%d exceeds the LDS-resident limit 8192", N);
    // ref_color == adv_color selects the ResGCN variants' smooth(adv, adv): gradient through both arguments
    const int symmetric = ref_color == adv_color && ref_stride == adv_stride;
    if (symmetric) PSG_CHECK_HIP(hipMemsetAsync(grad_out, 0, (size_t)B * N * 3 * sizeof(float), (hipStream_t)stream));
    // list length per lane: the neighbour count itself for the usual nb = 5 (every step of the insertion network counts:
    // with 64 lanes a wave enters it in most passes), else 8 or 16
    const bool wide = (size_t)B * psg::ceil_div(N, SM_T / 4) >= 256;   // enough 256-query workgroups to fill the chip
    const int sub = wide ? 4 : 16;
    const size_t lds = (size_t)4 * sub * ((((N + sub - 1) / sub + 3) & ~3) + 8) * sizeof(float);
    const dim3 grid(psg::ceil_div(N, SM_T / (wide ? 4 : 16)), B);
#define PSG_SMOOTH_LAUNCH(NBT, SUB)                                                                                              \
    do {                                                                                                                         \
        if (lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)smooth_knn_kernel<NBT, SUB>));                       \
        hipLaunchKernelGGL((smooth_knn_kernel<NBT, SUB>), grid, dim3(SM_T), lds, (hipStream_t)stream, adv_color, adv_stride,     \
                           ref_color, ref_stride, N, nb, dist_sum, grad_out, symmetric, adv_room_stride, ref_room_stride,        \
                           nn_io, have_prev);                                                                                    \
    } while (0)
    if (wide) {
        if (nb <= 5) PSG_SMOOTH_LAUNCH(5, 4);
        else if (nb <= 8) PSG_SMOOTH_LAUNCH(8, 4);
        else PSG_SMOOTH_LAUNCH(16, 4);
    } else {
        if (nb <= 5) PSG_SMOOTH_LAUNCH(5, 16);
        else if (nb <= 8) PSG_SMOOTH_LAUNCH(8, 16);
        else PSG_SMOOTH_LAUNCH(16, 16);
    }
#undef PSG_SMOOTH_LAUNCH
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_smooth_knn(const float *adv_color, int adv_stride, const float *ref_color, int ref_stride, int N,
                              int nb, float *dist_sum, float *grad_out, psg_stream stream)
{
    return smooth_knn_launch(adv_color, adv_stride, 0, ref_color, ref_stride, 0, 1, N, nb, dist_sum, grad_out, stream);
}

// B rooms at once: room b's colours start at adv_color + b * adv_room_stride floats (likewise ref); dist_sum [B], grad_out [B][N][3]
extern "C" int psg_smooth_knn_rooms(const float *adv_color, int adv_stride, size_t adv_room_stride, const float *ref_color,
                                    int ref_stride, size_t ref_room_stride, int B, int N, int nb, float *dist_sum_rooms,
                                    float *grad_out, int32_t *nn_state, int have_prev, psg_stream stream)
{
    PSG_REQUIRE(adv_color != ref_color, "psg_smooth_knn_rooms: the symmetric variant is one room at a time");
    return smooth_knn_launch(adv_color, adv_stride, adv_room_stride, ref_color, ref_stride, ref_room_stride, B, N, nb,
                             dist_sum_rooms, grad_out, stream, nn_state, nn_state ? have_prev : 0);
}

// smooth(adv, adv) for G rooms without float atomics on the gradient: see smooth_knn_sym_own_kernel.  The lists the second
// pass reads go to nn_out, or - the caller wants none - to a scratch buffer this host thread keeps and grows (never inside a
// stream capture: the NU windows always pass their lists).
extern "C" int psg_smooth_knn_sym_rooms(const float *adv_color, int adv_stride, size_t adv_room_stride, int G, int N, int nb,
                                        float *dist_sum_rooms, float *grad_out, const uint8_t *room_active, int32_t *nn_out,
                                        psg_stream stream)
{
    PSG_REQUIRE(adv_color && grad_out && dist_sum_rooms && N > 0 && G > 0 && G <= 65535 && adv_stride >= 3,
                "psg_smooth_knn_sym_rooms: bad argument");
    PSG_REQUIRE(nb > 0 && nb <= SM_MAX_NB, "psg_smooth_knn_sym_rooms: neighbour count %d out of range (1..%d)", nb, SM_MAX_NB);
    PSG_REQUIRE(N <= 8192, "psg_smooth_knn_sym_rooms: N=%d exceeds the LDS-resident limit 8192", N);
    hipStream_t st = (hipStream_t)stream;
    if (!nn_out) {
        static thread_local int32_t *scratch = nullptr;
        static thread_local size_t scratch_n = 0;
        const size_t need = (size_t)G * N * nb;
        if (need > scratch_n) {
            PSG_CHECK_HIP(hipStreamSynchronize(st));            // (launches that still read the old block)
            if (scratch) (void)hipFree(scratch);
            scratch = nullptr; scratch_n = 0;
            PSG_CHECK_HIP(hipMalloc((void **)&scratch, need * sizeof(int32_t)));
            scratch_n = need;
        }
        nn_out = scratch;
    }
    const bool wide = (size_t)G * psg::ceil_div(N, SM_T / 4) >= 256;   // as smooth_knn_launch
    const int sub = wide ? 4 : 16;
    const size_t lds = (size_t)4 * sub * ((((N + sub - 1) / sub + 3) & ~3) + 8) * sizeof(float);
    const dim3 grid(psg::ceil_div(N, SM_T / sub), G);
#define PSG_SMOOTH_SYM_LAUNCH(NBT, SUB)                                                                                          \
    do {                                                                                                                         \
        if (lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)smooth_knn_sym_own_kernel<NBT, SUB>));               \
        hipLaunchKernelGGL((smooth_knn_sym_own_kernel<NBT, SUB>), grid, dim3(SM_T), lds, st, adv_color, adv_stride, N, nb,       \
                           dist_sum_rooms, grad_out, adv_room_stride, nn_out, room_active);                                      \
    } while (0)
    if (wide) {
        if (nb <= 5) PSG_SMOOTH_SYM_LAUNCH(5, 4);
        else if (nb <= 8) PSG_SMOOTH_SYM_LAUNCH(8, 4);
        else PSG_SMOOTH_SYM_LAUNCH(16, 4);
    } else {
        if (nb <= 5) PSG_SMOOTH_SYM_LAUNCH(5, 16);
        else if (nb <= 8) PSG_SMOOTH_SYM_LAUNCH(8, 16);
        else PSG_SMOOTH_SYM_LAUNCH(16, 16);
    }
#undef PSG_SMOOTH_SYM_LAUNCH
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(smooth_sym_incoming_kernel, dim3(psg::ceil_div(N, SI_T / SI_SUB), G), dim3(SI_T), 0, st, adv_color, adv_stride,
                       adv_room_stride, N, nb, nn_out, grad_out, room_active);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_nu_adam_step(float *w, float *m, float *v, const uint8_t *mask, const float *dx0, const float *x0,
                                const float *ori, const float *smooth_grad, float c_smooth, float c_l2, float lr,
                                float beta1, float beta2, float eps, int step, int B, int N, float *l2_sum,
                                psg_stream stream)
{
    PSG_REQUIRE(w && m && v && dx0 && x0 && ori && B > 0 && N > 0 && step >= 1, "psg_nu_adam_step: bad argument");
    const psg::AdamConsts k = psg::adam_consts(lr, beta1, beta2, step);
    size_t rows = (size_t)B * N;
    hipLaunchKernelGGL(nu_adam_step_kernel, dim3(grid_for(rows * 3)), dim3(256), 0, (hipStream_t)stream, w, m, v, mask,
                       dx0, x0, ori, smooth_grad, c_smooth, c_l2, beta1, beta2, eps, k.step_size, k.bc2_sqrt, N, rows, l2_sum,
                       (const uint8_t *)nullptr, g_nu_dconsts);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// the same update for B one-room attacks in lockstep: mask [B][N], smooth_grad [B][N][3], l2_sum [B]; room_active [B] (or NULL)
extern "C" int psg_nu_adam_step_rooms(float *w, float *m, float *v, const uint8_t *mask_rooms, const float *dx0, const float *x0,
                                      const float *ori, const float *smooth_grad_rooms, float c_smooth, float c_l2, float lr,
                                      float beta1, float beta2, float eps, int step, int B, int N, const uint8_t *room_active,
                                      float *l2_sum_rooms, psg_stream stream)
{
    PSG_REQUIRE(w && m && v && dx0 && x0 && ori && B > 1 && B <= 65535 && N > 0 && step >= 1, "psg_nu_adam_step_rooms: bad argument (B >= 2)");
    const psg::AdamConsts k = psg::adam_consts(lr, beta1, beta2, step);
    // (12 workgroups per room, four elements per thread at 4096 points: 12 atomics per room sum)
    hipLaunchKernelGGL(nu_adam_step_kernel, dim3(std::min(grid_for((size_t)N * 3), 12), B), dim3(256), 0, (hipStream_t)stream, w, m, v, mask_rooms,
                       dx0, x0, ori, smooth_grad_rooms, c_smooth, c_l2, beta1, beta2, eps, k.step_size, k.bc2_sqrt, N, (size_t)N, l2_sum_rooms,
                       room_active, g_nu_dconsts);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// Per-step statistics + exit latch of the NU attacks (see nu_step_latch_kernel): G attacks of `rows` batch rows each.
// pred / labels [G*rows][N]; mask [G][N] or NULL (mode 0); n_mask [G] (modes 1, 2); scal [3][G] = this step's f, Smooth, L2
// sums (zeroed by the call); hist_step [5][G] receives n_correct, n_hits, f, Smooth, L2; x0 [G*rows][N][9], out
// [G*rows][9][N]; active [G] bytes, exit_step [G] (-1 until the group's exit test fires).
extern "C" int psg_nu_step_latch(const int32_t *pred, const int32_t *labels, int target, const uint8_t *mask_groups,
                                 const int32_t *n_mask, int G, int rows, int N, int mode, float *scal, float *hist_step,
                                 const float *x0, float *out_cn, uint8_t *active, int32_t *exit_step, int step, psg_stream stream)
{
    PSG_REQUIRE(pred && labels && scal && hist_step && x0 && out_cn && active && exit_step && G > 0 && rows > 0 && N > 0,
                "psg_nu_step_latch: null / empty argument");
    PSG_REQUIRE(mode == 0 || (mode >= 1 && mode <= 2 && mask_groups && n_mask), "psg_nu_step_latch: modes 1 and 2 need mask and n_mask");
    hipLaunchKernelGGL(nu_step_latch_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, pred, labels, target, mask_groups, n_mask, rows,
                       N, mode, scal, hist_step, x0, out_cn, active, exit_step, step, G, g_nu_dconsts);
    PSG_LAUNCH_CHECK();
    if (rows > 1) {
        const size_t total = (size_t)G * rows * N * 9;
        hipLaunchKernelGGL(nu_latch_snapshot_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x0, out_cn,
                           exit_step, step, rows, N, total, g_nu_dconsts);
        PSG_LAUNCH_CHECK();
    }
    return PSG_OK;
}

// ---- Restart of tar_NU_attack (target.py:127-132) for the groups `flags` selects, one workgroup per group of `rows` batch
// rows:  colour[:, :, mask] += noise;  x.clamp_(0, 1) on ALL nine channels;  extra_l2 = sum((x - x_orig)^2) over channels
// 0:3 and 6:9.  The group's noise block is [rows][3][k] (k = its mask count) as torch.empty(rows, 3, k).uniform_() lays it
// out: entry j of a channel belongs to the j-th masked point in ascending order, i.e. to the point's rank within the mask -
// a ballot prefix count per 256-point chunk plus the running count of the chunks before it.  Each chunk's 256 x 9 floats
// are then one contiguous piece handled as coalesced dwords.  The sum has a fixed order: per thread over its elements in
// ascending order, then a tree over the 256 threads.  Groups that are not flagged are not touched.
__global__ __launch_bounds__(256) void nu_restart_rooms_kernel(float *__restrict__ x0, const float *__restrict__ x0_orig,
                                                                const uint8_t *__restrict__ mask, const int32_t *__restrict__ n_mask,
                                                                const uint8_t *__restrict__ flags, const float *__restrict__ noise,
                                                                const long long *__restrict__ noise_off, int rows, int N,
                                                                float *__restrict__ extra_l2)
{
    __shared__ int s_rank[256];
    __shared__ int s_cnt[4];
    __shared__ float s_red[256];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!flags[g]) return;                                   // (uniform over the workgroup)
    const uint8_t *mk = mask + (size_t)g * N;
    const int k = n_mask[g];
    const float *nz = noise + noise_off[g];
    float acc = 0.0f;
    for (int row = 0; row < rows; ++row) {
        const size_t r = (size_t)g * rows + row;
        int before = 0;                                      // masked points of this row's earlier chunks
        for (int p0 = 0; p0 < N; p0 += 256) {
            const int p = p0 + tid;
            const bool in = p < N && mk[p] != 0;
            const unsigned long long bal = __ballot(in);
            if (lane == 0) s_cnt[wave] = __popcll(bal);
            __syncthreads();
            int pre = before;
            for (int w = 0; w < wave; ++w) pre += s_cnt[w];
            s_rank[tid] = in ? pre + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
            before += (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            __syncthreads();
            const int np = min(256, N - p0);
            float *xc = x0 + (r * N + p0) * 9;
            const float *oc = x0_orig + (r * N + p0) * 9;
            for (int e = tid; e < np * 9; e += 256) {
                const int pl = e / 9, ch = e % 9, rk = s_rank[pl];
                float v = xc[e];
                if (ch >= 3 && ch < 6) {
                    if (rk >= 0 && rk < k) v = v + nz[((size_t)row * 3 + (ch - 3)) * k + rk];
                    v = fminf(fmaxf(v, 0.0f), 1.0f);
                } else {
                    v = fminf(fmaxf(v, 0.0f), 1.0f);
                    const float d = v - oc[e];
                    acc += d * d;
                }
                xc[e] = v;
            }
            __syncthreads();                                 // s_rank / s_cnt are rewritten by the next chunk
        }
    }
    s_red[tid] = acc;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) s_red[tid] += s_red[tid + st];
        __syncthreads();
    }
    if (tid == 0) extra_l2[g] = s_red[0];
}

// x0 / x0_orig [G*rows][N][9]; mask_groups [G][N], n_mask [G]; flags [G] bytes (non-zero: restart this group); noise: the
// flagged groups' blocks [rows][3][n_mask[g]], group g's at float offset noise_off[g]; extra_l2 [G] (written for flagged
// groups only).
extern "C" int psg_nu_restart_rooms(float *x0, const float *x0_orig, const uint8_t *mask_groups, const int32_t *n_mask,
                                    const uint8_t *flags, const float *noise, const long long *noise_off, int G, int rows, int N,
                                    float *extra_l2, psg_stream stream)
{
    PSG_REQUIRE(x0 && x0_orig && mask_groups && n_mask && flags && noise && noise_off && extra_l2, "psg_nu_restart_rooms: null argument");
    PSG_REQUIRE(G > 0 && G <= 65535 && rows > 0 && N > 0, "psg_nu_restart_rooms: G=%d rows=%d N=%d out of range", G, rows, N);
    hipLaunchKernelGGL(nu_restart_rooms_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, x0, x0_orig, mask_groups, n_mask, flags, noise,
                       noise_off, rows, N, extra_l2);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// One step sequence of a window (shared by the eager and the captured path); dconsts: the step's device row or null.
static int nu_window_steps(const psg_nu_window_args *a, const float *dconsts_rows, psg_stream stream)
{
    const bool rooms = a->G > 1;
    const int B = a->G * a->rows, N = a->N, G = a->G;
    int rc = PSG_OK;
    for (int i = 0; i < a->n_steps && rc == PSG_OK; ++i) {
        const int step = a->step0 + i, slot = a->slot0 + i, adam_t = a->adam_t0 + i + 1;
        const int32_t *f_labels = a->use_target ? nullptr : a->labels;
        const int f_target = a->use_target ? a->target : 0;
        if ((rc = rooms ? psg_nu_tanh_color_rooms(a->w, a->mask, B, N, a->x0, stream) : psg_nu_tanh_color(a->w, a->mask, B, N, a->x0, stream)))
            break;
        if ((rc = psg::pn2_forward_lean(a->model, a->ws, slot, a->x0, a->logp, stream))) break;
        if ((rc = rooms ? psg_nu_f_loss_grad_rooms(a->logp, f_labels, f_target, B, N, PSG_PN2_NUM_CLASSES, a->kappa, a->tsign, a->dlogp,
                                                   a->scal, a->pred, stream)
                        : psg_nu_f_loss_grad(a->logp, f_labels, f_target, B * N, PSG_PN2_NUM_CLASSES, a->kappa, a->tsign, a->dlogp, a->scal,
                                             a->pred, stream)))
            break;
        if ((rc = psg::pn2_backward_colour(a->model, a->ws, slot, a->dlogp, a->dx0, stream))) break;   // (the Adam step reads the colours only)
        if ((rc = psg_smooth_knn_rooms(a->x0 + 3, 9, (size_t)N * 9, a->ori, 3, (size_t)N * 3, G, N, a->neighbour, a->scal + G, a->sgrad,
                                       a->nn_state, (i > 0 || a->warm_first) ? 1 : 0, stream)))
            break;
        psg::NuStepConsts consts(dconsts_rows ? dconsts_rows + 4 * i : nullptr);
        rc = psg::nu_colour_adam(a, a->c_smooth, a->c_l2, a->rows, adam_t, stream);
        if (rc == PSG_OK) rc = psg::nu_latch(a, a->rows, a->hist + (size_t)i * 5 * G, step, stream);
    }
    return rc;
}

// A window replayed as a hipGraph.  A one-room attack step is ~30 short launches, and the host's launch rate - not the GPU
// - bounded the reference's one-call-per-room protocol; windows of the same shape (same buffers, same plan slots) differ only
// in {step number, Adam bias corrections, lr}, which the captured kernels read from a device row written before each
// replay.  The handle remembers ONE window shape: the first window of a shape runs eagerly (it also sets kernel
// attributes outside any capture), the second is captured, later ones are replayed.
struct psg_nu_graph {
    psg::GraphSlot slot;
    std::vector<unsigned char> key;               // the window's argument block, step0 / adam_t0 / lr zeroed
    uint64_t key_model_gen = 0, key_ws_gen = 0;   // generation numbers of the key's model / ws: addresses can be re-used (psg_common.h)
    bool have_key = false;
    float *dconsts = nullptr;       // device [PSG_NU_GRAPH_MAX_STEPS][4]
    float host[PSG_NU_GRAPH_MAX_STEPS * 4];
};

extern "C" int psg_nu_graph_create(psg_nu_graph **out)
{
    PSG_REQUIRE(out, "psg_nu_graph_create: null out pointer");
    psg_nu_graph *g = new psg_nu_graph();
    if (hipMalloc(&g->dconsts, sizeof(g->host)) != hipSuccess) { delete g; psg::set_error("psg_nu_graph_create: hipMalloc failed"); return PSG_ERR_HIP; }
    *out = g;
    return PSG_OK;
}

extern "C" int psg_nu_graph_destroy(psg_nu_graph *g)
{
    if (!g) return PSG_OK;
    g->slot.destroy();
    (void)hipFree(g->dconsts);
    delete g;
    return PSG_OK;
}

// out4 = {captures tried, captures failed, windows replayed as a graph, windows that ran eagerly} of this handle (the two
// eager windows every shape starts with included)
extern "C" int psg_nu_graph_stats(const psg_nu_graph *g, long long *out4)
{
    PSG_REQUIRE(g && out4, "psg_nu_graph_stats: null argument");
    const psg::CaptureCounters &c = g->slot.cap;
    out4[0] = c.tried; out4[1] = c.failed; out4[2] = c.replays; out4[3] = c.eager;
    return PSG_OK;
}

void psg::nu_set_step_consts(const float *row) { g_nu_dconsts = row; }
const float *psg::nu_step_consts() { return g_nu_dconsts; }

int psg::nu_graph_window(psg_nu_graph *graph, const void *key, size_t key_bytes, uint64_t model_gen, uint64_t ws_gen, int n_steps,
                         int step0, int adam_t0, float lr, float beta1, float beta2, hipStream_t st,
                         const std::function<int(const float *)> &steps, const float *slot3)
{
    // (PSG_NU_NO_GRAPH=1: eager windows, for counter passes - per-dispatch counter rows need per-dispatch launches)
    static const bool no_graph = psg::env_int("PSG_NU_NO_GRAPH", 0) != 0;
    if (!graph || no_graph || n_steps > PSG_NU_GRAPH_MAX_STEPS || psg::trace_sync_enabled()) return steps(nullptr);
    // the step-dependent constants of this window
    for (int i = 0; i < n_steps; ++i) {
        const psg::AdamConsts k = psg::adam_consts(lr, beta1, beta2, adam_t0 + i + 1);
        graph->host[4 * i] = __builtin_bit_cast(float, step0 + i);
        graph->host[4 * i + 1] = k.step_size;
        graph->host[4 * i + 2] = k.bc2_sqrt;
        graph->host[4 * i + 3] = slot3 ? slot3[i] : 0.0f;     // (psg_rla_nu_window: TF1 Adam's lr_t)
    }
    PSG_CHECK_HIP(hipMemcpyAsync(graph->dconsts, graph->host, (size_t)n_steps * 16, hipMemcpyHostToDevice, st));
    const bool same = graph->have_key && graph->key.size() == key_bytes && memcmp(graph->key.data(), key, key_bytes) == 0 &&
                      graph->key_model_gen == model_gen && graph->key_ws_gen == ws_gen;
    psg::GraphSlot &slot = graph->slot;
    // second window of this shape: capture it, then replay (a failed capture is counted - psg_nu_graph_stats,
    // psg_capture_stats - and the shape is not tried again: its windows run eagerly below)
    if (same && !slot.exec && !slot.capture_failed) slot.capture(st, [&] { return steps(graph->dconsts); });
    if (same && slot.exec) {
        PSG_CHECK_HIP(slot.replay(st));
        return PSG_OK;
    }
    if (!same) {
        PSG_CHECK_HIP(slot.forget(st));              // another shape: forget the old one
        graph->key.assign((const unsigned char *)key, (const unsigned char *)key + key_bytes);
        graph->key_model_gen = model_gen;
        graph->key_ws_gen = ws_gen;
        graph->have_key = true;
    }
    slot.note_eager();
    return steps(graph->dconsts);
}

extern "C" int psg_pn2_nu_window(const psg_nu_window_args *a, psg_nu_graph *graph, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->w && a->m && a->v && a->x0 && a->ori && a->labels && a->logp && a->dlogp && a->dx0 &&
                    a->sgrad && a->pred && a->scal && a->nn_state && a->hist && a->out && a->active && a->exit_step,
                "psg_pn2_nu_window: null argument");
    PSG_REQUIRE(a->n_steps > 0 && a->G > 0 && a->rows > 0 && (a->G == 1 || a->rows == 1), "psg_pn2_nu_window: (G, rows) must be (1, B) or (R, 1)");
    psg_nu_window_args key = *a;
    key.step0 = 0; key.adam_t0 = 0; key.lr = 0.0f;      // what the device row carries
    return psg::nu_graph_window(graph, &key, sizeof(key), psg::pn2_model_generation(a->model), psg::pn2_ws_generation(a->ws), a->n_steps,
                                a->step0, a->adam_t0, a->lr, a->beta1, a->beta2, (hipStream_t)stream,
                                [&](const float *rows) { return nu_window_steps(a, rows, stream); });
}

// NU attacks on the coordinate field of the PointNet++ SSG network (kernels and entry points)
#include "psg_nu_field.cuh"
