// The colour attacks on RandLA-Net (psg_randla_net.hip): the "colper" loss, the BIM update and loop (ares/ares/attack/
// bim.py:66-116, :190-236), NUattack / tar_NUattack (NUattack.py:12-74, tar_NUattack.py:12-84) and TBIM / tar_NBattack
// (bim.py:277-505), for one cloud and for G clouds in lockstep; and the two NU attacks on the point positions (DESIGN.md 5s:
// psg_rla_nu_coord_apply_clouds / _coord_adam_clouds / _field_latch_clouds, psg_rla_nu_field_window), G clouds in lockstep, and
// the BIM family's lockstep window on the same field (psg_rla_tbim_retire_field_clouds, psg_rla_bim_field_window;
// its field step, psg_rla_bim_step_field_clouds, is compiled without contraction in psg_randla_coord.hip).
//
// Every update kernel exists once, in the G-cloud form: blockIdx.y = cloud (blockIdx.x for the one-workgroup-per-cloud kernels),
// a cloud whose `running` / `active` byte is clear is skipped by whole workgroups, a null byte array runs every cloud.  The
// one-cloud entry points launch the same kernels at G = 1.  The reductions use no float atomics (nu_color_kernel, whose ABI
// has no room for partial sums, is the exception): a fixed slice per workgroup, partial sums added in index order - the same
// bits in every run, whatever the other clouds do.
#include <cmath>
#include <cstring>

#include "psg_common.h"
#include "psg_randla_net.h"

using namespace psg;

namespace {

constexpr float kNuBound = 1.0f - 1e-6f;
constexpr int kNuParts = PSG_RLA_NU_PARTS;

// the limits of the G-cloud entry points: G is a grid dimension, G * n rows are indexed by 32-bit ints on the host side
int check_clouds(const char *entry, int G, int n)
{
    PSG_REQUIRE(G > 0 && G <= 65535 && n > 0 && (size_t)G * n <= (size_t)1 << 20, "%s: G=%d n=%d out of range", entry, G, n);
    return PSG_OK;
}

// TF1 Adam's step size at step t = 1, 2, ..
float adam_lr_t(float lr, int t)
{
    const double b1 = 0.9, b2 = 0.999;
    return (float)((double)lr * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t)));
}

// "colper" loss of the BIM attack (bim.py:110-116): sum_n max(0, max_k((1 - onehot) * z)_k - z_y); gradient w.r.t. z.
// mask (TBIM / tar_NUattack, bim.py:393-397, tar_NUattack.py:105-110): the per-point loss is multiplied by mask[n] (the
// points of the origin class); `sign` multiplies the gradient (goal 't': grad = -grad, bim.py:350-351).
__global__ void colper_grad_kernel(const float *__restrict__ z, const int32_t *__restrict__ y, const uint8_t *__restrict__ mask,
                                   float sign, int n, float *__restrict__ dz, float *__restrict__ loss)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float l = 0.0f;
    if (i < n) {
        const float *zi = z + (size_t)i * RNCLS;
        const int yi = y[i];
        float other = 0.0f;          // the masked entry of the true class is 0 and takes part in the max
        int oi = yi;
        for (int k = 0; k < RNCLS; ++k)
            if (k != yi && zi[k] > other) { other = zi[k]; oi = k; }
        const float real = zi[yi];
        const bool on = other - real > 0.0f && (!mask || mask[i]);
        l = on ? other - real : 0.0f;
        for (int k = 0; k < RNCLS; ++k) dz[(size_t)i * RNCLS + k] = 0.0f;
        if (on) {
            dz[(size_t)i * RNCLS + yi] = -sign;
            if (oi != yi) dz[(size_t)i * RNCLS + oi] = sign;
        }
    }
    if (loss) {
        for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o);
        if ((threadIdx.x & 63) == 0 && l != 0.0f) atomicAdd(loss, l);
    }
}

// ---- BIM update of the colours (bim.py:84-98), goal 'ut' (ascent).  l_inf: clip(adv + alpha*sign(g), x-eps, x+eps);
// l_2: x + clip_by_norm(adv - x + alpha * g/|g|, eps); then clip to [0, 1], PER CLOUD (bim.py:84-98 normalises every sample
// of the batch by its own norms): norms[g] = |g_g|^2, norms[G + g] = |delta_g|^2.

// squared norm of the colour part of ONE CLOUD per workgroup (blockIdx.x = cloud): every thread adds its strided elements in
// double, then a fixed tree - one writer, a fixed order: the l_2 update is bit-reproducible.
__global__ __launch_bounds__(1024) void sq_norm_clouds_kernel(const float *__restrict__ a, int ld, int c0, size_t nc,
                                                              const uint8_t *__restrict__ running, float *__restrict__ out)
{
    __shared__ double s_part[16];
    if (running && !running[blockIdx.x]) return;
    const float *p = a + (size_t)blockIdx.x * nc * ld;
    double s = 0.0;
    for (size_t t = threadIdx.x; t < nc * 3; t += blockDim.x) {
        const float v = p[(t / 3) * ld + c0 + (t % 3)];
        s += (double)v * (double)v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += s_part[w];
        out[blockIdx.x] = (float)tot;
    }
}

__global__ void bim_linf_clouds_kernel(float *__restrict__ feat, const float *__restrict__ dfeat, const float *__restrict__ ori,
                                       const uint8_t *__restrict__ running, size_t n, float alpha, float eps)
{
    const int cl = blockIdx.y;
    if (running && !running[cl]) return;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const size_t i = (size_t)cl * n + t / 3;
    const int c = (int)(t % 3);
    t += (size_t)cl * n * 3;
    const float g = dfeat[i * 6 + 3 + c], x = ori[t];
    const float sg = g > 0.0f ? 1.0f : (g < 0.0f ? -1.0f : 0.0f);
    float v = feat[i * 6 + 3 + c] + alpha * sg;
    v = fminf(fmaxf(v, x - eps), x + eps);
    feat[i * 6 + 3 + c] = fminf(fmaxf(v, 0.0f), 1.0f);
}

__global__ void bim_l2_delta_clouds_kernel(const float *__restrict__ feat, const float *__restrict__ dfeat, const float *__restrict__ ori,
                                           const uint8_t *__restrict__ running, size_t n, float alpha,
                                           const float *__restrict__ gnorm2, float *__restrict__ delta)
{
    const int cl = blockIdx.y;
    if (running && !running[cl]) return;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const size_t i = (size_t)cl * n + t / 3;
    const int c = (int)(t % 3);
    t += (size_t)cl * n * 3;
    const float gn = fmaxf(1e-12f, sqrtf(gnorm2[cl]));            // the cloud's own gradient norm
    delta[t] = feat[i * 6 + 3 + c] - ori[t] + alpha * (dfeat[i * 6 + 3 + c] / gn);
}

__global__ void bim_l2_apply_clouds_kernel(float *__restrict__ feat, const float *__restrict__ ori, const float *__restrict__ delta,
                                           const uint8_t *__restrict__ running, size_t n, float eps, const float *__restrict__ dnorm2)
{
    const int cl = blockIdx.y;
    if (running && !running[cl]) return;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const size_t i = (size_t)cl * n + t / 3;
    const int c = (int)(t % 3);
    t += (size_t)cl * n * 3;
    const float dn = sqrtf(dnorm2[cl]);
    const float scale = dn > eps ? eps / dn : 1.0f;
    feat[i * 6 + 3 + c] = fminf(fmaxf(ori[t] + delta[t] * scale, 0.0f), 1.0f);
}

// One BIM update of the colour half of feat [G][n][6] from its gradient dfeat [G][n][6]: one launch for l_inf, four for l_2
// (norms [2][G] and delta [G][n][3] are its scratch).  The one copy behind psg_rla_bim_step (G = 1), the iteration of
// psg_rla_bim_attack (the workspace's clouds) and psg_rla_bim_step_clouds.
int bim_step(float *feat, const float *dfeat, const float *ori, const uint8_t *running, int G, int n, float eps, float alpha, int l2,
             float *norms, float *delta, hipStream_t st)
{
    const size_t N = (size_t)n;
    const dim3 grid(blocks_for(N * 3), G);
    if (!l2) {
        hipLaunchKernelGGL(bim_linf_clouds_kernel, grid, dim3(256), 0, st, feat, dfeat, ori, running, N, alpha, eps);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    hipLaunchKernelGGL(sq_norm_clouds_kernel, dim3(G), dim3(1024), 0, st, dfeat, 6, 3, N, running, norms);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(bim_l2_delta_clouds_kernel, grid, dim3(256), 0, st, (const float *)feat, dfeat, ori, running, N, alpha,
                       (const float *)norms, delta);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(sq_norm_clouds_kernel, dim3(G), dim3(1024), 0, st, (const float *)delta, 3, 0, N, running, norms + G);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(bim_l2_apply_clouds_kernel, grid, dim3(256), 0, st, feat, ori, (const float *)delta, running, N, eps,
                       (const float *)(norms + G));
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// ---- NUattack / tar_NUattack: Adam on d_ws in tanh space.
//   ws = atanh(2 b x - b) + d_ws (b = 1 - 1e-6), adv = (tanh(ws) + 1) / 2, masked: adv = mask adv + (1 - mask) x;
//   loss = |adv - x|_2 + c * score;  TF1 Adam: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), d_ws -= lr_t m / (sqrt(v) + 1e-8).

// the colour map of one element, unmasked; th = tanh(ws), which the map's derivative (1 - th^2) / 2 needs
__device__ __forceinline__ float nu_color_map(float x, float dws, float &th)
{
    const float w = atanhf(2.0f * kNuBound * x - kNuBound) + dws;
    th = tanhf(w);
    return 0.5f * (th + 1.0f);
}

// (not nu_color_clouds_kernel at G = 1: this one sums dist2 with float atomics and its ABI has no scratch for partials)
__global__ void nu_color_kernel(const float *__restrict__ xs, const float *__restrict__ dws, const uint8_t *__restrict__ mask,
                                size_t n, float *__restrict__ feat, float *__restrict__ dist2)
{
    float s = 0.0f;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * 3; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t / 3;
        const int c = (int)(t % 3);
        const float x = xs[t];
        float th, adv = nu_color_map(x, dws[t], th);
        if (mask && !mask[i]) adv = x;
        feat[i * 6 + 3 + c] = adv;
        const float d = adv - x;
        s += d * d;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(dist2, s);
}

// kNuParts workgroups per cloud, each with one partial sum of |adv - x|^2 in double
__global__ __launch_bounds__(256) void nu_color_clouds_kernel(const float *__restrict__ xs, const float *__restrict__ dws,
                                                              const uint8_t *__restrict__ mask, const uint8_t *__restrict__ active,
                                                              size_t n, float *__restrict__ feat, double *__restrict__ partials)
{
    __shared__ double s_part[4];
    const int g = blockIdx.y;
    if (active && !active[g]) return;
    const size_t base = (size_t)g * n;
    double s = 0.0;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * 3; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t / 3;
        const int c = (int)(t % 3);
        const float x = xs[base * 3 + t];
        float th, adv = nu_color_map(x, dws[base * 3 + t], th);
        if (mask && !mask[base + i]) adv = x;
        feat[(base + i) * 6 + 3 + c] = adv;
        const double d = (double)adv - (double)x;       // exact; the sum is of the colours as written, like sq_norm_clouds_kernel's
        s += d * d;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[(size_t)g * gridDim.x + blockIdx.x] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

__global__ void nu_dist2_clouds_kernel(const double *__restrict__ partials, const uint8_t *__restrict__ active, int G, int parts,
                                       float *__restrict__ dist2)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G || (active && !active[g])) return;
    double tot = 0.0;
    for (int p = 0; p < parts; ++p) tot += partials[(size_t)g * parts + p];
    dist2[g] = (float)tot;
}

// one Adam step with the cloud's own distance; lr_t = consts[3] inside a window (psg_common.h: nu_set_step_consts), else lr_arg
__global__ void nu_adam_clouds_kernel(const float *__restrict__ xs, float *__restrict__ dws, float *__restrict__ m, float *__restrict__ v,
                                      const uint8_t *__restrict__ mask, const uint8_t *__restrict__ active,
                                      const float *__restrict__ feat, const float *__restrict__ dfeat, const float *__restrict__ dist2,
                                      size_t n, float c, float lr_arg, const float *__restrict__ consts, float b1, float b2, float eps)
{
    const int g = blockIdx.y;
    if (active && !active[g]) return;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const float lr_t = consts ? consts[3] : lr_arg;
    const size_t i = (size_t)g * n + t / 3;
    const int ch = (int)(t % 3);
    t += (size_t)g * n * 3;
    const float x = xs[t];
    float th;
    nu_color_map(x, dws[t], th);
    const float adv = feat[i * 6 + 3 + ch];
    const float dist = sqrtf(dist2[g]);
    // d loss / d adv = (adv - x) / |adv - x|_2 + c * d score / d adv;  d adv / d d_ws = mask * (1 - tanh^2) / 2
    float gr = (dist > 0.0f ? (adv - x) / dist : 0.0f) + c * dfeat[i * 6 + 3 + ch];
    gr *= (mask && !mask[i]) ? 0.0f : 0.5f * (1.0f - th * th);
    const float mm = b1 * m[t] + (1.0f - b1) * gr;
    const float vv = b2 * v[t] + (1.0f - b2) * gr * gr;
    m[t] = mm;
    v[t] = vv;
    dws[t] -= lr_t * mm / (sqrtf(vv) + eps);
}

// ---- the latch of the lockstep attacks: count (shared), then the attack's own commit.  scratch[g] = {was the cloud live when
// the latch began, then per part {#(pred == labels), #(mask & pred == ys)}}.

// rows [lo, hi) of a cloud that workgroup blockIdx.x of `parts` owns
__device__ __forceinline__ void latch_slice(int n, int parts, int &lo, int &hi)
{
    const int chunk = (n + parts - 1) / parts;
    lo = min(n, (int)blockIdx.x * chunk);
    hi = min(n, lo + chunk);
}

// the cloud's two counts: its parts in index order
__device__ __forceinline__ void latch_counts(const int32_t *sc, int parts, int &nc, int &nh)
{
    nc = 0; nh = 0;
    for (int p = 0; p < parts; ++p) { nc += sc[1 + 2 * p]; nh += sc[2 + 2 * p]; }
}

// the cloud's history row {nc, nh, d2} and, for a snapshot, the same as its statistics
__device__ __forceinline__ void latch_rows(int g, int nc, int nh, float d2, bool snapshot, float *hist_row, float *out_stats)
{
    const float row[3] = {(float)nc, (float)nh, d2};
    for (int k = 0; k < 3; ++k) hist_row[g * 3 + k] = row[k];
    if (snapshot)
        for (int k = 0; k < 3; ++k) out_stats[g * 3 + k] = row[k];
}

// Latch, first half: pred = first maximum of the 13 logits; every workgroup counts its slice of the cloud into scratch;
// scratch[g][0] records whether the cloud was active (the second half clears `active`, so its workgroups must not read it)
__global__ __launch_bounds__(256) void nu_latch_count_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels,
                                                             const int32_t *__restrict__ ys, const uint8_t *__restrict__ mask,
                                                             const uint8_t *__restrict__ active, int n, int32_t *__restrict__ pred,
                                                             int32_t *__restrict__ scratch)
{
    __shared__ int s_cnt[4][2];
    const int g = blockIdx.y, parts = gridDim.x;
    int32_t *sc = scratch + (size_t)g * (2 * parts + 1);
    const bool live = active[g] != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc[0] = live ? 1 : 0;
    if (!live) return;
    int lo, hi;
    latch_slice(n, parts, lo, hi);
    int c0 = 0, c1 = 0;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const size_t r = (size_t)g * n + i;
        const float *z = logits + r * RNCLS;
        float best = z[0];
        int bi = 0;
        for (int k = 1; k < RNCLS; ++k)
            if (z[k] > best) { best = z[k]; bi = k; }
        pred[r] = bi;
        c0 += bi == labels[r] ? 1 : 0;
        c1 += (mask && mask[r] && bi == ys[r]) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o); }
    if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6][0] = c0; s_cnt[threadIdx.x >> 6][1] = c1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sc[1 + 2 * blockIdx.x] = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
        sc[2 + 2 * blockIdx.x] = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    }
}

// NU latch, second half: every workgroup of a live cloud adds the cloud's counts, takes the exit decision (integers) and, for a
// snapshot, copies its slice; workgroup 0 writes the history row, the snapshot's statistics, exit_step and active.
__global__ __launch_bounds__(256) void nu_latch_commit_kernel(const float *__restrict__ feat, const int32_t *__restrict__ pred,
                                                              const float *__restrict__ dist2, const int32_t *__restrict__ n_mask,
                                                              const int32_t *__restrict__ scratch, int n, int mode, int num, int den,
                                                              int step_arg, int can_exit, int final, const float *__restrict__ consts,
                                                              float *__restrict__ hist_row, float *__restrict__ out_adv,
                                                              int32_t *__restrict__ out_pred, float *__restrict__ out_stats,
                                                              uint8_t *__restrict__ active, int32_t *__restrict__ exit_step)
{
    const int g = blockIdx.y, parts = gridDim.x;
    const int32_t *sc = scratch + (size_t)g * (2 * parts + 1);
    if (!sc[0]) return;
    const int step = consts ? __builtin_bit_cast(int, consts[0]) : step_arg;
    int nc, nh;
    latch_counts(sc, parts, nc, nh);
    const bool fire = mode == 0 ? (long long)den * nc < (long long)num * n : (long long)den * nh > (long long)num * n_mask[g];
    const bool exits = fire && can_exit && step >= 1;
    if (exits || final) {
        int lo, hi;
        latch_slice(n, parts, lo, hi);
        for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            const size_t r = (size_t)g * n + i;
            out_adv[r * 3] = feat[r * 6 + 3];
            out_adv[r * 3 + 1] = feat[r * 6 + 4];
            out_adv[r * 3 + 2] = feat[r * 6 + 5];
            out_pred[r] = pred[r];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        latch_rows(g, nc, nh, dist2[g], exits || final, hist_row, out_stats);
        if (exits) { exit_step[g] = step; active[g] = 0; }
    }
}

// TBIM latch, second half, with TBIM.batch_attack's ordering: the exit is decided on the forward BEFORE the iteration's update,
// the leaving cloud still takes that update, and only then are its colours snapshot and it is retired (tbim_retire_kernel).
// Every workgroup of a live cloud adds the cloud's counts and takes the exit decision (integers); a leaving cloud (or, final,
// every live one) gets its slice of out_pred; workgroup 0 writes the history row, the statistics, exit_step and the leaving
// byte.  `active` is read by nobody here and written by nobody.
__global__ __launch_bounds__(256) void tbim_latch_commit_kernel(const int32_t *__restrict__ pred, const int32_t *__restrict__ n_mask,
                                                                const int32_t *__restrict__ scratch, int n, int num, int den, int it_arg,
                                                                int final, const float *__restrict__ consts, float *__restrict__ hist_row,
                                                                int32_t *__restrict__ out_pred, float *__restrict__ out_stats,
                                                                uint8_t *__restrict__ leaving, int32_t *__restrict__ exit_step)
{
    const int g = blockIdx.y, parts = gridDim.x;
    const int32_t *sc = scratch + (size_t)g * (2 * parts + 1);
    if (!sc[0]) return;
    const int it = consts ? __builtin_bit_cast(int, consts[0]) : it_arg;
    int nc, nh;
    latch_counts(sc, parts, nc, nh);
    const bool exits = it >= 1 && (long long)den * nh > (long long)num * n_mask[g];
    if (exits || final) {
        int lo, hi;
        latch_slice(n, parts, lo, hi);
        for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            const size_t r = (size_t)g * n + i;
            out_pred[r] = pred[r];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        latch_rows(g, nc, nh, 0.0f, exits || final, hist_row, out_stats);
        if (exits) exit_step[g] = it;
        leaving[g] = exits ? 1 : 0;
    }
}

// one workgroup per cloud: the flags are read before anything is written, the colours copied, then the flags cleared
__global__ __launch_bounds__(1024) void tbim_retire_kernel(const float *__restrict__ feat, size_t n, int final, float *__restrict__ out_adv,
                                                           uint8_t *__restrict__ active, uint8_t *__restrict__ leaving)
{
    const int g = blockIdx.x;
    const bool go = active[g] != 0 && (leaving[g] != 0 || final != 0);
    __syncthreads();
    if (!go) return;
    const size_t base = (size_t)g * n;
    for (size_t t = threadIdx.x; t < n * 3; t += blockDim.x) out_adv[base * 3 + t] = feat[(base + t / 3) * 6 + 3 + (t % 3)];
    if (threadIdx.x == 0) { active[g] = 0; leaving[g] = 0; }
}

// tbim_retire_kernel with both halves of feat snapshot (the coordinate-field TBIM / BIM): columns 0..2 to
// out_adv_xyz, 3..5 to out_adv.  leaving null (the untargeted window, which has no latch): only `final` retires.
__global__ __launch_bounds__(1024) void tbim_retire_field_kernel(const float *__restrict__ feat, size_t n, int final,
                                                                 float *__restrict__ out_adv, float *__restrict__ out_adv_xyz,
                                                                 uint8_t *__restrict__ active, uint8_t *__restrict__ leaving)
{
    const int g = blockIdx.x;
    const bool go = active[g] != 0 && ((leaving && leaving[g] != 0) || final != 0);
    __syncthreads();
    if (!go) return;
    const size_t base = (size_t)g * n;
    for (size_t t = threadIdx.x; t < n * 3; t += blockDim.x) {
        const float *row = feat + (base + t / 3) * 6 + (t % 3);
        out_adv_xyz[base * 3 + t] = row[0];
        out_adv[base * 3 + t] = row[3];
    }
    if (threadIdx.x == 0) {
        active[g] = 0;
        if (leaving) leaving[g] = 0;
    }
}

// ---- NUattack / tar_NUattack on the coordinate field: Adam on delta [G][n][3] in metres, no tanh space.
//   xyz = ori + delta (masked: the other points keep ori), loss = |xyz - ori|_2 + c * score.

// nu_color_clouds_kernel's scheme for the positions: kNuParts workgroups per cloud, each with one partial sum of
// |xyz - ori|^2 in double; the positions go to feat's columns 0..2 and to the contiguous xyz the pyramid is rebuilt from
__global__ __launch_bounds__(256) void nu_coord_apply_clouds_kernel(const float *__restrict__ ori, const float *__restrict__ delta,
                                                                    const uint8_t *__restrict__ mask, const uint8_t *__restrict__ active,
                                                                    size_t n, float *__restrict__ feat, float *__restrict__ xyz,
                                                                    double *__restrict__ partials)
{
    __shared__ double s_part[4];
    const int g = blockIdx.y;
    if (active && !active[g]) return;
    const size_t base = (size_t)g * n;
    double s = 0.0;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * 3; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t / 3;
        const int c = (int)(t % 3);
        const float x = ori[base * 3 + t];
        float p = x + delta[base * 3 + t];
        if (mask && !mask[base + i]) p = x;
        feat[(base + i) * 6 + c] = p;
        xyz[base * 3 + t] = p;
        const double d = (double)p - (double)x;         // exact; the sum is of the positions as written
        s += d * d;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[(size_t)g * gridDim.x + blockIdx.x] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

// nu_adam_clouds_kernel without the tanh chain: d xyz / d delta = mask; the score's gradient is the feature path's plus the
// position branch's, one fp32 add (psg_rla_bim_step_field)
__global__ void nu_coord_adam_clouds_kernel(const float *__restrict__ ori, float *__restrict__ delta, float *__restrict__ m,
                                            float *__restrict__ v, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ active,
                                            const float *__restrict__ xyz, const float *__restrict__ dfeat, const float *__restrict__ dxyz,
                                            const float *__restrict__ dist2, size_t n, float c, float lr_arg,
                                            const float *__restrict__ consts, float b1, float b2, float eps)
{
    const int g = blockIdx.y;
    if (active && !active[g]) return;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const float lr_t = consts ? consts[3] : lr_arg;
    const size_t i = (size_t)g * n + t / 3;
    const int ch = (int)(t % 3);
    t += (size_t)g * n * 3;
    const float x = ori[t], p = xyz[t];
    const float dist = sqrtf(dist2[g]);
    const float ds = dfeat[i * 6 + ch] + dxyz[t];
    float gr = (dist > 0.0f ? (p - x) / dist : 0.0f) + c * ds;
    if (mask && !mask[i]) gr = 0.0f;                    // (not a product: whatever the gradient buffers hold there)
    const float mm = b1 * m[t] + (1.0f - b1) * gr;
    const float vv = b2 * v[t] + (1.0f - b2) * gr * gr;
    m[t] = mm;
    v[t] = vv;
    delta[t] -= lr_t * mm / (sqrtf(vv) + eps);
}

// Field latch, second half: nu_latch_commit_kernel with the 4-column row {nc, nh, d2_rgb, d2_xyz} and a snapshot that carries
// the positions too.  Workgroup 0 writes the row, the statistics, exit_step and active.
__global__ __launch_bounds__(256) void nu_field_latch_commit_kernel(const float *__restrict__ feat, const int32_t *__restrict__ pred,
                                                                    const float *__restrict__ dist2_rgb, const float *__restrict__ dist2_xyz,
                                                                    const int32_t *__restrict__ n_mask, const int32_t *__restrict__ scratch,
                                                                    int n, int mode, int num, int den, int step_arg, int can_exit, int final,
                                                                    const float *__restrict__ consts, float *__restrict__ hist_row,
                                                                    float *__restrict__ out_adv_xyz, float *__restrict__ out_adv,
                                                                    int32_t *__restrict__ out_pred, float *__restrict__ out_stats,
                                                                    uint8_t *__restrict__ active, int32_t *__restrict__ exit_step)
{
    const int g = blockIdx.y, parts = gridDim.x;
    const int32_t *sc = scratch + (size_t)g * (2 * parts + 1);
    if (!sc[0]) return;
    const int step = consts ? __builtin_bit_cast(int, consts[0]) : step_arg;
    int nc, nh;
    latch_counts(sc, parts, nc, nh);
    const bool fire = mode == 0 ? (long long)den * nc < (long long)num * n : (long long)den * nh > (long long)num * n_mask[g];
    const bool exits = fire && can_exit && step >= 1;
    if (exits || final) {
        int lo, hi;
        latch_slice(n, parts, lo, hi);
        for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            const size_t r = (size_t)g * n + i;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                out_adv_xyz[r * 3 + k] = feat[r * 6 + k];
                out_adv[r * 3 + k] = feat[r * 6 + 3 + k];
            }
            out_pred[r] = pred[r];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float row[4] = {(float)nc, (float)nh, dist2_rgb ? dist2_rgb[g] : 0.0f, dist2_xyz[g]};
        for (int k = 0; k < 4; ++k) hist_row[g * 4 + k] = row[k];
        if (exits || final)
            for (int k = 0; k < 4; ++k) out_stats[g * 4 + k] = row[k];
        if (exits) { exit_step[g] = step; active[g] = 0; }
    }
}

}  // namespace

// ---- one cloud

extern "C" int psg_rla_colper_grad_masked(const float *logits, const int32_t *ys, const uint8_t *mask, float sign, int n,
                                          float *dlogits, float *loss_out, psg_stream stream)
{
    PSG_REQUIRE(logits && ys && dlogits && n > 0, "psg_rla_colper_grad_masked: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (loss_out) PSG_CHECK_HIP(hipMemsetAsync(loss_out, 0, 4, st));
    hipLaunchKernelGGL(colper_grad_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, logits, ys, mask, sign, n, dlogits, loss_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_rla_colper_grad(const float *logits, const int32_t *labels, int n, float *dlogits, float *loss_out, psg_stream stream)
{
    PSG_REQUIRE(logits && labels && dlogits && n > 0, "psg_rla_colper_grad: bad argument");
    return psg_rla_colper_grad_masked(logits, labels, nullptr, 1.0f, n, dlogits, loss_out, stream);
}

// One BIM update of the colour half of feat [n][6] from its gradient dfeat [n][6] (norms: 2 floats of scratch).  The step of
// psg_rla_bim_attack as an entry of its own, for the attacks whose loop lives on the host because the reference reads an
// accuracy back every iteration (TBIM's `sr > 0.9` exit).
extern "C" int psg_rla_bim_step(float *feat, const float *dfeat, const float *ori, int n, float eps, float alpha, int l2_metric,
                                float *norms, float *delta, psg_stream stream)
{
    PSG_REQUIRE(feat && dfeat && ori && n > 0 && (!l2_metric || (norms && delta)), "psg_rla_bim_step: bad argument");
    return bim_step(feat, dfeat, ori, nullptr, 1, n, eps, alpha, l2_metric, norms, delta, (hipStream_t)stream);
}

// adv colours of d_ws into feat [n][6] (columns 3..5) and dist2[0] = |adv - x|_2^2 (cleared here)
extern "C" int psg_rla_nu_color(const float *xs, const float *dws, const uint8_t *mask, int n, float *feat, float *dist2,
                                psg_stream stream)
{
    PSG_REQUIRE(xs && dws && feat && dist2 && n > 0, "psg_rla_nu_color: bad argument");
    hipStream_t st = (hipStream_t)stream;
    PSG_CHECK_HIP(hipMemsetAsync(dist2, 0, 4, st));
    hipLaunchKernelGGL(nu_color_kernel, dim3(256), dim3(256), 0, st, xs, dws, mask, (size_t)n, feat, dist2);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// one Adam step (t = 1, 2, ..) on d_ws from dfeat = d score / d features [n][6] of the forward that psg_rla_nu_color fed.
// Never inside a window: its step size is the argument's, whatever step constants the thread has set.
extern "C" int psg_rla_nu_adam_step(const float *xs, float *dws, float *m, float *v, const uint8_t *mask, const float *feat,
                                    const float *dfeat, const float *dist2, int n, float c, float lr, int t, psg_stream stream)
{
    PSG_REQUIRE(xs && dws && m && v && feat && dfeat && dist2 && n > 0 && t >= 1, "psg_rla_nu_adam_step: bad argument");
    hipLaunchKernelGGL(nu_adam_clouds_kernel, dim3(blocks_for((size_t)n * 3), 1), dim3(256), 0, (hipStream_t)stream, xs, dws, m, v, mask,
                       (const uint8_t *)nullptr, feat, dfeat, dist2, (size_t)n, c, adam_lr_t(lr, t), (const float *)nullptr, 0.9f, 0.999f,
                       1e-8f);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// BIM (ares/ares/attack/bim.py:190-236): `iters` gradient steps on the colour half of the features of the workspace's clouds.
extern "C" int psg_rla_bim_attack(psg_rla_model *m, psg_rla_ws *ws, const float *features, const int32_t *labels, float eps,
                                  float alpha, int iters, int l2_metric, float *adv_features_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && features && labels && adv_features_out && iters > 0, "psg_rla_bim_attack: bad argument");
    ProfBind bind(ws);
    hipStream_t st = (hipStream_t)stream;
    const size_t N = ws->N;
    int rc;
    PSG_CHECK_HIP(hipMemcpyAsync(ws->feat, features, N * 6 * 4, hipMemcpyDeviceToDevice, st));
    PSG_CHECK_HIP(hipMemcpyAsync(ws->labels, labels, N * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(copy_cols_kernel, dim3(blocks_for(N * 3)), dim3(256), 0, st, features, 6, 3, 3, N, ws->ori, 3, 0);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(copy_cols_kernel, dim3(blocks_for(N * 3)), dim3(256), 0, st, features, 6, 0, 3, N, ws->xyz_all, 3, 0);
    PSG_LAUNCH_CHECK();
    if ((rc = build_pyramid(ws, stream))) return rc;        // geometry: once per cloud, the attack moves colours only
    auto iteration = [&]() -> int {
        int r;
        if ((r = psg_rla_forward(m, ws, ws->feat, ws->logits, stream))) return r;
        if ((r = psg_rla_colper_grad(ws->logits, ws->labels, (int)N, ws->dlogits, nullptr, stream))) return r;
        if ((r = psg_rla_backward(m, ws, ws->dlogits, ws->dfeat, stream))) return r;
        return bim_step(ws->feat, ws->dfeat, ws->ori, nullptr, ws->B, ws->Nc, eps, alpha, l2_metric, ws->norms, ws->delta, st);
    };
    // The first iteration runs eagerly (it computes the xyz branch and sets kernel attributes outside any capture); the
    // others enqueue the same launches with the same arguments, so they are captured once into a hipGraph kept in the
    // workspace and replayed: one graph launch instead of ~150 kernel launches per iteration, which is what lets several
    // long attacks on different streams actually overlap (the host would otherwise spend its time filling one stream's
    // queue).  Capture is impossible on the legacy default stream; the loop then stays eager.
    if ((rc = iteration())) return rc;
    int it = 1;
    static const bool use_graph = !((psg::env_int("PSG_RLA_NO_GRAPH", 0) != 0)) && !trace_sync_enabled();   // (the tracer synchronises after every launch)
    if (use_graph && !ws->prof.on && iters - it >= 2) {
        const bool same_key = ws->bim_model_gen == m->gen && ws->bim_eps == eps && ws->bim_alpha == alpha && ws->bim_metric == l2_metric;
        if (!same_key) PSG_CHECK_HIP(ws->bim.forget(st));
        if (!ws->bim.exec && !ws->bim.capture_failed) {
            ws->bim.capture(st, iteration);
            ws->bim_model_gen = m->gen; ws->bim_eps = eps; ws->bim_alpha = alpha; ws->bim_metric = l2_metric;
        }
        if (ws->bim.exec) {
            PSG_CHECK_HIP(ws->bim.replay(st, iters - it));
            it = iters;
        } else {
            ws->bim.note_eager(iters - it);
        }
    }
    for (; it < iters; ++it)
        if ((rc = iteration())) return rc;
    PSG_CHECK_HIP(hipMemcpyAsync(adv_features_out, ws->feat, N * 6 * 4, hipMemcpyDeviceToDevice, st));
    return PSG_OK;
}

// ---- NUattack / tar_NUattack on G clouds in lockstep (the batch workspace: one launch of every network kernel serves all clouds)

extern "C" int psg_rla_nu_color_clouds(const float *xs, const float *dws, const uint8_t *mask, const uint8_t *active, int G, int n,
                                       float *feat, float *dist2, double *partials, psg_stream stream)
{
    PSG_REQUIRE(xs && dws && feat && dist2 && partials, "psg_rla_nu_color_clouds: null argument");
    if (int rc = check_clouds("psg_rla_nu_color_clouds", G, n)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nu_color_clouds_kernel, dim3(kNuParts, G), dim3(256), 0, st, xs, dws, mask, active, (size_t)n, feat, partials);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nu_dist2_clouds_kernel, dim3(ceil_div(G, 64)), dim3(64), 0, st, partials, active, G, kNuParts, dist2);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_rla_nu_adam_clouds(const float *xs, float *dws, float *m, float *v, const uint8_t *mask, const uint8_t *active,
                                      const float *feat, const float *dfeat, const float *dist2, int G, int n, float c, float lr, int t,
                                      psg_stream stream)
{
    PSG_REQUIRE(xs && dws && m && v && feat && dfeat && dist2 && t >= 1, "psg_rla_nu_adam_clouds: bad argument");
    if (int rc = check_clouds("psg_rla_nu_adam_clouds", G, n)) return rc;
    hipLaunchKernelGGL(nu_adam_clouds_kernel, dim3(blocks_for((size_t)n * 3), G), dim3(256), 0, (hipStream_t)stream, xs, dws, m, v, mask,
                       active, feat, dfeat, dist2, (size_t)n, c, adam_lr_t(lr, t), psg::nu_step_consts(), 0.9f, 0.999f, 1e-8f);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_rla_nu_latch_clouds(const float *logits, const int32_t *labels, const int32_t *ys, const uint8_t *mask,
                                       const int32_t *n_mask, const float *feat, const float *dist2, int G, int n, int mode, int num,
                                       int den, int step, int can_exit, int final, float *hist_row, int32_t *pred, float *out_adv,
                                       int32_t *out_pred, float *out_stats, uint8_t *active, int32_t *exit_step, int32_t *scratch,
                                       psg_stream stream)
{
    PSG_REQUIRE(logits && labels && feat && dist2 && hist_row && pred && out_adv && out_pred && out_stats && active && exit_step && scratch,
                "psg_rla_nu_latch_clouds: null argument");
    if (int rc = check_clouds("psg_rla_nu_latch_clouds", G, n)) return rc;
    PSG_REQUIRE(mode == 0 || mode == 1, "psg_rla_nu_latch_clouds: mode %d out of range", mode);
    PSG_REQUIRE(!mask || ys, "psg_rla_nu_latch_clouds: a mask needs ys");
    PSG_REQUIRE(mode == 0 || (mask && n_mask), "psg_rla_nu_latch_clouds: mode 1 needs mask and n_mask");
    PSG_REQUIRE(num >= 0 && den > 0 && step >= 0, "psg_rla_nu_latch_clouds: num=%d den=%d step=%d out of range", num, den, step);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nu_latch_count_kernel, dim3(kNuParts, G), dim3(256), 0, st, logits, labels, ys, mask, (const uint8_t *)active, n, pred,
                       scratch);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nu_latch_commit_kernel, dim3(kNuParts, G), dim3(256), 0, st, feat, (const int32_t *)pred, dist2, n_mask,
                       (const int32_t *)scratch, n, mode, num, den, step, can_exit, final, psg::nu_step_consts(), hist_row, out_adv, out_pred,
                       out_stats, active, exit_step);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// One step sequence of a window, shared by the eager and the captured path; rows: the window's step-constant device rows
// {evaluation index, -, -, lr_t} or null.  Everything in it is a launch on `stream`: a single chain.
static int rla_nu_window_steps(const psg_rla_nu_window_args *a, const float *rows, psg_stream stream)
{
    const int G = a->G, N = a->N;
    const int total = a->n_steps + (a->tail_eval ? 1 : 0);
    int rc = PSG_OK;
    for (int i = 0; i < total && rc == PSG_OK; ++i) {
        const int t = a->adam_t0 + i;                // Adam index of the step; the forward before it evaluates index t - 1
        const bool tail = i == a->n_steps;
        if ((rc = psg_rla_nu_color_clouds(a->xs, a->dws, a->mask, a->active, G, N, a->feat, a->dist2, a->partials, stream))) break;
        if ((rc = psg_rla_forward(a->model, a->ws, a->feat, a->logits, stream))) break;
        psg::NuStepConsts consts(rows ? rows + 4 * i : nullptr);
        // (a captured window serves every later one: there the latch's own `step >= 1` rule keeps the start from exiting)
        rc = psg_rla_nu_latch_clouds(a->logits, a->labels, a->ys, a->mask, a->n_mask, a->feat, a->dist2, G, N, a->mode, a->num, a->den,
                                     t - 1, (rows || t - 1 >= 1) ? 1 : 0, tail ? 1 : 0, a->hist + (size_t)i * 3 * G, a->pred, a->out_adv,
                                     a->out_pred, a->out_stats, a->active, a->exit_step, a->scratch, stream);
        if (rc == PSG_OK && !tail) {
            if ((rc = psg_rla_colper_grad_masked(a->logits, a->ys, a->mask, 1.0f, G * N, a->dlogits, nullptr, stream)) == PSG_OK &&
                (rc = psg_rla_backward(a->model, a->ws, a->dlogits, a->dfeat, stream)) == PSG_OK)
                rc = psg_rla_nu_adam_clouds(a->xs, a->dws, a->m, a->v, a->mask, a->active, a->feat, a->dfeat, a->dist2, G, N, a->cs, a->lr, t,
                                            stream);
        }
    }
    return rc;
}

extern "C" int psg_rla_nu_window(const psg_rla_nu_window_args *a, psg_nu_graph *graph, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->xs && a->dws && a->m && a->v && a->labels && a->ys && a->feat && a->logits && a->dlogits &&
                    a->dfeat && a->dist2 && a->partials && a->pred && a->scratch && a->hist && a->out_adv && a->out_pred && a->out_stats &&
                    a->active && a->exit_step,
                "psg_rla_nu_window: null argument");
    PSG_REQUIRE(a->G == a->ws->B && a->N == a->ws->Nc, "psg_rla_nu_window: the workspace is for %d clouds of %d points, the window for %d of %d",
                a->ws->B, a->ws->Nc, a->G, a->N);
    PSG_REQUIRE(a->n_steps >= 1 && a->n_steps <= PSG_NU_GRAPH_MAX_STEPS, "psg_rla_nu_window: n_steps=%d outside 1..%d", a->n_steps,
                PSG_NU_GRAPH_MAX_STEPS);
    PSG_REQUIRE(a->adam_t0 >= 1, "psg_rla_nu_window: adam_t0=%d (the first step is 1)", a->adam_t0);
    PSG_REQUIRE(a->mode == 0 || a->mode == 1, "psg_rla_nu_window: mode %d out of range", a->mode);
    PSG_REQUIRE(a->mode == 0 || (a->mask && a->n_mask), "psg_rla_nu_window: mode 1 needs mask and n_mask");
    PSG_REQUIRE(a->num >= 0 && a->den > 0, "psg_rla_nu_window: threshold %d / %d out of range", a->num, a->den);
    if (!a->ws->cloud_set) { set_error("psg_rla_nu_window: psg_rla_set_cloud has not been called"); return PSG_ERR_STATE; }
    ProfBind bind(a->ws);
    // what a captured window is valid for: the argument block without what the device rows carry
    psg_rla_nu_window_args key;
    memset(&key, 0, sizeof(key));
    key = *a;
    key.adam_t0 = 0; key.lr = 0.0f;
    const int total = a->n_steps + (a->tail_eval ? 1 : 0);
    float lr_rows[PSG_NU_GRAPH_MAX_STEPS + 1];
    for (int i = 0; i < total; ++i)        // psg_rla_nu_adam_clouds' lr_t (the tail's row has no Adam step)
        lr_rows[i] = i < a->n_steps ? adam_lr_t(a->lr, a->adam_t0 + i) : 0.0f;
    // no graph while the profiler is on (per-launch events) or before the first forward of (cloud, model), which computes the
    // xyz branch: a capture would either bake it in or, replayed after a new cloud, skip it
    const bool plain = a->ws->prof.on || a->ws->xyz_branch_model != a->model->gen;
    return nu_graph_window(plain ? nullptr : graph, &key, sizeof(key), a->model->gen, a->ws->gen, total, a->adam_t0 - 1, a->adam_t0 - 1, a->lr,
                           0.9f, 0.999f, (hipStream_t)stream, [&](const float *rows) { return rla_nu_window_steps(a, rows, stream); }, lr_rows);
}

// ---- TBIM / tar_NBattack on G clouds in lockstep

extern "C" int psg_rla_bim_step_clouds(float *feat, const float *dfeat, const float *ori, const uint8_t *running, int G, int n, float eps,
                                       float alpha, int l2_metric, float *norms, float *delta, psg_stream stream)
{
    PSG_REQUIRE(feat && dfeat && ori && (!l2_metric || (norms && delta)), "psg_rla_bim_step_clouds: null argument");
    if (int rc = check_clouds("psg_rla_bim_step_clouds", G, n)) return rc;
    return bim_step(feat, dfeat, ori, running, G, n, eps, alpha, l2_metric, norms, delta, (hipStream_t)stream);
}

extern "C" int psg_rla_tbim_latch_clouds(const float *logits, const int32_t *labels, const int32_t *hit_ys, const uint8_t *mask,
                                         const int32_t *n_mask, int G, int n, int num, int den, int it, int final, float *hist_row,
                                         int32_t *pred, int32_t *out_pred, float *out_stats, const uint8_t *active, uint8_t *leaving,
                                         int32_t *exit_step, int32_t *scratch, psg_stream stream)
{
    PSG_REQUIRE(logits && labels && hit_ys && hist_row && pred && out_pred && out_stats && active && leaving && exit_step && scratch,
                "psg_rla_tbim_latch_clouds: null argument");
    PSG_REQUIRE(mask && n_mask, "psg_rla_tbim_latch_clouds: mask and n_mask are required");
    if (int rc = check_clouds("psg_rla_tbim_latch_clouds", G, n)) return rc;
    PSG_REQUIRE(num >= 0 && den > 0 && it >= 0, "psg_rla_tbim_latch_clouds: num=%d den=%d it=%d out of range", num, den, it);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nu_latch_count_kernel, dim3(kNuParts, G), dim3(256), 0, st, logits, labels, hit_ys, mask, active, n, pred, scratch);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(tbim_latch_commit_kernel, dim3(kNuParts, G), dim3(256), 0, st, (const int32_t *)pred, n_mask,
                       (const int32_t *)scratch, n, num, den, it, final, psg::nu_step_consts(), hist_row, out_pred, out_stats, leaving,
                       exit_step);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_rla_tbim_retire_clouds(const float *feat, int G, int n, int final, float *out_adv, uint8_t *active, uint8_t *leaving,
                                          psg_stream stream)
{
    PSG_REQUIRE(feat && out_adv && active && leaving, "psg_rla_tbim_retire_clouds: null argument");
    if (int rc = check_clouds("psg_rla_tbim_retire_clouds", G, n)) return rc;
    hipLaunchKernelGGL(tbim_retire_kernel, dim3(G), dim3(1024), 0, (hipStream_t)stream, feat, (size_t)n, final, out_adv, active, leaving);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// One step sequence of a TBIM window, shared by the eager and the captured path; rows: the window's step-constant device rows
// {iteration index, -, -, -} or null.  Everything in it is a launch on `stream`: a single chain.
static int rla_tbim_window_steps(const psg_rla_tbim_window_args *a, const float *rows, psg_stream stream)
{
    const int G = a->G, N = a->N;
    int rc = PSG_OK;
    for (int i = 0; i < a->n_steps && rc == PSG_OK; ++i) {
        const int final = (a->final && i == a->n_steps - 1) ? 1 : 0;
        if ((rc = psg_rla_forward(a->model, a->ws, a->feat, a->logits, stream))) break;
        {
            psg::NuStepConsts consts(rows ? rows + 4 * i : nullptr);
            rc = psg_rla_tbim_latch_clouds(a->logits, a->labels, a->hit_ys, a->mask, a->n_mask, G, N, a->num, a->den, a->it0 + i, final,
                                           a->hist + (size_t)i * 3 * G, a->pred, a->out_pred, a->out_stats, a->active, a->leaving,
                                           a->exit_step, a->scratch, stream);
        }
        if (rc == PSG_OK && (rc = psg_rla_colper_grad_masked(a->logits, a->loss_ys, a->mask, a->sign, G * N, a->dlogits, nullptr, stream)) == PSG_OK &&
            (rc = psg_rla_backward(a->model, a->ws, a->dlogits, a->dfeat, stream)) == PSG_OK &&
            (rc = psg_rla_bim_step_clouds(a->feat, a->dfeat, a->ori, a->active, G, N, a->eps, a->alpha, a->l2_metric, a->norms, a->delta,
                                          stream)) == PSG_OK)
            rc = psg_rla_tbim_retire_clouds(a->feat, G, N, final, a->out_adv, a->active, a->leaving, stream);
    }
    return rc;
}

extern "C" int psg_rla_tbim_window(const psg_rla_tbim_window_args *a, psg_nu_graph *graph, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->ori && a->labels && a->hit_ys && a->loss_ys && a->feat && a->logits && a->dlogits && a->dfeat &&
                    a->pred && a->scratch && a->hist && a->out_adv && a->out_pred && a->out_stats && a->active && a->leaving && a->exit_step,
                "psg_rla_tbim_window: null argument");
    PSG_REQUIRE(a->mask && a->n_mask, "psg_rla_tbim_window: mask and n_mask are required");
    PSG_REQUIRE(!a->l2_metric || (a->norms && a->delta), "psg_rla_tbim_window: the l_2 metric needs norms and delta");
    PSG_REQUIRE(a->G == a->ws->B && a->N == a->ws->Nc, "psg_rla_tbim_window: the workspace is for %d clouds of %d points, the window for %d of %d",
                a->ws->B, a->ws->Nc, a->G, a->N);
    PSG_REQUIRE(a->n_steps >= 1 && a->n_steps <= PSG_NU_GRAPH_MAX_STEPS, "psg_rla_tbim_window: n_steps=%d outside 1..%d", a->n_steps,
                PSG_NU_GRAPH_MAX_STEPS);
    PSG_REQUIRE(a->it0 >= 0, "psg_rla_tbim_window: it0=%d (the first iteration is 0)", a->it0);
    PSG_REQUIRE(a->num >= 0 && a->den > 0, "psg_rla_tbim_window: threshold %d / %d out of range", a->num, a->den);
    if (!a->ws->cloud_set) { set_error("psg_rla_tbim_window: psg_rla_set_cloud has not been called"); return PSG_ERR_STATE; }
    ProfBind bind(a->ws);
    // what a captured window is valid for: the argument block (padding bytes as the caller holds them) without what the device
    // rows carry
    psg_rla_tbim_window_args key;
    memcpy(&key, a, sizeof(key));
    key.it0 = 0;
    // no graph while the profiler is on (per-launch events) or before the first forward of (cloud, model), which computes the
    // xyz branch: a capture would either bake it in or, replayed after a new cloud, skip it
    const bool plain = a->ws->prof.on || a->ws->xyz_branch_model != a->model->gen;
    return nu_graph_window(plain ? nullptr : graph, &key, sizeof(key), a->model->gen, a->ws->gen, a->n_steps, a->it0, a->it0, 0.0f, 0.9f, 0.999f,
                           (hipStream_t)stream, [&](const float *rows) { return rla_tbim_window_steps(a, rows, stream); });
}

// ---- NUattack / tar_NUattack on the coordinate field, G clouds in lockstep

extern "C" int psg_rla_nu_coord_apply_clouds(const float *ori_xyz, const float *delta, const uint8_t *mask, const uint8_t *active, int G,
                                             int n, float *feat, float *xyz, float *dist2_xyz, double *partials, psg_stream stream)
{
    PSG_REQUIRE(ori_xyz && delta && feat && xyz && dist2_xyz && partials, "psg_rla_nu_coord_apply_clouds: null argument");
    if (int rc = check_clouds("psg_rla_nu_coord_apply_clouds", G, n)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nu_coord_apply_clouds_kernel, dim3(kNuParts, G), dim3(256), 0, st, ori_xyz, delta, mask, active, (size_t)n, feat, xyz,
                       partials);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nu_dist2_clouds_kernel, dim3(ceil_div(G, 64)), dim3(64), 0, st, (const double *)partials, active, G, kNuParts,
                       dist2_xyz);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_rla_nu_coord_adam_clouds(const float *ori_xyz, float *delta, float *m_xyz, float *v_xyz, const uint8_t *mask,
                                            const uint8_t *active, const float *xyz, const float *dfeat, const float *dxyz,
                                            const float *dist2_xyz, int G, int n, float c, float lr, int t, psg_stream stream)
{
    PSG_REQUIRE(ori_xyz && delta && m_xyz && v_xyz && xyz && dfeat && dxyz && dist2_xyz && t >= 1, "psg_rla_nu_coord_adam_clouds: bad argument");
    if (int rc = check_clouds("psg_rla_nu_coord_adam_clouds", G, n)) return rc;
    hipLaunchKernelGGL(nu_coord_adam_clouds_kernel, dim3(blocks_for((size_t)n * 3), G), dim3(256), 0, (hipStream_t)stream, ori_xyz, delta,
                       m_xyz, v_xyz, mask, active, xyz, dfeat, dxyz, dist2_xyz, (size_t)n, c, adam_lr_t(lr, t), psg::nu_step_consts(), 0.9f,
                       0.999f, 1e-8f);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_rla_nu_field_latch_clouds(const float *logits, const int32_t *labels, const int32_t *ys, const uint8_t *mask,
                                             const int32_t *n_mask, const float *feat, const float *dist2_rgb, const float *dist2_xyz, int G,
                                             int n, int mode, int num, int den, int step, int can_exit, int final, float *hist_row,
                                             int32_t *pred, float *out_adv_xyz, float *out_adv, int32_t *out_pred, float *out_stats,
                                             uint8_t *active, int32_t *exit_step, int32_t *scratch, psg_stream stream)
{
    PSG_REQUIRE(logits && labels && feat && dist2_xyz && hist_row && pred && out_adv_xyz && out_adv && out_pred && out_stats && active &&
                    exit_step && scratch,
                "psg_rla_nu_field_latch_clouds: null argument");
    if (int rc = check_clouds("psg_rla_nu_field_latch_clouds", G, n)) return rc;
    PSG_REQUIRE(mode == 0 || mode == 1, "psg_rla_nu_field_latch_clouds: mode %d out of range", mode);
    PSG_REQUIRE(!mask || ys, "psg_rla_nu_field_latch_clouds: a mask needs ys");
    PSG_REQUIRE(mode == 0 || (mask && n_mask), "psg_rla_nu_field_latch_clouds: mode 1 needs mask and n_mask");
    PSG_REQUIRE(num >= 0 && den > 0 && step >= 0, "psg_rla_nu_field_latch_clouds: num=%d den=%d step=%d out of range", num, den, step);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nu_latch_count_kernel, dim3(kNuParts, G), dim3(256), 0, st, logits, labels, ys, mask, (const uint8_t *)active, n, pred,
                       scratch);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nu_field_latch_commit_kernel, dim3(kNuParts, G), dim3(256), 0, st, feat, (const int32_t *)pred, dist2_rgb, dist2_xyz,
                       n_mask, (const int32_t *)scratch, n, mode, num, den, step, can_exit, final, psg::nu_step_consts(), hist_row, out_adv_xyz,
                       out_adv, out_pred, out_stats, active, exit_step);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// the positions of the step into the workspace and the pyramid of all clouds on them: psg_rla_set_cloud's two steps, from the
// window's own device buffer; stream-ordered, nothing is read back
static int rla_field_pyramid(psg_rla_ws *ws, const float *xyz, psg_stream stream)
{
    PSG_CHECK_HIP(hipMemcpyAsync(ws->xyz_all, xyz, (size_t)ws->N * 3 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return build_pyramid(ws, stream);
}

extern "C" int psg_rla_nu_field_window(const psg_rla_nu_field_window_args *a, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws, "psg_rla_nu_field_window: null argument");
    PSG_REQUIRE(a->field == PSG_NU_FIELD_COORD || a->field == PSG_NU_FIELD_BOTH, "psg_rla_nu_field_window: field %d is neither coord nor both",
                a->field);
    const bool both = a->field == PSG_NU_FIELD_BOTH;
    PSG_REQUIRE(a->delta && a->m_xyz && a->v_xyz && a->ori_xyz && a->xyz && a->dxyz && a->labels && a->ys && a->feat && a->logits &&
                    a->dlogits && a->dfeat && a->dist2_xyz && a->partials_xyz && a->pred && a->scratch && a->hist && a->out_adv &&
                    a->out_adv_xyz && a->out_pred && a->out_stats && a->active && a->exit_step,
                "psg_rla_nu_field_window: null argument");
    PSG_REQUIRE(!both || (a->xs && a->dws && a->m && a->v && a->dist2 && a->partials),
                "psg_rla_nu_field_window: field both needs the colour variable (xs, dws, m, v, dist2, partials)");
    PSG_REQUIRE(a->ws->full, "psg_rla_nu_field_window: the workspace was not made by psg_rla_ws_create_full");
    PSG_REQUIRE(a->G == a->ws->B && a->N == a->ws->Nc,
                "psg_rla_nu_field_window: the workspace is for %d clouds of %d points, the window for %d of %d", a->ws->B, a->ws->Nc, a->G, a->N);
    if (int rc = check_clouds("psg_rla_nu_field_window", a->G, a->N)) return rc;
    PSG_REQUIRE(a->n_steps >= 1, "psg_rla_nu_field_window: n_steps=%d (at least 1)", a->n_steps);
    PSG_REQUIRE(a->adam_t0 >= 1, "psg_rla_nu_field_window: adam_t0=%d (the first step is 1)", a->adam_t0);
    PSG_REQUIRE(a->mode == 0 || a->mode == 1, "psg_rla_nu_field_window: mode %d out of range", a->mode);
    PSG_REQUIRE(a->mode == 0 || (a->mask && a->n_mask), "psg_rla_nu_field_window: mode 1 needs mask and n_mask");
    PSG_REQUIRE(a->num >= 0 && a->den > 0, "psg_rla_nu_field_window: threshold %d / %d out of range", a->num, a->den);
    ProfBind bind(a->ws);
    const int G = a->G, N = a->N;
    const int total = a->n_steps + (a->tail_eval ? 1 : 0);
    const float *d2_rgb = both ? a->dist2 : nullptr;
    int rc = PSG_OK;
    for (int i = 0; i < total && rc == PSG_OK; ++i) {
        const int t = a->adam_t0 + i;                // Adam index of the step; the forward before it evaluates index t - 1
        const bool tail = i == a->n_steps;
        if ((rc = psg_rla_nu_coord_apply_clouds(a->ori_xyz, a->delta, a->mask, a->active, G, N, a->feat, a->xyz, a->dist2_xyz,
                                                a->partials_xyz, stream)))
            break;
        if (both && (rc = psg_rla_nu_color_clouds(a->xs, a->dws, a->mask, a->active, G, N, a->feat, a->dist2, a->partials, stream))) break;
        if ((rc = rla_field_pyramid(a->ws, a->xyz, stream))) break;
        if ((rc = psg_rla_forward(a->model, a->ws, a->feat, a->logits, stream))) break;
        rc = psg_rla_nu_field_latch_clouds(a->logits, a->labels, a->ys, a->mask, a->n_mask, a->feat, d2_rgb, a->dist2_xyz, G, N, a->mode,
                                           a->num, a->den, t - 1, t - 1 >= 1 ? 1 : 0, tail ? 1 : 0, a->hist + (size_t)i * 4 * G, a->pred,
                                           a->out_adv_xyz, a->out_adv, a->out_pred, a->out_stats, a->active, a->exit_step, a->scratch, stream);
        if (rc != PSG_OK || tail) continue;
        if ((rc = psg_rla_colper_grad_masked(a->logits, a->ys, a->mask, 1.0f, G * N, a->dlogits, nullptr, stream))) break;
        if ((rc = psg_rla_backward_full(a->model, a->ws, a->dlogits, a->dfeat, a->dxyz, stream))) break;
        if ((rc = psg_rla_nu_coord_adam_clouds(a->ori_xyz, a->delta, a->m_xyz, a->v_xyz, a->mask, a->active, a->xyz, a->dfeat, a->dxyz,
                                               a->dist2_xyz, G, N, a->cs, a->coord_lr, t, stream)))
            break;
        if (both)
            rc = psg_rla_nu_adam_clouds(a->xs, a->dws, a->m, a->v, a->mask, a->active, a->feat, a->dfeat, a->dist2, G, N, a->cs, a->lr, t,
                                        stream);
    }
    return rc;
}

// ---- BIM / TBIM on the coordinate field, G clouds in lockstep

extern "C" int psg_rla_tbim_retire_field_clouds(const float *feat, int G, int n, int final, float *out_adv, float *out_adv_xyz,
                                                uint8_t *active, uint8_t *leaving, psg_stream stream)
{
    PSG_REQUIRE(feat && out_adv && out_adv_xyz && active && leaving, "psg_rla_tbim_retire_field_clouds: null argument");
    if (int rc = check_clouds("psg_rla_tbim_retire_field_clouds", G, n)) return rc;
    hipLaunchKernelGGL(tbim_retire_field_kernel, dim3(G), dim3(1024), 0, (hipStream_t)stream, feat, (size_t)n, final, out_adv, out_adv_xyz,
                       active, leaving);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_rla_bim_field_window(const psg_rla_bim_field_window_args *a, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws, "psg_rla_bim_field_window: null argument");
    PSG_REQUIRE(a->mode == 0 || a->mode == 1, "psg_rla_bim_field_window: mode %d out of range", a->mode);
    PSG_REQUIRE(a->field == PSG_NU_FIELD_COORD || a->field == PSG_NU_FIELD_BOTH, "psg_rla_bim_field_window: field %d is neither coord nor both",
                a->field);
    const bool both = a->field == PSG_NU_FIELD_BOTH, tbim = a->mode == 1;
    PSG_REQUIRE(a->ori_xyz && a->xyz && a->dxyz && a->out_adv_xyz && a->labels && a->feat && a->logits && a->dlogits && a->dfeat && a->pred &&
                    a->scratch && a->out_adv && a->out_pred && a->out_stats && a->active,
                "psg_rla_bim_field_window: null argument");
    PSG_REQUIRE(!tbim || (a->mask && a->n_mask && a->hit_ys && a->loss_ys && a->hist && a->leaving && a->exit_step),
                "psg_rla_bim_field_window: mode 1 needs mask, n_mask, hit_ys, loss_ys, hist, leaving and exit_step");
    PSG_REQUIRE(!a->l2_metric || (a->norms_xyz && a->delta && (!both || a->norms)),
                "psg_rla_bim_field_window: the l_2 metric needs norms_xyz and delta (field both: norms too)");
    PSG_REQUIRE(!both || a->ori, "psg_rla_bim_field_window: field both needs ori (the clean colours)");
    PSG_REQUIRE(a->ws->full, "psg_rla_bim_field_window: the workspace was not made by psg_rla_ws_create_full");
    PSG_REQUIRE(a->G == a->ws->B && a->N == a->ws->Nc,
                "psg_rla_bim_field_window: the workspace is for %d clouds of %d points, the window for %d of %d", a->ws->B, a->ws->Nc, a->G, a->N);
    if (int rc = check_clouds("psg_rla_bim_field_window", a->G, a->N)) return rc;
    PSG_REQUIRE(a->n_steps >= 1, "psg_rla_bim_field_window: n_steps=%d (at least 1)", a->n_steps);
    PSG_REQUIRE(a->it0 >= 0, "psg_rla_bim_field_window: it0=%d (the first iteration is 0)", a->it0);
    PSG_REQUIRE(a->num >= 0 && a->den > 0, "psg_rla_bim_field_window: threshold %d / %d out of range", a->num, a->den);
    ProfBind bind(a->ws);
    hipStream_t st = (hipStream_t)stream;
    const int G = a->G, N = a->N;
    int rc = PSG_OK;
    for (int i = 0; i < a->n_steps && rc == PSG_OK; ++i) {
        const int final = (a->final && i == a->n_steps - 1) ? 1 : 0;
        if ((rc = rla_field_pyramid(a->ws, a->xyz, stream))) break;
        if ((rc = psg_rla_forward(a->model, a->ws, a->feat, a->logits, stream))) break;
        if (tbim) {
            if ((rc = psg_rla_tbim_latch_clouds(a->logits, a->labels, a->hit_ys, a->mask, a->n_mask, G, N, a->num, a->den, a->it0 + i, final,
                                                a->hist + (size_t)i * 3 * G, a->pred, a->out_pred, a->out_stats, a->active, a->leaving,
                                                a->exit_step, a->scratch, stream)))
                break;
            rc = psg_rla_colper_grad_masked(a->logits, a->loss_ys, a->mask, a->sign, G * N, a->dlogits, nullptr, stream);
        } else {
            rc = psg_rla_colper_grad_masked(a->logits, a->labels, nullptr, 1.0f, G * N, a->dlogits, nullptr, stream);
        }
        if (rc) break;
        if ((rc = psg_rla_backward_full(a->model, a->ws, a->dlogits, a->dfeat, a->dxyz, stream))) break;
        if ((rc = psg_rla_bim_step_field_clouds(a->feat, a->dfeat, a->dxyz, a->ori_xyz, a->active, G, N, a->coord_eps, a->coord_alpha,
                                                a->l2_metric, a->norms_xyz, a->delta, a->xyz, stream)))
            break;
        if (both && (rc = psg_rla_bim_step_clouds(a->feat, a->dfeat, a->ori, a->active, G, N, a->eps, a->alpha, a->l2_metric, a->norms,
                                                  a->delta, stream)))
            break;
        if (tbim || final) {        // (the untargeted loop has no latch and no exit: only the cap retires, every cloud)
            hipLaunchKernelGGL(tbim_retire_field_kernel, dim3(G), dim3(1024), 0, st, (const float *)a->feat, (size_t)N, final, a->out_adv,
                               a->out_adv_xyz, a->active, a->leaving);
            PSG_LAUNCH_CHECK();
        }
    }
    return rc;
}
