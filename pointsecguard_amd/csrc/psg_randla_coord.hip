// RandLA-Net, coordinate field: the two geometry kernels of the position-branch gradient and the BIM
// step on the coordinate half of the features.  Compiled with -ffp-contract=off: the unit vector rel / dist is an IEEE
// division followed by a product, and the sums run in the fixed order the float64 stage reference states
// (tests/rla_coord_ref64.py); psg_randla_net.hip holds the workspace and launches these from psg_rla_backward_full.
#include "psg_randla_coord.h"

using namespace psg;

namespace {

constexpr int RK = 16;

inline unsigned blocks_for(size_t total) { return (unsigned)((total + 255) / 256); }

// relpos[e] = [dist, rel (3), x_i (3), x_j (3)] with rel = x_i - x_j.  d dist / d rel = rel / dist; dist == 0 (every point is
// its own first neighbour; coincident points) contributes exactly zero from the distance column: rel is identically zero on a
// self edge, so zero is the derivative there, and for two distinct coincident points it is the convention.
__global__ void relpos_bwd_kernel(const float *__restrict__ relpos, const float *__restrict__ g_rp, size_t edges,
                                  float4 *__restrict__ side_i, float4 *__restrict__ side_j)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= edges) return;
    const float *r = relpos + e * 10, *g = g_rp + e * 10;
    const float dist = r[0], g0 = g[0];
    float gr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float unit = dist == 0.0f ? 0.0f : r[1 + c] / dist;
        gr[c] = dist == 0.0f ? g[1 + c] : g[1 + c] + g0 * unit;
    }
    side_i[e] = make_float4(gr[0] + g[4], gr[1] + g[5], gr[2] + g[6], 0.0f);
    side_j[e] = make_float4(g[7] - gr[0], g[8] - gr[1], g[9] - gr[2], 0.0f);
}

// one writer per row, a fixed order, no float atomics
__global__ void point_sum_kernel(const float4 *__restrict__ side_i, const float4 *__restrict__ side_j, const int32_t *__restrict__ inv_off,
                                 const int32_t *__restrict__ inv_ent, const float *__restrict__ g_next, int nc, int nc_sub, size_t n,
                                 float *__restrict__ gxyz)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
#pragma unroll
    for (int k = 0; k < RK; ++k) {
        const float4 v = side_i[p * RK + k];
        ax += v.x; ay += v.y; az += v.z;
    }
    const int e1 = inv_off[p + 1];
    for (int t = inv_off[p]; t < e1; ++t) {
        const float4 v = side_j[inv_ent[t]];
        ax += v.x; ay += v.y; az += v.z;
    }
    const size_t b = p / (size_t)nc, q = p - b * (size_t)nc;
    if (g_next && q < (size_t)nc_sub) {
        const float *s = g_next + (b * (size_t)nc_sub + q) * 3;
        ax += s[0]; ay += s[1]; az += s[2];
    }
    gxyz[p * 3] = ax; gxyz[p * 3 + 1] = ay; gxyz[p * 3 + 2] = az;
}

// ---- BIM step on the coordinate columns 0:3 of feat [G][n][6] (bim.py:84-96), g = dfeat[:, 0:3] + dxyz as one fp32 add; no clip
// to a box.  One copy of the kernels for 1 and G clouds, as bim_step's in psg_randla_attack.hip: blockIdx.y = cloud (blockIdx.x
// for the norm kernel), a cloud whose `running` byte is clear is skipped by whole workgroups, a null byte array runs every
// cloud.  The l_2 norms in psg_rla_bim_step's order: one workgroup per cloud, every thread its strided elements in double, a
// fixed tree.  The apply kernels also write the new position into the contiguous xyz_out [G][n][3] when it is given.
__device__ __forceinline__ float field_grad(const float *__restrict__ dfeat, const float *__restrict__ dxyz, size_t t)
{
    return dfeat[(t / 3) * 6 + (t % 3)] + dxyz[t];
}

// dfeat / dxyz (delta null) or delta: the arrays of all clouds; out[cloud]
__global__ __launch_bounds__(1024) void field_sq_norm_kernel(const float *__restrict__ dfeat, const float *__restrict__ dxyz,
                                                              const float *__restrict__ delta, const uint8_t *__restrict__ running,
                                                              size_t n, float *__restrict__ out)
{
    __shared__ double s_part[16];
    if (running && !running[blockIdx.x]) return;
    const size_t base = (size_t)blockIdx.x * n * 3;
    double s = 0.0;
    for (size_t t = threadIdx.x; t < n * 3; t += blockDim.x) {
        const float v = delta ? delta[base + t] : field_grad(dfeat, dxyz, base + t);
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

__global__ void field_linf_kernel(float *__restrict__ feat, const float *__restrict__ dfeat, const float *__restrict__ dxyz,
                                  const float *__restrict__ ori, const uint8_t *__restrict__ running, size_t n, float alpha, float eps,
                                  float *__restrict__ xyz_out)
{
    const int cl = blockIdx.y;
    if (running && !running[cl]) return;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    t += (size_t)cl * n * 3;
    const size_t at = (t / 3) * 6 + (t % 3);
    const float g = field_grad(dfeat, dxyz, t), x = ori[t];
    const float sg = g > 0.0f ? 1.0f : (g < 0.0f ? -1.0f : 0.0f);
    const float v = feat[at] + alpha * sg;
    const float p = fminf(fmaxf(v, x - eps), x + eps);
    feat[at] = p;
    if (xyz_out) xyz_out[t] = p;
}

__global__ void field_l2_delta_kernel(const float *__restrict__ feat, const float *__restrict__ dfeat, const float *__restrict__ dxyz,
                                      const float *__restrict__ ori, const uint8_t *__restrict__ running, size_t n, float alpha,
                                      const float *__restrict__ gnorm2, float *__restrict__ delta)
{
    const int cl = blockIdx.y;
    if (running && !running[cl]) return;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    t += (size_t)cl * n * 3;
    const float gn = fmaxf(1e-12f, sqrtf(gnorm2[cl]));            // the cloud's own gradient norm
    delta[t] = feat[(t / 3) * 6 + (t % 3)] - ori[t] + alpha * (field_grad(dfeat, dxyz, t) / gn);
}

__global__ void field_l2_apply_kernel(float *__restrict__ feat, const float *__restrict__ ori, const float *__restrict__ delta,
                                      const uint8_t *__restrict__ running, size_t n, float eps, const float *__restrict__ dnorm2,
                                      float *__restrict__ xyz_out)
{
    const int cl = blockIdx.y;
    if (running && !running[cl]) return;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    t += (size_t)cl * n * 3;
    const float dn = sqrtf(dnorm2[cl]);
    const float scale = dn > eps ? eps / dn : 1.0f;
    const float p = ori[t] + delta[t] * scale;
    feat[(t / 3) * 6 + (t % 3)] = p;
    if (xyz_out) xyz_out[t] = p;
}

// One field step of the running clouds: one launch for l_inf, four for l_2 (norms [2][G] and delta [G][n][3] are its scratch).
// The one copy behind psg_rla_bim_step_field (G = 1) and psg_rla_bim_step_field_clouds.
int field_step(float *feat, const float *dfeat, const float *dxyz, const float *ori, const uint8_t *running, int G, int n, float eps,
               float alpha, int l2, float *norms, float *delta, float *xyz_out, hipStream_t st)
{
    const size_t N = (size_t)n;
    const dim3 grid(blocks_for(N * 3), G);
    if (!l2) {
        hipLaunchKernelGGL(field_linf_kernel, grid, dim3(256), 0, st, feat, dfeat, dxyz, ori, running, N, alpha, eps, xyz_out);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    hipLaunchKernelGGL(field_sq_norm_kernel, dim3(G), dim3(1024), 0, st, dfeat, dxyz, (const float *)nullptr, running, N, norms);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(field_l2_delta_kernel, grid, dim3(256), 0, st, (const float *)feat, dfeat, dxyz, ori, running, N, alpha,
                       (const float *)norms, delta);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(field_sq_norm_kernel, dim3(G), dim3(1024), 0, st, dfeat, dxyz, (const float *)delta, running, N, norms + G);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(field_l2_apply_kernel, grid, dim3(256), 0, st, feat, ori, (const float *)delta, running, N, eps,
                       (const float *)(norms + G), xyz_out);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

}  // namespace

int psg::rla_relpos_bwd(const float *relpos, const float *g_rp, size_t edges, float4 *side_i, float4 *side_j, hipStream_t st)
{
    hipLaunchKernelGGL(relpos_bwd_kernel, dim3(blocks_for(edges)), dim3(256), 0, st, relpos, g_rp, edges, side_i, side_j);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

int psg::rla_point_sum(const float4 *side_i, const float4 *side_j, const int32_t *inv_off, const int32_t *inv_ent, const float *g_next,
                       int nc, int nc_sub, size_t n, float *gxyz, hipStream_t st)
{
    hipLaunchKernelGGL(point_sum_kernel, dim3(blocks_for(n)), dim3(256), 0, st, side_i, side_j, inv_off, inv_ent, g_next, nc, nc_sub, n, gxyz);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_rla_bim_step_field(float *feat, const float *dfeat, const float *dxyz, const float *ori_xyz, int n, float eps,
                                      float alpha, int l2_metric, float *norms, float *delta, psg_stream stream)
{
    PSG_REQUIRE(feat && dfeat && dxyz && ori_xyz && n > 0 && (!l2_metric || (norms && delta)), "psg_rla_bim_step_field: bad argument");
    return field_step(feat, dfeat, dxyz, ori_xyz, nullptr, 1, n, eps, alpha, l2_metric, norms, delta, nullptr, (hipStream_t)stream);
}

// psg_rla_bim_step_field's update of every running cloud with that cloud's own norms (the limits: psg_randla_attack.hip's
// check_clouds - G is a grid dimension, G * n rows are indexed by 32-bit ints on the host side)
extern "C" int psg_rla_bim_step_field_clouds(float *feat, const float *dfeat, const float *dxyz, const float *ori_xyz, const uint8_t *running,
                                             int G, int n, float eps, float alpha, int l2_metric, float *norms, float *delta, float *xyz_out,
                                             psg_stream stream)
{
    PSG_REQUIRE(feat && dfeat && dxyz && ori_xyz && (!l2_metric || (norms && delta)), "psg_rla_bim_step_field_clouds: null argument");
    PSG_REQUIRE(G > 0 && G <= 65535 && n > 0 && (size_t)G * n <= (size_t)1 << 20, "psg_rla_bim_step_field_clouds: G=%d n=%d out of range", G, n);
    return field_step(feat, dfeat, dxyz, ori_xyz, running, G, n, eps, alpha, l2_metric, norms, delta, xyz_out, (hipStream_t)stream);
}
