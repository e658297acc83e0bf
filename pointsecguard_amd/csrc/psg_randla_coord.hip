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

// ---- BIM step on the coordinate columns 0:3 of feat [n][6] (bim.py:84-96), g = dfeat[:, 0:3] + dxyz as one fp32 add; no clip
// to a box.  The l_2 norms in psg_rla_bim_step's order: one workgroup, every thread its strided elements in double, a fixed tree.
__device__ __forceinline__ float field_grad(const float *__restrict__ dfeat, const float *__restrict__ dxyz, size_t t)
{
    return dfeat[(t / 3) * 6 + (t % 3)] + dxyz[t];
}

__global__ __launch_bounds__(1024) void field_sq_norm_kernel(const float *__restrict__ dfeat, const float *__restrict__ dxyz,
                                                              const float *__restrict__ delta, size_t n, float *__restrict__ out)
{
    __shared__ double s_part[16];
    double s = 0.0;
    for (size_t t = threadIdx.x; t < n * 3; t += blockDim.x) {
        const float v = delta ? delta[t] : field_grad(dfeat, dxyz, t);
        s += (double)v * (double)v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += s_part[w];
        out[0] = (float)tot;
    }
}

__global__ void field_linf_kernel(float *__restrict__ feat, const float *__restrict__ dfeat, const float *__restrict__ dxyz,
                                  const float *__restrict__ ori, size_t n, float alpha, float eps)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const size_t at = (t / 3) * 6 + (t % 3);
    const float g = field_grad(dfeat, dxyz, t), x = ori[t];
    const float sg = g > 0.0f ? 1.0f : (g < 0.0f ? -1.0f : 0.0f);
    const float v = feat[at] + alpha * sg;
    feat[at] = fminf(fmaxf(v, x - eps), x + eps);
}

__global__ void field_l2_delta_kernel(const float *__restrict__ feat, const float *__restrict__ dfeat, const float *__restrict__ dxyz,
                                      const float *__restrict__ ori, size_t n, float alpha, const float *__restrict__ gnorm2,
                                      float *__restrict__ delta)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const float gn = fmaxf(1e-12f, sqrtf(gnorm2[0]));
    delta[t] = feat[(t / 3) * 6 + (t % 3)] - ori[t] + alpha * (field_grad(dfeat, dxyz, t) / gn);
}

__global__ void field_l2_apply_kernel(float *__restrict__ feat, const float *__restrict__ ori, const float *__restrict__ delta, size_t n,
                                      float eps, const float *__restrict__ dnorm2)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const float dn = sqrtf(dnorm2[0]);
    const float scale = dn > eps ? eps / dn : 1.0f;
    feat[(t / 3) * 6 + (t % 3)] = ori[t] + delta[t] * scale;
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
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)n;
    if (!l2_metric) {
        hipLaunchKernelGGL(field_linf_kernel, dim3(blocks_for(N * 3)), dim3(256), 0, st, feat, dfeat, dxyz, ori_xyz, N, alpha, eps);
        PSG_LAUNCH_CHECK();
        return PSG_OK;
    }
    hipLaunchKernelGGL(field_sq_norm_kernel, dim3(1), dim3(1024), 0, st, dfeat, dxyz, (const float *)nullptr, N, norms);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(field_l2_delta_kernel, dim3(blocks_for(N * 3)), dim3(256), 0, st, feat, dfeat, dxyz, ori_xyz, N, alpha, norms, delta);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(field_sq_norm_kernel, dim3(1), dim3(1024), 0, st, dfeat, dxyz, (const float *)delta, N, norms + 1);
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(field_l2_apply_kernel, dim3(blocks_for(N * 3)), dim3(256), 0, st, feat, ori_xyz, delta, N, eps, norms + 1);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}
