// Coordinate gradient of the PointNet++ SSG network through its two differentiable geometric paths (DESIGN.md section
// 5k), with the FPS / ball-query / 3-NN INDICES constant, as the reference's autograd has them:
//   * relative coordinates of a set-abstraction level (pointnet_util.py:126-140): grouped_xyz_norm = xyz[idx] - new_xyz,
//     so a grouped row's g_rel = W1x^T dZ1 goes + to its source point and - (summed over the group) to the group's centre;
//   * 3-NN interpolation weights of a feature-propagation level (pointnet_util.py:301-309): w_k = r_k / sum r,
//     r_k = 1 / (d_k + 1e-8), d = square_distance(xyz1, xyz2);
//   * new_xyz = xyz[fps_idx]: a level's coordinate gradient goes down through the (injective) FPS table.
// Gather / small-dot kernels: every output has one writer and a fixed summation order (no float atomics), so two runs are
// bit-equal and the result is exactly linear in the upstream gradient.  Launched by psg_pn2_backward_full only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psg_mlp.cuh"      // xcd_tile
#include "psg_sqdist.cuh"

namespace psg {

constexpr int GG_NT = 256;      // threads per workgroup
constexpr int GG_LANES = 16;    // lanes that share one row (a quarter wave: 16-byte pieces of a 64 .. 512 float row)

// sum over the 16 lanes of a row group (xor butterfly inside the quarter wave; every lane ends with the same sum, formed
// in the same order)
__device__ __forceinline__ float gg_sum16(float v)
{
#pragma unroll
    for (int m = GG_LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, GG_LANES);
    return v;
}

// g_rel of a split SA level (1 - 3): sa_bwd stored the masked dZ1 rows [C1] in list order (slot = ginv_pos[row]; padding
// rows are not listed and carry zero); grel[slot] = {W1x^T dZ1, 0} with the layer's three xyz columns w1x [3][C1] in LDS.
// n_listed of a room = the end of its last inverse list.  C1 is a multiple of 64.
__global__ __launch_bounds__(GG_NT) void sa_grel_kernel(const float *__restrict__ dz1, const int32_t *__restrict__ ginv_off,
                                                        int n_src, int g_rows, const float *__restrict__ w1x, int C1,
                                                        float4 *__restrict__ grel)
{
    extern __shared__ float s_w1x[];   // [3][C1]
    for (int i = threadIdx.x; i < 3 * C1; i += GG_NT) s_w1x[i] = w1x[i];
    __syncthreads();
    int bx, b;
    xcd_tile(bx, b);   // consecutive workgroups of one room on one XCD, like the module kernels
    const int q = threadIdx.x & (GG_LANES - 1), rg = threadIdx.x / GG_LANES;
    const int n_listed = min(ginv_off[(size_t)b * (n_src + 1) + n_src], g_rows);
    const float *rows = dz1 + (size_t)b * g_rows * C1;
    float4 *out = grel + (size_t)b * g_rows;
    constexpr int RG = GG_NT / GG_LANES;
    for (int slot = bx * RG + rg; slot < n_listed; slot += gridDim.x * RG) {
        const float *row = rows + (size_t)slot * C1;
        float ax = 0.f, ay = 0.f, az = 0.f;
        for (int c = 4 * q; c < C1; c += 4 * GG_LANES) {
            const float4 v = *(const float4 *)(row + c);
            const float4 wx = *(const float4 *)(s_w1x + c), wy = *(const float4 *)(s_w1x + C1 + c),
                         wz = *(const float4 *)(s_w1x + 2 * C1 + c);
            ax += v.x * wx.x + v.y * wx.y + v.z * wx.z + v.w * wx.w;
            ay += v.x * wy.x + v.y * wy.y + v.z * wy.z + v.w * wy.w;
            az += v.x * wz.x + v.y * wz.y + v.z * wz.z + v.w * wz.w;
        }
        ax = gg_sum16(ax); ay = gg_sum16(ay); az = gg_sum16(az);
        if (q == 0) out[slot] = make_float4(ax, ay, az, 0.f);
    }
}

// d loss / d (squared distance) of the three neighbours of every fine point of an FP level:
//   dL/dw_k = <dint_i, src[idx_k]>   (dint: the interpolated part's gradient rows; src: the rows that were interpolated -
//                                     the coarse level's T rows under the FP split, its feature rows otherwise)
//   w = r / norm, r = 1 / (d + 1e-8):  dL/dr_k = dL/dw_k / norm - (sum_j dL/dw_j r_j) / norm^2,  dL/dd_k = -r_k^2 dL/dr_k
// with d_k recomputed as three_nn_kernel computed it (psg::sqdist: the forward's own distances, rounding noise at
// coincident points included).  out[i] = {dL/dd_0, dL/dd_1, dL/dd_2, 0}.  C is a multiple of 64.
__global__ __launch_bounds__(GG_NT) void fp_wgrad_kernel(const float *__restrict__ dint, const float *__restrict__ src, int C,
                                                         const int32_t *__restrict__ nn_idx, const float *__restrict__ xyz1,
                                                         const float *__restrict__ xyz2, int N, int S, float4 *__restrict__ out)
{
    int bx, b;
    xcd_tile(bx, b);
    const int q = threadIdx.x & (GG_LANES - 1), rg = threadIdx.x / GG_LANES;
    constexpr int RG = GG_NT / GG_LANES;
    const int32_t *idx = nn_idx + (size_t)b * N * 3;
    const float *f = xyz1 + (size_t)b * N * 3, *c = xyz2 + (size_t)b * S * 3;
    for (int i = bx * RG + rg; i < N; i += gridDim.x * RG) {
        int j[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) j[k] = min(max(idx[3 * i + k], 0), S - 1);
        const float *g = dint + ((size_t)b * N + i) * C;
        const float *s0 = src + ((size_t)b * S + j[0]) * C, *s1 = src + ((size_t)b * S + j[1]) * C,
                    *s2 = src + ((size_t)b * S + j[2]) * C;
        float dw0 = 0.f, dw1 = 0.f, dw2 = 0.f;
        for (int ch = 4 * q; ch < C; ch += 4 * GG_LANES) {
            const float4 v = *(const float4 *)(g + ch);
            const float4 a0 = *(const float4 *)(s0 + ch), a1 = *(const float4 *)(s1 + ch), a2 = *(const float4 *)(s2 + ch);
            dw0 += v.x * a0.x + v.y * a0.y + v.z * a0.z + v.w * a0.w;
            dw1 += v.x * a1.x + v.y * a1.y + v.z * a1.z + v.w * a1.w;
            dw2 += v.x * a2.x + v.y * a2.y + v.z * a2.z + v.w * a2.w;
        }
        dw0 = gg_sum16(dw0); dw1 = gg_sum16(dw1); dw2 = gg_sum16(dw2);
        if (q != 0) continue;
        const float fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2], fsq = sumsq3(fx, fy, fz);
        float r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float cx = c[3 * j[k]], cy = c[3 * j[k] + 1], cz = c[3 * j[k] + 2];
            const float d = sqdist(fx, fy, fz, fsq, cx, cy, cz, sumsq3(cx, cy, cz));
            r[k] = __fdiv_rn(1.0f, __fadd_rn(d, 1e-8f));
        }
        const float norm = __fadd_rn(__fadd_rn(r[0], r[1]), r[2]);
        const float dnorm = -((dw0 * r[0] + dw1 * r[1]) + dw2 * r[2]) / (norm * norm);
        out[(size_t)b * N + i] = make_float4(-(dw0 / norm + dnorm) * r[0] * r[0], -(dw1 / norm + dnorm) * r[1] * r[1],
                                             -(dw2 / norm + dnorm) * r[2] * r[2], 0.f);
    }
}

// The coordinate gradient of the points of ONE level (room-local arrays, already offset to the plan slot), one thread per
// point; any of the four parts is switched off by a null table.  Summation order: source rows (ascending slot), group rows
// (ascending sample), own 3-NN (k = 0, 1, 2), fine points that interpolate from this one (ascending fine point).
struct GxArgs {
    int n;                          // points of this level per room
    // this level's points as SOURCES of its own SA grouping: + g_rel over the point's inverse group list
    const int32_t *src_off;         // [B][n + 1]
    const float *src_rows;          // [B][src_n][src_ld], g_rel at columns src_col .. src_col + 2, list order
    int src_n, src_ld, src_col;
    // this level's points as CENTRES of the finer level's grouping: - g_rel over the K samples of group q
    const int32_t *grp_pos;         // [B][n * K] slot of a grouped row, -1 = padding
    const float *grp_rows;
    int K, grp_n, grp_ld, grp_col;
    // this level's points as the FINE side of FP module `level`: d = square_distance(fine, coarse), dd/dfine = 2 (x1 - x2)
    const int32_t *nn_idx;          // [B][n][3]
    const float4 *fpg;              // [B][n] dL/dd of the three neighbours (fp_wgrad_kernel)
    const float *xyz;               // [B][n][3] this level
    const float *xyz_c;             // [B][n_c][3] the coarser level
    int n_c;
    // this level's points as the COARSE side of FP module `level - 1`: dd/dcoarse = -2 (x1 - x2), gathered through the
    // inverse 3-NN lists of the plan
    const int32_t *cinv_off;        // [B][n + 1]
    const int2 *cinv_ent;           // [B][3 n_f] {fine point, weight bits}
    const int32_t *f_nn_idx;        // [B][n_f][3]
    const float4 *f_fpg;            // [B][n_f]
    const float *xyz_f;             // [B][n_f][3]
    int n_f;
    float *out;                     // [B][n][out_ld], channels 0..2
    int out_ld, accumulate;         // accumulate: out += (level 0: onto the feature-path gradient of channels 0:3)
};

__global__ __launch_bounds__(GG_NT) void gx_level_kernel(GxArgs a, int B)
{
    const size_t total = (size_t)B * a.n;
    for (size_t t = (size_t)blockIdx.x * GG_NT + threadIdx.x; t < total; t += (size_t)gridDim.x * GG_NT) {
        const int b = (int)(t / a.n), q = (int)(t - (size_t)b * a.n);
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (a.src_off) {
            const int32_t *off = a.src_off + (size_t)b * (a.n + 1) + q;
            const float *rows = a.src_rows + (size_t)b * a.src_n * a.src_ld + a.src_col;
            const int e1 = min(off[1], a.src_n);
            for (int e = max(off[0], 0); e < e1; ++e) {
                const float *r = rows + (size_t)e * a.src_ld;
                gx += r[0]; gy += r[1]; gz += r[2];
            }
        }
        if (a.grp_pos) {
            const int32_t *pos = a.grp_pos + ((size_t)b * a.n + q) * a.K;
            const float *rows = a.grp_rows + (size_t)b * a.grp_n * a.grp_ld + a.grp_col;
            float sx = 0.f, sy = 0.f, sz = 0.f;
            for (int k = 0; k < a.K; ++k) {
                const int p = pos[k];
                if (p < 0 || p >= a.grp_n) continue;      // padding rows are not listed (their gradient is zero)
                const float *r = rows + (size_t)p * a.grp_ld;
                sx += r[0]; sy += r[1]; sz += r[2];
            }
            gx -= sx; gy -= sy; gz -= sz;
        }
        if (a.nn_idx) {
            const float *x1 = a.xyz + ((size_t)b * a.n + q) * 3;
            const float4 g = a.fpg[(size_t)b * a.n + q];
            const float gk[3] = {g.x, g.y, g.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int j = min(max(a.nn_idx[((size_t)b * a.n + q) * 3 + k], 0), a.n_c - 1);
                const float *x2 = a.xyz_c + ((size_t)b * a.n_c + j) * 3;
                gx += 2.0f * (x1[0] - x2[0]) * gk[k]; gy += 2.0f * (x1[1] - x2[1]) * gk[k]; gz += 2.0f * (x1[2] - x2[2]) * gk[k];
            }
        }
        if (a.cinv_off) {
            const int32_t *off = a.cinv_off + (size_t)b * (a.n + 1) + q;
            const int2 *ent = a.cinv_ent + (size_t)b * 3 * a.n_f;
            const float *x2 = a.xyz + ((size_t)b * a.n + q) * 3;
            const int e1 = min(off[1], 3 * a.n_f);
            for (int e = max(off[0], 0); e < e1; ++e) {
                const int i = min(max(ent[e].x, 0), a.n_f - 1);
                const int32_t *nn = a.f_nn_idx + ((size_t)b * a.n_f + i) * 3;
                const float4 g = a.f_fpg[(size_t)b * a.n_f + i];
                const float gk = nn[0] == q ? g.x : (nn[1] == q ? g.y : (nn[2] == q ? g.z : 0.f));   // (the three are distinct)
                const float *x1 = a.xyz_f + ((size_t)b * a.n_f + i) * 3;
                gx -= 2.0f * (x1[0] - x2[0]) * gk; gy -= 2.0f * (x1[1] - x2[1]) * gk; gz -= 2.0f * (x1[2] - x2[2]) * gk;
            }
        }
        float *o = a.out + ((size_t)b * a.n + q) * a.out_ld;
        if (a.accumulate) { o[0] += gx; o[1] += gy; o[2] += gz; }
        else { o[0] = gx; o[1] = gy; o[2] = gz; }
    }
}

// new_xyz = xyz[fps_idx] (pointnet_util.py:126): the coarser level's complete coordinate gradient is added to the rows of
// the points FPS chose.  FPS picks distinct points while the cloud has unpicked positions left; a cloud with fewer distinct
// positions than S (a block padded by sampling with replacement, at a level with S = N) makes it pick one index again and
// again, and the gather's transpose then SUMS those coarse rows.  One workgroup per room, the room's table in LDS: the
// first coarse point s that names a fine row p owns it and adds g[s], then g[s''] of every later s'' that names p, in
// ascending s'' - one writer per row and a fixed order, whatever the table; an injective table gives the single add.
constexpr int GX_FPS_MAX_S = 1024;
__global__ __launch_bounds__(GG_NT) void gx_fps_down_kernel(const float *__restrict__ g_coarse, const int32_t *__restrict__ fps,
                                                            int B, int S, int n_fine, float *__restrict__ out, int out_ld)
{
    __shared__ int32_t s_fps[GX_FPS_MAX_S];
    const int b = blockIdx.x;
    if (b >= B || S > GX_FPS_MAX_S) return;
    for (int s = threadIdx.x; s < S; s += GG_NT) s_fps[s] = fps[(size_t)b * S + s];
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += GG_NT) {
        const int p = s_fps[s];
        if (p < 0 || p >= n_fine) continue;
        bool owner = true;
        for (int j = 0; j < s; ++j)
            if (s_fps[j] == p) { owner = false; break; }
        if (!owner) continue;
        float *o = out + ((size_t)b * n_fine + p) * out_ld;
        const float *g = g_coarse + ((size_t)b * S + s) * 3;
        float ox = o[0] + g[0], oy = o[1] + g[1], oz = o[2] + g[2];
        for (int j = s + 1; j < S; ++j) {
            if (s_fps[j] != p) continue;
            const float *gj = g_coarse + ((size_t)b * S + j) * 3;
            ox += gj[0]; oy += gj[1]; oz += gj[2];
        }
        o[0] = ox; o[1] = oy; o[2] = oz;
    }
}

}  // namespace psg
