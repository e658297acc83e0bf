// NU attacks on the COORDINATE field of the PointNet++ SSG network; included by psg_attack.hip.
// An extension of the reference API (the reference ships the colour half only): delta [G][N][3] in metres is optimised
// directly by Adam - no tanh space, coordinates have no box -, xyz = ori_xyz + delta on masked points of active rooms.
// Rooms form only: G independent one-room attacks in lockstep.
//
// Three kernels and the step that strings them with the existing entry points:
//   smooth_knn_xyz_kernel      the Smooth term (nontarget.py:131-135) on channels 0:3 with DIRECT differences
//   nu_coord_apply_kernel      x0[.][0:3] = ori_xyz + delta
//   nu_coord_adam_kernel       gradient assembly + torch.optim.Adam on delta, per-room sum(delta^2)
//   psg_pn2_nu_field_step      apply, plan, forward, f-loss, full backward, Smooth term(s), Adam step(s), latch
// and, for the same attacks on ResGCN (the window that strings them is psg_gcn_nu_field_window in
// psg_resgcn.hip), at the end of the file:
//   smooth_xyz_sym_incoming_kernel   second pass of smooth(adv, adv) on coordinates (psg_smooth_knn_xyz_sym_rooms)
//   nu_coord_adam_w_kernel           the Adam step with separate Smooth / L2 weights and device-row step constants
#pragma once

namespace {

// Smooth term on coordinates.  smooth_knn_kernel evaluates |a|^2 + |r|^2 - 2 a.r like torch.cdist's matmul path, which is
// what the reference's colours in [0, 1] see; on coordinates in metres that expansion cancels to noise of the order of a
// millimetre - more than the perturbation, whose own distance |delta| is the dominant term.  Here
//   d^2 = fma(dz, dz, fma(dy, dy, dx * dx)),  dx = a.x - r.x, ..,  d = sqrt(d^2):
// one rounding per difference, three in the chain, one in the root, |d_fp32 - d| <= 4 * 2^-24 d.
// Structure of the colour kernel: the room's reference points in LDS as three planes split into SUB runs (run s holds the
// references s, s + SUB, ..), SUB lanes per query, each scanning its run with a sorted top-NBT in registers, then nb pops
// of the SUB-way merge by (distance, index), lower index first.  The scan compares d^2 against a bound that is never below
// the square of the distance bound (so it only admits more), the root is taken and compared exactly on the few
// candidates that pass.  One configuration serves every launch: SUB = 8, 128 queries per workgroup of 1024 threads.
constexpr int SMX_SUB = 8;
constexpr int SMX_T = 1024;
constexpr int SMX_REFRESH = 64;

template <int NBT>
__global__ __launch_bounds__(SMX_T) void smooth_knn_xyz_kernel(const float *__restrict__ adv, int adv_stride, size_t adv_room_stride,
                                                               const float *__restrict__ ref, int ref_stride, size_t ref_room_stride,
                                                               int N, int nb, float *__restrict__ dist_sum, float *__restrict__ grad,
                                                               const uint8_t *__restrict__ room_active, int32_t *__restrict__ nn_out)
{
    if (room_active && !room_active[blockIdx.y]) return;            // (uniform over the workgroup) an inactive room is untouched
    if (nn_out) nn_out += (size_t)blockIdx.y * N * nb;
    adv += blockIdx.y * adv_room_stride;
    ref += blockIdx.y * ref_room_stride;
    grad += (size_t)blockIdx.y * N * 3;
    if (dist_sum) dist_sum += blockIdx.y;
    constexpr int QPB = SMX_T / SMX_SUB;
    const int tps = ((N + SMX_SUB - 1) / SMX_SUB + 3) & ~3, run = tps + 8;
    extern __shared__ float s_xyz[];
    float *s_x = s_xyz, *s_y = s_xyz + SMX_SUB * run, *s_z = s_xyz + 2 * SMX_SUB * run;
    for (int p = threadIdx.x; p < SMX_SUB * tps; p += SMX_T) {
        const int sr = p / tps, t = p - sr * tps, i = sr + SMX_SUB * t;
        // slots past N: every difference is -inf, d^2 = +inf, and +inf passes no bound
        float x = INFINITY, y = INFINITY, z = INFINITY;
        if (i < N) { x = ref[(size_t)i * ref_stride]; y = ref[(size_t)i * ref_stride + 1]; z = ref[(size_t)i * ref_stride + 2]; }
        s_x[sr * run + t] = x; s_y[sr * run + t] = y; s_z[sr * run + t] = z;
    }
    __syncthreads();
    const int ql = threadIdx.x / SMX_SUB, sub = threadIdx.x % SMX_SUB;
    const int i = blockIdx.x * QPB + ql;
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (i < N) { ax = adv[(size_t)i * adv_stride]; ay = adv[(size_t)i * adv_stride + 1]; az = adv[(size_t)i * adv_stride + 2]; }
    float bd[NBT];
    int bi[NBT];
#pragma unroll
    for (int t = 0; t < NBT; ++t) { bd[t] = INFINITY; bi[t] = 0x7FFFFFFF; }
    // thr (a distance): a candidate is wanted only below min(this lane's worst kept distance, the nb-th smallest distance
    // the query's lanes hold together at the last refresh) - exact for the reason given in smooth_knn_kernel: what is
    // kept has a lower index than anything scanned later, so a later candidate AT the bound loses the tie.
    // thr2 >= thr^2 (a few ulps up, and never 0): sqrt(d2) rounded < thr implies d2 < thr^2 <= thr2.
    float thr = i < N ? INFINITY : -INFINITY, thr2 = thr;
    const sm_v2f ax2 = {ax, ax}, ay2 = {ay, ay}, az2 = {az, az};
    const float *px = s_x + sub * run, *py = s_y + sub * run, *pz = s_z + sub * run;
    for (int t0 = 0; t0 < tps; t0 += SMX_REFRESH) {
        const int t1 = t0 + SMX_REFRESH < tps ? t0 + SMX_REFRESH : tps;
        for (int t = t0; t < t1; t += 4) {
            const float4 X = *(const float4 *)(px + t), Y = *(const float4 *)(py + t), Z = *(const float4 *)(pz + t);
            // two references per instruction; per component exactly fma(dz, dz, fma(dy, dy, dx * dx)) on rounded differences
            const sm_v2f dxa = ax2 - sm_v2f{X.x, X.y}, dxb = ax2 - sm_v2f{X.z, X.w};
            const sm_v2f dya = ay2 - sm_v2f{Y.x, Y.y}, dyb = ay2 - sm_v2f{Y.z, Y.w};
            const sm_v2f dza = az2 - sm_v2f{Z.x, Z.y}, dzb = az2 - sm_v2f{Z.z, Z.w};
            sm_v2f da = dxa * dxa, db = dxb * dxb;
            da = __builtin_elementwise_fma(dya, dya, da); db = __builtin_elementwise_fma(dyb, dyb, db);
            da = __builtin_elementwise_fma(dza, dza, da); db = __builtin_elementwise_fma(dzb, dzb, db);
            const float d2[4] = {da[0], da[1], db[0], db[1]};
            if (fminf(fminf(d2[0], d2[1]), fminf(d2[2], d2[3])) < thr2) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d2[u] < thr2) {
                        float cd = sqrtf(d2[u]);
                        if (cd < thr) {
                            int ci = sub + SMX_SUB * (t + u);
#pragma unroll
                            for (int k = 0; k < NBT; ++k) {   // sorted insertion with static indexing (arrays stay in registers)
                                if (cd < bd[k]) {
                                    float td = bd[k]; int ti = bi[k];
                                    bd[k] = cd; bi[k] = ci;
                                    cd = td; ci = ti;
                                }
                            }
                            thr = fminf(thr, bd[NBT - 1]);
                            thr2 = __fadd_rn(__fmul_rn(__fmul_rn(thr, thr), 1.000001f), 1e-30f);
                        }
                    }
                }
            }
        }
        if (t1 < tps) {   // another chunk follows (uniform over the workgroup)
            float cdist[NBT];
            int cidx[NBT];
#pragma unroll
            for (int t = 0; t < NBT; ++t) { cdist[t] = bd[t]; cidx[t] = bi[t]; }
            float kth = INFINITY;
            int kidx;
            for (int t = 0; t < nb; ++t) smooth_pop_min<NBT, SMX_SUB>(cdist, cidx, kth, kidx);
            if (kth < thr) {
                thr = kth;
                thr2 = __fadd_rn(__fmul_rn(__fmul_rn(thr, thr), 1.000001f), 1e-30f);
            }
        }
    }
    // SUB-way merge: nb times the smallest head by (distance, index); the gradient adds up in ascending rank order
    float local = 0.0f, gx = 0.f, gy = 0.f, gz = 0.f;
    for (int t = 0; t < nb; ++t) {
        float best;
        int bidx;
        smooth_pop_min<NBT, SMX_SUB>(bd, bi, best, bidx);
        if (bidx == 0x7FFFFFFF) break;   // fewer than nb references (uniform over the query's lanes)
        if (sub == 0 && i < N) {
            if (nn_out) nn_out[(size_t)i * nb + t] = bidx;
            local += best;
            if (best > 0.0f) {           // a neighbour at distance 0 (the point's own original before it moved) adds exactly 0
                const int pos = (bidx % SMX_SUB) * run + bidx / SMX_SUB;
                gx += __fdiv_rn(__fsub_rn(ax, s_x[pos]), best);
                gy += __fdiv_rn(__fsub_rn(ay, s_y[pos]), best);
                gz += __fdiv_rn(__fsub_rn(az, s_z[pos]), best);
            }
        }
    }
    if (sub == 0 && i < N) { grad[(size_t)i * 3] = gx; grad[(size_t)i * 3 + 1] = gy; grad[(size_t)i * 3 + 2] = gz; }
    for (int o = 32; o >= 1; o >>= 1) local += __shfl_xor(local, o);
    if ((threadIdx.x & 63) == 0 && dist_sum) atomicAdd(dist_sum, local);
}

// x0[b][i][0:3] = ori_xyz + delta on masked points of active rooms; every other byte of x0 stays
__global__ void nu_coord_apply_kernel(const float *__restrict__ delta, const float *__restrict__ ori_xyz, const uint8_t *__restrict__ mask,
                                      const uint8_t *__restrict__ room_active, float *__restrict__ x0, int N)
{
    const size_t y = blockIdx.y;
    if (room_active && !room_active[y]) return;
    const size_t o3 = y * (size_t)N * 3;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < (size_t)N * 3; t += (size_t)gridDim.x * blockDim.x) {
        const size_t pt = t / 3;
        if (mask && !mask[y * N + pt]) continue;
        x0[(y * N + pt) * 9 + t % 3] = __fadd_rn(ori_xyz[o3 + t], delta[o3 + t]);
    }
}

// g = dx0[0:3] + 2 coord_c delta + coord_c sgrad_xyz, then torch.optim.Adam's single-tensor update of delta / m / v
// (the operation order of nu_adam_step_kernel), on masked points of active rooms; sum(delta^2) of the delta the step
// STARTED from is added to the room's L2 slot (one atomic per workgroup).
__global__ __launch_bounds__(256) void nu_coord_adam_kernel(float *__restrict__ delta, float *__restrict__ m, float *__restrict__ v,
                                                             const uint8_t *__restrict__ mask, const float *__restrict__ dx0,
                                                             const float *__restrict__ sgrad, float coord_c, float beta1, float beta2,
                                                             float eps, float step_size, float bc2_sqrt, int N,
                                                             const uint8_t *__restrict__ room_active, float *__restrict__ l2_sum)
{
    const size_t y = blockIdx.y;
    if (room_active && !room_active[y]) return;
    const size_t o3 = y * (size_t)N * 3;
    float l2 = 0.0f;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < (size_t)N * 3; t += (size_t)gridDim.x * blockDim.x) {
        const size_t pt = t / 3;
        if (mask && !mask[y * N + pt]) continue;
        const float d = delta[o3 + t];
        l2 += d * d;
        float g = dx0[(y * N + pt) * 9 + t % 3] + coord_c * 2.0f * d;
        if (sgrad) g += coord_c * sgrad[o3 + t];
        delta[o3 + t] = psg::adam_update(d, m[o3 + t], v[o3 + t], g, beta1, beta2, eps, step_size, bc2_sqrt);
    }
    for (int o = 32; o >= 1; o >>= 1) l2 += __shfl_xor(l2, o);
    if (!l2_sum) return;
    __shared__ float s_l2[4];
    if ((threadIdx.x & 63) == 0) s_l2[threadIdx.x >> 6] = l2;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(l2_sum + y, (s_l2[0] + s_l2[1]) + (s_l2[2] + s_l2[3]));
}

// the step's Smooth_xyz / L2_xyz sums (scal rows 3, 4) into rows 5, 6 of the history row, zeroed for the next step - what
// the latch does for rows 0..2
__global__ void nu_field_hist_tail_kernel(float *__restrict__ scal, float *__restrict__ hist_step, int G)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * G) return;
    hist_step[5 * G + t] = scal[3 * G + t];
    scal[3 * G + t] = 0.0f;
}

}  // namespace

extern "C" int psg_smooth_knn_xyz_rooms(const float *adv_xyz, int adv_stride, size_t adv_room_stride, const float *ref_xyz,
                                        int ref_stride, size_t ref_room_stride, int B, int N, int nb, float *dist_sum_rooms,
                                        float *grad_out, const uint8_t *room_active, int32_t *nn_out, psg_stream stream)
{
    PSG_REQUIRE(adv_xyz && ref_xyz && grad_out && adv_xyz != ref_xyz && N > 0 && B > 0 && B <= 65535 && adv_stride >= 3 && ref_stride >= 3,
                "psg_smooth_knn_xyz_rooms: bad argument");
    PSG_REQUIRE(nb > 0 && nb <= SM_MAX_NB, "psg_smooth_knn_xyz_rooms: neighbour count %d out of range (1..%d)", nb, SM_MAX_NB);
    PSG_REQUIRE(N <= 8192, "psg_smooth_knn_xyz_rooms: N=%d exceeds the LDS-resident limit 8192", N);
    const size_t lds = (size_t)3 * SMX_SUB * ((((N + SMX_SUB - 1) / SMX_SUB + 3) & ~3) + 8) * sizeof(float);
    const dim3 grid(psg::ceil_div(N, SMX_T / SMX_SUB), B);
#define PSG_SMOOTH_XYZ_LAUNCH(NBT)                                                                                               \
    do {                                                                                                                         \
        if (lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)smooth_knn_xyz_kernel<NBT>));                        \
        hipLaunchKernelGGL((smooth_knn_xyz_kernel<NBT>), grid, dim3(SMX_T), lds, (hipStream_t)stream, adv_xyz, adv_stride,       \
                           adv_room_stride, ref_xyz, ref_stride, ref_room_stride, N, nb, dist_sum_rooms, grad_out, room_active,  \
                           nn_out);                                                                                              \
    } while (0)
    // list length per lane: the two neighbour counts the attacks use (tar_NU 5, NU 10), else 16
    if (nb <= 5) PSG_SMOOTH_XYZ_LAUNCH(5);
    else if (nb <= 10) PSG_SMOOTH_XYZ_LAUNCH(10);
    else PSG_SMOOTH_XYZ_LAUNCH(16);
#undef PSG_SMOOTH_XYZ_LAUNCH
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_nu_coord_apply_rooms(const float *delta, const float *ori_xyz, const uint8_t *mask_rooms, int B, int N,
                                        const uint8_t *room_active, float *x0, psg_stream stream)
{
    PSG_REQUIRE(delta && ori_xyz && x0 && B > 0 && B <= 65535 && N > 0, "psg_nu_coord_apply_rooms: bad argument");
    hipLaunchKernelGGL(nu_coord_apply_kernel, dim3(std::min(grid_for((size_t)N * 3), 12), B), dim3(256), 0, (hipStream_t)stream, delta,
                       ori_xyz, mask_rooms, room_active, x0, N);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_nu_coord_adam_step_rooms(float *delta, float *m, float *v, const uint8_t *mask_rooms, const float *dx0,
                                            const float *sgrad_xyz, float coord_c, float coord_lr, float beta1, float beta2, float eps,
                                            int step, int B, int N, const uint8_t *room_active, float *l2_sum_rooms, psg_stream stream)
{
    PSG_REQUIRE(delta && m && v && dx0 && B > 0 && B <= 65535 && N > 0 && step >= 1, "psg_nu_coord_adam_step_rooms: bad argument");
    const psg::AdamConsts k = psg::adam_consts(coord_lr, beta1, beta2, step);
    hipLaunchKernelGGL(nu_coord_adam_kernel, dim3(std::min(grid_for((size_t)N * 3), 12), B), dim3(256), 0, (hipStream_t)stream, delta, m, v,
                       mask_rooms, dx0, sgrad_xyz, coord_c, beta1, beta2, eps, k.step_size, k.bc2_sqrt, N, room_active, l2_sum_rooms);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// One whole step of the coordinate-field NU attacks, enqueued on the caller's stream (no graph: the plan is rebuilt from the
// moved points every step, and its FPS starts change with it).
extern "C" int psg_pn2_nu_field_step(const psg_nu_field_args *a, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->delta && a->m_xyz && a->v_xyz && a->ori_xyz && a->x0 && a->labels && a->starts && a->logp &&
                    a->dlogp && a->dx0 && a->sgrad_xyz && a->pred && a->scal && a->hist && a->out && a->active && a->exit_step,
                "psg_pn2_nu_field_step: null argument");
    PSG_REQUIRE(a->field == PSG_NU_FIELD_COORD || a->field == PSG_NU_FIELD_BOTH, "psg_pn2_nu_field_step: field %d is neither coord (%d) nor both (%d)",
                a->field, PSG_NU_FIELD_COORD, PSG_NU_FIELD_BOTH);
    const bool both = a->field == PSG_NU_FIELD_BOTH;
    PSG_REQUIRE(!both || (a->w && a->m && a->v && a->ori && a->sgrad && a->nn_state), "psg_pn2_nu_field_step: field both needs the colour state");
    PSG_REQUIRE(a->G > 0 && a->N > 0 && a->adam_t >= 1 && a->step >= 0, "psg_pn2_nu_field_step: G=%d N=%d adam_t=%d step=%d out of range", a->G,
                a->N, a->adam_t, a->step);
    PSG_REQUIRE(a->mode >= 0 && a->mode <= 2 && (a->mode == 0 || (a->mask && a->n_mask)), "psg_pn2_nu_field_step: modes 1 and 2 need mask and n_mask");
    if (int rc = psg::pn2_full_grad_check(a->model, a->ws, "psg_pn2_nu_field_step")) return rc;
    const int G = a->G, N = a->N;
    const int32_t *f_labels = a->use_target ? nullptr : a->labels;
    const int f_target = a->use_target ? a->target : 0;
    int rc;
    if ((rc = psg_nu_coord_apply_rooms(a->delta, a->ori_xyz, a->mask, G, N, a->active, a->x0, stream))) return rc;
    if (both && (rc = psg_nu_tanh_color_rooms(a->w, a->mask, G, N, a->x0, stream))) return rc;
    if ((rc = psg_pn2_plan_build(a->ws, a->x0, a->starts, 1, stream))) return rc;
    if ((rc = psg_pn2_forward(a->model, a->ws, 0, a->x0, a->logp, nullptr, stream))) return rc;
    if ((rc = psg_nu_f_loss_grad_rooms(a->logp, f_labels, f_target, G, N, PSG_PN2_NUM_CLASSES, a->kappa, a->tsign, a->dlogp, a->scal, a->pred,
                                       stream)))
        return rc;
    if ((rc = psg_pn2_backward_full(a->model, a->ws, 0, a->dlogp, a->dx0, stream))) return rc;
    if (both) {
        if ((rc = psg_smooth_knn_rooms(a->x0 + 3, 9, (size_t)N * 9, a->ori, 3, (size_t)N * 3, G, N, a->neighbour, a->scal + G, a->sgrad,
                                       a->nn_state, a->warm ? 1 : 0, stream)))
            return rc;
    }
    if ((rc = psg_smooth_knn_xyz_rooms(a->x0, 9, (size_t)N * 9, a->ori_xyz, 3, (size_t)N * 3, G, N, a->neighbour, a->scal + 3 * G, a->sgrad_xyz,
                                       a->active, nullptr, stream)))
        return rc;
    // (no step-constants row: this step is never captured, its kernels take the constants from their arguments)
    if (both && (rc = psg::nu_colour_adam(a, a->c, a->c, 1, a->adam_t, stream))) return rc;
    if ((rc = psg_nu_coord_adam_step_rooms(a->delta, a->m_xyz, a->v_xyz, a->mask, a->dx0, a->sgrad_xyz, a->coord_c, a->coord_lr, a->beta1,
                                           a->beta2, a->eps, a->adam_t, G, N, a->active, a->scal + 4 * G, stream)))
        return rc;
    if ((rc = psg::nu_latch(a, 1, a->hist, a->step, stream))) return rc;
    hipLaunchKernelGGL(nu_field_hist_tail_kernel, dim3(psg::ceil_div(2 * G, 256)), dim3(256), 0, (hipStream_t)stream, a->scal, a->hist, G);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

namespace {

// ---- smooth(adv, adv) on COORDINATES for G rooms in lockstep (psg_smooth_knn_xyz_sym_rooms; the ResGCN Smooth of
// colper.py:115-120 / tcolper.py:165-170 on channels 0:3).  The two-launch scheme of
// psg_smooth_knn_sym_rooms on direct differences:
//   1. smooth_knn_xyz_kernel with the room's own points as references, one-sided: grad[i] = sum over i's neighbours in
//      ascending rank of u(i, j) = (a_i - a_j) / d(i, j), the lists to nn, the distances to the room's sum.
//   2. smooth_xyz_sym_incoming_kernel: grad[i] -= u(k, i) for every k that holds i among its neighbours, in ascending k.
// Point i is a neighbour of k exactly when (d(k, i), i) <= (d(k, j*), j*) for k's LAST neighbour j*: pass 1 selects by the
// total order (distance, index) on d = sqrtf(fma(dz, dz, fma(dy, dy, dx * dx))), so the membership test compares THAT d,
// never d^2 (two different d^2 can round to one d, and the index then decides).  The direct-difference distance is
// BIT-SYMMETRIC in its two points - a - b and b - a differ in sign only, the squares and everything after them are the same
// operations on the same values - so d(k, i) evaluated here with k in the query's role is the d(i, k) any other evaluation
// gives; the colour kernel's expansion is not, which is why it re-evaluates in pass 1's orientation.
// Every workgroup stages each k's point with a pre-test bound and k's key (one gather per k) in 24-byte LDS slots, 2048 k at
// a time; a point's 16 lanes walk the k in ascending order 16 at a time.  The pre-test is pass 1's: d^2 against a bound a
// few ulps above key^2 (it only admits more), the root is taken and compared exactly on what passes.
constexpr int SXI_T = 1024;                 // threads of the second pass
constexpr int SXI_SUB = 16;                 // lanes per point
constexpr int SXI_TILE = 2048;              // k staged at a time: 2048 x (16 + 8) bytes = 48 KB

__global__ __launch_bounds__(SXI_T) void smooth_xyz_sym_incoming_kernel(const float *__restrict__ adv, int adv_stride, size_t adv_room_stride,
                                                                        int N, int nb, const int32_t *__restrict__ nn,
                                                                        float *__restrict__ grad, const uint8_t *__restrict__ room_active)
{
    if (room_active && !room_active[blockIdx.y]) return;
    adv += blockIdx.y * adv_room_stride;
    nn += (size_t)blockIdx.y * N * nb;
    grad += (size_t)blockIdx.y * N * 3;
    __shared__ float4 s_k[SXI_TILE];        // {x, y, z of point k, bound on d^2 (-1: no such k)}
    __shared__ float2 s_key[SXI_TILE];      // k's last neighbour: {d(k, j*), index bits}
    const int sub = threadIdx.x % SXI_SUB;
    const int i = blockIdx.x * (SXI_T / SXI_SUB) + threadIdx.x / SXI_SUB;
    const int last = (nb < N ? nb : N) - 1;                     // rank of the last neighbour every point actually holds
    float rx = 0.f, ry = 0.f, rz = 0.f;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (i < N) {
        rx = adv[(size_t)i * adv_stride]; ry = adv[(size_t)i * adv_stride + 1]; rz = adv[(size_t)i * adv_stride + 2];
        gx = grad[(size_t)i * 3]; gy = grad[(size_t)i * 3 + 1]; gz = grad[(size_t)i * 3 + 2];   // own terms (pass 1)
    }
    for (int k0 = 0; k0 < N; k0 += SXI_TILE) {
        if (k0) __syncthreads();
        for (int t = threadIdx.x; t < SXI_TILE; t += SXI_T) {
            const int k = k0 + t;
            float4 q = {0.f, 0.f, 0.f, -1.0f};
            float2 key = {-1.0f, 0.0f};
            if (k < N) {
                q.x = adv[(size_t)k * adv_stride]; q.y = adv[(size_t)k * adv_stride + 1]; q.z = adv[(size_t)k * adv_stride + 2];
                const int j = nn[(size_t)k * nb + last];
                if (j >= 0 && j < N) {
                    const float dx = __fsub_rn(q.x, adv[(size_t)j * adv_stride]), dy = __fsub_rn(q.y, adv[(size_t)j * adv_stride + 1]),
                                dz = __fsub_rn(q.z, adv[(size_t)j * adv_stride + 2]);
                    const float d = sqrtf(__fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx))));
                    key = float2{d, __int_as_float(j)};
                    // sqrt(d2) rounded <= d implies d2 <= d^2 (1 + 3 ulp) < the bound; a NaN / inf key admits nothing
                    q.w = d < INFINITY ? __fadd_rn(__fmul_rn(__fmul_rn(d, d), 1.000001f), 1e-30f) : -1.0f;
                }
            }
            s_k[t] = q;
            s_key[t] = key;
        }
        __syncthreads();
        const int nt = min(SXI_TILE, N - k0);
        for (int t = sub; t < nt + sub; t += SXI_SUB) {         // (the 16 lanes of a point stay together: t - sub < nt)
            const bool in = t < nt && i < N;
            const float4 q = s_k[in ? t : 0];
            const float dx = __fsub_rn(q.x, rx), dy = __fsub_rn(q.y, ry), dz = __fsub_rn(q.z, rz);   // k in the query's role
            const float d2 = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
            const bool cand = in && d2 <= q.w;
            if (__ballot(cand) == 0ull) continue;               // (uniform over the wave)
            bool hit = false;
            float ux = 0.f, uy = 0.f, uz = 0.f;
            if (cand) {
                const float2 key = s_key[t];
                const float d = sqrtf(d2);
                hit = d < key.x || (d == key.x && i <= __float_as_int(key.y));
                if (hit && d > 0.0f) { ux = __fdiv_rn(dx, d); uy = __fdiv_rn(dy, d); uz = __fdiv_rn(dz, d); }
            }
            const unsigned long long bal = __ballot(hit);
            // the hits of this point's 16 lanes, in lane (= ascending k) order; the lanes of a point see the same bits
            unsigned mine = (unsigned)(bal >> (threadIdx.x & 48)) & 0xFFFFu;
            while (mine) {
                const int s = __ffs(mine) - 1;
                mine &= mine - 1;
                gx -= __shfl(ux, s, SXI_SUB); gy -= __shfl(uy, s, SXI_SUB); gz -= __shfl(uz, s, SXI_SUB);
            }
        }
    }
    if (sub == 0 && i < N) { grad[(size_t)i * 3] = gx; grad[(size_t)i * 3 + 1] = gy; grad[(size_t)i * 3 + 2] = gz; }
}

// nu_coord_adam_kernel with separate weights of the Smooth and the L2 term, g = dx0[0:3] + 2 c_l2 delta + c_smooth sgrad_xyz,
// and - inside a window that is (or will be) replayed - the step constants from the window's device row: slot 3 carries
// coord_lr / (1 - beta1^t) (slot 1 is the colour variable's, field "both" runs two learning rates), slot 2 sqrt(1 - beta2^t).
__global__ __launch_bounds__(256) void nu_coord_adam_w_kernel(float *__restrict__ delta, float *__restrict__ m, float *__restrict__ v,
                                                               const uint8_t *__restrict__ mask, const float *__restrict__ dx0,
                                                               const float *__restrict__ sgrad, float c_smooth, float c_l2, float beta1,
                                                               float beta2, float eps, float step_size, float bc2_sqrt, int N,
                                                               const uint8_t *__restrict__ room_active, float *__restrict__ l2_sum,
                                                               const float *__restrict__ dconsts)
{
    if (dconsts) { step_size = dconsts[3]; bc2_sqrt = dconsts[2]; }
    const size_t y = blockIdx.y;
    if (room_active && !room_active[y]) return;
    const size_t o3 = y * (size_t)N * 3;
    float l2 = 0.0f;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < (size_t)N * 3; t += (size_t)gridDim.x * blockDim.x) {
        const size_t pt = t / 3;
        if (mask && !mask[y * N + pt]) continue;
        const float d = delta[o3 + t];
        l2 += d * d;
        float g = dx0[(y * N + pt) * 9 + t % 3] + c_l2 * 2.0f * d;
        if (sgrad) g += c_smooth * sgrad[o3 + t];
        delta[o3 + t] = psg::adam_update(d, m[o3 + t], v[o3 + t], g, beta1, beta2, eps, step_size, bc2_sqrt);
    }
    for (int o = 32; o >= 1; o >>= 1) l2 += __shfl_xor(l2, o);
    if (!l2_sum) return;
    __shared__ float s_l2[4];
    if ((threadIdx.x & 63) == 0) s_l2[threadIdx.x >> 6] = l2;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(l2_sum + y, (s_l2[0] + s_l2[1]) + (s_l2[2] + s_l2[3]));
}

}  // namespace

// smooth(adv, adv) on coordinates without float atomics on the gradient: see smooth_xyz_sym_incoming_kernel.  The lists the
// second pass reads go to nn_out, or - the caller wants none - to a scratch buffer this host thread keeps and grows (never
// inside a stream capture: the NU windows always pass their lists).
extern "C" int psg_smooth_knn_xyz_sym_rooms(const float *adv_xyz, int adv_stride, size_t adv_room_stride, int G, int N, int nb,
                                            float *dist_sum_rooms, float *grad_out, const uint8_t *room_active, int32_t *nn_out,
                                            psg_stream stream)
{
    PSG_REQUIRE(adv_xyz && grad_out && dist_sum_rooms && N > 0 && G > 0 && G <= 65535 && adv_stride >= 3,
                "psg_smooth_knn_xyz_sym_rooms: bad argument");
    PSG_REQUIRE(nb > 0 && nb <= SM_MAX_NB, "psg_smooth_knn_xyz_sym_rooms: neighbour count %d out of range (1..%d)", nb, SM_MAX_NB);
    PSG_REQUIRE(N <= 8192, "psg_smooth_knn_xyz_sym_rooms: N=%d exceeds the LDS-resident limit 8192", N);
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
    const size_t lds = (size_t)3 * SMX_SUB * ((((N + SMX_SUB - 1) / SMX_SUB + 3) & ~3) + 8) * sizeof(float);
    const dim3 grid(psg::ceil_div(N, SMX_T / SMX_SUB), G);
#define PSG_SMOOTH_XYZ_SYM_LAUNCH(NBT)                                                                                           \
    do {                                                                                                                         \
        if (lds > 48 * 1024) PSG_CHECK_HIP(psg::allow_big_lds((const void *)smooth_knn_xyz_kernel<NBT>));                        \
        hipLaunchKernelGGL((smooth_knn_xyz_kernel<NBT>), grid, dim3(SMX_T), lds, st, adv_xyz, adv_stride, adv_room_stride,       \
                           adv_xyz, adv_stride, adv_room_stride, N, nb, dist_sum_rooms, grad_out, room_active, nn_out);          \
    } while (0)
    if (nb <= 5) PSG_SMOOTH_XYZ_SYM_LAUNCH(5);
    else if (nb <= 10) PSG_SMOOTH_XYZ_SYM_LAUNCH(10);
    else PSG_SMOOTH_XYZ_SYM_LAUNCH(16);
#undef PSG_SMOOTH_XYZ_SYM_LAUNCH
    PSG_LAUNCH_CHECK();
    hipLaunchKernelGGL(smooth_xyz_sym_incoming_kernel, dim3(psg::ceil_div(N, SXI_T / SXI_SUB), G), dim3(SXI_T), 0, st, adv_xyz, adv_stride,
                       adv_room_stride, N, nb, nn_out, grad_out, room_active);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

extern "C" int psg_nu_coord_adam_step_rooms_w(float *delta, float *m, float *v, const uint8_t *mask_rooms, const float *dx0,
                                              const float *sgrad_xyz, float c_smooth, float c_l2, float coord_lr, float beta1, float beta2,
                                              float eps, int step, int B, int N, const uint8_t *room_active, float *l2_sum_rooms,
                                              psg_stream stream)
{
    PSG_REQUIRE(delta && m && v && dx0 && B > 0 && B <= 65535 && N > 0 && step >= 1, "psg_nu_coord_adam_step_rooms_w: bad argument");
    const psg::AdamConsts k = psg::adam_consts(coord_lr, beta1, beta2, step);
    hipLaunchKernelGGL(nu_coord_adam_w_kernel, dim3(std::min(grid_for((size_t)N * 3), 12), B), dim3(256), 0, (hipStream_t)stream, delta, m, v,
                       mask_rooms, dx0, sgrad_xyz, c_smooth, c_l2, beta1, beta2, eps, k.step_size, k.bc2_sqrt, N, room_active, l2_sum_rooms,
                       g_nu_dconsts);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}

// the step's Smooth_xyz / L2_xyz sums (scal rows 3, 4) into rows 5, 6 of the history row hist_step [7][G], zeroed for the
// next step (psg_gcn_nu_field_window; psg_pn2_nu_field_step launches the kernel itself)
int psg::nu_field_hist_tail(float *scal, float *hist_step, int G, hipStream_t st)
{
    hipLaunchKernelGGL(nu_field_hist_tail_kernel, dim3(psg::ceil_div(2 * G, 256)), dim3(256), 0, st, scal, hist_step, G);
    PSG_LAUNCH_CHECK();
    return PSG_OK;
}
