// Fused set-abstraction / feature-propagation kernels (forward and input-gradient backward) for
// PointNet++ SSG on gfx950.  One workgroup owns P points (P/32 ball-query groups for SA); the whole
// MLP chain of the module runs out of LDS, only module inputs/outputs, ReLU bit-masks and max-pool
// arg-indices touch HBM.
//
// Reference semantics (paths relative to /root/reference):
//   SA  forward  PointNet/models/pointnet_util.py:126-140 (gather, grouped_xyz - new_xyz, concat
//                [rel_xyz, feats]) + :200-205 (3 x conv1x1+BN+ReLU, max over the 32 samples)
//   FP  forward  pointnet_util.py:308-319 (3-NN weighted sum, concat [points1, interp], conv1x1+BN+ReLU)
//   head         PointNet/models/pointnet2_sem_seg.py:36-38 (conv1+bn1+ReLU, conv2, log_softmax)
//   backward     what autograd derives for d/d(input features); geometry is constant w.r.t. colour.
#pragma once
#include "psg_ce_row.cuh"
#include "psg_mlp.cuh"

// Timing-diagnosis switches (tools/diag_*.sh: skip a kernel section to see what it costs; the results are then wrong).
// They exist ONLY in a diagnostic build (make EXTRA=-DPSG_DIAG_BUILD): in the default library every test below is the
// constant 0, the compiler removes the branches, and no environment variable can make a kernel skip its work.
#ifdef PSG_DIAG_BUILD
#define PSG_DIAGBIT(a, bit) ((a).diag & (bit))
#else
#define PSG_DIAGBIT(a, bit) 0
#endif

namespace psg {

struct SaFwdArgs {
    const float *xyz;      // [B][Np][xyz_stride], first 3 floats of a row = xyz
    const float *feat;     // [B][Np][D]
    const float *new_xyz;  // [B][S][3]
    const int32_t *gidx;   // [B][S][KS]
    float *out;            // [B][S][ld_out], this module's C3 channels at column c_out (MSG scales share a row)
    uint8_t *arg;          // [B][S][C3] arg-max sample, 255 = no gradient (max <= 0)
    FwdLayer l1, l2;
    const float4 *w3;      // last layer, packed like FwdLayer::w, used as the B operand (flipped tile)
    const float *b3;
    int k8_3, nb3;
    int xyz_stride, D, Np, S, C3;
    int ld_out, c_out;
    // SPLIT kernels (see sa_fwd_kernel): per-point first-layer products T = feats . W1f^T + b1, rows [B][Np][ldt]; l1 then
    // holds the xyz columns of the first layer only (k8 = 1)
    const float *tfeat;
    int ldt;
    int diag;              // timing diagnostics only (-DPSG_DIAG_BUILD libraries only): skip sections, results are then wrong
    // packed kernels (sa_fwd_packed_kernel): the plan's workgroup descriptors (sa_pack_plan_kernel) and the float offset of the
    // workgroup's row maps behind the LDS activation buffer
    const int4 *pk_desc;   // [B][gridDim.x] one descriptor per workgroup (below)
    int pk_tab_off;
};

struct SaBwdArgs {
    // The pooled-output gradient of this module is columns [c_off, c_off + C3) of rows of `ld` floats (ld = all
    // channels of the level: an MSG level concatenates its scales); dout, dint and gsa rows all have that stride.
    const float *dout;    // [B][S][ld] (direct), or null when the gradient is gathered through nninv_*
    // gather form: dout[s][c] = sum over the fine points p whose 3-NN lists contain s of w * dint[p][c]
    const int32_t *nninv_off;   // [B][S+1]
    const int2 *nninv_ent;      // [B][3*n_fine] {fine point, weight bits}, sorted by fine point per list
    const float *dint;          // [B][n_fine][C3]
    int n_fine;
    // grouping-transpose form: dout[s][c] += sum over the grouped rows e of the next SA level that gathered point s
    const int32_t *ginv_off;    // [B][S+1] or null: list of point s = rows [off[s], off[s+1]) of gsa
    const float *gsa;           // [B][g_rows][ld] gradient rows written by the next level's sa_bwd IN LIST ORDER
    int g_rows;
    const int32_t *ginv_off2;   // second scale of the next level (MSG), or null
    const float *gsa2;
    int g_rows2;
    int ld, c_off;
    float *gsa_out;             // [B][S*KS][cg_out]: this module's grouped-input gradient rows (plain stores), row
    const int32_t *gpos_out;    // (group*KS + sample) stored at position gpos_out[row] = its slot in the consumer's lists
    int cg_out;
    const uint8_t *arg;   // [B][S][C3]
    const int32_t *gidx;  // [B][S][KS]
    BwdLayer l3t, l2t, l1t;
    int D, Np, S, C3;
    int c_lo, c_hi;       // feature channels [c_lo, c_hi) of the grouped-input gradient are scattered
    int split;            // 1: the rows stored are dZ1 (the first layer's pre-activation gradient, channels [c_lo, c_hi) =
                          // [0, C1)), the first layer's transpose is NOT applied here (pw_bwd_kernel applies it per POINT)
    int dsrc_blk;         // LDS block where the gathered pooled-output gradient is staged
    // colour-only request at level 0 (the attack loop): the first layer's feature columns, plain rows [C1][D] (w1c; null: the
    // transposed layer runs on the matrix pipe as everywhere else); the three wanted columns are staged behind dsrc
    const float *w1c;
    int C1, w1c_off;      // first layer's width (16 or 32); float offset of the LDS copy from the start of the staging block
    int pos_off;          // float offset (staging block) of the LDS copy of the workgroup's P output slots
    // sparse max-pool transpose (sa_pool_t_sparse; kernels with SPV > 0 only): the third layer's weights as plain rows [C3][C2],
    // and the float offset (staging block) of the item list, its per-chunk offset table and the row starts
    const float *w3r;
    int sp_off;
    int diag;             // timing diagnostics only (-DPSG_DIAG_BUILD libraries only)
};

// sa_bwd_packed_kernel: the above (its row map [P] lies behind the P output slots at pos_off) and the workgroup descriptors the
// packed forward of the level ran on
struct SaBwdPackedArgs {
    SaBwdArgs a;
    const int4 *pk_desc;  // [B][gridDim.x]
};

struct FpFwdArgs {
    const float *feat1;     // skip features [B][N][C1] or null
    const float *feat2;     // coarse features [B][S][C2]
    const int32_t *nn_idx;  // [B][N][3]
    const float *nn_w;      // [B][N][3]
    float *out;             // [B][N][Cout] or null
    float *logp;            // [B][N][n_cls] or null: log_softmax of the last layer's first n_cls rows
    FwdLayer layer[MAX_LAYERS];
    int n_layers;
    int C1, C2, N, S, Cout, n_cls;
    // FP split (see fp_layer1_split).  Consumer side: tsrc = rows [B][S][ldt] of the interpolated part's first-layer product,
    // computed per COARSE point by the coarser module; layer[0] then holds the skip columns only (k8 = C1 / 8, possibly 0).
    const float *tsrc;
    int ldt;
    // Producer side: after its own last layer the module runs `extra` (the finer module's interpolated-part columns, no bias,
    // no ReLU) over its output and writes those rows to out2 [B][N][Cout2]
    float *out2;
    int Cout2;
    FwdLayer extra;
    int diag;               // timing diagnostics only (-DPSG_DIAG_BUILD libraries only): skip sections, results are then wrong
    unsigned long long *dbg; // diag & 256: per-workgroup {memtime, memrealtime} at entry and exit
};

struct FpBwdArgs {
    const float *dout;          // [B][N][Cout] gradient of the last layer's (post-ReLU) output, or null
    // gather form of dout (deterministic transpose of the finer module's 3-NN interpolation):
    const int32_t *nninv_off;   // [B][N+1] or null
    const int2 *nninv_ent;      // [B][3*n_fine]
    const float *dint;          // [B][n_fine][Cg] interpolated-part gradient rows written by the finer module
    int n_fine;
    int Cg;                     // = Cout, or (finer module split) the width of ITS first layer: the rows are its dZ1
    BwdLayer pre;               // finer module split (pre.w != null): gathered rows -> . W1b(finer)^T, masked by mask_last
    float *dint_out;            // [B][N][C2]: this module's interpolated-part gradient rows (plain stores); split: its dZ1
                                // rows [B][N][Cd], written BEFORE the skip columns' transpose `skipT` (C1 > 0) runs
    int split, Cd;
    BwdLayer skipT;
    const uint16_t *mask_last;  // ReLU mask of that layer
    const float *logp;          // head mode: [B][N][n_cls]
    const float *dlogp;         // head mode: [B][N][n_cls]
    const int32_t *nn_idx;
    const float *nn_w;
    float *dfeat1;              // [B][N][C1] skip-link gradient rows (plain stores) or null
    BwdLayer layer[MAX_LAYERS];
    int n_layers;
    int C1, C2, N, S, Cout, n_cls, mb_last;
};

// ------------------------------------------------------------------------------------------ SA fwd
// LDS channel order of the grouped input: [feats(D), rel_xyz(3), zero pad to a multiple of 8]; the
// first layer's weight columns are permuted accordingly at pack time (reference order is
// [rel_xyz, feats], pointnet_util.py:137).
// KS = samples per group (32, or 16 for the small-radius scale of an MSG level: two groups per 32-point tile);
// MAXT = tiles a wave may hold in the first two layers.
//
// SPLIT (round 5): the first layer is linear in the concatenation, W1 . [x_j - c_i ; f_j] = W1f . f_j + W1x . (x_j - c_i),
// and its feature part depends on the SOURCE POINT j only - a level has 8 x fewer points than grouped rows (1024 / 256 / 64
// points against 8192 / 2048 / 512 rows per room at levels 1 - 3).  T[j] = W1f . f_j + b1 is computed once per point by a
// separate per-point launch; here the rows of T are gathered through the group table straight into the MFMA ACCUMULATORS
// of the first layer's tiles (lane (j, h) of a tile reads the 4 x 16 bytes of row gidx[j] that its accumulator registers
// hold: the same bytes per grouped row as the feature gather it replaces, and no LDS staging), and the layer itself is
// ONE k8-chunk (the three relative coordinates) instead of (D + 3) / 8 chunks: 9 -> 1, 17 -> 1, 33 -> 1 at levels 1 - 3,
// i.e. 24 % of the module's matrix instructions.  The coordinates are NOT split (W1x x_j - W1x c_i would cancel: |x| ~ 3
// against |x_j - c_i| < r): the difference is formed first, as the reference does.
template <int P, int NW, int MAXT, int KS>
__device__ __forceinline__ void sa_layer1_split(const SaFwdArgs &a, int b, int s0, float *__restrict__ buf, size_t wg_linear)
{
    constexpr int PB = P / 32;
    const FwdLayer &L = a.l1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int ntask = L.mb * PB;
    const int first = (wave + (int)(wg_linear & (NW - 1))) & (NW - 1);
    const int32_t *gi = a.gidx + ((size_t)b * a.S + s0) * KS;          // the workgroup's P grouped rows are contiguous
    const float *trows = a.tfeat + (size_t)b * a.Np * a.ldt;
    f32x16 acc[MAXT];
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        const int task = first + i * NW;
        if (task < ntask) {
            const int mb = task / PB, pb = task - mb * PB;
            const int src = gi[pb * 32 + j];
            // accumulator registers 4g .. 4g+3 of lane (j, h) are channels mb*32 + 8g + 4h + (0..3) of point j
            const float4 *tp = (const float4 *)(trows + __umul24((unsigned)src, (unsigned)a.ldt) + mb * 32 + 4 * h);
            const float4 t0 = tp[0], t1 = tp[2], t2 = tp[4], t3 = tp[6];
            f32x16 c;
            c[0] = t0.x; c[1] = t0.y; c[2] = t0.z; c[3] = t0.w;
            c[4] = t1.x; c[5] = t1.y; c[6] = t1.z; c[7] = t1.w;
            c[8] = t2.x; c[9] = t2.y; c[10] = t2.z; c[11] = t2.w;
            c[12] = t3.x; c[13] = t3.y; c[14] = t3.z; c[15] = t3.w;
            const float4 wx = L.w[(size_t)mb * 64 + lane];               // k8 = 1: one chunk per 32-channel block
            const float4 rx = *(const float4 *)(buf + (pb * 32 + j) * 8 + 4 * h);
            c = mfma4<false>(wx, rx, c);
            mfma_fence(c);                                               // (compiler MFMAs -> inline-asm consumer: psg_mlp.cuh)
            const unsigned m = relu_bits(c);
            if (L.mask) L.mask[(wg_linear * ntask + task) * 64 + lane] = (uint16_t)m;
            acc[i] = c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        const int task = first + i * NW;
        if (task < ntask) {
            const int mb = task / PB, pb = task - mb * PB;
            store_tile<P>(buf, mb, pb * 32 + j, h, acc[i]);
        }
    }
}

// the workgroup (bx, b) of sa_fwd_kernel: groups [bx * G, (bx + 1) * G) of room b (also what sa_fwd_packed_kernel runs for a
// workgroup of full groups on that boundary).  wg keys the workgroup's ReLU mask slots: the linear index of (bx, b), or
// (KEYED) the packed workgroup's own where the masks are keyed by packed workgroup (sa_fwd_packed_kernel, PKM)
template <int P, int NW, int KS, int MAXT, bool SPLIT, bool KEYED = false>
__device__ __forceinline__ void sa_fwd_body(SaFwdArgs a, int bx, int b, size_t key = 0)
{
    using L = Lds<P>;
    static_assert(KS == 32 || KS == 16, "groups of 32 or 16 samples");
    constexpr int G = P / KS, PB = P / 32, NT = NW * 64, NPART = NT / P;
    extern __shared__ float lds[];
    float *buf0 = lds;   // the one activation buffer (layers run in place)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = bx * G;
    const size_t wg = KEYED ? key : (size_t)b * gridDim.x + bx;

    if (SPLIT) {
        // block 0 of the buffer = [x_j - c_i, 0 x 5] of the P grouped rows; the feature part arrives through T (below)
        if (tid < P) {
            const int j = tid, s = s0 + j / KS;
            const int src = a.gidx[((size_t)b * a.S + s) * KS + (j & (KS - 1))];
            const float *xr = a.xyz + ((size_t)b * a.Np + src) * a.xyz_stride;
            const float *cr = a.new_xyz + ((size_t)b * a.S + s) * 3;
            *(float4 *)(buf0 + j * 8) = make_float4(xr[0] - cr[0], xr[1] - cr[1], xr[2] - cr[2], 0.0f);
            *(float4 *)(buf0 + j * 8 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else if (!PSG_DIAGBIT(a, 1)) {   // gather the P grouped points
        const int j = tid % P, part = tid / P;
        const int s = s0 + j / KS;
        const int src = a.gidx[((size_t)b * a.S + s) * KS + (j & (KS - 1))];
        const float *frow = a.feat + ((size_t)b * a.Np + src) * a.D;
        const float *xr = a.xyz + ((size_t)b * a.Np + src) * a.xyz_stride;
        const float *cr = a.new_xyz + ((size_t)b * a.S + s) * 3;
        if ((a.D & 3) == 0) {
            const float4 *f4 = (const float4 *)frow;
            for (int q = part; q < (a.D >> 2); q += NPART) *(float4 *)(buf0 + L::off(4 * q, j)) = f4[q];
            if (part == 0) {
                *(float4 *)(buf0 + L::off(a.D, j)) = make_float4(xr[0] - cr[0], xr[1] - cr[1], xr[2] - cr[2], 0.0f);
                if ((a.D & 7) == 0) *(float4 *)(buf0 + L::off(a.D + 4, j)) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else if (part == 0) {
            // sa1: D = 9 -> [f0..f8, rx, ry, rz, 0, 0, 0, 0] (two 8-channel blocks)
            float f[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) f[c] = frow[c];
            *(float4 *)(buf0 + L::off(0, j)) = make_float4(f[0], f[1], f[2], f[3]);
            *(float4 *)(buf0 + L::off(4, j)) = make_float4(f[4], f[5], f[6], f[7]);
            *(float4 *)(buf0 + L::off(8, j)) = make_float4(f[8], xr[0] - cr[0], xr[1] - cr[1], xr[2] - cr[2]);
            *(float4 *)(buf0 + L::off(12, j)) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // zero any further 8-channel blocks the first layer reads (its K is ceil((D + 3) / 8) blocks: normally none)
        for (int blk = ((a.D + 3) >> 3) + 1 + part; blk < a.l1.k8; blk += NPART) {
            float *z = buf0 + (size_t)blk * L::BLK + j * 8;
            *(float4 *)z = make_float4(0.f, 0.f, 0.f, 0.f);
            *(float4 *)(z + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __syncthreads();
    // biases of this wave's last-layer tiles: fetched now, so their latency is spent under the first two layers
    // (an SSG level has nb3 * PB = 2 * NW last-layer tiles, i.e. two per wave; MSG scales have at most that)
    const int jj = lane & 31, h = lane >> 5;
    constexpr int T3 = 2;
    // pairs (psg_mlp.cuh): with exactly two last-layer tiles per wave, a wave takes the point blocks g, g + 1 of ONE output block
    // on one weight stream (tile_mac4x2) instead of one point block of two output blocks
    constexpr int HP = PB / 2 > 0 ? PB / 2 : 1;
    constexpr bool PAIR3 = PSG_MLP_PAIRS && PB >= 2 && (PB & 1) == 0;
    const bool pair3 = PAIR3 && a.nb3 * PB == 2 * NW;
    float bias3[T3];
#pragma unroll
    for (int i = 0; i < T3; ++i) {
        const int task = pair3 ? (wave / HP) * PB : wave + i * NW;
        bias3[i] = task < a.nb3 * PB ? a.b3[(task / PB) * 32 + jj] : 0.0f;
    }
    if (SPLIT) sa_layer1_split<P, NW, MAXT, KS>(a, b, s0, buf0, wg);
    else if (!PSG_DIAGBIT(a, 8)) layer_fwd<P, NW, MAXT>(a.l1, buf0, wg);
    if (!PSG_DIAGBIT(a, 16)) __syncthreads();
    if (!PSG_DIAGBIT(a, 8)) layer_fwd<P, NW, MAXT>(a.l2, buf0, wg);
    if (!PSG_DIAGBIT(a, 16)) __syncthreads();
    if (PSG_DIAGBIT(a, 32)) return;

    // last layer with the tile flipped (D[point][channel]) so the max over the 32 samples of a
    // group is an in-lane max over 16 accumulators + one exchange between lane halves.
    auto pool = [&](const f32x16 &acc, int nb, int g) {   // g = 32-point tile of the workgroup
        if (KS == 32) {
            // max(relu(x)) = relu(max(x)): the raw maximum first (v_max3: 8 instructions for 16 values), then the lowest row
            // that holds it (descending scan: the last match written is the lowest), the ReLU once at the end - the values and
            // arg bytes of the per-element compare / select chain (80 instructions), in about half of them
            float best = fmaxf(fmaxf(acc[0], acc[1]), acc[2]);
#pragma unroll
            for (int r = 3; r < 15; r += 2) best = fmaxf(fmaxf(best, acc[r]), acc[r + 1]);
            best = fmaxf(best, acc[15]);
            int bidx = acc_row(15, h);
#pragma unroll
            for (int r = 14; r >= 0; --r) bidx = acc[r] == best ? acc_row(r, h) : bidx;
            best = best > 0.0f ? best : 0.0f;                 // (+0 for a non-positive maximum, as the element-wise ReLU gave)
            float ob = __shfl_xor(best, 32);
            int oi = __shfl_xor(bidx, 32);
            if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
            if (h == 0) {
                const size_t row = (size_t)b * a.S + s0 + g;
                a.out[row * a.ld_out + a.c_out + nb * 32 + jj] = best;
                a.arg[row * a.C3 + nb * 32 + jj] = best > 0.0f ? (uint8_t)bidx : (uint8_t)255;
            }
        } else {
            // two groups of 16 samples per tile: accumulators 0..7 hold points 0..15, 8..15 hold points 16..31
            float best[2] = {-1.0f, -1.0f};
            int bidx[2] = {0, 0};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[r] > 0.0f ? acc[r] : 0.0f;
                if (v > best[r >> 3]) { best[r >> 3] = v; bidx[r >> 3] = acc_row(r, h) & 15; }
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float ob = __shfl_xor(best[q], 32);
                int oi = __shfl_xor(bidx[q], 32);
                if (ob > best[q] || (ob == best[q] && oi < bidx[q])) { best[q] = ob; bidx[q] = oi; }
            }
            // lane half h writes group h of the tile
            const float bv = h ? best[1] : best[0];
            const int bi = h ? bidx[1] : bidx[0];
            const size_t row = (size_t)b * a.S + s0 + 2 * g + h;
            a.out[row * a.ld_out + a.c_out + nb * 32 + jj] = bv;
            a.arg[row * a.C3 + nb * 32 + jj] = bv > 0.0f ? (uint8_t)bi : (uint8_t)255;
        }
    };
    if (pair3) {
        const int nb = wave / HP, g = 2 * (wave - nb * HP);
        f32x16 c0, c1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { c0[r] = bias3[0]; c1[r] = bias3[0]; }
        tile_mac_x2<L::BLK, true>(a.w3 + (size_t)nb * a.k8_3 * 64 + lane, a.k8_3, buf0 + (g * 32 + jj) * 8 + 4 * h, c0, c1);
        pool(c0, nb, g);
        pool(c1, nb, g + 1);
        return;
    }
#pragma unroll
    for (int i = 0; i < T3; ++i) {
        const int task = wave + i * NW;
        if (task >= a.nb3 * PB) break;
        const int nb = task / PB, g = task - nb * PB;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias3[i];
        acc = tile_mac<L::BLK, true>(a.w3 + (size_t)nb * a.k8_3 * 64 + lane, a.k8_3, buf0 + (g * 32 + jj) * 8 + 4 * h,
                                     acc);
        pool(acc, nb, g);
    }
}

template <int P, int NW, int KS = 32, int MAXT = 1, bool SPLIT = false>
__global__ __launch_bounds__(NW * 64) void sa_fwd_kernel(SaFwdArgs a)
{
    int bx, b;
    xcd_tile(bx, b);
    sa_fwd_body<P, NW, KS, MAXT, SPLIT>(a, bx, b);
}

// ------------------------------------------------------------------------------------------ SA fwd, packed
// query_ball_point fills a group of 32 with copies of its first member (pointnet_util.py:104-106), and a 0.1 m ball of a
// 4096-point room holds about five points: most grouped rows are bit-for-bit copies of row 0 of their group.  A copy has row
// 0's MLP output, never wins the max-pool (a tie goes to the lowest row) and gets no gradient, so the forward runs the VALID rows
// only: cnt[s] = the leading rows of group s up to the first k > 0 with gidx[k] == gidx[0] (the rule of build_inv_group_kernel;
// an empty ball, gidx[0] = Np, counts as 32 rows and behaves as in sa_fwd_kernel).
//
// Plan (sa_pack_plan_kernel, once per psg_pn2_plan_build, one workgroup per problem): the counts, and a greedy segmentation of
// the S groups into workgroups - consecutive groups while their valid rows stay BELOW the kernel's P rows (the last row of the
// LDS pool holds the workgroup's group table) and within SA_PACK_GCAP groups; the one workgroup that holds P rows is P / 32 full
// groups, which pools in registers.  seg[0] = workgroups in use, seg[1 + i] = first group of workgroup i, seg[1 + seg[0]] = S.
// A group has at most 32 rows, so a closed workgroup holds at least P / 32 groups: the unpacked grid (S / (P / 32) per problem)
// is the worst case and stays the launch grid - nothing is read back, surplus workgroups read their descriptor and return.
// What a workgroup reads is ONE 16-byte descriptor (a uniform load; counts and segment tables would be three dependent loads
// in front of the gather): x = first group | groups << 16 (0 groups: surplus), y / z / w = cnt - 1 of its groups, five bits
// each, six to a word.  cnt and seg stay in the plan for read-back (psg_pn2_plan_ptr).
constexpr int SA_PACK_GCAP = 16;
constexpr int SA_PACK_CHAN = 8;    // sa_bwd_packed_kernel's last template argument: SPV + this = the channel-ordered transpose

__device__ __forceinline__ int sa_pack_cnt(const int4 &d, int i)
{
    const int w = i < 6 ? d.y : (i < 12 ? d.z : d.w);
    return ((w >> (5 * (i % 6))) & 31) + 1;
}

__global__ __launch_bounds__(256) void sa_pack_plan_kernel(const int32_t *__restrict__ gidx, int S, int Np, int P,
                                                           int32_t *__restrict__ cnt, int32_t *__restrict__ seg,
                                                           int4 *__restrict__ desc)
{
    __shared__ int s_cnt[1024], s_next[1024], s_first[1025], s_nseg;
    const size_t p = blockIdx.x;
    const int32_t *gi = gidx + p * S * 32;
    for (int s = threadIdx.x; s < S; s += 256) {
        const int32_t *row = gi + (size_t)s * 32;
        const int first = row[0];
        int n = 32;
        if (first < Np) {
            n = 1;
            while (n < 32 && row[n] != first) ++n;
        }
        s_cnt[s] = n;
        cnt[p * S + s] = n;
    }
    __syncthreads();
    // every group's segment end, had a segment begun there (the greedy rule, at most SA_PACK_GCAP steps): all S in parallel
    for (int s0 = threadIdx.x; s0 < S; s0 += 256) {
        int s = s0, rows = 0, g = 0;
        while (s < S && g < SA_PACK_GCAP) {
            const int c = s_cnt[s];
            if (!(rows + c < P || (rows + c == P && rows == 32 * g && g + 1 == P / 32))) break;
            rows += c; ++s; ++g;
        }
        s_next[s0] = s;
    }
    __syncthreads();
    // the chain of segment starts is all that stays serial: one LDS read per segment
    const int gx = S / (P / 32);
    int32_t *sg = seg + p * (gx + 2);
    int4 *dg = desc + p * gx;
    if (threadIdx.x == 0) {
        int nseg = 0;
        for (int s = 0; s < S; s = s_next[s]) s_first[nseg++] = s;
        s_first[nseg] = S;
        s_nseg = nseg;
    }
    __syncthreads();
    const int nseg = s_nseg;
    for (int i = threadIdx.x; i <= nseg; i += 256) sg[1 + i] = s_first[i];
    if (threadIdx.x == 0) sg[0] = nseg;
    for (int i = threadIdx.x; i < gx; i += 256) {
        int4 d = make_int4(0, 0, 0, 0);
        if (i < nseg) {
            const int lo = s_first[i], n = s_first[i + 1] - lo;
            d.x = lo | (n << 16);
            for (int g = 0; g < n; ++g) {
                const int f = (s_cnt[lo + g] - 1) << (5 * (g % 6));
                if (g < 6) d.y |= f; else if (g < 12) d.z |= f; else d.w |= f;
            }
        }
        dg[i] = d;
    }
}

// The kernel: sa_fwd_kernel's chain (KS = 32, one tile per wave in the first two layers) over the workgroup's packed rows.
//   * rows: the valid rows of the descriptor's groups in order, nrows <= P of them in nblk = ceil(nrows / 32) blocks;
//     the tail of the last block repeats the last valid row (tile columns are independent: it changes nothing and is never read);
//   * layers run over the nblk active blocks only, every valid row through the k-loop and epilogue it had unpacked: the values are
//     the same bits;
//   * ReLU masks go to the slots of the UNPACKED layout (workgroup s / G, tile (mb, s % G), lane (h, k)), one 2-byte store per
//     lane: the backward kernels read them where they always did.  The words of padding rows are not written: their gradient
//     rows are exactly zero before the mask is applied (AND with a zero) and are not stored (gpos_out = -1).  Where the level's
//     backward runs packed too (PKM, below) the words are keyed by packed workgroup and block instead;
//   * max-pool: groups are runs of packed rows that may cross a block, so the last layer's tiles go to LDS as plain rows
//     [row][C3] (over the dead activation buffer: P x C3 floats, twice the buffer) and one thread per (group, channel) scans
//     the group's rows in ascending order with a strict compare - the lowest row that attains the maximum, as the in-register
//     pool finds it; 255 for a maximum <= 0.  A workgroup whose groups are all full (nothing to skip) pools in registers as
//     sa_fwd_kernel does.
// LDS: P x C3 floats and not a byte more (32 / 32 / 32 / 64 KiB at levels 0 - 3, against 16 / 16 / 16 / 32 KiB unpacked: five
// workgroups of levels 0 - 2 per CU are exactly the 160 KiB, which is also what 88 VGPRs allow).  The row tables live inside:
// the group starts in pool row P - 1, which a packed workgroup never fills (the plan keeps it below P rows), the row maps
// behind the activation buffer in the half of the pool that is dead until the last layer is done.
__device__ __forceinline__ void sa_pool32(const SaFwdArgs &a, const f32x16 &acc, int h, int jj, size_t row, int nb)
{
    float best = fmaxf(fmaxf(acc[0], acc[1]), acc[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) best = fmaxf(fmaxf(best, acc[r]), acc[r + 1]);
    best = fmaxf(best, acc[15]);
    int bidx = acc_row(15, h);
#pragma unroll
    for (int r = 14; r >= 0; --r) bidx = acc[r] == best ? acc_row(r, h) : bidx;
    best = best > 0.0f ? best : 0.0f;
    float ob = __shfl_xor(best, 32);
    int oi = __shfl_xor(bidx, 32);
    if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    if (h == 0) {
        a.out[row * a.ld_out + a.c_out + nb * 32 + jj] = best;
        a.arg[row * a.C3 + nb * 32 + jj] = best > 0.0f ? (uint8_t)bidx : (uint8_t)255;
    }
}

// slot of the mask word of unpacked row om = group * 32 + sample, tile row mb of a layer with lmb 32-channel blocks
template <int P>
__device__ __forceinline__ size_t sa_pack_mask_slot(int om, int b, int gx, int mb, int lmb, int h)
{
    constexpr int G = P / 32;
    const int s = om >> 5, k = om & 31;
    const size_t wgo = (size_t)b * gx + s / G;
    return ((wgo * lmb + mb) * G + (s % G)) * 64 + h * 32 + k;
}

template <int P, int NW, bool PKM>
__device__ __forceinline__ void sa_layer_fwd_packed(const FwdLayer &L, float *__restrict__ buf, int nblk, int first,
                                                    const int *__restrict__ omap, int b, size_t wg)
{
    constexpr int BLK = Lds<P>::BLK, PB = P / 32;
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const bool act = first < L.mb * nblk;
    int mb = 0, pb = 0;
    f32x16 c;
    if (act) {
        mb = first / nblk; pb = first - mb * nblk;
        const float4 *bp = (const float4 *)(L.bias + mb * 32 + 4 * h);
        const float4 bq0 = bp[0], bq1 = bp[2], bq2 = bp[4], bq3 = bp[6];
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = 0.0f;
        c = tile_mac<BLK, false>(L.w + (size_t)mb * L.k8 * 64 + lane, L.k8, buf + (pb * 32 + j) * 8 + 4 * h, c);
        c[0] += bq0.x; c[1] += bq0.y; c[2] += bq0.z; c[3] += bq0.w;
        c[4] += bq1.x; c[5] += bq1.y; c[6] += bq1.z; c[7] += bq1.w;
        c[8] += bq2.x; c[9] += bq2.y; c[10] += bq2.z; c[11] += bq2.w;
        c[12] += bq3.x; c[13] += bq3.y; c[14] += bq3.z; c[15] += bq3.w;
        if (L.relu) {
            const unsigned m = relu_bits(c);
            if constexpr (PKM) {
                if (L.mask) L.mask[((wg * L.mb + mb) * PB + pb) * 64 + lane] = (uint16_t)m;
            } else {
                const int om = omap[pb * 32 + j];
                if (L.mask && om >= 0) L.mask[sa_pack_mask_slot<P>(om, b, gridDim.x, mb, L.mb, h)] = (uint16_t)m;
            }
        }
    }
    __syncthreads();
    if (act) store_tile<P>(buf, mb, pb * 32 + j, h, c);
}

// PKM (the levels whose backward is sa_bwd_packed_kernel; psg_pn2.hip: sa_pack_bwd_level): the ReLU mask word of tile (mb, pb)
// goes to slot ((wg * L.mb + mb) * PB + pb) * 64 + lane of the PACKED workgroup wg - where layer_bwd looks for task mb * PB + pb
// of workgroup wg, so the level's backward runs on the same packed rows.  One coalesced store per wave and no row map; the
// words of tail rows land in slots this workgroup owns (their gradient is zero).  The buffers keep their size: wg, mb and pb
// stay inside the unpacked extents.  PKM = false is the kernel of round 16, instruction for instruction.
template <int P, int NW, bool SPLIT, bool PKM = false>
__global__ __launch_bounds__(NW * 64) void sa_fwd_packed_kernel(SaFwdArgs a)
{
    using L = Lds<P>;
    constexpr int PB = P / 32, NT = NW * 64, GCAP = SA_PACK_GCAP;
    static_assert(GCAP >= PB && GCAP < 64, "a workgroup's groups: at least P / 32, and one scan lane each");
    extern __shared__ float lds[];
    float *buf0 = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, b;
    xcd_tile(bx, b);
    const size_t wg = (size_t)b * gridDim.x + bx;
    const int4 desc = a.pk_desc[wg];
    const int ng = desc.x >> 16, sA = desc.x & 0xFFFF;
    if (ng == 0) return;                                        // surplus workgroup (uniform: no barrier has been reached)
    if (ng == PB && (sA & (PB - 1)) == 0) {
        // P / 32 groups on an unpacked workgroup's boundary: if they are all full there is nothing to skip, and the rows, mask
        // slots and pool are sa_fwd_kernel's own - its body runs, at its cost (rooms of full balls: tools/sa_pack_probe.py)
        int rows = 0;
        for (int i = 0; i < PB; ++i) rows += sa_pack_cnt(desc, i);
        if (rows == P) {
            // (the mask key is separate from the group origin: unpacked-keyed, slot sA / PB is this workgroup's; packed-keyed
            // it belongs to another workgroup)
            sa_fwd_body<P, NW, 32, 1, SPLIT, PKM>(a, sA / PB, b, wg);
            return;
        }
    }
    int *gstart = (int *)(lds + (size_t)(P - 1) * a.C3);        // [GCAP + 1] first packed row of each group, then nrows
    int *omap = (int *)(lds + a.pk_tab_off);                    // [P] unpacked row (group * 32 + sample) of a packed row, -1 = tail
    int *srcl = omap + P;                                       // [P] its source point (both dead before the pool is written)
    int nrows = 0;
    for (int i = 0; i < ng; ++i) {                              // (uniform; the pool scan at the end reads the starts from LDS)
        if (tid == i) gstart[i] = nrows;
        nrows += sa_pack_cnt(desc, i);
    }
    if (tid == ng) gstart[ng] = nrows;
    const int nblk = (nrows + 31) >> 5;
    {
        // packed row j of this thread (the parts of the unsplit gather each find it themselves: a search over <= GCAP starts)
        const int j = tid % P, part = tid / P;
        constexpr int NPART = NT / P > 0 ? NT / P : 1;
        if (tid < NPART * P && j < nblk * 32) {
            const int pe = min(j, nrows - 1);
            int g = 0, st = 0, c = sa_pack_cnt(desc, 0);
            while (st + c <= pe) { st += c; ++g; c = sa_pack_cnt(desc, g); }   // (pe < nrows: ends at a group < ng)
            const int k = pe - st, s = sA + g;
            const int src = a.gidx[((size_t)b * a.S + s) * 32 + k];
            if (part == 0) {
                if constexpr (!PKM) omap[j] = j < nrows ? s * 32 + k : -1;
                srcl[j] = src;
            }
            const float *xr = a.xyz + ((size_t)b * a.Np + src) * a.xyz_stride;
            const float *cr = a.new_xyz + ((size_t)b * a.S + s) * 3;
            if (SPLIT) {
                if (part == 0) {
                    *(float4 *)(buf0 + j * 8) = make_float4(xr[0] - cr[0], xr[1] - cr[1], xr[2] - cr[2], 0.0f);
                    *(float4 *)(buf0 + j * 8 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
                const float *frow = a.feat + ((size_t)b * a.Np + src) * a.D;
                if ((a.D & 3) == 0) {
                    const float4 *f4 = (const float4 *)frow;
                    for (int q = part; q < (a.D >> 2); q += NPART) *(float4 *)(buf0 + L::off(4 * q, j)) = f4[q];
                    if (part == 0) {
                        *(float4 *)(buf0 + L::off(a.D, j)) = make_float4(xr[0] - cr[0], xr[1] - cr[1], xr[2] - cr[2], 0.0f);
                        if ((a.D & 7) == 0) *(float4 *)(buf0 + L::off(a.D + 4, j)) = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                } else if (part == 0) {
                    // sa1: D = 9 -> [f0..f8, rx, ry, rz, 0, 0, 0, 0] (two 8-channel blocks)
                    float f[9];
#pragma unroll
                    for (int c = 0; c < 9; ++c) f[c] = frow[c];
                    *(float4 *)(buf0 + L::off(0, j)) = make_float4(f[0], f[1], f[2], f[3]);
                    *(float4 *)(buf0 + L::off(4, j)) = make_float4(f[4], f[5], f[6], f[7]);
                    *(float4 *)(buf0 + L::off(8, j)) = make_float4(f[8], xr[0] - cr[0], xr[1] - cr[1], xr[2] - cr[2]);
                    *(float4 *)(buf0 + L::off(12, j)) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                for (int blk = ((a.D + 3) >> 3) + 1 + part; blk < a.l1.k8; blk += NPART) {
                    float *z = buf0 + (size_t)blk * L::BLK + j * 8;
                    *(float4 *)z = make_float4(0.f, 0.f, 0.f, 0.f);
                    *(float4 *)(z + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
    }
    __syncthreads();
    const int jj = lane & 31, h = lane >> 5;
    const int first = (wave + (int)(wg & (NW - 1))) & (NW - 1);
    if (SPLIT) {
        // sa_layer1_split over the active blocks: the rows of T into the accumulators, one k8-chunk of relative coordinates
        const FwdLayer &L1 = a.l1;
        const bool act = first < L1.mb * nblk;
        int mb = 0, pb = 0;
        f32x16 c;
        if (act) {
            mb = first / nblk; pb = first - mb * nblk;
            const int src = srcl[pb * 32 + jj];
            const float *trows = a.tfeat + (size_t)b * a.Np * a.ldt;
            const float4 *tp = (const float4 *)(trows + __umul24((unsigned)src, (unsigned)a.ldt) + mb * 32 + 4 * h);
            const float4 t0 = tp[0], t1 = tp[2], t2 = tp[4], t3 = tp[6];
            c[0] = t0.x; c[1] = t0.y; c[2] = t0.z; c[3] = t0.w;
            c[4] = t1.x; c[5] = t1.y; c[6] = t1.z; c[7] = t1.w;
            c[8] = t2.x; c[9] = t2.y; c[10] = t2.z; c[11] = t2.w;
            c[12] = t3.x; c[13] = t3.y; c[14] = t3.z; c[15] = t3.w;
            const float4 wx = L1.w[(size_t)mb * 64 + lane];
            const float4 rx = *(const float4 *)(buf0 + (pb * 32 + jj) * 8 + 4 * h);
            c = mfma4<false>(wx, rx, c);
            mfma_fence(c);
            const unsigned m = relu_bits(c);
            if constexpr (PKM) {
                if (L1.mask) L1.mask[((wg * L1.mb + mb) * PB + pb) * 64 + lane] = (uint16_t)m;
            } else {
                const int om = omap[pb * 32 + jj];
                if (L1.mask && om >= 0) L1.mask[sa_pack_mask_slot<P>(om, b, gridDim.x, mb, L1.mb, h)] = (uint16_t)m;
            }
        }
        __syncthreads();
        if (act) store_tile<P>(buf0, mb, pb * 32 + jj, h, c);
    } else {
        sa_layer_fwd_packed<P, NW, PKM>(a.l1, buf0, nblk, first, omap, b, wg);
    }
    __syncthreads();
    sa_layer_fwd_packed<P, NW, PKM>(a.l2, buf0, nblk, first, omap, b, wg);
    __syncthreads();

    // last layer, tile flipped (D[point][channel]): two tiles per wave, as sa_fwd_kernel deals them
    f32x16 c0, c1;
    int nb0 = 0, nb1 = 0, g0 = 0, g1 = 0;
    bool act0 = false, act1 = false;
    if constexpr (PSG_MLP_PAIRS && PB >= 2) {
        // the point blocks g, g + 1 of one output block on one weight stream; an odd last block pairs with a block nobody reads
        const int hp = (nblk + 1) >> 1;
        if (wave < a.nb3 * hp) {
            nb0 = nb1 = wave / hp;
            g0 = 2 * (wave - nb0 * hp); g1 = g0 + 1;
            act0 = true; act1 = g1 < nblk;
            const float bias = a.b3[nb0 * 32 + jj];
#pragma unroll
            for (int r = 0; r < 16; ++r) { c0[r] = bias; c1[r] = bias; }
            tile_mac_x2<L::BLK, true>(a.w3 + (size_t)nb0 * a.k8_3 * 64 + lane, a.k8_3, buf0 + (g0 * 32 + jj) * 8 + 4 * h, c0, c1);
        }
    } else if constexpr (PB >= 2) {
        // -DPSG_MLP_PAIRS=0: single tiles (output block, point block), two per wave at most
        const int nt = a.nb3 * nblk;
        act0 = wave < nt; act1 = wave + NW < nt;
        nb0 = wave / nblk; g0 = wave - nb0 * nblk;
        nb1 = (wave + NW) / nblk; g1 = wave + NW - nb1 * nblk;
        if (act0) {
            const float bias0 = a.b3[nb0 * 32 + jj];
#pragma unroll
            for (int r = 0; r < 16; ++r) c0[r] = bias0;
            c0 = tile_mac<L::BLK, true>(a.w3 + (size_t)nb0 * a.k8_3 * 64 + lane, a.k8_3, buf0 + (g0 * 32 + jj) * 8 + 4 * h, c0);
        }
        if (act1) {
            const float bias1 = a.b3[nb1 * 32 + jj];
#pragma unroll
            for (int r = 0; r < 16; ++r) c1[r] = bias1;
            c1 = tile_mac<L::BLK, true>(a.w3 + (size_t)nb1 * a.k8_3 * 64 + lane, a.k8_3, buf0 + (g1 * 32 + jj) * 8 + 4 * h, c1);
        }
    } else {
        nb0 = wave; nb1 = wave + NW;
        act0 = nb0 < a.nb3; act1 = nb1 < a.nb3;
        const float bias0 = act0 ? a.b3[nb0 * 32 + jj] : 0.0f, bias1 = act1 ? a.b3[nb1 * 32 + jj] : 0.0f;
        if (act0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) c0[r] = bias0;
            c0 = tile_mac<L::BLK, true>(a.w3 + (size_t)nb0 * a.k8_3 * 64 + lane, a.k8_3, buf0 + jj * 8 + 4 * h, c0);
        }
        if (act1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) c1[r] = bias1;
            c1 = tile_mac<L::BLK, true>(a.w3 + (size_t)nb1 * a.k8_3 * 64 + lane, a.k8_3, buf0 + jj * 8 + 4 * h, c1);
        }
    }
    if (nrows == P) {               // P / 32 full groups (the plan packs nothing else into P rows): block g is group sA + g
        if (act0) sa_pool32(a, c0, h, jj, (size_t)b * a.S + sA + g0, nb0);
        if (act1) sa_pool32(a, c1, h, jj, (size_t)b * a.S + sA + g1, nb1);
        return;
    }
    __syncthreads();                // the activation buffer is dead: the tiles go over it as plain rows [row][C3]
    float *pool = lds;
    if (act0) {                     // (rows < nrows <= P - 1 only: row P - 1 holds gstart)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (g0 * 32 + acc_row(r, h) < nrows) pool[(size_t)(g0 * 32 + acc_row(r, h)) * a.C3 + nb0 * 32 + jj] = c0[r];
    }
    if (act1) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (g1 * 32 + acc_row(r, h) < nrows) pool[(size_t)(g1 * 32 + acc_row(r, h)) * a.C3 + nb1 * 32 + jj] = c1[r];
    }
    __syncthreads();
    for (int t = tid; t < ng * a.C3; t += NT) {
        const int g = t / a.C3, c = t - g * a.C3;
        const int r0 = gstart[g], n = gstart[g + 1] - r0;
        const float *col = pool + (size_t)r0 * a.C3 + c;
        float best = col[0];
        int bi = 0;
        for (int k = 1; k < n; ++k) {
            const float v = col[(size_t)k * a.C3];
            if (v > best) { best = v; bi = k; }
        }
        const size_t row = (size_t)b * a.S + sA + g;
        a.out[row * a.ld_out + a.c_out + c] = best > 0.0f ? best : 0.0f;
        a.arg[row * a.C3 + c] = best > 0.0f ? (uint8_t)bi : (uint8_t)255;
    }
}

// ------------------------------------------------------------------------------------------ SA bwd
// Level 0 of the attack loop wants THREE of the first layer's twelve input-gradient channels (the colours).  As a transposed
// MFMA layer that is a 32-row output tile per 32 points, sixteen matrix instructions and a barrier for 3 useful rows, then a
// pass that picks them out of LDS again.  Here: the lanes of a wave take its 32 grouped rows twice - lane half h sums the
// channels [h C1 / 2, (h + 1) C1 / 2) of dZ1 against the three colour columns (a 3 x C1 table in LDS, read as broadcasts), the
// halves are added across the wave and lane half 0 stores the compact {r, g, b, 0} row straight from registers.
// 3 x C1 MACs per row on the vector pipe instead of 32 x C1 on the matrix pipe (sa1 backward 7.8 -> 6.9 ms per attack).
template <int P, int NW, int C1>
__device__ __forceinline__ void sa_l1t_colour(const SaBwdArgs &a, const float *__restrict__ buf0, const float *__restrict__ tab,
                                              const int32_t *__restrict__ pos, float *__restrict__ orow)
{
    using L = Lds<P>;
    static_assert(P == 32 * NW, "one 32-row tile per wave");
    constexpr int KH = C1 / 2;                           // channels per lane half: 8 or 16
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane & 31, h = lane >> 5, j = 32 * wave + rr;
    const int pj = pos[j];
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    const float *t = tab + h * 3 * KH;
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
        const int c = h * KH + 4 * q;
        const float4 z = *(const float4 *)(buf0 + L::off(c, j));
        const float4 w0 = *(const float4 *)(t + 4 * q), w1 = *(const float4 *)(t + KH + 4 * q), w2 = *(const float4 *)(t + 2 * KH + 4 * q);
        g0 = fmaf(z.x, w0.x, g0); g0 = fmaf(z.y, w0.y, g0); g0 = fmaf(z.z, w0.z, g0); g0 = fmaf(z.w, w0.w, g0);
        g1 = fmaf(z.x, w1.x, g1); g1 = fmaf(z.y, w1.y, g1); g1 = fmaf(z.z, w1.z, g1); g1 = fmaf(z.w, w1.w, g1);
        g2 = fmaf(z.x, w2.x, g2); g2 = fmaf(z.y, w2.y, g2); g2 = fmaf(z.z, w2.z, g2); g2 = fmaf(z.w, w2.w, g2);
    }
    // lower channels first: (sum over half 0) + (sum over half 1), the same order in both lanes of a pair
    const float o0 = __shfl_xor(g0, 32), o1 = __shfl_xor(g1, 32), o2 = __shfl_xor(g2, 32);
    if (h == 0 && pj >= 0) *(float4 *)(orow + (size_t)pj * 4) = make_float4(g0 + o0, g1 + o1, g2 + o2, 0.0f);   // padding rows are not listed
}

// Sparse max-pool transpose (round 8).  The max-pool gradient reaches ONE sample per (group, channel), so dZ3 is 31/32 zeros and
// the dense first layer of the backward (W3^T dZ3 on the matrix pipe, K = C3) multiplies mostly zeros.  Here the non-zero
// entries of dZ3 become one flat item list per workgroup, sorted by sample row (stable: ascending channel inside a row), and
// dZ2[row] = sum over the row's items (c, d) of d * W3[c] is a stream of plain weight rows:
//   1. ranks: the lanes of a wave hold 64 consecutive channels of one group (thread t = channel t of the workgroup's G groups);
//      six ballots on the key bits give each lane the lanes with its key, hence its rank among them and their count, which the
//      lowest of them writes to tab[wave][key];
//   2. wave 0 turns the counts into row starts (an exclusive scan over the P rows) and per-chunk list offsets;
//   3. every item is scattered to its slot {row << 16 | channel, gradient};
//   4. the waves take runs of the list cut at row boundaries, about T / NW items each; lanes span the C2 output columns
//      (SPV = C2 / 64 floats per lane: one wave covers a whole weight row), the list is read 64 entries at a time and
//      broadcast with v_readlane, and 16 weight rows are in flight per wave.  All addresses of a batch are known before its
//      first FMA - the round-5 pass (row by row: compact, then fetch) had a dependent list / gradient / weights chain per row.
//      A row's sum stays in registers and is stored once, in the tile layout layer_bwd writes; rows without items store zeros;
//   5. the layer-2 ReLU mask is applied tile by tile, from the slots the forward wrote (mask words fetched before the stream).
// Each output element is one fmaf chain over ascending channels, owned by one lane: no atomics, bit-reproducible.  (Not
// bit-identical to the dense layer: a 32x32x2 MFMA adds two k-products in one step.)  SSG levels 1 - 3 only: KS = 32, P <= 64,
// G * C3 <= NT, C2 in {64, 128, 256} (run_sa_bwd checks).
template <int SPV> struct SpVec;
template <> struct SpVec<1> { using T = float; };
template <> struct SpVec<2> { using T = float2; };
template <> struct SpVec<4> { using T = float4; };

// register r of lane (j, h) = element g = r / 4, component r % 4 of its float4s: the ReLU mask word m over tile (mb, pb) of dZ2
template <int P>
__device__ __forceinline__ void sa_mask_tile(float *__restrict__ buf0, int mb, int pb, int j, int h, unsigned m)
{
    using L = Lds<P>;
    float *o = buf0 + (size_t)(mb * 4) * L::BLK + (pb * 32 + j) * 8 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float4 v = *(float4 *)(o + (size_t)g * L::BLK);
        v.x = __uint_as_float(__float_as_uint(v.x) & (unsigned)__builtin_amdgcn_sbfe((int)m, 4 * g, 1));
        v.y = __uint_as_float(__float_as_uint(v.y) & (unsigned)__builtin_amdgcn_sbfe((int)m, 4 * g + 1, 1));
        v.z = __uint_as_float(__float_as_uint(v.z) & (unsigned)__builtin_amdgcn_sbfe((int)m, 4 * g + 2, 1));
        v.w = __uint_as_float(__float_as_uint(v.w) & (unsigned)__builtin_amdgcn_sbfe((int)m, 4 * g + 3, 1));
        *(float4 *)(o + (size_t)g * L::BLK) = v;
    }
}

// PACKED (sa_bwd_packed_kernel, one batch of G = P / 32 groups of a packed workgroup): the item of thread tid is (key, dval)
// instead of (key, dsrc[tid]); a finished row r = g * 32 + k of the batch goes to PACKED row gst[g] + k of the buffer, and only
// where k is below the group's count gst[g + 1] - gst[g] (a row at or past the count holds no item: the forward's arg-max is
// below the count); steps 1 - 4 only - the mask pass belongs to the caller, once, after its last batch.
// Timing diagnosis (diagnostic builds only): PSG_DIAG bit 128 = no stream (step 4), 1024 = no list build and no stream (steps
// 1 - 4), 2048 = no mask pass (step 5; sa_bwd_body then skips l2t as well), 8192 = every item reads weight row 0 (the same
// loads and FMAs on 256 * SPV bytes of W3 instead of all of it: what the stream costs beyond its bytes).
template <int P, int NW, int MAXT, int SPV, bool PACKED = false>
__device__ __forceinline__ void sa_pool_t_sparse(const SaBwdArgs &a, float *__restrict__ buf0, float *__restrict__ dsrc, int key,
                                                 size_t wg, const int *__restrict__ gst = nullptr, float dval = 0.0f)
{
    using L = Lds<P>;
    using VT = typename SpVec<SPV>::T;
    constexpr int KS = 32, C2 = 64 * SPV, NT = NW * 64, PB = P / 32, U = 16;
    static_assert(P <= 64, "one scan lane per row");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int2 *items = (int2 *)(dsrc + a.sp_off);   // [NT]
    int *tab = (int *)(items + NT);            // [NW][KS]: counts, then list offsets (zeroed by the caller before its barrier)
    int *rs = tab + NW * KS;                   // [P + 1] row starts
    if (!PSG_DIAGBIT(a, 1024)) {
        // 1. rank among the lanes with the same key (key KS = no gradient)
        unsigned long long same = ~0ull;
#pragma unroll
        for (int bit = 0; bit < 6; ++bit) {
            const unsigned long long bb = __ballot((key >> bit) & 1);
            same &= ((key >> bit) & 1) ? bb : ~bb;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        if (key < KS && rank == 0) tab[wave * KS + key] = __popcll(same);
        __syncthreads();
        // 2. row r = g * KS + k (lane r of wave 0): chunks g * cpg .. g * cpg + cpg - 1 hold the channels of group g
        if (wave == 0) {
            const int cpg = a.C3 >> 6, g = lane / KS, k = lane & (KS - 1);
            int tot = 0;
            if (lane < P)
                for (int q = 0; q < cpg; ++q) tot += tab[(g * cpg + q) * KS + k];
            int inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(inc, o);
                if (lane >= o) inc += v;
            }
            int run = inc - tot;
            if (lane < P) {
                rs[lane] = run;
                for (int q = 0; q < cpg; ++q) {
                    int *t = tab + (g * cpg + q) * KS + k;
                    const int c = *t;
                    *t = run;
                    run += c;
                }
            }
            if (lane == 63) rs[P] = inc;   // (lanes >= P count nothing)
        }
        __syncthreads();
        // 3. scatter
        if (key < KS) {
            const int g = tid / a.C3, c = tid - g * a.C3;
            items[tab[wave * KS + key] + rank] = make_int2(((g * KS + key) << 16) | c, __float_as_int(PACKED ? dval : dsrc[tid]));
        }
    }   // (PSG_DIAG bit 1024)
    // mask words of this wave's tiles of dZ2 (layer_bwd's slots), fetched now so that they arrive under the stream
    const int ntask = (C2 / 32) * PB;
    unsigned msk[MAXT];
    if constexpr (!PACKED) {
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            const int task = wave + i * NW;
            msk[i] = 0xFFFFu;
            if (task < ntask && a.l3t.mask && !PSG_DIAGBIT(a, 2048)) msk[i] = a.l3t.mask[(wg * ntask + task) * 64 + lane];
        }
    }
    __syncthreads();
    if (!PSG_DIAGBIT(a, 128 | 1024)) {
        // 4. stream: this wave's rows [r_lo, r_hi) = the rows whose start lies in its share [lo, hi) of the T items
        const int T = __builtin_amdgcn_readfirstlane(rs[P]);
        const int lo = wave * T / NW, hi = (wave + 1) * T / NW;
        const int rsl = lane < P ? rs[lane] : 0x7fffffff;
        const int r_lo = __popcll(__ballot(rsl < lo));
        const int r_hi = wave == NW - 1 ? P : __popcll(__ballot(rsl < hi));
        const int e_lo = __builtin_amdgcn_readfirstlane(rs[r_lo]), e_hi = __builtin_amdgcn_readfirstlane(rs[r_hi]);
        const float *wr = a.w3r + lane * SPV;
        float acc[SPV];
#pragma unroll
        for (int e = 0; e < SPV; ++e) acc[e] = 0.0f;
        int cur = r_lo;
        // PACKED: lane r holds where the batch's row r goes in the packed buffer, -1 for a row at or past its group's count
        // (one LDS look-up per batch; put() then reads it with a scalar lane index, no memory access inside the stream)
        int dstv = -1;
        if constexpr (PACKED) {
            if (lane < P) {
                const int st = gst[lane >> 5], k = lane & 31;
                if (k < gst[(lane >> 5) + 1] - st) dstv = st + k;
            }
            if (lane < KS) tab[wave * KS + lane] = 0;   // this wave's counts for the next batch (its own slice: read above, dead now)
        }
        auto put = [&](int r) {
            if constexpr (PACKED) {
                r = __builtin_amdgcn_readlane(dstv, r);
                if (r < 0) return;   // (no item ever names such a row: acc is still zero)
            }
            float *o = buf0 + L::off(lane * SPV, r);
            if constexpr (SPV == 4) *(float4 *)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else if constexpr (SPV == 2) *(float2 *)o = make_float2(acc[0], acc[1]);
            else *o = acc[0];
#pragma unroll
            for (int e = 0; e < SPV; ++e) acc[e] = 0.0f;
        };
        for (int w0 = e_lo; w0 < e_hi; w0 += 64) {
            const int n = min(64, e_hi - w0);
            const int2 mine = lane < n ? items[w0 + lane] : make_int2(0, 0);
            for (int q = 0; q < n; q += U) {
                VT w[U];
                int xs[U];
                float ds[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    xs[u] = __builtin_amdgcn_readlane(mine.x, q + u);
                    ds[u] = __int_as_float(__builtin_amdgcn_readlane(mine.y, q + u));
                    if (q + u < n) w[u] = *(const VT *)(wr + (size_t)(PSG_DIAGBIT(a, 8192) ? 0 : xs[u] & 0xFFFF) * C2);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (q + u < n) {
                        const int row = xs[u] >> 16;
                        while (cur < row) put(cur++);
                        const float *wv = (const float *)&w[u];
#pragma unroll
                        for (int e = 0; e < SPV; ++e) acc[e] = fmaf(ds[u], wv[e], acc[e]);
                    }
                }
            }
        }
        while (cur < r_hi) put(cur++);
    }   // (PSG_DIAG bits 128, 1024)
    if constexpr (!PACKED) {
        __syncthreads();
        // 5. ReLU mask of layer 2, tile by tile
        const int j = lane & 31, h = lane >> 5;
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            const int task = wave + i * NW;
            if (task < ntask && !PSG_DIAGBIT(a, 2048)) {   // (sa_mask_tile, in place)
                const int mb = task / PB, pb = task - mb * PB;
                float *o = buf0 + (size_t)(mb * 4) * L::BLK + (pb * 32 + j) * 8 + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float4 v = *(float4 *)(o + (size_t)g * L::BLK);
                    v.x = __uint_as_float(__float_as_uint(v.x) & (unsigned)__builtin_amdgcn_sbfe((int)msk[i], 4 * g, 1));
                    v.y = __uint_as_float(__float_as_uint(v.y) & (unsigned)__builtin_amdgcn_sbfe((int)msk[i], 4 * g + 1, 1));
                    v.z = __uint_as_float(__float_as_uint(v.z) & (unsigned)__builtin_amdgcn_sbfe((int)msk[i], 4 * g + 2, 1));
                    v.w = __uint_as_float(__float_as_uint(v.w) & (unsigned)__builtin_amdgcn_sbfe((int)msk[i], 4 * g + 3, 1));
                    *(float4 *)(o + (size_t)g * L::BLK) = v;
                }
            }
        }
    }
}

// level 3's pooled-output gradient (sa_bwd_body's nninv gather for one (group, channel), the same chain): dout[s][c] = sum over
// the fine points whose 3-NN lists contain s of w * dint[p][c], in list order
__device__ __forceinline__ float sa_nninv_grad(const SaBwdArgs &a, int b, int s, int c)
{
    const int32_t *off = a.nninv_off + (size_t)b * (a.S + 1) + s;
    const int2 *ent = a.nninv_ent + (size_t)b * 3 * a.n_fine;
    const float *drows = a.dint + (size_t)b * a.n_fine * a.ld + a.c_off + c;
    const int e1 = off[1];
    int e = off[0];
    float acc = 0.0f;
    for (; e + 4 <= e1; e += 4) {
        const int2 p0 = ent[e], p1 = ent[e + 1], p2 = ent[e + 2], p3 = ent[e + 3];
        const float v0 = drows[(size_t)p0.x * a.ld], v1 = drows[(size_t)p1.x * a.ld], v2 = drows[(size_t)p2.x * a.ld],
                    v3 = drows[(size_t)p3.x * a.ld];
        acc += __int_as_float(p0.y) * v0; acc += __int_as_float(p1.y) * v1;
        acc += __int_as_float(p2.y) * v2; acc += __int_as_float(p3.y) * v3;
    }
    for (; e < e1; ++e) {
        const int2 pe = ent[e];
        acc += __int_as_float(pe.y) * drows[(size_t)pe.x * a.ld];
    }
    return acc;
}

// SPV > 0: the max-pool transpose runs as the sparse stream above (sa_pool_t_sparse) instead of dZ3 in LDS + the dense l3t
// (the kernels sa_bwd_kernel / sa_bwd_sparse_kernel below)
// KEYED (sa_bwd_packed_kernel, a workgroup of full groups): the workgroup (kbx, kb) with its ReLU masks at the slots of workgroup kwg
template <int P, int NW, int MAXT, int KS, int SPV, bool KEYED = false>
__device__ __forceinline__ void sa_bwd_body(const SaBwdArgs &a, int kbx = 0, int kb = 0, size_t kwg = 0)
{
    using L = Lds<P>;
    static_assert(KS == 32 || KS == 16, "groups of 32 or 16 samples");
    constexpr bool SPARSE = SPV > 0;
    static_assert(!SPARSE || KS == 32, "sparse max-pool transpose: groups of 32 samples");
    constexpr int G = P / KS, NT = NW * 64;
    extern __shared__ float lds[];
    float *buf0 = lds;   // the one activation buffer (layers run in place)
    const int tid = threadIdx.x;
    int bx, b;
    if constexpr (KEYED) { bx = kbx; b = kb; }
    else xcd_tile(bx, b);
    const int s0 = bx * G;
    const size_t wg = KEYED ? kwg : (size_t)b * gridDim.x + bx;

    // gradient of the pooled output: read directly, or gathered (no atomics, fixed summation order) from the
    // interpolated-part rows of the feature-propagation module that upsampled this level
    // arg-max bytes of this workgroup's groups: issued first, so their latency overlaps the gradient gather below
    const int nblk = a.C3 >> 3;
    constexpr int NTASK = 4;   // (point, 8-channel block) tasks per thread: P * C3 / 8 / NT = 4 for every SSG level (<= 4 for MSG)
    uint2 am_pre[NTASK];
    int key = KS;   // sparse: the arg-max sample of channel slot tid of the G groups (KS = no gradient)
    if constexpr (SPARSE) {
        if (tid < G * a.C3) {
            const int v = a.arg[((size_t)b * a.S + s0) * a.C3 + tid];
            key = v == 255 ? KS : v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NTASK; ++i) {
            const int t = tid + i * NT;
            am_pre[i] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
            if (t < P * nblk && !PSG_DIAGBIT(a, 1)) {
                const int pnt = t % P, blk = t / P;
                am_pre[i] = *(const uint2 *)(a.arg + ((size_t)b * a.S + s0 + pnt / KS) * a.C3 + blk * 8);
            }
        }
    }
    // dout[s][c] = skip-link gradient (plain rows) + transposed 3-NN interpolation + transposed grouping of the
    // next level, every sum in a fixed order (ascending fine point / grouped row)
    float *dsrc = lds + (size_t)a.dsrc_blk * L::BLK;   // staging block(s) behind the activation buffer
    if (SPARSE && tid < NW * KS) ((int *)(dsrc + a.sp_off) + 2 * NT)[tid] = 0;   // sa_pool_t_sparse's count table
    // the rows' slots in the consumer's lists: read now (one coalesced load), used after the last layer - fetched there they
    // were a cache-line miss at the tail of every workgroup
    int32_t *s_pos = (int32_t *)(dsrc + a.pos_off);
    if (!a.w1c && tid < P) s_pos[tid] = a.gpos_out[(size_t)b * a.S * KS + (size_t)s0 * KS + tid];   // (the colour path reads its one slot per lane itself)
    if (a.w1c && tid < 3 * a.C1) {   // table [half][column][C1 / 2] of the wanted columns (read after the barriers of the layers below)
        const int kh = a.C1 >> 1, hh = tid / (3 * kh), r = (tid / kh) % 3, cc = tid % kh;
        dsrc[a.w1c_off + tid] = a.w1c[(hh * kh + cc) * a.D + a.c_lo + r];
    }
    for (int t = tid; t < G * a.C3; t += NT) {
        const int g = t / a.C3, c = t - g * a.C3;
        if (PSG_DIAGBIT(a, 4096)) { dsrc[t] = 0.0f; continue; }   // (timing diagnosis: no pooled-gradient prologue)
        const int cc = a.c_off + c;
        float acc = a.dout ? a.dout[((size_t)b * a.S + s0 + g) * a.ld + cc] : 0.0f;
        if (a.nninv_off) {
            const int32_t *off = a.nninv_off + (size_t)b * (a.S + 1) + s0 + g;
            const int2 *ent = a.nninv_ent + (size_t)b * 3 * a.n_fine;
            const float *drows = a.dint + (size_t)b * a.n_fine * a.ld + cc;
            const int e1 = off[1];
            int e = off[0];
            for (; e + 4 <= e1; e += 4) {   // four entries and their rows in flight; added in list order
                const int2 p0 = ent[e], p1 = ent[e + 1], p2 = ent[e + 2], p3 = ent[e + 3];
                const float v0 = drows[(size_t)p0.x * a.ld], v1 = drows[(size_t)p1.x * a.ld], v2 = drows[(size_t)p2.x * a.ld],
                            v3 = drows[(size_t)p3.x * a.ld];
                acc += __int_as_float(p0.y) * v0; acc += __int_as_float(p1.y) * v1;
                acc += __int_as_float(p2.y) * v2; acc += __int_as_float(p3.y) * v3;
            }
            for (; e < e1; ++e) {
                const int2 pe = ent[e];
                acc += __int_as_float(pe.y) * drows[(size_t)pe.x * a.ld];
            }
        }
        if (a.ginv_off) {
            // the producer stored its rows in list order: the rows of point s are contiguous, ascending grouped row
            const int32_t *off = a.ginv_off + (size_t)b * (a.S + 1) + s0 + g;
            const float *rows = a.gsa + (size_t)b * a.g_rows * a.ld + cc;
            const int e1 = off[1];
            for (int e = off[0]; e < e1; e += 8) {   // absent entries add +0.0f: still the ascending chain
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = e + u < e1 ? rows[(size_t)(e + u) * a.ld] : 0.0f;
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
        }
        if (a.ginv_off2) {   // second scale of the next (MSG) level, same scheme
            const int32_t *off = a.ginv_off2 + (size_t)b * (a.S + 1) + s0 + g;
            const float *rows = a.gsa2 + (size_t)b * a.g_rows2 * a.ld + cc;
            const int e1 = off[1];
            for (int e = off[0]; e < e1; e += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = e + u < e1 ? rows[(size_t)(e + u) * a.ld] : 0.0f;
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
        }
        dsrc[t] = acc;
    }
    __syncthreads();
    if constexpr (SPARSE) {
        if (!PSG_DIAGBIT(a, 8)) sa_pool_t_sparse<P, NW, MAXT, SPV>(a, buf0, dsrc, key, wg);
    } else {
        // max-pool backward: dZ3[c][g*32+k] = dout[g][c] if k == arg[g][c] else 0.
        // One (point, 8-channel block) per thread; arg/dout reads are broadcasts across the 32 samples.
#pragma unroll
        for (int i = 0; i < NTASK; ++i) {
            const int t = tid + i * NT;
            if (t >= P * nblk || PSG_DIAGBIT(a, 1)) break;
            const int pnt = t % P, blk = t / P;
            const int g = pnt / KS, k = pnt & (KS - 1);
            const uint2 am = am_pre[i];
            const float *dp = dsrc + (size_t)g * a.C3 + blk * 8;
            const float4 d0 = *(const float4 *)dp, d1 = *(const float4 *)(dp + 4);
            float4 v0, v1;
            v0.x = (int)(am.x & 0xFF) == k ? d0.x : 0.f;
            v0.y = (int)((am.x >> 8) & 0xFF) == k ? d0.y : 0.f;
            v0.z = (int)((am.x >> 16) & 0xFF) == k ? d0.z : 0.f;
            v0.w = (int)(am.x >> 24) == k ? d0.w : 0.f;
            v1.x = (int)(am.y & 0xFF) == k ? d1.x : 0.f;
            v1.y = (int)((am.y >> 8) & 0xFF) == k ? d1.y : 0.f;
            v1.z = (int)((am.y >> 16) & 0xFF) == k ? d1.z : 0.f;
            v1.w = (int)(am.y >> 24) == k ? d1.w : 0.f;
            float *dst = buf0 + (size_t)blk * L::BLK + pnt * 8;
            *(float4 *)dst = v0;
            *(float4 *)(dst + 4) = v1;
        }
        __syncthreads();
        if (!PSG_DIAGBIT(a, 8)) layer_bwd<P, NW, MAXT>(a.l3t, buf0, wg);
    }
    if (!PSG_DIAGBIT(a, 16)) __syncthreads();
    if (!PSG_DIAGBIT(a, 8 | 2048)) layer_bwd<P, NW, MAXT>(a.l2t, buf0, wg);
    if (!PSG_DIAGBIT(a, 16)) __syncthreads();
    if constexpr (P == 32 * NW) {
        if (a.w1c) {   // colour-only request at level 0: three columns of the first layer on the vector pipe (sa_l1t_colour)
            float *orowc = a.gsa_out + (size_t)b * a.S * KS * 4;
            const int32_t *posc = a.gpos_out + (size_t)b * a.S * KS + (size_t)s0 * KS;
            if (a.C1 == 32) sa_l1t_colour<P, NW, 32>(a, buf0, dsrc + a.w1c_off, posc, orowc);
            else sa_l1t_colour<P, NW, 16>(a, buf0, dsrc + a.w1c_off, posc, orowc);
            return;
        }
    }
    if (!a.split) {   // (split: the rows stored below are dZ1 itself; W1f^T is applied per point by pw_bwd_kernel)
        if (!PSG_DIAGBIT(a, 8)) layer_bwd<P, NW, MAXT>(a.l1t, buf0, wg);
        __syncthreads();
    }
    if (PSG_DIAGBIT(a, 32)) return;
    // index_points backward (pointnet_util.py:119,131): the feature rows [c_lo, c_hi) of the grouped-input gradient
    // are stored as plain rows; the consumer (previous level's sa_bwd, or dx0_gather_kernel) sums them through the
    // inverse group lists.  (LDS channel order is [feats, rel_xyz]: LDS channel c is feature channel c.)
    const int nc = a.c_hi - a.c_lo;
    const int32_t *pos = s_pos;
    float *orow = a.gsa_out + (size_t)b * a.S * KS * a.cg_out;
    if (a.cg_out == 4) {   // colour-only request of the attack loop: one 16-byte row {c_lo, c_lo+1, c_lo+2, 0} per lane
        for (int j = tid; j < P; j += NT) {
            const float4 v = make_float4(buf0[L::off(a.c_lo, j)], buf0[L::off(a.c_lo + 1, j)], buf0[L::off(a.c_lo + 2, j)], 0.0f);
            if (pos[j] >= 0) *(float4 *)(orow + (size_t)pos[j] * 4) = v;   // padding rows (always zero) are not listed
        }
        return;
    }
    if (((nc | a.c_lo | a.cg_out) & 3) == 0) {
        // 16 bytes per thread, 32 lanes per row (see fp_bwd_kernel: the element-wise loop below costs a run-time division,
        // a 4-byte LDS read and a 4-byte store per element, 16 rounds per thread at levels 1-3)
        constexpr int RG = NT / 32;
        const int ql = tid & 31, rg = tid >> 5;
        for (int j = rg; j < P; j += RG) {
            const int pj = pos[j];
            if (pj < 0) continue;                                                   // padding rows are not listed
            float *o = orow + (size_t)pj * a.cg_out + a.c_lo;
            for (int q = ql; q < (nc >> 2); q += 32) *(float4 *)(o + 4 * q) = *(const float4 *)(buf0 + L::off(a.c_lo + 4 * q, j));
        }
        return;
    }
    for (int t = tid; t < P * nc; t += NT) {
        const int j = t / nc, c = a.c_lo + (t - j * nc);
        if (pos[j] >= 0) orow[(size_t)pos[j] * a.cg_out + c] = buf0[L::off(c, j)];   // padding rows are not listed
    }
}

template <int P, int NW, int MAXT, int KS = 32>
__global__ __launch_bounds__(NW * 64) void sa_bwd_kernel(SaBwdArgs a) { sa_bwd_body<P, NW, MAXT, KS, 0>(a); }

// SSG levels 1 - 3 with the sparse max-pool transpose (run_sa_bwd: PSG_PN2_POOLT_SPARSE); SPV = C2 / 64
template <int P, int NW, int MAXT, int SPV>
__global__ __launch_bounds__(NW * 64) void sa_bwd_sparse_kernel(SaBwdArgs a) { sa_bwd_body<P, NW, MAXT, 32, SPV>(a); }

// ------------------------------------------------------------------------------------------ SA bwd, packed
// The backward of a level whose forward ran packed (sa_fwd_packed_kernel<.., PKM>), over the same packed rows through the same
// descriptors: a padding row's gradient is exactly zero before any mask is applied and is never stored (gpos_out = -1), so
// the transposed layers run over the workgroup's nblk = ceil(nrows / 32) active blocks only.  Launched on the unpacked grid
// (fixed launch shape, nothing read back); a surplus workgroup returns on its zero descriptor.
//   * masks: read at the packed key ((wg * L.mb + mb) * PB + pb) * 64 + lane, where the packed forward stored them;
//   * tile columns are independent and every valid row passes through the k-loops and epilogues it had unpacked: the rows
//     stored are the same bytes as sa_bwd_kernel's;
//   * a workgroup of P / 32 full groups on an unpacked boundary runs sa_bwd_body with that origin and its own mask key, at
//     sa_bwd_kernel's cost (rooms with nothing to skip); an unaligned one takes the packed path with nrows == P;
//   * stores go to gsa_out through gpos_out[group * 32 + sample], looked up through the row map: the consumers see the
//     layout they always saw.
// SPV = 0 (dense max-pool transpose, SSG level 0): the pooled-output gradient of that level arrives as plain
// rows (a.dout = the per-point sums of the split level above: run_sa_bwd checks), so dZ3 is built per (packed row, 8-channel
// block) straight from those rows and the arg-max bytes - the loads sa_bwd_kernel issues per (row, block), without its
// staging pass.  LDS: sa_bwd_kernel's of the level plus the row map [P] in its staging block (the same number of blocks).
template <int P, int NW, int MAXT>
__device__ __forceinline__ void sa_layer_bwd_packed(const BwdLayer &L, float *__restrict__ buf, int nblk, size_t wg)
{
    constexpr int PB = P / 32, BLK = Lds<P>::BLK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int ntask = L.mb * nblk;
    const int first = (wave + (int)(wg & (NW - 1))) & (NW - 1);
    f32x16 acc[MAXT];
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        const int task = first + i * NW;
        if (task < ntask) {
            const int mb = task / nblk, pb = task - mb * nblk;
            unsigned m = 0xFFFFu;
            if (L.mask) m = L.mask[((wg * L.mb + mb) * PB + pb) * 64 + lane];
            f32x16 c;
#pragma unroll
            for (int r = 0; r < 16; ++r) c[r] = 0.0f;
            c = tile_mac<BLK, false>(L.w + (size_t)mb * L.k8 * 64 + lane, L.k8, buf + (pb * 32 + j) * 8 + 4 * h, c);
            apply_bits(c, m);
            acc[i] = c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        const int task = first + i * NW;
        if (task < ntask) {
            const int mb = task / nblk, pb = task - mb * nblk;
            store_tile<P>(buf, mb, pb * 32 + j, h, acc[i]);
        }
    }
}

// The sparse levels (SPV > 0: SSG levels 1 - 3, split, the rows stored are dZ1).  The max-pool transpose stays the sparse stream
// of sa_pool_t_sparse - per (row, column) one fmaf chain from 0 over the row's items in ascending channel order, which the
// dense transposed layer does not reproduce bit for bit - so the items are NOT packed: the workgroup's ng groups pass through
// the stream in batches of G = P / 32 groups (G * C3 = NT: a batch is exactly the pass of one unpacked workgroup, thread tid =
// channel tid of the batch's groups, the same key and gradient per thread, the same lists), and only where a finished row
// goes changes: batch row g * 32 + k to packed row gstart[g0 + g] + k.  What shrinks is behind the stream: the mask pass, l2t
// and the stores run once over the nblk active blocks of ng groups, and there are ng / G times fewer workgroup lifetimes.
//   * every valid row is written exactly once, zero rows included: the waves' row ranges [r_lo, r_hi) partition the batch's P
//     rows, and put() stores each row below its group's count; rows at or past the count are never named by an item (the
//     packed forward's scan returns bi < n, the in-register pool of a full group any of its 32 rows), so nothing is dropped;
//   * a batch without a live item (T = 0): lo = hi = 0 in every wave, r_lo = 0, r_hi = 0 but for the last wave, which owns
//     all P rows with e_lo = e_hi = rs[0] = rs[P] = 0 - the item loop does not run and put() zero-fills the batch's rows;
//   * a last batch of fewer than G groups: the threads of the missing groups hold key KS (no item), and gstart[ng ..] = nrows
//     gives their rows the count 0;
//   * three barriers per batch (after the counts, the scan and the scatter).  A wave zeroes ITS slice of the count table
//     behind the scatter's barrier and writes only that slice in the next batch's step 1, so a wave that has finished its
//     stream goes straight on to the next batch's ranks; the row starts and the item list are rewritten only behind the
//     counts' barrier, which every wave reaches after its stream.  The rows of different batches are disjoint: the buffer
//     needs no barrier between them;
//   * the mask word of this wave's tile is loaded before the first batch.  Loading batch i + 1's arg-max bytes and gradient
//     values before batch i's list build was tried and dropped: 100.4 against 100.7 us per level-1 launch, inside the 0.2 %
//     two traces of one library differ by.
// LDS: the staging of sa_bwd_sparse_kernel (its dsrc slots stay unused: a thread's gradient value stays in its register) and
// gstart [SA_PACK_GCAP + 1] behind the row starts - the same number of blocks at all three levels (run_sa_bwd).
template <int P, int NW, int SPV>
__device__ __forceinline__ void sa_bwd_packed_sparse(const SaBwdArgs &a, float *__restrict__ buf0, float *__restrict__ dsrc,
                                                     const int4 &desc, int b, size_t wg, int nrows)
{
    using L = Lds<P>;
    constexpr int G = P / 32, PB = P / 32, NT = NW * 64, KS = 32, C2 = 64 * SPV, GCAP = SA_PACK_GCAP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ng = desc.x >> 16, sA = desc.x & 0xFFFF;
    const int nblk = (nrows + 31) >> 5;
    int *tab = (int *)(dsrc + a.sp_off) + 2 * NT;               // sa_pool_t_sparse's count table [NW][32], row starts [P + 1]
    int *gstart = tab + NW * KS + P + 1;                        // [GCAP + 1] first packed row of each group; nrows from ng on
    {
        int st = 0;
        for (int i = 0; i < ng; ++i) {                          // (uniform)
            if (tid == i) gstart[i] = st;
            st += sa_pack_cnt(desc, i);
        }
        if (tid >= ng && tid <= GCAP) gstart[tid] = nrows;
    }
    // the tail of the last block: zeroed once (no batch writes it)
    for (int t = tid; t < (nblk * 32 - nrows) * (C2 / 4); t += NT) {
        const int r = nrows + t / (C2 / 4), q = t % (C2 / 4);
        *(float4 *)(buf0 + L::off(4 * q, r)) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // layer 2's ReLU mask word of this wave's tile (mb, pb) of dZ2, at the packed key the forward stored it at
    const int mb = wave / nblk, pb = wave - mb * nblk;
    const bool mtile = wave < (C2 / 32) * nblk;
    unsigned msk = 0xFFFFu;
    if (mtile && a.l3t.mask) msk = a.l3t.mask[((wg * (C2 / 32) + mb) * PB + pb) * 64 + lane];
    // thread tid = channel c of group gl of a batch (G * C3 == NT: run_sa_bwd checks)
    const int gl = tid / a.C3, c = tid - gl * a.C3;
    const uint8_t *arow = a.arg + ((size_t)b * a.S + sA) * a.C3 + c;
    const bool plain = !a.nninv_off;                            // (plain rows, or level 3's gather: uniform)
    const float *drow = plain ? a.dout + ((size_t)b * a.S + sA) * a.ld + a.c_off + c : nullptr;
    if (tid < NW * KS) tab[tid] = 0;
    __syncthreads();
    for (int g0 = 0; g0 < ng; g0 += G) {
        int key = KS;   // the arg-max sample of channel c of group g0 + gl (KS = no gradient, or no such group) and its gradient
        float dv = 0.0f;
        if (g0 + gl < ng) {
            const int v = arow[(size_t)(g0 + gl) * a.C3];
            key = v == 255 ? KS : v;
            dv = plain ? drow[(size_t)(g0 + gl) * a.ld] : sa_nninv_grad(a, b, sA + g0 + gl, c);
        }
        sa_pool_t_sparse<P, NW, 1, SPV, true>(a, buf0, dsrc, key, wg, gstart + g0, dv);
    }
    __syncthreads();
    if (mtile) sa_mask_tile<P>(buf0, mb, pb, lane & 31, lane >> 5, msk);
    __syncthreads();
}

// The same transpose in CHANNEL order (round 27; PSG_PN2_POOLT_ORDER=row keeps the batches above).  A packed workgroup holds at
// most P live rows, so one accumulator per (live row, column) fits in registers and the pass can walk the channels once for
// all of the workgroup's groups: no item list (ballots, scan, scatter), no batches, no barrier per batch, and W3 is read once
// per wave, in address order, instead of once per group as a gather.
//   * the waves are dealt as (64-column slice of C2) x (range of groups): wave = range slot * SPV + slice.  The ranges are cut
//     from the workgroup's groups in order, a new one after per = ceil(ng / NR) groups (NR = NW / SPV range slots) or where the
//     next group would take the range past 32 rows; range i goes to slot i % NR.  Every group lies in exactly one range, a
//     range holds at most 32 rows = the 32 accumulators of a lane (acc[r] = packed row row0 + r, column slice * 64 + lane),
//     and a slot that is dealt more than one range (many small groups behind two large ones) runs them one after another;
//   * a wave walks its range CH = 8 channels at a time: the 8 weight rows W3[c][slice] of the NEXT chunk are loaded while this
//     one is summed (16 at a time cost 102 - 104 VGPRs, a wave per SIMD fewer than the batches run at); lane (q, u) holds the
//     item of the q-th group of a set of 8 of the range at channel 8 * chunk + u, as {accumulator index or -1, pooled
//     gradient}, read straight from the arg-max bytes and the pooled-gradient rows, also one chunk ahead; the items are
//     broadcast with v_readlane at constant lanes and acc[index] is updated at the wave-uniform index; an item without a row (arg-max 255, or a sample at or past the group's count) is
//     skipped by a uniform branch;
//   * per (row, column) this is sa_pool_t_sparse's chain: fmaf from 0 over the row's items in ascending channel order - a row
//     belongs to one group, a group to one range, and within a range the order is (chunk, set, group, channel): for one
//     group, ascending channels.  Rows without items store the zeros they started from.  The bytes do not change;
//   * every live row is stored exactly once (the ranges partition the groups, a range stores rows [row0, row0 + rows)); the
//     tail of the last 32-row block is zero-filled as before; one barrier, then the mask pass.
// Levels 1 and 2 (C2 = 64 / 128, the pooled gradient as plain rows).  Level 3 keeps the batches: its channel-ordered kernel (the
// nninv sums staged once per workgroup, four column slices) took 129 us per launch against 99 us unpacked and 122 us in batches
//  - every slice pays the per-item chain again and the level has too few workgroups to hide it.
// LDS: gstart [SA_PACK_GCAP + 1] at sp_off (inside the staging the batches use).
template <int P, int NW, int SPV>
__device__ __forceinline__ void sa_bwd_packed_chan(const SaBwdArgs &a, float *__restrict__ buf0, float *__restrict__ dsrc,
                                                   const int4 &desc, int b, size_t wg, int nrows)
{
    using L = Lds<P>;
    constexpr int PB = P / 32, NT = NW * 64, C2 = 64 * SPV, GCAP = SA_PACK_GCAP, NR = NW / SPV, CH = 8, GQ = 64 / CH;
    static_assert(NW % SPV == 0 && NR >= 1, "whole range slots");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ng = desc.x >> 16, sA = desc.x & 0xFFFF;
    const int nblk = (nrows + 31) >> 5;
    int *gstart = (int *)(dsrc + a.sp_off);                     // [GCAP + 1] first packed row of each group; nrows from ng on
    {
        int st = 0;
        for (int i = 0; i < ng; ++i) {                          // (uniform)
            if (tid == i) gstart[i] = st;
            st += sa_pack_cnt(desc, i);
        }
        if (tid >= ng && tid <= GCAP) gstart[tid] = nrows;
    }
    // the tail of the last block: zeroed once (no range writes it)
    for (int t = tid; t < (nblk * 32 - nrows) * (C2 / 4); t += NT) {
        const int r = nrows + t / (C2 / 4), q = t % (C2 / 4);
        *(float4 *)(buf0 + L::off(4 * q, r)) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // layer 2's ReLU mask word of this wave's tile (mb, pb) of dZ2, at the packed key the forward stored it at
    const int mb = wave / nblk, pb = wave - mb * nblk;
    const bool mtile = wave < (C2 / 32) * nblk;
    unsigned msk = 0xFFFFu;
    if (mtile && a.l3t.mask) msk = a.l3t.mask[((wg * (C2 / 32) + mb) * PB + pb) * 64 + lane];
    __syncthreads();
    if (!PSG_DIAGBIT(a, 128 | 1024)) {
        const int slice = wave % SPV, slot = wave / SPV;
        // W3 through a buffer descriptor: one vector offset (the lane's column), the row as the scalar offset
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void *)a.w3r, 0, a.C3 * C2 * 4, 0x00020000);
        const unsigned coff = (slice * 64 + lane) * 4u;
        const uint8_t *arow = a.arg + ((size_t)b * a.S + sA) * a.C3;
        const float *drow = a.dout + ((size_t)b * a.S + sA) * a.ld + a.c_off;   // (plain rows: run_sa_bwd checks)
        const int per = (ng + NR - 1) / NR, nch = a.C3 / CH;
        const int lq = lane / CH, lu = lane % CH;
        int ga = 0, row0 = 0, rows = 0, rid = 0;
        for (int i = 0; i <= ng; ++i) {                         // (uniform; the counts from the table: gstart[ng] = nrows)
            const int cnt = i < ng ? __builtin_amdgcn_readfirstlane(gstart[i + 1] - gstart[i]) : 0;
            if (i > ga && (i == ng || i - ga == per || rows + cnt > 32)) {   // groups [ga, i) are range rid, rows [row0, row0 + rows)
                if (rid % NR == slot) {
                    const int gb = i, nset = (gb - ga + GQ - 1) / GQ;
                    float acc[32];
#pragma unroll
                    for (int r = 0; r < 32; ++r) acc[r] = 0.0f;
                    // lane (lq, lu) holds the item of group ga + GQ * j + lq (set j) at channel k * CH + lu: its arg-max byte and
                    // gradient are loaded a chunk ahead and turned into {accumulator index or -1, gradient} where they are used
                    auto raw = [&](int k, int j, int &v, float &dv) {
                        const int g = ga + GQ * j + lq, c = k * CH + lu;
                        v = 255;
                        dv = 0.0f;
                        if (g < gb) {
                            v = arow[(size_t)g * a.C3 + c];
                            dv = drow[(size_t)g * a.ld + c];
                        }
                    };
                    auto base = [&](int j, int &st, int &cn) {   // the group's first accumulator and its count (0: no such group)
                        const int g = ga + GQ * j + lq;
                        st = 0;
                        cn = 0;
                        if (g < gb) {
                            const int s0 = gstart[g];
                            cn = gstart[g + 1] - s0;
                            st = s0 - row0;
                        }
                    };
                    int st0, cn0, vn;
                    float wn[CH], dvn;
                    base(0, st0, cn0);
#pragma unroll
                    for (int u = 0; u < CH; ++u) wn[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rw, coff, u * C2 * 4, 0));
                    raw(0, 0, vn, dvn);
                    for (int k = 0; k < nch; ++k) {
                        float w[CH], dv = dvn;
                        int v = vn, st = st0, cn = cn0;
#pragma unroll
                        for (int u = 0; u < CH; ++u) w[u] = wn[u];
                        if (k + 1 < nch) {
                            const int r1 = PSG_DIAGBIT(a, 8192) ? 0 : (k + 1) * CH;
#pragma unroll
                            for (int u = 0; u < CH; ++u) wn[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rw, coff, (r1 + u) * C2 * 4, 0));
                            raw(k + 1, 0, vn, dvn);
                        }
                        for (int j = 0; j < nset; ++j) {
                            if (j > 0) {
                                raw(k, j, v, dv);
                                base(j, st, cn);
                            }
                            const int dl = v < cn ? st + v : -1;   // (255 = no gradient: below no count)
#pragma unroll
                            for (int q = 0; q < GQ; ++q) {
                                if (ga + GQ * j + q < gb) {
#pragma unroll
                                    for (int u = 0; u < CH; ++u) {
                                        const int xs = __builtin_amdgcn_readlane(dl, q * CH + u);
                                        if (xs >= 0) {
                                            const float ds = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dv), q * CH + u));
                                            acc[xs] = fmaf(ds, w[u], acc[xs]);
                                        }
                                    }
                                }
                            }
                        }
                    }
                    float *o = buf0 + L::off(slice * 64 + lane, row0);
#pragma unroll
                    for (int r = 0; r < 32; ++r)
                        if (r < rows) o[r * 8] = acc[r];
                }
                ++rid;
                row0 += rows;
                rows = 0;
                ga = i;
            }
            rows += cnt;
        }
    }   // (PSG_DIAG bits 128, 1024)
    __syncthreads();
    if (mtile) sa_mask_tile<P>(buf0, mb, pb, lane & 31, lane >> 5, msk);
    __syncthreads();
}

// SPVO = SPV, plus SA_PACK_CHAN where the sparse max-pool transpose runs in channel order (sa_bwd_packed_chan: levels 1 and 2)
template <int P, int NW, int MAXT, int SPVO>
__global__ __launch_bounds__(NW * 64) void sa_bwd_packed_kernel(SaBwdPackedArgs pa)
{
    constexpr int SPV = SPVO & (SA_PACK_CHAN - 1);
    constexpr bool CHAN = SPVO >= SA_PACK_CHAN;
    const SaBwdArgs &a = pa.a;
    using L = Lds<P>;
    static_assert(MAXT == 1 && (SPV > 0 ? P <= 64 : P == 32 * NW), "one tile per wave in every layer");
    constexpr int PB = P / 32, NT = NW * 64, KS = 32;
    extern __shared__ float lds[];
    float *buf0 = lds;
    const int tid = threadIdx.x, wave = tid >> 6;
    int bx, b;
    xcd_tile(bx, b);
    const size_t wg = (size_t)b * gridDim.x + bx;
    const int4 desc = pa.pk_desc[wg];
    const int ng = desc.x >> 16, sA = desc.x & 0xFFFF;
    if (ng == 0) return;                                        // surplus workgroup (uniform: no barrier has been reached)
    // packed row tid lies in group rg_g, which starts at packed row rg_st (a uniform walk over the descriptor's counts: the
    // per-lane search of the forward would index the descriptor by lane)
    int nrows = 0, rg_g = 0, rg_st = 0;
    for (int i = 0; i < ng; ++i) {
        if (tid >= nrows) { rg_g = i; rg_st = nrows; }
        nrows += sa_pack_cnt(desc, i);
    }
    if (ng == PB && (sA & (PB - 1)) == 0 && nrows == P) {       // nothing to skip: sa_bwd_kernel's body, masks at this key
        // (the sparse levels: the two tiles a wave may hold in sa_bwd_sparse_kernel, so that the body is the one that kernel runs)
        sa_bwd_body<P, NW, (SPV > 0 ? 2 : MAXT), KS, SPV, true>(a, sA / PB, b, wg);
        return;
    }
    const int nblk = (nrows + 31) >> 5, nact = nblk * 32;
    float *dsrc = lds + (size_t)a.dsrc_blk * L::BLK;
    int32_t *s_pos = (int32_t *)(dsrc + a.pos_off);             // [P] output slot of a packed row, -1 = padding or tail
    if constexpr (SPV > 0) {
        // the sparse levels: dZ2 of the packed rows by batches of the sparse stream, masked (ends behind a barrier)
        if (tid < P) s_pos[tid] = tid < nrows ? a.gpos_out[(size_t)b * a.S * KS + (size_t)(sA + rg_g) * KS + tid - rg_st] : -1;
        if constexpr (CHAN) sa_bwd_packed_chan<P, NW, SPV>(a, buf0, dsrc, desc, b, wg, nrows);
        else sa_bwd_packed_sparse<P, NW, SPV>(a, buf0, dsrc, desc, b, wg, nrows);
    } else {
        int *s_row = s_pos + P;                                     // [P] local group << 5 | sample of a packed row, -1 = tail
        if (tid < P) {
            int om = -1, pj = -1;
            if (tid < nrows) {
                const int k = tid - rg_st;
                om = (rg_g << 5) | k;
                pj = a.gpos_out[(size_t)b * a.S * KS + (size_t)(sA + rg_g) * KS + k];
            }
            s_row[tid] = om;
            s_pos[tid] = pj;
        }
        if (a.w1c && tid < 3 * a.C1) {   // sa_bwd_body's table [half][column][C1 / 2] of the wanted columns
            const int kh = a.C1 >> 1, hh = tid / (3 * kh), r = (tid / kh) % 3, cc = tid % kh;
            dsrc[a.w1c_off + tid] = a.w1c[(hh * kh + cc) * a.D + a.c_lo + r];
        }
        __syncthreads();
        // max-pool backward over the active blocks: dZ3[c][row] = dout[group][c] if sample == arg[group][c] else 0; a half-wave
        // takes (8-channel block, 32-row block) q = blk * nblk + pb, nblk rounds for every thread
        {
            const float *drows = a.dout + (size_t)b * a.S * a.ld + a.c_off;
            const uint8_t *arows = a.arg + (size_t)b * a.S * a.C3;
            const int nq = nblk * (a.C3 >> 3);
            const int rcp = (65536 + nblk - 1) / nblk;              // q / nblk = q * rcp >> 16 (q < 2^9, nblk <= P / 32)
#pragma unroll
            for (int i = 0; i < 4; ++i) {                           // (P * C3 / 8 tasks at most: four per thread, run_sa_bwd checks)
                const int q = (tid >> 5) + i * (NT / 32);
                if (q < nq) {
                    const int blk = (q * rcp) >> 16, pb = q - blk * nblk, j = pb * 32 + (tid & 31);
                    const int om = s_row[j];
                    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
                    if (om >= 0) {
                        const int s = sA + (om >> 5), k = om & 31;
                        const uint2 am = *(const uint2 *)(arows + (size_t)s * a.C3 + blk * 8);
                        const float *dp = drows + (size_t)s * a.ld + blk * 8;
                        const float4 d0 = *(const float4 *)dp, d1 = *(const float4 *)(dp + 4);
                        v0.x = (int)(am.x & 0xFF) == k ? d0.x : 0.f;
                        v0.y = (int)((am.x >> 8) & 0xFF) == k ? d0.y : 0.f;
                        v0.z = (int)((am.x >> 16) & 0xFF) == k ? d0.z : 0.f;
                        v0.w = (int)(am.x >> 24) == k ? d0.w : 0.f;
                        v1.x = (int)(am.y & 0xFF) == k ? d1.x : 0.f;
                        v1.y = (int)((am.y >> 8) & 0xFF) == k ? d1.y : 0.f;
                        v1.z = (int)((am.y >> 16) & 0xFF) == k ? d1.z : 0.f;
                        v1.w = (int)(am.y >> 24) == k ? d1.w : 0.f;
                    }
                    float *dst = buf0 + (size_t)blk * L::BLK + j * 8;
                    *(float4 *)dst = v0;
                    *(float4 *)(dst + 4) = v1;
                }
            }
        }
        __syncthreads();
        sa_layer_bwd_packed<P, NW, MAXT>(a.l3t, buf0, nblk, wg);
        __syncthreads();
    }
    sa_layer_bwd_packed<P, NW, MAXT>(a.l2t, buf0, nblk, wg);
    __syncthreads();
    if constexpr (SPV == 0) {   // (the sparse levels are split and store dZ1: run_sa_bwd checks)
        if (a.w1c) {   // colour-only request: wave w takes block w (sa_l1t_colour), its slots from the row map
            if (wave < nblk) {
                float *orowc = a.gsa_out + (size_t)b * a.S * KS * 4;
                if (a.C1 == 32) sa_l1t_colour<P, NW, 32>(a, buf0, dsrc + a.w1c_off, s_pos, orowc);
                else sa_l1t_colour<P, NW, 16>(a, buf0, dsrc + a.w1c_off, s_pos, orowc);
            }
            return;
        }
        if (!a.split) {
            sa_layer_bwd_packed<P, NW, MAXT>(a.l1t, buf0, nblk, wg);   // (no mask: run_sa_bwd leaves l1t.mask null)
            __syncthreads();
        }
    }
    // the three store paths of sa_bwd_body over the active rows
    const int nc = a.c_hi - a.c_lo;
    const int32_t *pos = s_pos;
    float *orow = a.gsa_out + (size_t)b * a.S * KS * a.cg_out;
    if (a.cg_out == 4) {
        for (int j = tid; j < nact; j += NT) {
            const float4 v = make_float4(buf0[L::off(a.c_lo, j)], buf0[L::off(a.c_lo + 1, j)], buf0[L::off(a.c_lo + 2, j)], 0.0f);
            if (pos[j] >= 0) *(float4 *)(orow + (size_t)pos[j] * 4) = v;
        }
        return;
    }
    if (((nc | a.c_lo | a.cg_out) & 3) == 0) {
        constexpr int RG = NT / 32;
        const int ql = tid & 31, rg = tid >> 5;
        for (int j = rg; j < nact; j += RG) {
            const int pj = pos[j];
            if (pj < 0) continue;
            float *o = orow + (size_t)pj * a.cg_out + a.c_lo;
            for (int q = ql; q < (nc >> 2); q += 32) *(float4 *)(o + 4 * q) = *(const float4 *)(buf0 + L::off(a.c_lo + 4 * q, j));
        }
        return;
    }
    for (int t = tid; t < nact * nc; t += NT) {
        const int j = t / nc, c = a.c_lo + (t - j * nc);
        if (pos[j] >= 0) orow[(size_t)pos[j] * a.cg_out + c] = buf0[L::off(c, j)];
    }
}

// ------------------------------------------------------------------------------------------ FP fwd
// FP split (round 5): the 3-NN interpolation is linear, so the interpolated part of a module's first layer commutes with it,
//     W1 . [f1 ; interp(f2)] = W1a . f1 + interp(W1b . f2),
// and W1b . f2 is a property of the COARSE point: 4 x fewer points than the module has (1024 / 256 / 64 against 4096 / 1024 / 256
// for fp1 / fp2 / fp3).  The coarser module computes T = out . W1b^T as one more layer behind its own last one (FpFwdArgs::extra,
// rows out2); here a point's three rows of T are gathered, weighted, straight into the MFMA ACCUMULATORS of the first layer's
// tiles (lane (j, h) reads the 4 x 16 bytes of each row that its registers hold - the bytes the interpolation read before), and
// the layer's matrix work is the skip columns only: none at all for fp1 (128 of its 128 input channels are interpolated: one
// of the five layers of fp1 + head gone), 64 of 320 for fp2, 128 of 384 for fp3.
template <int P, int NW>
__device__ __forceinline__ void fp_layer1_split(const FpFwdArgs &a, int b, int n0, float *__restrict__ buf, size_t wg_linear)
{
    // up to PB tiles per wave (the layer has mb * PB tiles, at most PB * NW: run_fp_fwd checks mb <= NW), dealt like layer_fwd's
    constexpr int PB = P / 32, BLK = Lds<P>::BLK;
    const FwdLayer &L = a.layer[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int ntask = L.mb * PB;
    const int first = (wave + (int)(wg_linear & (NW - 1))) & (NW - 1);
    f32x16 acc[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int task = first + i * NW;
        if (task >= ntask) continue;
        f32x16 c;
        const int mb = task / PB, pb = task - mb * PB;
        const size_t n3 = ((size_t)b * a.N + n0 + pb * 32 + j) * 3;
        const int i0 = a.nn_idx[n3], i1 = a.nn_idx[n3 + 1], i2 = a.nn_idx[n3 + 2];
        const float w0 = a.nn_w[n3], w1 = a.nn_w[n3 + 1], w2 = a.nn_w[n3 + 2];
        const float *tb = a.tsrc + (size_t)b * a.S * a.ldt + mb * 32 + 4 * h;
        const float4 *r0 = (const float4 *)(tb + __umul24((unsigned)i0, (unsigned)a.ldt));
        const float4 *r1 = (const float4 *)(tb + __umul24((unsigned)i1, (unsigned)a.ldt));
        const float4 *r2 = (const float4 *)(tb + __umul24((unsigned)i2, (unsigned)a.ldt));
        const float4 *bp = (const float4 *)(L.bias + mb * 32 + 4 * h);
        // accumulator registers 4g .. 4g+3 of lane (j, h) are channels mb*32 + 8g + 4h + (0..3) of point j.
        // Two halves of six row pieces each, fenced, the bias behind them: with all twelve pieces and the bias in flight the
        // kernel does not fit the 96 VGPRs of five waves per SIMD (see fp_fwd_kernel).
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int g = 2 * half; g < 2 * half + 2; ++g) {
                const float4 u0 = r0[2 * g], u1 = r1[2 * g], u2 = r2[2 * g];
                c[4 * g] = u0.x * w0 + u1.x * w1 + u2.x * w2;
                c[4 * g + 1] = u0.y * w0 + u1.y * w1 + u2.y * w2;
                c[4 * g + 2] = u0.z * w0 + u1.z * w1 + u2.z * w2;
                c[4 * g + 3] = u0.w * w0 + u1.w * w1 + u2.w * w2;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const float4 bq0 = bp[0], bq1 = bp[2], bq2 = bp[4], bq3 = bp[6];
        if (L.k8) c = tile_mac<BLK, false>(L.w + (size_t)mb * L.k8 * 64 + lane, L.k8, buf + (pb * 32 + j) * 8 + 4 * h, c);
        c[0] += bq0.x; c[1] += bq0.y; c[2] += bq0.z; c[3] += bq0.w;
        c[4] += bq1.x; c[5] += bq1.y; c[6] += bq1.z; c[7] += bq1.w;
        c[8] += bq2.x; c[9] += bq2.y; c[10] += bq2.z; c[11] += bq2.w;
        c[12] += bq3.x; c[13] += bq3.y; c[14] += bq3.z; c[15] += bq3.w;
        const unsigned m = relu_bits(c);
        if (L.mask) L.mask[((unsigned)wg_linear * (unsigned)ntask + (unsigned)task) * 64u + (unsigned)lane] = (uint16_t)m;
        acc[i] = c;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int task = first + i * NW;
        if (task >= ntask) continue;
        const int mb = task / PB, pb = task - mb * PB;
        store_tile<P>(buf, mb, pb * 32 + j, h, acc[i]);
    }
}

// BIG: the concatenated input does not fit LDS (MSG fp4: 512 + 1024 channels): the first layer's K is streamed
// through the buffer in chunks of KC blocks, its accumulators staying in registers across the chunks.
template <int P, int NW, bool BIG = false>
// (five waves per SIMD = at most 96 VGPRs: the split first layer and the extra layer took the allocator from 88 to 112 registers,
// i.e. from five resident workgroups per CU to four; with fp_layer1_split's row pieces fenced into two halves it fits 96 unspilled)
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(P == 32 ? 5 : 4))) void fp_fwd_kernel(FpFwdArgs a)
{
    using L = Lds<P>;
    constexpr int NT = NW * 64;
    extern __shared__ float lds[];
    float *buf0 = lds;   // the one activation buffer (layers run in place)
    const int tid = threadIdx.x;
    int bx, b;
    xcd_tile(bx, b);
    const int n0 = bx * P;
    const size_t wg = (size_t)b * gridDim.x + bx;
    if (PSG_DIAGBIT(a, 512) && (tid & 63) == 0) a.dbg[(wg * 8 + (tid >> 6)) * 16 + 15] = __builtin_amdgcn_s_memtime();
    if (PSG_DIAGBIT(a, 256) && tid == 0) {
        a.dbg[wg * 4 + 0] = __builtin_amdgcn_s_memtime();
        a.dbg[wg * 4 + 1] = __builtin_amdgcn_s_memrealtime();
    }
    if (BIG) {
        static_assert(!BIG || P == 32, "streamed first layer: one 32-point tile per workgroup");
        constexpr int KC = 64;                       // blocks (of 8 channels) per chunk
        constexpr int RG = NT / 32, JI = P / RG;
        const int ql = tid & 31, rg = tid >> 5;
        const int lane = tid & 63, wave = tid >> 6, jj = lane & 31, h = lane >> 5;
        int i0[JI], i1[JI], i2[JI];
        float w0[JI], w1[JI], w2[JI];
#pragma unroll
        for (int u = 0; u < JI; ++u) {
            const size_t n = (size_t)b * a.N + n0 + rg + u * RG;
            i0[u] = a.nn_idx[n * 3]; i1[u] = a.nn_idx[n * 3 + 1]; i2[u] = a.nn_idx[n * 3 + 2];
            w0[u] = a.nn_w[n * 3]; w1[u] = a.nn_w[n * 3 + 1]; w2[u] = a.nn_w[n * 3 + 2];
        }
        const FwdLayer &L0 = a.layer[0];
        const int ntask = L0.mb;                     // P == 32: one tile per 32 output channels
        const int first = (wave + (int)(wg & (NW - 1))) & (NW - 1);
        f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = 0.0f;
        for (int kb = 0; kb < L0.k8; kb += KC) {
            const int nb = min(KC, L0.k8 - kb), c_lo = kb * 8, c_hi = (kb + nb) * 8;
            // skip-link rows, channels [c_lo, min(c_hi, C1))
#pragma unroll
            for (int u = 0; u < JI; ++u) {
                const int j = rg + u * RG;
                const float4 *f4 = (const float4 *)(a.feat1 + ((size_t)b * a.N + n0 + j) * a.C1);
                for (int q = (c_lo >> 2) + ql; 4 * q < min(c_hi, a.C1); q += 32) *(float4 *)(buf0 + L::off(4 * q - c_lo, j)) = f4[q];
            }
            // interpolated rows, concat channels [max(c_lo, C1), c_hi)
#pragma unroll
            for (int u = 0; u < JI; ++u) {
                const int j = rg + u * RG;
                const float4 *g0 = (const float4 *)(a.feat2 + ((size_t)b * a.S + i0[u]) * a.C2);
                const float4 *g1 = (const float4 *)(a.feat2 + ((size_t)b * a.S + i1[u]) * a.C2);
                const float4 *g2 = (const float4 *)(a.feat2 + ((size_t)b * a.S + i2[u]) * a.C2);
                const int lo = max(c_lo, a.C1) - a.C1, hi = c_hi - a.C1;
                for (int q = (lo >> 2) + ql; 4 * q < hi; q += 32) {
                    const float4 u0 = g0[q], u1 = g1[q], u2 = g2[q];
                    float4 r;
                    r.x = u0.x * w0[u] + u1.x * w1[u] + u2.x * w2[u];
                    r.y = u0.y * w0[u] + u1.y * w1[u] + u2.y * w2[u];
                    r.z = u0.z * w0[u] + u1.z * w1[u] + u2.z * w2[u];
                    r.w = u0.w * w0[u] + u1.w * w1[u] + u2.w * w2[u];
                    *(float4 *)(buf0 + L::off(a.C1 + 4 * q - c_lo, j)) = r;
                }
            }
            __syncthreads();
            if (first < ntask)
                c = tile_mac<L::BLK, false>(L0.w + ((size_t)first * L0.k8 + kb) * 64 + lane, nb, buf0 + jj * 8 + 4 * h, c);
            __syncthreads();
        }
        if (first < ntask) {   // bias, ReLU, mask bits and write-back exactly like layer_fwd
            const float *bp = L0.bias + first * 32 + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) c[r] += bp[8 * (r >> 2) + (r & 3)];
            const unsigned m = relu_bits(c);
            if (L0.mask) L0.mask[(wg * ntask + first) * 64 + lane] = (uint16_t)m;
            store_tile<P>(buf0, first, jj, h, c);
        }
        __syncthreads();
    } else if (!PSG_DIAGBIT(a, 1)) {
        // 32 consecutive lanes read consecutive float4 of ONE source row (512 contiguous bytes per row group), so a
        // wave-wide load touches 8 cache lines instead of 64; neighbour indices / weights are broadcast loads.
        constexpr int RG = NT / 32, JI = P / RG;
        static_assert(P % RG == 0, "row groups must tile the points");
        const int ql = tid & 31, rg = tid >> 5;
        // address arithmetic: the room's bases are wave-uniform (scalar 64-bit), the per-row offsets are 24-bit products
        // (row < 2^12 .. 2^16, channels < 2^11: v_mul_u32_u24 runs at full rate, a 32-bit v_mul_lo at a quarter of it, and
        // the 64-bit per-thread versions of these cost ~10 % of this kernel's matrix time: vector work is not hidden)
        const int32_t *nn_i = a.nn_idx + ((size_t)b * a.N + n0) * 3;
        const float *nn_wp = a.nn_w + ((size_t)b * a.N + n0) * 3;
        const float *f1b = a.feat1 ? a.feat1 + ((size_t)b * a.N + n0) * a.C1 : nullptr;
        const float *f2b = a.feat2 + (size_t)b * a.S * a.C2;
        int i0[JI], i1[JI], i2[JI];
        float w0[JI], w1[JI], w2[JI];
        if (!a.tsrc) {
#pragma unroll
            for (int u = 0; u < JI; ++u) {
                const int n3 = (rg + u * RG) * 3;
                i0[u] = nn_i[n3]; i1[u] = nn_i[n3 + 1]; i2[u] = nn_i[n3 + 2];
                w0[u] = nn_wp[n3]; w1[u] = nn_wp[n3 + 1]; w2[u] = nn_wp[n3 + 2];
            }
        }
        if (a.feat1) {
#pragma unroll
            for (int u = 0; u < JI; ++u) {
                const int j = rg + u * RG;
                const unsigned o1 = __umul24((unsigned)j, (unsigned)a.C1);
                for (int q = ql; q < (a.C1 >> 2); q += 32) *(float4 *)(buf0 + L::off(4 * q, j)) = *(const float4 *)(f1b + (o1 + 4u * q));
            }
        }
#pragma unroll
        for (int u = 0; u < JI; ++u) {
            if (a.tsrc) break;          // split first layer: the interpolated part arrives through fp_layer1_split
            const int j = rg + u * RG;
            // (uniform base + 32-bit offset: the loads take the SGPR-base form, no 64-bit vector adds per address)
            const unsigned o0 = __umul24((unsigned)i0[u], (unsigned)a.C2), oa = __umul24((unsigned)i1[u], (unsigned)a.C2),
                           ob = __umul24((unsigned)i2[u], (unsigned)a.C2);
            for (int q = ql; q < (a.C2 >> 2); q += 32) {
                const float4 u0 = *(const float4 *)(f2b + (o0 + 4u * q)), u1 = *(const float4 *)(f2b + (oa + 4u * q)),
                             u2 = *(const float4 *)(f2b + (ob + 4u * q));
                float4 r;
                r.x = u0.x * w0[u] + u1.x * w1[u] + u2.x * w2[u];
                r.y = u0.y * w0[u] + u1.y * w1[u] + u2.y * w2[u];
                r.z = u0.z * w0[u] + u1.z * w1[u] + u2.z * w2[u];
                r.w = u0.w * w0[u] + u1.w * w1[u] + u2.w * w2[u];
                *(float4 *)(buf0 + L::off(a.C1 + 4 * q, j)) = r;
            }
        }
    }
    __syncthreads();
    float *in = buf0;
    if (PSG_DIAGBIT(a, 512) && (tid & 63) == 0) a.dbg[(wg * 8 + (tid >> 6)) * 16 + 0] = __builtin_amdgcn_s_memtime();
    int l0 = BIG ? 1 : 0;
    if constexpr (P > 32) {
        // (the split first layer peeled off the layer loop: with two tiles per wave, its addresses and the layer_fwd paths'
        // hoisted together across the loop did not fit the registers and went to scratch)
        if (a.tsrc) {
            fp_layer1_split<P, NW>(a, b, n0, in, wg);
            if (PSG_DIAGBIT(a, 512) && (tid & 63) == 0) a.dbg[(wg * 8 + (tid >> 6)) * 16 + 1] = __builtin_amdgcn_s_memtime();
            if (!PSG_DIAGBIT(a, 16)) __syncthreads();
            if (PSG_DIAGBIT(a, 512) && (tid & 63) == 0) a.dbg[(wg * 8 + (tid >> 6)) * 16 + 2] = __builtin_amdgcn_s_memtime();
            l0 = 1;
        }
    }
    for (int l = l0; l < a.n_layers; ++l) {
        if (P == 32 && !BIG && l == 0 && a.tsrc) fp_layer1_split<P, NW>(a, b, n0, in, wg);
        else if (!PSG_DIAGBIT(a, 8)) layer_fwd<P, NW, P / 32>(a.layer[l], in, wg);
        if (PSG_DIAGBIT(a, 512) && (tid & 63) == 0) a.dbg[(wg * 8 + (tid >> 6)) * 16 + 1 + 2 * l] = __builtin_amdgcn_s_memtime();
        if (!PSG_DIAGBIT(a, 16)) __syncthreads();
        if (PSG_DIAGBIT(a, 512) && (tid & 63) == 0) a.dbg[(wg * 8 + (tid >> 6)) * 16 + 2 + 2 * l] = __builtin_amdgcn_s_memtime();
    }
    // `in` now holds the last layer's output
    if (a.out) {
        if ((a.Cout & 3) == 0) {   // 16 bytes per thread, 32 lanes per row (see fp_bwd_kernel's output rows)
            constexpr int RG = NT / 32;
            const int ql = tid & 31, rg = tid >> 5;
            float *ob = a.out + ((size_t)b * a.N + n0) * a.Cout;
            for (int j = rg; j < P; j += RG) {
                const unsigned o = __umul24((unsigned)j, (unsigned)a.Cout);
                for (int q = ql; q < (a.Cout >> 2); q += 32) *(float4 *)(ob + (o + 4u * q)) = *(const float4 *)(in + L::off(4 * q, j));
            }
        } else {
            for (int t = tid; t < P * a.Cout; t += NT) {
                const int j = t / a.Cout, c = t - j * a.Cout;
                a.out[((size_t)b * a.N + n0 + j) * a.Cout + c] = in[L::off(c, j)];
            }
        }
    }
    if (a.out2) {
        // producer side of the finer module's split first layer (fp_layer1_split): T = out . W1b^T, in place over the output
        // (layer_fwd's barrier sits between the row reads above and its stores)
        layer_fwd<P, NW, P / 32>(a.extra, in, wg);
        __syncthreads();
        constexpr int RG = NT / 32;
        const int ql = tid & 31, rg = tid >> 5;
        float *ob = a.out2 + ((size_t)b * a.N + n0) * a.Cout2;
        for (int j = rg; j < P; j += RG) {
            const unsigned o = __umul24((unsigned)j, (unsigned)a.Cout2);
            for (int q = ql; q < (a.Cout2 >> 2); q += 32) *(float4 *)(ob + (o + 4u * q)) = *(const float4 *)(in + L::off(4 * q, j));
        }
    }
    if (a.logp && !PSG_DIAGBIT(a, 4)) {
        // log_softmax over the n_cls (<= 16) head rows: 8 lanes per point, classes q and q + 8 per lane
        for (int t = tid; t < P * 8; t += NT) {
            const int j = t >> 3, q = t & 7;
            const bool has0 = q < a.n_cls;
            const float z0 = has0 ? in[L::off(q, j)] : -INFINITY;
            const bool has1 = q + 8 < a.n_cls;
            const float z1 = has1 ? in[L::off(q + 8, j)] : -INFINITY;
            float m = fmaxf(z0, z1);
            m = fmaxf(m, __shfl_xor(m, 1));
            m = fmaxf(m, __shfl_xor(m, 2));
            m = fmaxf(m, __shfl_xor(m, 4));
            float s = (has0 ? expf(z0 - m) : 0.0f) + (has1 ? expf(z1 - m) : 0.0f);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            const float lse = logf(s);
            float *o = a.logp + ((size_t)b * a.N + n0 + j) * a.n_cls;
            if (has0) o[q] = (z0 - m) - lse;
            if (has1) o[q + 8] = (z1 - m) - lse;
        }
    }
    if (PSG_DIAGBIT(a, 256) && tid == 0) {
        a.dbg[wg * 4 + 2] = __builtin_amdgcn_s_memtime();
        a.dbg[wg * 4 + 3] = __builtin_amdgcn_s_memrealtime();
    }
}

// ------------------------------------------------------------------------------------------ FP bwd
// Transposed 3-NN interpolation of the finer module, for the 32 points of a workgroup: buf[c][j] = sum over the list of
// point j of w * dint[fine][c] (CSR by coarse point, ascending fine point: the order the sums always had).
// The lists of a room are as uneven as its point density - a coarse point inside a dense patch is the neighbour of hundreds
// of fine points while the mean is 12 - so the rows are not dealt to lanes (one lane walking one list, everybody waiting
// for the longest) but to WAVES by entry count: wave w takes the consecutive rows whose lists start inside the w-th
// NW-th of the workgroup's entry range, walks their entries in order with all 64 lanes on one gradient row (a coalesced
// Cout-float read per entry, eight rows in flight) and writes every row it owns exactly once (zeros for an empty list).
// A wave's share is at most the even share plus one list.  VW = Cg / 64 channels per lane (2 or 4).
template <int P, int NW, int VW>
__device__ __forceinline__ void fp_bwd_gather_rows(const FpBwdArgs &a, int b, int n0, float *__restrict__ buf, int lane, int wave)
{
    static_assert(P == 32, "one 32-point tile per workgroup");
    // gradient rows in flight per wave: the walk is a chain of L2 / MALL round trips (26 % of fp2 backward, 24 % of fp3's: skipped
    // for timing, 5.4 / 2.9 -> 4.0 / 2.2 ms), so as many as the registers allow: 16 two-float pieces, 8 four-float ones
    constexpr int INF = VW <= 2 ? 16 : 8;
    typedef float vwf __attribute__((ext_vector_type(VW)));
    const int32_t *offp = a.nninv_off + (size_t)b * (a.N + 1) + n0;
    const int2 *ent = a.nninv_ent + (size_t)b * 3 * a.n_fine;
    const int offl = offp[lane < 32 ? lane : 32];                       // lanes 32.. hold the end of the range
    const int e0 = __builtin_amdgcn_readfirstlane(offl), e_end = __builtin_amdgcn_readlane(offl, 32);
    const int ltot = e_end - e0;
    const int t_lo = (int)(((long long)ltot * wave) / NW), t_hi = (int)(((long long)ltot * (wave + 1)) / NW);
    const int r_lo = __popcll(__ballot(lane < 32 && offl - e0 < t_lo));
    const int r_hi = wave == NW - 1 ? 32 : __popcll(__ballot(lane < 32 && offl - e0 < t_hi));
    if (r_lo >= r_hi) return;
    const int lo = __builtin_amdgcn_readlane(offl, r_lo), hi = __builtin_amdgcn_readlane(offl, r_hi);
    const float *rows = a.dint + (size_t)b * a.n_fine * a.Cg + lane * VW;
    float *dst = buf + ((lane * VW) >> 3) * Lds<P>::BLK + ((lane * VW) & 7);    // + 8 * point
    int cur = r_lo, next = __builtin_amdgcn_readlane(offl, r_lo + 1);
    vwf acc = 0.0f;
    for (int base = lo; base < hi; base += 64) {
        const int n = hi - base < 64 ? hi - base : 64;
        const int2 pe = lane < n ? ent[base + lane] : make_int2(0, 0);  // (an absent entry reads row 0 with weight 0)
        for (int i = 0; i < n; i += INF) {
            vwf v[INF];
            float w[INF];
#pragma unroll
            for (int k = 0; k < INF; ++k) {
                const int fine = __builtin_amdgcn_readlane(pe.x, i + k);
                w[k] = __int_as_float(__builtin_amdgcn_readlane(pe.y, i + k));
                v[k] = *(const vwf *)(rows + (size_t)fine * a.Cg);
            }
#pragma unroll
            for (int k = 0; k < INF; ++k) {
                if (i + k < n) {
                    const int e = base + i + k;
                    while (e >= next) {                                 // the row is complete (or empty): write it, take the next
                        *(vwf *)(dst + 8 * cur) = acc;
                        acc = 0.0f;
                        ++cur;
                        next = __builtin_amdgcn_readlane(offl, cur + 1);
                    }
                    acc += w[k] * v[k];
                }
            }
        }
    }
    for (; cur < r_hi; ++cur) {
        *(vwf *)(dst + 8 * cur) = acc;
        acc = 0.0f;
    }
}

// BIG: the gradient of the concatenated input does not fit LDS (MSG fp4: 1536 channels): the last transposed layer
// is not run in place; NW output tiles at a time go through a staging area behind its input and out to HBM.
template <int P, int NW, int MAXT, bool BIG = false>
__global__ __launch_bounds__(NW * 64) void fp_bwd_kernel(FpBwdArgs a)
{
    using L = Lds<P>;
    constexpr int PB = P / 32, NT = NW * 64;
    extern __shared__ float lds[];
    float *buf0 = lds;   // the one activation buffer (layers run in place)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, b;
    xcd_tile(bx, b);
    const int n0 = bx * P;
    const size_t wg = (size_t)b * gridDim.x + bx;

    if (a.dout || a.nninv_off) {
        // dZ_last = dout * mask_last, loaded tile-wise so the mask bits line up with the forward epilogue
        const int j = lane & 31, h = lane >> 5;
        const int ntask = a.mb_last * PB;
        // the gathered gradient goes through the activation buffer itself: waves gather whole rows (balanced by entry
        // count), then every lane masks its own tile elements in place
        const bool staged = P == 32 && a.nninv_off && (a.Cg == 128 || a.Cg == 256);
        if constexpr (P == 32) {
            if (staged) {
                if (a.Cg == 128) fp_bwd_gather_rows<P, NW, 2>(a, b, n0, buf0, lane, wave);
                else fp_bwd_gather_rows<P, NW, 4>(a, b, n0, buf0, lane, wave);
                __syncthreads();
            }
        }
        // finer module split: the rows gathered are the gradient of T = out . W1b^T (fp_layer1_split), one transposed layer
        // away from the gradient of this module's output; mask_last is that layer's mask (the host only sets `pre` with a
        // staged gather)
        if (a.pre.w) layer_bwd<P, NW, MAXT>(a.pre, buf0, wg);
        else
        for (int task = wave; task < ntask; task += NW) {
            const int mb = task / PB, pb = task - mb * PB;
            const unsigned m = a.mask_last[(wg * ntask + task) * 64 + lane];
            float4 dq[4];
            if (staged) {
                const float *o = buf0 + (size_t)(mb * 4) * L::BLK + (pb * 32 + j) * 8 + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) dq[g] = *(const float4 *)(o + (size_t)g * L::BLK);
            } else if (a.nninv_off) {
                // deterministic transpose of the finer module's interpolation: sum_w * (its gradient rows)
                const int32_t *off = a.nninv_off + (size_t)b * (a.N + 1) + n0 + pb * 32 + j;
                const int2 *ent = a.nninv_ent + (size_t)b * 3 * a.n_fine;
#pragma unroll
                for (int g = 0; g < 4; ++g) dq[g] = make_float4(0.f, 0.f, 0.f, 0.f);
                const int e1 = off[1];
                // two list entries per pass (both entry records first, then their 8 row pieces): half the dependent
                // memory round trips; an absent second entry contributes w = 0 times row 0
                for (int e = off[0]; e < e1; e += 2) {
                    const int2 pa = ent[e];
                    const int2 pb = e + 1 < e1 ? ent[e + 1] : make_int2(0, 0);
                    const float wa = __int_as_float(pa.y), wb = __int_as_float(pb.y);
                    const float *sa = a.dint + ((size_t)b * a.n_fine + pa.x) * a.Cout + mb * 32 + 4 * h;
                    const float *sb = a.dint + ((size_t)b * a.n_fine + pb.x) * a.Cout + mb * 32 + 4 * h;
                    float4 da[4], db[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) { da[g] = *(const float4 *)(sa + 8 * g); db[g] = *(const float4 *)(sb + 8 * g); }
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        dq[g].x += wa * da[g].x; dq[g].y += wa * da[g].y; dq[g].z += wa * da[g].z; dq[g].w += wa * da[g].w;
                    }
                    if (e + 1 < e1) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            dq[g].x += wb * db[g].x; dq[g].y += wb * db[g].y; dq[g].z += wb * db[g].z; dq[g].w += wb * db[g].w;
                        }
                    }
                }
            } else {
                const float *row = a.dout + ((size_t)b * a.N + n0 + pb * 32 + j) * a.Cout + mb * 32 + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) dq[g] = *(const float4 *)(row + 8 * g);
            }
            f32x16 v;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 d = dq[g];
                v[4 * g] = ((m >> (4 * g)) & 1u) ? d.x : 0.0f;
                v[4 * g + 1] = ((m >> (4 * g + 1)) & 1u) ? d.y : 0.0f;
                v[4 * g + 2] = ((m >> (4 * g + 2)) & 1u) ? d.z : 0.0f;
                v[4 * g + 3] = ((m >> (4 * g + 3)) & 1u) ? d.w : 0.0f;
            }
            store_tile<P>(buf0, mb, pb * 32 + j, h, v);
        }
    } else {
        // log_softmax backward: dz = dlogp - exp(logp) * sum(dlogp)   (pointnet2_sem_seg.py:38).
        // The workgroup's 32 rows of logp and dlogp are two contiguous runs of 32 x n_cls floats: all threads copy them into
        // LDS (coalesced), then four lanes per point share the row - the first sums dlogp in class order (the order the sum
        // always had), each computes the classes q, q + 4, q + 8, q + 12.  (One thread per point walking its two rows in
        // global memory was a chain of 2 x 13 scattered loads at the head of every workgroup: fp1 backward 10.45 -> 10.1 ms.)
        float *s_lp = buf0 + (size_t)4 * L::BLK, *s_dl = buf0 + (size_t)6 * L::BLK;     // blocks 4 .. 7: free until the first layer stores
        const int nrow = P * a.n_cls;
        const float *lp_g = a.logp + ((size_t)b * a.N + n0) * a.n_cls, *dl_g = a.dlogp + ((size_t)b * a.N + n0) * a.n_cls;
        for (int i = tid; i < nrow; i += NT) { s_lp[i] = lp_g[i]; s_dl[i] = dl_g[i]; }
        __syncthreads();
        for (int t = tid; t < P * 4; t += NT) {
            const int j = t >> 2, q = t & 3;
            const float *lp = s_lp + j * a.n_cls, *dl = s_dl + j * a.n_cls;
            float s = 0.0f;
            if (q == 0)
                for (int c = 0; c < a.n_cls; ++c) s += dl[c];
            s = __shfl(s, (tid & 63) & ~3);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = q + 4 * i;
                buf0[L::off(c, j)] = c < a.n_cls ? dl[c] - expf(lp[c]) * s : 0.0f;
            }
        }
        for (int t = tid; t < P * (a.layer[0].k8 - 2); t += NT) {   // K-padding blocks of conv2^T (none for 13 classes)
            float *zp = buf0 + (size_t)(2 + t / P) * L::BLK + (t % P) * 8;
            *(float4 *)zp = make_float4(0.f, 0.f, 0.f, 0.f);
            *(float4 *)(zp + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __syncthreads();
    float *in = buf0;
    for (int l = 0; l < a.n_layers - (BIG ? 1 : 0); ++l) {
        layer_bwd<P, NW, MAXT>(a.layer[l], in, wg);
        __syncthreads();
    }
    if (BIG) {
        static_assert(!BIG || P == 32, "streamed last layer: one 32-point tile per workgroup");
        const BwdLayer &Lz = a.layer[a.n_layers - 1];   // first forward layer transposed: no mask behind it
        float *stage = buf0 + (size_t)Lz.k8 * L::BLK;   // NW tiles = NW * 4 blocks behind the layer's input
        const int jj = lane & 31, h = lane >> 5;
        for (int t0 = 0; t0 < Lz.mb; t0 += NW) {
            const int mb = t0 + wave;
            if (mb < Lz.mb) {
                f32x16 c;
#pragma unroll
                for (int r = 0; r < 16; ++r) c[r] = 0.0f;
                c = tile_mac<L::BLK, false>(Lz.w + (size_t)mb * Lz.k8 * 64 + lane, Lz.k8, buf0 + jj * 8 + 4 * h, c);
                store_tile<P>(stage, wave, jj, h, c);
            }
            __syncthreads();
            for (int t = tid; t < P * NW * 32; t += NT) {
                const int j = t / (NW * 32), cc = t - j * (NW * 32), c = t0 * 32 + cc;
                const float v = stage[L::off(cc, j)];
                const size_t n = (size_t)b * a.N + n0 + j;
                if (c < a.C1) a.dfeat1[n * a.C1 + c] = v;
                else if (c < a.C1 + a.C2) a.dint_out[n * a.C2 + (c - a.C1)] = v;
            }
            __syncthreads();
        }
        return;
    }
    // `in` = gradient of the concat input [C1 skip rows | C2 interpolated rows][point], written out as plain rows, 16 bytes per
    // thread: 32 consecutive lanes cover 512 contiguous bytes of one row (no division by a run-time channel count, one
    // ds_read_b128 and one global store per 4 channels; the element-wise loops this replaces cost a quarter-rate integer
    // division and a 4-byte LDS read + store per element: ~600 vector instructions per thread in fp2 backward).
    // The coarser module gathers the interpolated part through the inverse 3-NN lists (pointnet_util.py:308: the transpose
    // of index_points + weighted sum, without atomics).
    // Split first layer (a.split): the layers above stopped at dZ1.  Its rows ARE the interpolated part's gradient as the
    // coarser module wants it (it applies W1b^T per coarse point after its gather: FpBwdArgs::pre); the skip part is
    // W1a^T . dZ1, run after those rows have been read.
    constexpr int RG = NT / 32;
    const int ql = tid & 31, rg = tid >> 5;
    const int w2 = a.split ? a.Cd : a.C2, o2 = a.split ? 0 : a.C1;
    float *d1 = a.dfeat1 ? a.dfeat1 + ((size_t)b * a.N + n0) * a.C1 : nullptr;     // sole writer of the skip-link gradient
    float *d2 = a.dint_out + ((size_t)b * a.N + n0) * w2;
    for (int j = rg; j < P; j += RG) {
        const unsigned o = __umul24((unsigned)j, (unsigned)w2);
        for (int q = ql; q < (w2 >> 2); q += 32) *(float4 *)(d2 + (o + 4u * q)) = *(const float4 *)(in + L::off(o2 + 4 * q, j));
    }
    if (!d1) return;
    if (a.split) {
        layer_bwd<P, NW, MAXT>(a.skipT, in, wg);      // (its barrier separates the row reads above from its stores)
        __syncthreads();
    }
    for (int j = rg; j < P; j += RG) {
        const unsigned o = __umul24((unsigned)j, (unsigned)a.C1);
        for (int q = ql; q < (a.C1 >> 2); q += 32) *(float4 *)(d1 + (o + 4u * q)) = *(const float4 *)(in + L::off(4 * q, j));
    }
}

// ------------------------------------------------------------------------------------------ fp1 + head, there and back
// The NB loop's fp1 + head forward, CE gradient and fp1 + head backward in ONE launch (psg_pn2_nb_step): fp_fwd_kernel<64, 4>
// and fp_bwd_kernel<64, 4, 2> share their tiling - 64 points per workgroup, four waves, the one in-place LDS buffer, xcd_tile's
// order - and the backward needs nothing of the forward but the ReLU bits and the 13 log-probs of its own points.  A workgroup
// runs its tile from the gather of the T rows to the store of its dZ1 rows; what the three launches exchanged through HBM
// (logp, dlogp, the masks of four layers) stays in LDS and registers:
//   * a wave owns the tile pair (mb = first, pb = 0 / 1) of every 128-wide layer, forward and transposed (layer_fwd's and
//     layer_bwd's pair dealing: the same `first`); the 2 x 16 ReLU bits of a layer are one register per lane, kept from the
//     layer's forward epilogue to the transposed layer whose output they gate;
//   * the split first layer deals single tiles (fp_layer1_split), so the bits of a wave's pair have another owner there: the
//     wave reads them back from the layer's output in LDS (positive exactly where the bit was set);
//   * log-probs and their gradient are staged in LDS blocks 4 .. 7, which the head leaves free (fp_bwd_kernel's prologue).
// Every tile runs the k-loops, the epilogue and the row arithmetic of the separate kernels, expression for expression: the
// results are the same bits (tests/test_gpu_fp1_loop.py).  NC = the class count, a constant here so that the CE row's arrays
// are registers.
struct Fp1LoopArgs {
    FpFwdArgs fwd;          // what fp_layer1_split reads of the forward's arguments: nn_idx, nn_w, tsrc, ldt, N, S and layer[0]
                            // (the split first layer: its bias, k8 = 0, no mask pointer)
    FwdLayer f[3];          // fp1 layers 2 and 3, conv1 (ReLU; no mask pointer: the bits stay in registers)
    FwdLayer head;          // conv2
    BwdLayer t[4];          // conv2^T, conv1^T, fp1 layer 3^T, layer 2^T (no mask pointer)
    const int32_t *labels;  // [B][N], or null: `target` for every row
    int target, rows_active;
    float scale;
    float *dint_out;        // [B][N][128]: the dZ1 rows, where fp_bwd_kernel writes them for fp2's gather
    int N;
};

__device__ __forceinline__ void add_bias16(f32x16 &c, const float4 &bq0, const float4 &bq1, const float4 &bq2, const float4 &bq3)
{
    c[0] += bq0.x; c[1] += bq0.y; c[2] += bq0.z; c[3] += bq0.w;
    c[4] += bq1.x; c[5] += bq1.y; c[6] += bq1.z; c[7] += bq1.w;
    c[8] += bq2.x; c[9] += bq2.y; c[10] += bq2.z; c[11] += bq2.w;
    c[12] += bq3.x; c[13] += bq3.y; c[14] += bq3.z; c[15] += bq3.w;
}

// the ReLU bits of the wave's pair (first, 0 / 1) read back from the layer's output in LDS: an element is positive exactly where
// relu_bits set its bit (it stored x where 0 < x and 0 elsewhere)
template <int P>
__device__ __forceinline__ unsigned fp1_loop_pair_bits(const float *__restrict__ buf, int first, int lane)
{
    const int j = lane & 31, h = lane >> 5;
    const float *o = buf + (size_t)(first * 4) * Lds<P>::BLK + j * 8 + 4 * h;
    unsigned m = 0;
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 v = *(const float4 *)(o + (size_t)g * Lds<P>::BLK + pb * 32 * 8);
            m |= (v.x > 0.0f ? 1u : 0u) << (16 * pb + 4 * g);
            m |= (v.y > 0.0f ? 1u : 0u) << (16 * pb + 4 * g + 1);
            m |= (v.z > 0.0f ? 1u : 0u) << (16 * pb + 4 * g + 2);
            m |= (v.w > 0.0f ? 1u : 0u) << (16 * pb + 4 * g + 3);
        }
    }
    return m;
}

// the wave's pair (first, 0 / 1) of a 128-wide forward layer, in place: layer_fwd's pair path with the bits returned
// (low half: point block 0, high half: point block 1).  The caller places the barrier behind it, as behind layer_fwd.
template <int P>
__device__ __forceinline__ unsigned fp1_loop_pair_fwd(const FwdLayer &Lr, float *__restrict__ buf, int first, int lane)
{
    constexpr int BLK = Lds<P>::BLK;
    const int j = lane & 31, h = lane >> 5;
    const float4 *bp = (const float4 *)(Lr.bias + first * 32 + 4 * h);
    const float4 bq0 = bp[0], bq1 = bp[2], bq2 = bp[4], bq3 = bp[6];
    f32x16 c0, c1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { c0[r] = 0.0f; c1[r] = 0.0f; }
    tile_mac_x2<BLK, false>(Lr.w + (size_t)first * Lr.k8 * 64 + lane, Lr.k8, buf + j * 8 + 4 * h, c0, c1);
    add_bias16(c0, bq0, bq1, bq2, bq3);
    const unsigned m0 = relu_bits(c0);
    add_bias16(c1, bq0, bq1, bq2, bq3);
    const unsigned m1 = relu_bits(c1);
    __syncthreads();
    store_tile<P>(buf, first, j, h, c0);
    store_tile<P>(buf, first, 32 + j, h, c1);
    return m0 | (m1 << 16);
}

// the same pair of a transposed layer, gated by the bits `m` of the forward layer whose input gradient this is
template <int P>
__device__ __forceinline__ void fp1_loop_pair_bwd(const BwdLayer &Lt, float *__restrict__ buf, int first, int lane, unsigned m)
{
    constexpr int BLK = Lds<P>::BLK;
    const int j = lane & 31, h = lane >> 5;
    f32x16 c0, c1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { c0[r] = 0.0f; c1[r] = 0.0f; }
    tile_mac_x2<BLK, false>(Lt.w + (size_t)first * Lt.k8 * 64 + lane, Lt.k8, buf + j * 8 + 4 * h, c0, c1);
    apply_bits(c0, m);
    apply_bits(c1, m >> 16);
    __syncthreads();
    store_tile<P>(buf, first, j, h, c0);
    store_tile<P>(buf, first, 32 + j, h, c1);
}

template <int P, int NW, int NC>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(4))) void fp1_loop_kernel(Fp1LoopArgs a)
{
    static_assert(P == 64 && NW == 4 && NC <= 16, "one pair of tiles per wave and 128-wide layer; the classes in two LDS blocks");
    using L = Lds<P>;
    constexpr int NT = NW * 64;
    extern __shared__ float lds[];
    float *buf0 = lds;   // the one activation buffer (layers run in place), 16 blocks
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    int bx, b;
    xcd_tile(bx, b);
    const int n0 = bx * P;
    const size_t wg = (size_t)b * gridDim.x + bx;
    const int first = (wave + (int)(wg & (NW - 1))) & (NW - 1);

    // ---- forward: split first layer (fp_layer1_split itself: the compiler contracts its weighted sums element by element as
    // it sees fit, and only the same function gives the same bits), layers 2 and 3, conv1
    fp_layer1_split<P, NW>(a.fwd, b, n0, buf0, wg);
    __syncthreads();
    const unsigned m_l1 = fp1_loop_pair_bits<P>(buf0, first, lane);
    const unsigned m_l2 = fp1_loop_pair_fwd<P>(a.f[0], buf0, first, lane);
    __syncthreads();
    const unsigned m_l3 = fp1_loop_pair_fwd<P>(a.f[1], buf0, first, lane);
    __syncthreads();
    const unsigned m_c1 = fp1_loop_pair_fwd<P>(a.f[2], buf0, first, lane);
    __syncthreads();
    // conv2: one output block, two single tiles (layer_fwd's single-tile path: task = first < 2 is point block `first`)
    {
        f32x16 c;
        if (first < P / 32) {
            const float4 *bp = (const float4 *)(a.head.bias + 4 * h);
            const float4 bq0 = bp[0], bq1 = bp[2], bq2 = bp[4], bq3 = bp[6];
#pragma unroll
            for (int r = 0; r < 16; ++r) c[r] = 0.0f;
            c = tile_mac<L::BLK, false>(a.head.w + lane, a.head.k8, buf0 + (first * 32 + j) * 8 + 4 * h, c);
            add_bias16(c, bq0, bq1, bq2, bq3);
        }
        __syncthreads();
        if (first < P / 32) store_tile<P>(buf0, 0, first * 32 + j, h, c);
    }
    __syncthreads();

    // ---- log_softmax (fp_fwd_kernel's: 8 lanes per point, classes q and q + 8 per lane) into LDS blocks 4 .. 5
    float *s_lp = buf0 + (size_t)4 * L::BLK, *s_dl = buf0 + (size_t)6 * L::BLK;
    for (int t = tid; t < P * 8; t += NT) {
        const int pj = t >> 3, q = t & 7;
        const bool has0 = q < NC;
        const float z0 = has0 ? buf0[L::off(q, pj)] : -INFINITY;
        const bool has1 = q + 8 < NC;
        const float z1 = has1 ? buf0[L::off(q + 8, pj)] : -INFINITY;
        float m = fmaxf(z0, z1);
        m = fmaxf(m, __shfl_xor(m, 1));
        m = fmaxf(m, __shfl_xor(m, 2));
        m = fmaxf(m, __shfl_xor(m, 4));
        float s = (has0 ? expf(z0 - m) : 0.0f) + (has1 ? expf(z1 - m) : 0.0f);
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        const float lse = logf(s);
        float *o = s_lp + pj * NC;
        if (has0) o[q] = (z0 - m) - lse;
        if (has1) o[q + 8] = (z1 - m) - lse;
    }
    __syncthreads();
    // ---- CE row (psg_ce_row.cuh: ce_logp_grad_kernel's arithmetic), one thread per point = the first wave
    if (tid < P) {
        const int r = b * a.N + n0 + tid;
        const bool active = r < a.rows_active;
        const int y = !active ? -1 : a.labels ? a.labels[r] : a.target;
        ce_row_grad(s_lp + tid * NC, NC, y, a.scale, active, s_dl + tid * NC);
    }
    __syncthreads();
    // ---- log_softmax backward (fp_bwd_kernel's prologue): dz = dlogp - exp(logp) * sum(dlogp), four lanes per point
    for (int t = tid; t < P * 4; t += NT) {
        const int pj = t >> 2, q = t & 3;
        const float *lp = s_lp + pj * NC, *dl = s_dl + pj * NC;
        float s = 0.0f;
        if (q == 0)
            for (int c = 0; c < NC; ++c) s += dl[c];
        s = __shfl(s, (tid & 63) & ~3);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = q + 4 * i;
            buf0[L::off(c, pj)] = c < NC ? dl[c] - expf(lp[c]) * s : 0.0f;
        }
    }
    __syncthreads();

    // ---- backward: conv2^T, conv1^T, layer 3^T, layer 2^T, each gated by the bits of the layer below it
    fp1_loop_pair_bwd<P>(a.t[0], buf0, first, lane, m_c1);
    __syncthreads();
    fp1_loop_pair_bwd<P>(a.t[1], buf0, first, lane, m_l3);
    __syncthreads();
    fp1_loop_pair_bwd<P>(a.t[2], buf0, first, lane, m_l2);
    __syncthreads();
    fp1_loop_pair_bwd<P>(a.t[3], buf0, first, lane, m_l1);
    __syncthreads();
    // dZ1 rows, 16 bytes per thread, 32 lanes per row (fp_bwd_kernel's output rows of the split module)
    constexpr int RG = NT / 32, CD = 128;
    const int ql = tid & 31, rg = tid >> 5;
    float *d2 = a.dint_out + ((size_t)b * a.N + n0) * CD;
    for (int pj = rg; pj < P; pj += RG)
        *(float4 *)(d2 + (pj * CD + 4 * ql)) = *(const float4 *)(buf0 + L::off(4 * ql, pj));
}

// ------------------------------------------------------------------------------------------ per-point side of the SA split
// Backward of the split first layer (see sa_fwd_kernel): for the 32 points n of a workgroup
//     dT[n]   = sum of the dZ1 rows of the grouped rows that gathered point n  (the transpose of index_points, as a gather:
//               sa_bwd stored its rows in list order, so they are the CONTIGUOUS slots [off[n], off[n+1]), ascending row)
//     out[n]  = skip[n] + dT[n] . W1f                                            (C1 -> D channels, one MFMA layer)
// `out` is the complete gradient of the level's pooled features: the coarser FP module's skip-link rows plus the transposed
// grouping of the next SA level - what sa_bwd's prologue used to sum per (group, channel) thread by walking the list of its
// point (a wave waited for its longest list).  Here the workgroup's entry range is dealt to the WAVES by entry count, a wave
// walks its rows with all 64 lanes on one row (coalesced C1-float reads, eight in flight), exactly like fp_bwd_gather_rows.
struct PwBwdArgs {
    const int32_t *ginv_off;   // [B][N + 1]
    const float *gsa;          // [B][g_rows][C1] dZ1 rows in list order
    int g_rows;
    const float *skip;         // [B][N][D] or null
    float *out;                // [B][N][D]
    BwdLayer wt;               // W1f transposed: k8 = C1 / 8, mb = D / 32, no mask
    int N, C1, D;
};

template <int P, int NW, int VW>
__device__ __forceinline__ void pw_bwd_gather_rows(const PwBwdArgs &a, int b, int n0, float *__restrict__ buf, int lane, int wave)
{
    static_assert(P == 32, "one 32-point tile per workgroup");
    typedef float vwf __attribute__((ext_vector_type(VW)));
    const int32_t *offp = a.ginv_off + (size_t)b * (a.N + 1) + n0;
    const int offl = offp[lane < 32 ? lane : 32];                       // lanes 32.. hold the end of the range
    const int e0 = __builtin_amdgcn_readfirstlane(offl), e_end = __builtin_amdgcn_readlane(offl, 32);
    const int ltot = e_end - e0;
    const int t_lo = (int)(((long long)ltot * wave) / NW), t_hi = (int)(((long long)ltot * (wave + 1)) / NW);
    const int r_lo = __popcll(__ballot(lane < 32 && offl - e0 < t_lo));
    const int r_hi = wave == NW - 1 ? 32 : __popcll(__ballot(lane < 32 && offl - e0 < t_hi));
    if (r_lo >= r_hi) return;
    const int lo = __builtin_amdgcn_readlane(offl, r_lo), hi = __builtin_amdgcn_readlane(offl, r_hi);
    const float *rows = a.gsa + (size_t)b * a.g_rows * a.C1 + lane * VW;
    float *dst = buf + ((lane * VW) >> 3) * Lds<P>::BLK + ((lane * VW) & 7);    // + 8 * point
    int cur = r_lo, next = __builtin_amdgcn_readlane(offl, r_lo + 1);
    vwf acc = 0.0f;
    for (int base = lo; base < hi; base += 8) {
        vwf v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = base + k < hi ? *(const vwf *)(rows + (size_t)(base + k) * a.C1) : (vwf)0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = base + k;
            if (e < hi) {
                while (e >= next) {                                     // the point's list is complete (or empty): write, take the next
                    *(vwf *)(dst + 8 * cur) = acc;
                    acc = 0.0f;
                    ++cur;
                    next = __builtin_amdgcn_readlane(offl, cur + 1);
                }
                acc += v[k];
            }
        }
    }
    for (; cur < r_hi; ++cur) {
        *(vwf *)(dst + 8 * cur) = acc;
        acc = 0.0f;
    }
}

// MAXQ = float4 pieces of a skip-link row per thread (32 lanes on a row): D <= 128 * MAXQ.
template <int P, int NW, int MAXT = 1, int MAXQ = 4>
__global__ __launch_bounds__(NW * 64) void pw_bwd_kernel(PwBwdArgs a)
{
    using L = Lds<P>;
    constexpr int NT = NW * 64;
    extern __shared__ float lds[];
    float *buf0 = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, b;
    xcd_tile(bx, b);
    const int n0 = bx * P;
    const size_t wg = (size_t)b * gridDim.x + bx;
    if (a.C1 == 64) pw_bwd_gather_rows<P, NW, 1>(a, b, n0, buf0, lane, wave);
    else if (a.C1 == 128) pw_bwd_gather_rows<P, NW, 2>(a, b, n0, buf0, lane, wave);
    else pw_bwd_gather_rows<P, NW, 4>(a, b, n0, buf0, lane, wave);
    __syncthreads();
    // the skip-link rows this thread will add at the end: issued now, so the round trip runs under the layer (fetched inside the
    // store loop below they were a chain of misses at the tail of the workgroup); up to 8 pieces per thread (D <= 512)
    constexpr int RG = NT / 32, ROWS = P / RG;
    const int ql = tid & 31, rg = tid >> 5;
    const float *sb = a.skip ? a.skip + ((size_t)b * a.N + n0) * a.D : nullptr;
    float4 sk[ROWS][MAXQ];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int i = 0; i < MAXQ; ++i) {
            const int q = ql + 32 * i;
            sk[r][i] = (sb && q < (a.D >> 2)) ? *(const float4 *)(sb + (__umul24((unsigned)(rg + r * RG), (unsigned)a.D) + 4u * q))
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    layer_bwd<P, NW, MAXT>(a.wt, buf0, wg);
    __syncthreads();
    {
        float *ob = a.out + ((size_t)b * a.N + n0) * a.D;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int j = rg + r * RG;
            const unsigned o = __umul24((unsigned)j, (unsigned)a.D);
#pragma unroll
            for (int i = 0; i < MAXQ; ++i) {
                const int q = ql + 32 * i;
                if (q < (a.D >> 2)) {
                    float4 v = *(const float4 *)(buf0 + L::off(4 * q, j));
                    const float4 s = sk[r][i];
                    v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w;
                    *(float4 *)(ob + (o + 4u * q)) = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ per-point product, forward
// T = in . W1f^T + b1 for P = 32 points per workgroup (run_pw_fwd): the one layer of the split SA levels' per-point side.  It used to
// be a launch of fp_fwd_kernel<32, 8> with an empty interpolated part - eight waves whatever the layer's width
// (two of them with a tile at level 1, four at level 2) and a point's three neighbour entries read for nothing.  Here a
// workgroup has as many waves as it has output blocks, at most NW: blockIdx.z picks the NW blocks of 32 output channels it
// computes (level 3: 8 blocks = two workgroups of 4 waves per point tile, 256 workgroups at 64 rooms instead of 128 on 256
// CUs; each reads the tile's input rows, which the second finds in L2).  Every tile runs layer_fwd's k-loop and epilogue over
// the whole K: the rows are bit-identical to the borrowed kernel's.
struct PwFwdArgs {
    const float *in;    // [B][N][D]
    float *out;         // [B][N][C1]
    FwdLayer l;         // W1f with the layer's bias: k8 = D / 8, mb = C1 / 32, no ReLU, no mask
    int N, D, C1;
};

template <int P, int NW>
__global__ __launch_bounds__(NW * 64) void pw_fwd_kernel(PwFwdArgs a)
{
    using L = Lds<P>;
    constexpr int NT = NW * 64, RG = NT / 32;
    extern __shared__ float lds[];
    float *buf0 = lds;
    const int tid = threadIdx.x, ql = tid & 31, rg = tid >> 5;
    int bx, b;
    xcd_tile(bx, b);
    const int n0 = bx * P;
    const size_t wg = (size_t)b * gridDim.x + bx;
    const float *ib = a.in + ((size_t)b * a.N + n0) * a.D;
    for (int j = rg; j < P; j += RG) {
        const unsigned o = __umul24((unsigned)j, (unsigned)a.D);
        for (int q = ql; q < (a.D >> 2); q += 32) *(float4 *)(buf0 + L::off(4 * q, j)) = *(const float4 *)(ib + (o + 4u * q));
    }
    __syncthreads();
    FwdLayer l = a.l;   // this workgroup's output blocks [mb0, mb0 + l.mb), computed in place into LDS blocks 0 .. 4 * l.mb
    const int mb0 = (int)blockIdx.z * NW;
    l.w += (size_t)mb0 * l.k8 * 64;
    l.bias += mb0 * 32;
    l.mb = min(NW, a.l.mb - mb0);
    layer_fwd<P, NW, 1>(l, buf0, wg);
    __syncthreads();
    const int cq = l.mb * 8;    // float4 pieces of this workgroup's share of a row
    float *ob = a.out + ((size_t)b * a.N + n0) * a.C1 + mb0 * 32;
    for (int j = rg; j < P; j += RG) {
        const unsigned o = __umul24((unsigned)j, (unsigned)a.C1);
        for (int q = ql; q < cq; q += 32) *(float4 *)(ob + (o + 4u * q)) = *(const float4 *)(buf0 + L::off(4 * q, j));
    }
}

}  // namespace psg
