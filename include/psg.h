/*
 * psg.h -- C ABI of libpsg.so: the MI355X (gfx950) implementation of PointSecGuard's
 * data-parallel hot path (PointNet++ SSG semantic-segmentation forward + colour-gradient backward
 * inside the NB/NU colour-perturbation attack loops).
 *
 * The reference has no FFI layer: its boundary for this path is the Python API that the harness
 * scripts import.  Each entry point below names the reference expression it
 * replaces (paths relative to the reference checkout); INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless marked "host";
 *   - every call is stream-ordered and non-blocking on `stream` (a hipStream_t, 0 = default
 *     stream); no call synchronises the device or spawns threads;
 *   - objects (ctx / model / workspace) allocate their device memory at create time only;
 *   - return value: PSG_OK (0) or a negative PSG_ERR_*; psg_last_error() gives the thread-local text;
 *   - feature tensors are POINT-MAJOR fp32: [batch][points][channels]; indices are int32.
 */
#ifndef PSG_H
#define PSG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSG_OK 0
#define PSG_ERR_ARG (-1)   /* bad argument / unsupported size */
#define PSG_ERR_HIP (-2)   /* a HIP runtime call failed */
#define PSG_ERR_STATE (-3) /* object used out of order (e.g. backward before forward) */

typedef struct psg_ctx psg_ctx;
typedef struct psg_pn2_model psg_pn2_model;
typedef struct psg_pn2_ws psg_pn2_ws;
typedef void *psg_stream; /* hipStream_t */

const char *psg_last_error(void);
const char *psg_version(void);
/* Environment switches (all optional; they select between tested code paths or turn on diagnosis output).  Writes
 * "NAME=value:kind;..." for every switch libpsg knows that is SET in this process's environment ("" when none) and
 * returns their number (< 0: error).  kind: 'p' = another tested path with the same results (to rounding where a sum
 * changes order), 'd' = diagnosis output only, 'r' = changes results - timing bisection switches that exist only in
 * libraries built with -DPSG_DIAG_BUILD (psg_diag_build() == 1; the default library has none, and bench.py refuses to
 * run on such a library).  The reference has no counterpart: it is a measurement-hygiene entry point. */
int psg_env_switches(char *buf, int cap);
int psg_diag_build(void);

/* One context per (process, device). */
int psg_ctx_create(int device, psg_ctx **out);
int psg_ctx_destroy(psg_ctx *ctx);

/* ------------------------------------------------------------------------------------------
 * Geometry unit ops, batched over P independent problems.  Problem p reads cloud (p % n_clouds).
 * ------------------------------------------------------------------------------------------ */

/* square_distance, PointNet/models/pointnet_util.py:19-40: out[b][i][j] = ((-2*dot) + |src_i|^2) + |dst_j|^2
 * with the reference's fp32 evaluation order (bit-exact).  src [B][N][3], dst [B][M][3], out [B][N][M]. */
int psg_square_distance(psg_ctx *ctx, const float *src, const float *dst, int B, int N, int M, float *out,
                        psg_stream stream);

/* farthest_point_sample, PointNet/models/pointnet_util.py:63-84.
 * xyz [n_clouds][N][3]; start [P] = the torch.randint draw of :75; out_idx [P][S].
 * Lowest index wins distance ties (torch.max CPU behaviour).  N <= 8192. */
int psg_fps(psg_ctx *ctx, const float *xyz, int n_clouds, int P, int N, int S, const int32_t *start,
            int32_t *out_idx, psg_stream stream);

/* index_points, pointnet_util.py:43-60: out[p][s][:] = points[p % n_clouds][idx[p][s]][:]. */
int psg_gather_points(psg_ctx *ctx, const float *points, int n_clouds, int P, int N, int C, const int32_t *idx,
                      int S, float *out, psg_stream stream);

/* query_ball_point, pointnet_util.py:87-107.  xyz [n_clouds][N][3]; new_xyz [P][S][3];
 * r2 = float32(radius**2); out_idx [P][S][K]: first K indices j (ascending) with
 * !(square_distance(new_xyz, xyz) > r2), padded with the first hit.  N <= 8192. */
int psg_ball_query(psg_ctx *ctx, const float *xyz, int n_clouds, const float *new_xyz, int P, int N, int S,
                   float r2, int K, int32_t *out_idx, psg_stream stream);

/* 3-NN + inverse-distance weights, pointnet_util.py:301-307.  xyz1 [n_clouds1][N][3] (fine),
 * xyz2 [P][S][3] (coarse); out_idx/out_w [P][N][3].  Stable ascending order.  3 <= S <= 8192. */
int psg_three_nn(psg_ctx *ctx, const float *xyz1, int n_clouds1, const float *xyz2, int P, int N, int S,
                 int32_t *out_idx, float *out_w, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * PointNet++ SSG sem-seg network (get_model, PointNet/models/pointnet2_sem_seg.py:6-40), eval mode.
 * ------------------------------------------------------------------------------------------ */

#define PSG_PN2_NUM_LAYERS 23 /* sa1..sa4 (3 each), fp4, fp3, fp2 (2 each), fp1 (3), conv1, conv2 */
#define PSG_PN2_NUM_CLASSES 13
#define PSG_PN2_IN_CHANNELS 9
/* the two PointNet++ sem-seg architectures of the reference */
#define PSG_PN2_ARCH_SSG 0        /* PointNet/models/pointnet2_sem_seg.py: single-scale grouping, 23 conv layers */
#define PSG_PN2_ARCH_MSG 1        /* PointNet/models/pointnet2_sem_seg_msg.py: two radii per SA level, 35 conv layers */
#define PSG_PN2_MSG_NUM_LAYERS 35

/* Build the device-resident, MFMA-packed weights.  `weights[i]` / `biases[i]` are HOST pointers to the
 * row-major [cout][cin] weight and [cout] bias of layer i with the eval-mode BatchNorm already
 * folded in, in the order sa1.0-2, sa2.0-2, sa3.0-2, sa4.0-2, fp4.0-1, fp3.0-1, fp2.0-1, fp1.0-2,
 * conv1(+bn1), conv2.  Layer shapes are fixed by the architecture (pointnet2_sem_seg.py:9-19).
 * Blocking (uploads synchronously); not for use inside a timed loop. */
int psg_pn2_model_create(psg_ctx *ctx, const float *const *weights, const float *const *biases,
                         psg_pn2_model **out);
/* Same for either architecture.  PSG_PN2_ARCH_MSG (replaces pointnet2_sem_seg_msg.py:7-21 + pointnet_util.py:210-227)
 * takes its n_layers = 35 layers in state_dict order: sa1 scale 0 layers 0-2, sa1 scale 1 layers 0-2, sa2 ..., sa4
 * (conv_blocks.i.j + bn_blocks.i.j), fp4.0-1, fp3.0-1, fp2.0-1, fp1.0-2, conv1(+bn1), conv2. */
int psg_pn2_model_create_arch(psg_ctx *ctx, int arch, const float *const *weights, const float *const *biases,
                              int n_layers, psg_pn2_model **out);
int psg_pn2_model_destroy(psg_pn2_model *model);

/* Workspace: geometry plan for up to `max_forwards` forwards of a batch of `batch` rooms of
 * `n_point` points, plus activations / ReLU masks / gradient buffers for ONE forward in flight. */
int psg_pn2_ws_create(psg_ctx *ctx, int batch, int n_point, int max_forwards, psg_pn2_ws **out);
/* Workspace for a model of architecture `arch`; forward / backward / nb_attack refuse a mismatched pair. */
int psg_pn2_ws_create_arch(psg_ctx *ctx, int arch, int batch, int n_point, int max_forwards, psg_pn2_ws **out);
int psg_pn2_ws_destroy(psg_pn2_ws *ws);
size_t psg_pn2_ws_bytes(const psg_pn2_ws *ws);

/* Per-launch timing with HIP events recorded on the launch stream (bench.py's roofline figure).
 * While enabled every kernel launch of plan_build / forward / backward / nb_attack on this workspace is
 * bracketed by two events.  prof_read (blocking: waits for the events) sums the elapsed ms and counts per
 * kernel tag: 0-3 sa1-4 fwd, 4-7 fp1-4 fwd (4 = fp1+head), 8-11 fp1-4 bwd, 12-15 sa1-4 bwd, 16 fps,
 * 17 ball query, 18 three_nn, 19 gather, 20 ce grad, 21 pgd step, 22 input-gradient gather, 23 / 24 per-point first
 * layers fwd / bwd, 25-27 psg_pn2_backward_full only: g_rel rows, 3-NN weight gradients, per-level coordinate sums,
 * 28 packed-SA plan, 29 the NB loop's fp1+head forward, CE gradient and backward in one launch (then 4, 8 and 20 of that
 * loop are empty).  n_tags >= 30. */
int psg_pn2_prof_enable(psg_pn2_ws *ws, int on);
int psg_pn2_prof_read(psg_pn2_ws *ws, int n_tags, double *total_ms, int *counts);

/* Diagnostics (blocking): copies the in-kernel clock stamps written when the environment variable
 * PSG_DIAG has bit 256 set -- per workgroup of the fp1+head forward kernel {s_memtime, s_memrealtime} at
 * entry and exit -- used to report the shader clock the chip holds under this load. */
int psg_pn2_debug_read(psg_pn2_ws *ws, unsigned long long *host_out, int n_words);

/* Geometry for `n_forward` forwards at once (sample_and_group's FPS + ball query of the four SA
 * levels, and the 3-NN tables of the four FP levels; pointnet_util.py:110-143, :301-307).
 * x0 [batch][n_point][9] point-major rooms (only channels 0:3 are read);
 * starts [n_forward][4][batch] = the torch.randint draws in reference call order.
 * Geometry depends on xyz and the draws only, never on colour, so an attack builds it once for
 * all of its iterations (n_forward*batch independent problems fill the chip). */
int psg_pn2_plan_build(psg_pn2_ws *ws, const float *x0, const int32_t *starts, int n_forward, psg_stream stream);

/* Read-back of plan slices for parity tests (device pointers into the workspace).
 * what: 0 fps idx [S_l], 1 group idx [S_l][K] (MSG: scale 0, K = 16), 2 nn idx [N_l][3], 3 nn weights [N_l][3],
 * 4 xyz of level+1, 5 group idx of MSG scale 1 [S_l][32] (null for SSG);
 * packed SA forward (SSG, null under PSG_PN2_PACK=0): 6 valid rows per group, int32 [S_l]; 7 workgroup segmentation, int32
 * [S_l / G_l + 2] = {workgroups in use, first group of each, S_l} (G_l = 4, 2, 1, 1 groups per unpacked workgroup);
 * 8 (forward 0 only) the arg-max bytes [S_l][C3_l] that the resident forward left for `room`; 9 the workgroup descriptors,
 * int32 [S_l / G_l][4] = {first group | groups << 16 (0: workgroup not in use), valid rows - 1 of its groups, five bits each, six
 * to a word}.
 * The SA backward of a level runs over the same packed rows through the same descriptors where PSG_PN2_PACK_BWD (read once per
 * process) names the level: unset or 1 = the default set (levels 0 and 1: the levels whose launch is faster packed; levels 2 and
 * 3 have the kernel and are slower with it), 0 = none (the unpacked backward kernels and the unpacked-keyed ReLU masks), L followed
 * by level digits (L0, L0123) = exactly those levels, an error at launch where a named level does not fit the packed kernel's
 * configuration (SSG as shipped: level 0 whole, levels 1 - 3 split with the sparse max-pool transpose).  Results are the same
 * bytes under every value. */
const void *psg_pn2_plan_ptr(const psg_pn2_ws *ws, int what, int level, int forward, int room);

/* get_model.forward (pointnet2_sem_seg.py:22-40) with the geometry of plan slot `forward`.
 * x0 [batch][n_point][9]; logp_out [batch][n_point][13] = log_softmax; l4_out (nullable)
 * [batch][16][512] (MSG: [batch][16][1024]) = l4_points point-major.  Leaves the ReLU / arg-max masks in the
 * workspace.  For PSG_PN2_ARCH_MSG this is pointnet2_sem_seg_msg.py:23-42. */
int psg_pn2_forward(psg_pn2_model *model, psg_pn2_ws *ws, int forward, const float *x0, float *logp_out,
                    float *l4_out, psg_stream stream);

/* Input-gradient backward of the forward that last ran in `ws` (what autograd derives for a leaf on
 * the input features): dlogp [batch][n_point][13] = d loss / d log-probs;
 * dx0_out [batch][n_point][9] = d loss / d input features with the geometry treated as constant: channels
 * 3:9 are exact; channels 0:3 hold the feature path only and exclude the paths through relative coordinates and
 * 3-NN weights (the colour attacks never read them; psg_pn2_backward_full adds them).  No weight gradients (the
 * attack path never needs them). */
int psg_pn2_backward(psg_pn2_model *model, psg_pn2_ws *ws, int forward, const float *dlogp, float *dx0_out,
                     psg_stream stream);
/* The same contract with the COMPLETE derivative in dx0_out[.][0:3]: what the reference's autograd returns for a leaf on
 * the whole [B, 9, N] input - the feature path plus the relative coordinates of the four SA levels (pointnet_util.py:
 * 126-140, new_xyz = xyz[fps_idx] included) and the 3-NN interpolation weights of the four FP levels (:301-309), with the
 * FPS / ball-query / 3-NN indices constant.  Channels 3:9 are byte-identical to psg_pn2_backward.  No float atomics: two
 * runs are bit-equal.  PSG_PN2_ARCH_SSG only, with the split first layers (the default; not under PSG_PN2_SPLIT=0):
 * anything else returns PSG_ERR_ARG with a message, never a partial gradient. */
int psg_pn2_backward_full(psg_pn2_model *model, psg_pn2_ws *ws, int forward, const float *dlogp, float *dx0_out,
                          psg_stream stream);

/* The per-iteration launches of psg_pn2_nb_attack one at a time (round 6), so that a caller - the teacher-forced parity
 * tests - can drive exactly the kernels the fused attack loop runs between nontarget.py:29 and :39 / target.py:31 and :43:
 *   psg_pn2_forward_lean         psg_pn2_forward without the module outputs only psg_pn2_activation reads (no l4_out);
 *   psg_pn2_backward_colour      the input gradient on the colour channels only: dx0_out[.][3..5] are written, the other six
 *                                channels of a row are left untouched (level 0: compact rows, the first layer's three colour
 *                                columns on the vector pipe, one gather thread per point);
 *   psg_pn2_backward_colour_pgd  the same backward with the update of nontarget.py:37-39 / target.py:41-43 applied by the
 *                                gradient's last gather: x [batch][n_point][9] is updated in place on channels 3..5 exactly as
 *                                psg_pgd_step would (ori [batch][n_point][3], mask nullable [n_point], dir = +1 ascent / -1
 *                                descent, last = the reference's un-projected final step); no gradient is written. */
int psg_pn2_forward_lean(psg_pn2_model *model, psg_pn2_ws *ws, int forward, const float *x0, float *logp_out,
                         psg_stream stream);
int psg_pn2_backward_colour(psg_pn2_model *model, psg_pn2_ws *ws, int forward, const float *dlogp, float *dx0_out,
                            psg_stream stream);
int psg_pn2_backward_colour_pgd(psg_pn2_model *model, psg_pn2_ws *ws, int forward, const float *dlogp, float *x,
                                const float *ori, const uint8_t *mask, float alpha, float eps, float dir, int last,
                                psg_stream stream);

/* One iteration of psg_pn2_nb_attack's loop on plan slot `forward`, exactly as the attack runs it (its loop body is this call):
 * lean forward of x [batch][n_point][9], loss gradient (non-targeted: labels [batch][n_point], CE_sum / n_point; targeted:
 * labels ignored, class `target`, CE_mean of room 0), colour backward with the step applied to x in place (ori, mask, alpha,
 * eps, last as in psg_pn2_backward_colour_pgd).  By default fp1 + head forward, the loss gradient and fp1 + head backward are
 * ONE launch (same bits as the three launches, which PSG_PN2_FP1_LOOP=0 keeps); that launch writes neither log-probs nor masks
 * to memory, so afterwards NO forward is resident for psg_pn2_backward* - run psg_pn2_forward first. */
int psg_pn2_nb_step(psg_pn2_model *model, psg_pn2_ws *ws, int forward, float *x, const float *ori, const int32_t *labels,
                    const uint8_t *mask, float alpha, float eps, int targeted, int target, int last, psg_stream stream);
/* fp1's first-layer gradient rows [batch][n_point][128] as the last backward or step left them (what fp2's backward gathers;
 * with PSG_PN2_FPSPLIT=0 the rows are fp1's interpolated-input gradient instead).  Read-only device pointer, for tests. */
const float *psg_pn2_fp1_grad_ptr(const psg_pn2_ws *ws);

/* Per-layer activations of the last forward, for parity tests: which 0..3 = l1..l4 points (sa1..sa4
 * outputs), 4..6 = fp4, fp3, fp2 outputs.  Returns a device pointer [batch][points][channels]. */
const float *psg_pn2_activation_ptr(const psg_pn2_ws *ws, int which);
int psg_pn2_activation_channels(const psg_pn2_ws *ws, int which);   /* channels of that tensor (architecture dependent) */

/* ------------------------------------------------------------------------------------------
 * Attack-loop arithmetic (PointNet/attacks/torchattacks/attacks/nontarget.py, target.py).
 * ------------------------------------------------------------------------------------------ */

/* ------------------------------------------------------------------------------------------
 * Per-operator entry points: what the STAND-ALONE forwards of the reference's public modules run on
 * (inside get_model / DenseDeepGCN the same arithmetic is one fused kernel per module).  Point-major rows, device
 * pointers, stream-ordered, no allocation; BatchNorm (eval) is folded into w / bias by the caller.  Input gradients only.
 * ------------------------------------------------------------------------------------------ */
/* sample_and_group's row assembly, pointnet_util.py:126-140: rows[(b,s,k)] = [xyz[g] - new_xyz[s], feat[g]] with
 * g = gidx[b][s][k] (feat_first = 1: [feat, rel_xyz], the MSG order :251-254).  rows_out [B*S*K][3+D]. */
int psg_group_rows(const float *xyz, const float *feat, const float *new_xyz, const int32_t *gidx, int B, int N, int S,
                   int K, int D, int feat_first, float *rows_out, psg_stream stream);
/* its transpose w.r.t. the features (index_points backward, :136): dfeat [B][N][D], zeroed here. */
int psg_group_rows_bwd(const float *drows, const int32_t *gidx, int B, int N, int S, int K, int D, int feat_first,
                       float *dfeat, psg_stream stream);
/* one shared 1x1 convolution over rows (Conv -> BN(eval) -> ReLU, pointnet_util.py:200-203, 317-319):
 * out = [relu](in . w^T + bias) [* scale + shift], w [M][K]; scale / shift (or NULL): BatchNorm AFTER the ReLU, ResGCN's
 * BasicConv order (torch_nn.py:55-75); mask_out: ReLU bits [rows][ceil(M/32)] words or NULL (written with relu only).
 * Bit (c & 31) of word c >> 5 of a row is set where the pre-activation of channel c is > 0 (strictly).  Every word of
 * every row is written; the bits of the last word that lie at channels >= M are written as 0.  Columns >= M of an output
 * row with ld_out > M are not touched. */
int psg_pw_mlp_fwd(const float *in, int ld_in, int rows, int K, const float *w, const float *bias, int relu, int M,
                   float *out, int ld_out, uint32_t *mask_out, const float *scale, const float *shift, psg_stream stream);
/* its input gradient: din = (dout . w) * [ReLU bits of the layer below, or NULL]; wT [K][M] = w transposed. */
int psg_pw_mlp_bwd(const float *dout, int ld_dout, int rows, int M, const float *wT, const uint32_t *mask_below, int K,
                   float *din, int ld_din, psg_stream stream);
/* backward through a layer's own ReLU (and the BatchNorm scale after it, or NULL): g[row][c] = bit ? g * scale[c] : 0. */
int psg_apply_relu_bits(float *g, int ld, const uint32_t *bits, const float *scale, int rows, int M, psg_stream stream);
/* PointNetSetAbstraction.forward after grouping, pointnet_util.py:200-205: n_layers shared layers over the grouped rows
 * [n_groups*K][cin], max over the K samples.  scratch_a/b: [rows][max width]; masks[l]: ReLU bits of layer l (or NULL array);
 * out [n_groups][widths[n-1]], arg: winning sample (first on ties, like torch.max).  arg is a byte, so forward AND
 * backward require 1 <= K <= 255; both require 1 <= n_layers <= 8 and n_groups * K <= INT_MAX (anything else is
 * PSG_ERR_ARG before a launch). */
int psg_sa_mlp_max_fwd(const float *rows_in, int n_groups, int K, int cin, int n_layers, const int *widths,
                       const float *const *w, const float *const *bias, float *scratch_a, float *scratch_b,
                       uint32_t *const *masks, float *out, uint8_t *arg, psg_stream stream);
int psg_sa_mlp_max_bwd(const float *dout, const uint8_t *arg, int n_groups, int K, int cin, int n_layers,
                       const int *widths, const float *const *wT, const uint32_t *const *masks, float *scratch_a,
                       float *scratch_b, float *drows_in, psg_stream stream);
/* PointNetFeaturePropagation's interpolation + concat, pointnet_util.py:301-314: out [B][N][D1+D2] =
 * [feat1 (NULL when D1 = 0), sum_j w_j feat2[idx_j]]; idx / w from psg_three_nn. */
int psg_three_interp_fwd(const float *feat2, const int32_t *idx, const float *w, const float *feat1, int B, int N, int S,
                         int D1, int D2, float *out, psg_stream stream);
/* transpose: dfeat2 [B][S][D2] (zeroed here) += w_j * dout[b][n][col0 + c], dout rows of ld floats. */
int psg_three_interp_bwd(const float *dout, int ld, int col0, const int32_t *idx, const float *w, int B, int N, int S,
                         int D2, float *dfeat2, psg_stream stream);
/* pairwise_distance, ResGCN/gcn_lib/dense/torch_edge.py:32-42: x [B][N][C] -> out [B][N][N], the reference's fp32 order;
 * sq: scratch [B*N]. */
int psg_gcn_pairwise_distance(const float *x, int B, int N, int C, float *sq, float *out, psg_stream stream);
/* torch.max_pool2d(fusion, [N, 1]) of DenseDeepGCN.forward (ResGCN/sem_seg_dense/architecture.py:64) on point-major rows
 * x [B][N][C] (C a multiple of 64): out_max [B][C] = maximum over the N points, out_arg [B][C] = the row that holds it
 * (lowest row on equal values); scratch: [B*C] 8-byte words (cleared here).  SURVEY 8(b)'s `psg_global_max`. */
int psg_global_max(const float *x, int B, int N, int C, unsigned long long *scratch, float *out_max, int32_t *out_arg,
                   psg_stream stream);
/* EdgeConv2d.forward, torch_vertex.py:31-35 (BasicConv = Conv -> ReLU -> BatchNorm, torch_nn.py:55-75), 16 neighbours,
 * 64 output channels: y_i = max_k(scale * relu(W.[x_i, x_j - x_i] + b) + shift).  x [R][ld_x], nbr [R][16] room-local,
 * R = rooms * N; wcat [128][C] = [W1 - W2 ; W2], bcat [128] = [b, 0]; pq scratch [R][128]; arg [R][64]. */
int psg_edgeconv_fwd(const float *x, int ld_x, int R, int N, int C, const int32_t *nbr, const float *wcat,
                     const float *bcat, const float *scale, const float *shift, float *pq, float *out, int ld_out,
                     uint8_t *arg, psg_stream stream);
/* MRConv2d's gather, torch_vertex.py:16-19: cat [R][2C] = [x_i, max_k (x_j - x_i)], arg [R][C] = winning neighbour; the
 * BasicConv after it is psg_pw_mlp_fwd with scale / shift.  _bwd: dx [R][ld_dx] = dcat_x - dcat_m, + dcat_m at the winner. */
int psg_mrconv_gather_fwd(const float *x, int ld_x, int R, int N, int C, const int32_t *nbr, float *cat, uint8_t *arg,
                          psg_stream stream);
int psg_mrconv_gather_bwd(const float *dcat, int R, int N, int C, const int32_t *nbr, const uint8_t *arg, float *dx, int ld_dx,
                          psg_stream stream);
/* its input gradient: dx [R][ld_dx] (C columns); wcat_t [C][128]; dpq: scratch [R][128], holds [dP | dQ] when the
 * call returns (every element is written by the call: nothing needs zeroing; the result is bit-reproducible). */
int psg_edgeconv_bwd(const float *dy, int ld_dy, int R, int N, int C, const int32_t *nbr, const uint8_t *arg,
                     const float *scale, const float *wcat_t, float *dpq, float *dx, int ld_dx, psg_stream stream);

/* [B][C][N] channel-major (reference layout) <-> [B][N][C] point-major. */
int psg_to_point_major(const float *src_cn, int B, int C, int N, float *dst_nc, psg_stream stream);
int psg_to_channel_major(const float *src_nc, int B, int C, int N, float *dst_cn, psg_stream stream);

/* d/dlogp of scale * sum_i CE(logp_i, y_i) with CE applied ON TOP of the log-probs (a second
 * log_softmax), nontarget.py:26,34 / target.py:27,39.  labels [rows] int32, or a single class
 * when labels == NULL (`target`).  rows_active: only the first rows_active rows get a gradient
 * (target.py:36 uses batch row 0 only); the rest are zeroed.  cost_out (nullable): 1 float, += cost.
 * Every label must lie in [0, n_cls): the kernel does not check them. */
int psg_ce_logp_grad(const float *logp, const int32_t *labels, int target, int rows, int rows_active, int n_cls,
                     float scale, float *dlogp_out, float *cost_out, psg_stream stream);

/* One NB / tar_NB update on the colour channels 3:6 of point-major rooms x [B][N][9], in place:
 *   stepped = x + dir*alpha*sign(g);  eta = clamp(stepped - ori, -eps, eps);
 *   x = last ? stepped : clamp(ori + eta, 0, 1)          (nontarget.py:37-39, target.py:41-43)
 * `last` reproduces the reference returning the UN-projected final step.
 * grad [B][N][9] (channels 3:6 read), ori [B][N][3], mask (nullable) [N] uint8 shared by all rooms. */
int psg_pgd_step(float *x, const float *grad, const float *ori, const uint8_t *mask, int B, int N, float alpha,
                 float eps, float dir, int last, psg_stream stream);

/* The same update on either three-channel field of the rooms: c0 = 3 is psg_pgd_step (colours); c0 = 0 moves the
 * coordinates, channels 0:3 (the reference's loop body with the slice 0:3: sign step, eta clamped to +-eps, NO clamp to
 * [0, 1] - coordinates are metres).  ori [B][N][3] = the clean values of that field; grad channels c0:c0+3 are read. */
int psg_pgd_step_field(float *x, const float *grad, const float *ori, const uint8_t *mask, int B, int N, int c0,
                       float alpha, float eps, float dir, int last, psg_stream stream);

/* Fused NB_attack / tar_NB_attack on a batch (nontarget.py:18-42, target.py:18-45):
 * plan_build for `iters` forwards, then iters x (forward, CE grad, backward, pgd_step), all
 * stream-ordered on `stream` with no host synchronisation.
 * images/adv_out [B][9][N] channel-major (reference layout); labels [B][N] int32 (ignored when
 * targeted); starts [iters][4][B] int32 (device); mask (nullable) [N] uint8.
 * targeted = 0: ascent on CE_sum(all rooms)/N.  targeted = 1: descent on CE_mean(room 0, target). */
int psg_pn2_nb_attack(psg_pn2_model *model, psg_pn2_ws *ws, const float *images, const int32_t *labels,
                      const int32_t *starts, const uint8_t *mask, float eps, float alpha, int iters, int targeted,
                      int target, float *adv_out, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * Vanilla PointNet sem-seg network (get_model, PointNet/models/pointnet_sem_seg.py:8-38 with pointnet.py:10-130:
 * STN3d, PointNetEncoder(global_feat=False, feature_transform=True, channel=6), STNkd), eval mode.
 * ------------------------------------------------------------------------------------------ */
typedef struct psg_pointnet_model psg_pointnet_model;
typedef struct psg_pointnet_ws psg_pointnet_ws;
#define PSG_POINTNET_NUM_LAYERS 19
#define PSG_POINTNET_NUM_CLASSES 13
#define PSG_POINTNET_POINT_TILE 128  /* n_point must be a multiple of this */

/* weights[l] [out][in] row-major and biases[l] [out] (HOST pointers, BatchNorm folded, runtime.fold_pointnet_state_dict),
 * l in this order (out x in):
 *   feat.stn  conv1 64x6, conv2 128x64, conv3 1024x128, fc1 512x1024, fc2 256x512, fc3 9x256 (bias + identity)
 *   feat.conv1 64x6
 *   feat.fstn conv1 64x64, conv2 128x64, conv3 1024x128, fc1 512x1024, fc2 256x512, fc3 4096x256 (bias + identity)
 *   feat.conv2 128x64, feat.conv3 1024x128
 *   conv1 512x1088 (columns: [global 1024 | pointfeat 64]), conv2 256x512, conv3 128x256, conv4 13x128 */
int psg_pointnet_model_create(psg_ctx *ctx, const float *const *weights, const float *const *biases,
                              psg_pointnet_model **out);
int psg_pointnet_model_destroy(psg_pointnet_model *model);
/* Activations and gradient buffers for `batch` rooms of n_point points (a multiple of PSG_POINTNET_POINT_TILE). */
int psg_pointnet_ws_create(psg_ctx *ctx, int batch, int n_point, psg_pointnet_ws **out);
int psg_pointnet_ws_destroy(psg_pointnet_ws *ws);
/* x0 [B][N][9] point-major (channels 6:9 are not read: the reference uses x[:, :6]); logp_out [B][N][13] (nullable);
 * trans_out [B][3][3], trans_feat_out [B][64][64], pool_out [B][3][1024] (the pooled vectors of STN3d, STNkd and the
 * encoder; STN ones after their ReLU), arg_out [B][3][1024] (first arg-max point of each pooled channel): all nullable. */
int psg_pointnet_forward(psg_pointnet_model *model, psg_pointnet_ws *ws, const float *x0, float *logp_out, float *trans_out,
                         float *trans_feat_out, float *pool_out, int32_t *arg_out, psg_stream stream);
/* Input gradient of the last forward: dlogp [B][N][13], dtrans_feat [B][64][64] (nullable: the upstream gradient of
 * trans_feat, e.g. from get_loss's regulariser); dx0_out [B][N][9], channels 6:9 exactly zero. */
int psg_pointnet_backward(psg_pointnet_model *model, psg_pointnet_ws *ws, const float *dlogp, const float *dtrans_feat,
                          float *dx0_out, psg_stream stream);
/* Fused NB_attack / tar_NB_attack for this network: iters x (forward, psg_ce_logp_grad, backward, psg_pgd_step),
 * stream-ordered; arguments as psg_pn2_nb_attack without the FPS starts (the network draws no random numbers). */
int psg_pointnet_nb_attack(psg_pointnet_model *model, psg_pointnet_ws *ws, const float *images, const int32_t *labels,
                           const uint8_t *mask, float eps, float alpha, int iters, int targeted, int target, float *adv_out,
                           psg_stream stream);
/* Read-only tap into the workspace (tests): the device pointer of a named buffer with its row and column counts; NULL
 * with the error string set for a null workspace or an unknown `what`.  Launches nothing, allocates nothing, does not
 * synchronise.  float32 unless noted; B rooms of N points, R = B N rows, T = R / PSG_POINTNET_POINT_TILE tiles.
 *   forward state, valid from a forward call until the next forward call:
 *     per point:  0 a1 [R][64]  1 a2 [R][128]  2 h [R][64]  3 k1 [R][64]  4 k2 [R][128]  5 e2 [R][128]  6 z1 [R][512]
 *       7 z2 [R][256]  8 z3 [R][128]  9 logits [R][13]  10 logp [R][13]  11 x0in [R][9] (the forward's input)
 *     ReLU bits, uint32 words, cols = words per row, bit c%32 of word c/32 = (activation > 0):
 *       20 mh [R][2]  21 m1 [R][16]  22 m2 [R][8]  23 m3 [R][4]  24 mf1 [B][16]  25 mf2 [B][8]  26 mfk1 [B][16]  27 mfk2 [B][8]
 *     pools, columns [STN3d 1024 | STNkd 1024 | encoder 1024]:  30 pool [B][3072]  31 pidx [B][3072] (int32, room-local)
 *       32 part_val [T][1024]  33 part_idx [T][1024] (int32): the per-tile partial maxima; all three pooled layers write
 *       them in turn, so after a forward they hold the ENCODER pool's tiles only
 *     per room:  40 f1 [B][512]  41 f2 [B][256]  42 trans [B][9]  43 fk1 [B][512]  44 fk2 [B][256]  45 tf [B][4096]
 *       46 t1 [64][3B]  47 w1f [64B][8] (room b = rows 64b .. 64b+63)  48 c2f [128][64B]  49 h1pf [512][64B]  50 gb [B][512]
 *   gradient state, valid from a backward call until the next backward call:
 *     60 dz4 [R][13]  61 dz3 [R][128]  62 dz2 [R][256]  63 dz1 [R][512]  64 s1 [B][512]  65 dg [B][1024]  66 dpf [R][64]
 *     67 ht [64B][N]  68 dpft [64B][N] (the per-room transposes of h and dpf)  69 dtf [B][4096]  70 dfk2 [B][256]
 *     71 dfk1 [B][512]  72 dgk [B][1024]  73 dh [R][64]  74 dxu [R][8]  75 dtrans [B][9]  76 df2 [B][256]  77 df1 [B][512]
 *     78 dgs [B][1024]
 * The attack loops (psg_pointnet_nb_attack, psg_pointnet_nu_window) run forwards and backwards of their own in the same
 * workspace: after one of them the buffers hold its last iteration. */
const void *psg_pointnet_debug_ptr(const psg_pointnet_ws *ws, int what, int *rows_out, int *cols_out);

/* ---- NU (Adam in tanh space) attack arithmetic: nontarget.py:52-135, target.py:62-175 -------------
 * w / m / v are [B][N][3] fp32 (the attack variable and its Adam moments); colours live in channels 3:6
 * of the point-major rooms x0 [B][N][9]; `mask` (nullable, [N] uint8) restricts every op to masked points. */

/* w = 0.5*log((1+x)/(1-x)), x = 2c-1 (inverse_tanh_space, nontarget.py:110-116). */
int psg_nu_inverse_tanh(const float *x0, int B, int N, float *w_out, psg_stream stream);

/* colour = 1/2*(tanh(w)+1) written into x0 (tanh_space, nontarget.py:107-108). */
int psg_nu_tanh_color(const float *w, const uint8_t *mask, int B, int N, float *x0, psg_stream stream);

/* f-loss (nontarget.py:119-128 / target.py:148-168): per point clamp(tsign*(p_y - max_{k!=y} p_k), min=-kappa)
 * on p = softmax(log-probs); y = labels[row] or `target` when labels == NULL.  Writes d(sum f)/d(logp),
 * adds the sum to *f_sum (nullable) and the arg-max class to pred_out (nullable).  Every label must lie in
 * [0, n_cls): the kernel indexes the row with it unchecked (the same holds for the _rooms entry point). */
int psg_nu_f_loss_grad(const float *logp, const int32_t *labels, int target, int rows, int n_cls, float kappa,
                       float tsign, float *dlogp_out, float *f_sum, int32_t *pred_out, psg_stream stream);

/* f-loss of the ResGCN NU attacks on raw logits [rows][n_cls] (ResGCN/.../attacks/colper.py:108-113,
 * tcolper.py:145-163); the reference's one-hot masking makes a 0 take part in each max.  mode 0 = NU_attack.f over
 * all rows; mode 1 = tar_NU non_f, mode 2 = tar_NU tar_f (class `target`), both over batch row 0 under `mask` only.
 * Writes scale * d(sum f)/d(logits), adds sum f to *f_sum (nullable), arg-max class to pred_out (nullable).
 * Each max is torch.max's: the FIRST maximum among the class slots, the zeroed ones included, takes the gradient.
 * Every label must lie in [0, n_cls): the kernel indexes the row with it unchecked. */
int psg_gcn_f_loss_grad(const float *logits, const int32_t *labels, int target, const uint8_t *mask, int mode, int rows,
                        int n_point, int n_cls, float kappa, float tsign, float scale, float *dlogits_out, float *f_sum,
                        int32_t *pred_out, psg_stream stream);

/* Smooth loss (nontarget.py:131-135): for each of the N adversarial colours (rows of `adv_color`, stride
 * in floats) the nb smallest Euclidean distances to the N reference colours; adds their total to *dist_sum
 * and writes d(total)/d(adv colour) to grad_out [N][3].  Distances are evaluated directly (the reference's
 * cdist's matmul-expansion distance is reproduced).  Passing ref_color == adv_color selects the ResGCN
 * variants' smooth(adv, adv) (colper.py:115-120): the gradient then flows through both arguments.  nb <= 16, N <= 8192. */
int psg_smooth_knn(const float *adv_color, int adv_stride, const float *ref_color, int ref_stride, int N, int nb,
                   float *dist_sum, float *grad_out, psg_stream stream);

/* One optimiser step: g = dx0[colour] + 2*c_l2*(colour - ori) (+ c_smooth*smooth_grad on room 0), chained
 * through tanh_space, then torch.optim.Adam's single-tensor update (betas, eps, bias correction for `step`
 * >= 1) on w/m/v in place.  Adds sum((colour-ori)^2) to *l2_sum (nullable). */
int psg_nu_adam_step(float *w, float *m, float *v, const uint8_t *mask, const float *dx0, const float *x0,
                     const float *ori, const float *smooth_grad, float c_smooth, float c_l2, float lr, float beta1,
                     float beta2, float eps, int step, int B, int N, float *l2_sum, psg_stream stream);

/* B INDEPENDENT one-room attacks advanced in lockstep: the reference's NU / tar_NU attack called once per room
 * (target.py:62-133 and nontarget.py:52-105 at B = 1; BASELINE configs[2] applied per room), served by one launch per
 * operation instead of B.  Same arithmetic per room as the entry points above; what differs is the bookkeeping: the mask
 * is [B][N] (every room its own mask row), the smoothness term is evaluated for every room (grad_out [B][N][3]), the
 * loss sums are per room ([B] floats) and rooms whose loop has ended (room_active[b] == 0, nullable = all active) are
 * left untouched by the optimiser step.  N must be a multiple of 64 for the f-loss sums. */
int psg_nu_tanh_color_rooms(const float *w, const uint8_t *mask_rooms, int B, int N, float *x0, psg_stream stream);
int psg_nu_f_loss_grad_rooms(const float *logp, const int32_t *labels, int target, int B, int N, int n_cls, float kappa,
                             float tsign, float *dlogp_out, float *f_sum_rooms, int32_t *pred_out, psg_stream stream);
/* nn_state (nullable): int32 [B][N][nb], the neighbour indices of every colour; written by every call, and with
 * have_prev != 0 read first: the largest current distance to last call's neighbours is a rigorous upper bound of the
 * nb-th smallest distance, so the scan starts from it (same result; the optimiser moves colours a little per step). */
int psg_smooth_knn_rooms(const float *adv_color, int adv_stride, size_t adv_room_stride, const float *ref_color,
                         int ref_stride, size_t ref_room_stride, int B, int N, int nb, float *dist_sum_rooms,
                         float *grad_out, int32_t *nn_state, int have_prev, psg_stream stream);
int psg_nu_adam_step_rooms(float *w, float *m, float *v, const uint8_t *mask_rooms, const float *dx0, const float *x0,
                           const float *ori, const float *smooth_grad_rooms, float c_smooth, float c_l2, float lr,
                           float beta1, float beta2, float eps, int step, int B, int N, const uint8_t *room_active,
                           float *l2_sum_rooms, psg_stream stream);

/* The ResGCN f-loss (colper.py:108-113, tcolper.py:145-163) for G INDEPENDENT one-room attacks in one launch: per room what
 * psg_gcn_f_loss_grad does for a batch of one with that room's mask row (mask_rooms [G][N], nullable in mode 0) - the same
 * decisions (torch.max's first maximum, the zeroed slots taking part), dlogits_out [G][N][n_cls] and pred_out [G][N]
 * bit for bit.  Adds sum f of room g to f_sum_rooms[g] with one float atomic per workgroup. */
int psg_gcn_f_loss_grad_rooms(const float *logits, const int32_t *labels, int target, const uint8_t *mask_rooms, int mode,
                              int G, int N, int n_cls, float kappa, float tsign, float scale, float *dlogits_out,
                              float *f_sum_rooms, int32_t *pred_out, psg_stream stream);

/* smooth(adv, adv) of the ResGCN NU attacks (colper.py:115-120, tcolper.py:165-170) for G rooms: every colour's nb nearest
 * colours of its OWN room, the gradient flowing through both ends of every pair.  Strided rows and per-room strides in
 * floats, nb <= 16, N <= 8192; dist_sum_rooms [G] is added to, grad_out [G][N][3] written, a room with room_active[g] == 0
 * (nullable = all active) is not touched (sum, gradient, lists).  nn_out (nullable; the call then keeps the lists in a
 * scratch buffer of its own): int32 [G][N][nb], every colour's neighbours in rank order (with fewer than nb colours in the
 * room the missing ranks stay as they are).  Pair values are psg_smooth_knn's: d^2 = fma(-2 a.z, r.z, fma(-2 a.y, r.y,
 * -2 a.x * r.x)) + |a|^2 + |r|^2 clamped at 0 (the cdist expansion), neighbours strictly by (distance, index) - the one-room
 * kernel can order references at EXACTLY the same distance otherwise, DESIGN.md section 5m -, a pair at d == 0 adds exactly zero, u = (a - r) / d goes with + to the query and with - to the neighbour.  No float atomics on the
 * gradient and a FIXED order: a colour's own terms in ascending rank, then the terms it receives as a neighbour in
 * ascending index of the colour they come from.  Two launches for all rooms. */
int psg_smooth_knn_sym_rooms(const float *adv_color, int adv_stride, size_t adv_room_stride, int G, int N, int nb,
                             float *dist_sum_rooms, float *grad_out, const uint8_t *room_active, int32_t *nn_out,
                             psg_stream stream);

/* Per-step statistics and exit latch of the NU attacks: what the reference evaluates on the host after every optimiser
 * step - nontarget.py:87,95-96 (`correct / 4096 < 1 / 13`), target.py:105-121 (`target_acc` > 0.9, or < 1 / 13 for the
 * untargeted goal) - for G attacks of `rows` batch rows each (rows = B: one call on a batch; rows = 1: rooms in lockstep).
 * mode 0 = NU_attack, 1 = tar_NU_attack without a target (hits = correct points on the mask), 2 = with a target (hits =
 * points on the mask predicted as `target`).  scal [3][G]: the step's f / Smooth / L2 sums, moved into hist_step [5][G]
 * = {n_correct, n_hits, f, Smooth, L2} and zeroed.  The first step whose test fires copies the group's x0 rows
 * [rows][N][9] into out_cn [rows][9][N], stores the step in exit_step [G] (-1 before) and clears active [G]. */
int psg_nu_step_latch(const int32_t *pred, const int32_t *labels, int target, const uint8_t *mask_groups,
                      const int32_t *n_mask, int G, int rows, int N, int mode, float *scal, float *hist_step,
                      const float *x0, float *out_cn, uint8_t *active, int32_t *exit_step, int step, psg_stream stream);

/* A WINDOW of consecutive optimiser steps of NU_attack / tar_NU_attack on a PointNet++ network, enqueued by ONE call:
 * per step exactly the sequence the host loop of the reference runs (nontarget.py:77-96, target.py:93-121) -
 * psg_nu_tanh_color(_rooms), psg_pn2_forward on plan slot slot0 + i, psg_nu_f_loss_grad(_rooms), psg_pn2_backward,
 * psg_smooth_knn_rooms, psg_nu_adam_step(_rooms), psg_nu_step_latch - with the same arguments those entry points take.
 * (G, rows) = (1, B): one attack on a batch of B rows; (R, 1): R one-room attacks in lockstep.  The reference's host work
 * (restart test, learning-rate halving, exit) sits between windows; inside one nothing returns to the host. */
typedef struct psg_nu_window_args {
    psg_pn2_model *model;
    psg_pn2_ws *ws;
    int slot0, step0, n_steps;   /* steps step0 .. step0 + n_steps - 1 use plan slots slot0 .. */
    int G, rows, N, mode;        /* mode: see psg_nu_step_latch */
    int use_target, target;      /* the f-loss takes `target` instead of the labels */
    int neighbour, warm_first;   /* Smooth term: neighbour count; 1 = nn_state holds the previous step's lists */
    int adam_t0;                 /* optimiser steps taken since the optimiser was created */
    float kappa, tsign, c_smooth, c_l2, lr, beta1, beta2, eps;
    float *w, *m, *v;            /* [G*rows][N][3] */
    const uint8_t *mask;         /* [G][N] (rows = 1) or [N] (G = 1), nullable for NU_attack */
    const int32_t *n_mask;       /* [G], modes 1 and 2 */
    float *x0;                   /* [G*rows][N][9] */
    const float *ori;            /* [G*rows][N][3] */
    const int32_t *labels;       /* [G*rows][N] */
    float *logp, *dlogp, *dx0;   /* [G*rows][N][13], [..][13], [..][9] scratch */
    float *sgrad;                /* [G][N][3] */
    int32_t *pred;               /* [G*rows][N] */
    float *scal;                 /* [3][G], zero before the first window */
    int32_t *nn_state;           /* [G][N][neighbour] */
    float *hist;                 /* history rows [5][G] of the window's steps, row of step0 first */
    float *out;                  /* [G*rows][9][N] */
    uint8_t *active;             /* [G] */
    int32_t *exit_step;          /* [G] */
} psg_nu_window_args;
/* `graph` (nullable): a handle that lets windows of one SHAPE (same buffers, plan slots and step count; only step0, adam_t0
 * and lr differ) be replayed as a hipGraph - the first such window runs eagerly, the second is captured, later ones are
 * replayed with their step constants read from a device row.  Same results as the eager sequence. */
#define PSG_NU_GRAPH_MAX_STEPS 16
typedef struct psg_nu_graph psg_nu_graph;
int psg_nu_graph_create(psg_nu_graph **out);
int psg_nu_graph_destroy(psg_nu_graph *graph);
int psg_pn2_nu_window(const psg_nu_window_args *args, psg_nu_graph *graph, psg_stream stream);
/* Bookkeeping of a handle: out4 = {captures tried, captures failed, windows replayed as a graph, windows run eagerly}.  A
 * failed capture (the legacy default stream refuses capture; another API call can invalidate one) costs speed, not
 * correctness - the window runs eagerly - so it is counted instead of raised, and not retried for the same shape. */
int psg_nu_graph_stats(const psg_nu_graph *graph, long long *out4);
/* The same four counters summed over every replayed loop of the process (psg_pn2_nu_window, psg_gcn_nb_attack,
 * psg_rla_bim_attack; for the last two the unit is an attack iteration). */
int psg_capture_stats(long long *out4);

/* The same window on the vanilla PointNet network: per step psg_nu_tanh_color(_rooms), the PointNet forward, the f-loss
 * gradient, the PointNet input-gradient backward (no upstream gradient of trans_feat), psg_smooth_knn_rooms,
 * psg_nu_adam_step(_rooms), psg_nu_step_latch.  The fields are those of psg_nu_window_args without the plan slots (this
 * network draws no FPS starts).  fused_head != 0: the seam between forward and backward - log-softmax, f-loss gradient,
 * log-softmax backward - is one kernel on the head's logits (same dz and pred bit for bit; logp / dlogp are not used);
 * fused_head == 0: the three kernels, as the per-step entry points run them (dlogp required; logp, if given, receives the
 * step's log-probs).  `graph` as for the PointNet++ window; the captured sequence is a single chain on `stream`. */
typedef struct psg_pointnet_nu_window_args {
    psg_pointnet_model *model;
    psg_pointnet_ws *ws;         /* created for G*rows rooms of N points */
    int step0, n_steps;
    int G, rows, N, mode;
    int use_target, target;
    int neighbour, warm_first;
    int adam_t0, fused_head;
    float kappa, tsign, c_smooth, c_l2, lr, beta1, beta2, eps;
    float *w, *m, *v;            /* [G*rows][N][3] */
    const uint8_t *mask;         /* [G][N] (rows = 1) or [N] (G = 1), nullable for NU_attack */
    const int32_t *n_mask;       /* [G], modes 1 and 2 */
    float *x0;                   /* [G*rows][N][9] */
    const float *ori;            /* [G*rows][N][3] */
    const int32_t *labels;       /* [G*rows][N] */
    float *logp, *dlogp, *dx0;   /* [G*rows][N][13] nullable, [..][13] (fused_head == 0), [..][9] */
    float *sgrad;                /* [G][N][3] */
    int32_t *pred;               /* [G*rows][N] */
    float *scal;                 /* [3][G], zero before the first window */
    int32_t *nn_state;           /* [G][N][neighbour] */
    float *hist;                 /* history rows [5][G] of the window's steps, row of step0 first */
    float *out;                  /* [G*rows][9][N] */
    uint8_t *active;             /* [G] */
    int32_t *exit_step;          /* [G] */
} psg_pointnet_nu_window_args;
int psg_pointnet_nu_window(const psg_pointnet_nu_window_args *args, psg_nu_graph *graph, psg_stream stream);

/* The seam of that window on its own: logits [B][N][13] (N a multiple of PSG_POINTNET_POINT_TILE) -> dz_out [B][N][13] (the
 * gradient of the logits), pred_out [B][N], and the f sums ADDED to f_sum ([B] when per_room, else one float).  With both
 * scratch arrays ([B][N][13] each) it runs the three kernels of the per-step path, without them the fused kernel.
 * logits and dz_out must be 16-byte aligned (the fused kernel moves them as 16-byte words). */
int psg_pointnet_nu_head(const float *logits, const int32_t *labels, int target, int B, int N, int per_room, float kappa,
                         float tsign, float *logp_scratch, float *dlogp_scratch, float *dz_out, float *f_sum,
                         int32_t *pred_out, psg_stream stream);

/* The restart of tar_NU_attack (target.py:127-132) for the groups flags [G] selects (non-zero), in one launch: the group's
 * noise block [rows][3][n_mask[g]] (at float offset noise_off[g] of `noise`, laid out as torch.empty(rows, 3, k).uniform_
 * fills it) is added to the masked colours, entry j to the j-th masked point in ascending order; ALL nine channels of the
 * group's rows are clamped to [0, 1]; extra_l2[g] = sum((x0 - x0_orig)^2) over channels 0:3 and 6:9 in a fixed order.
 * x0 / x0_orig [G*rows][N][9], mask_groups [G][N].  Groups that are not flagged are left untouched, extra_l2 included. */
int psg_nu_restart_rooms(float *x0, const float *x0_orig, const uint8_t *mask_groups, const int32_t *n_mask,
                         const uint8_t *flags, const float *noise, const long long *noise_off, int G, int rows, int N,
                         float *extra_l2, psg_stream stream);

/* ---- NU attacks on the COORDINATE field (channels 0:3) of the PointNet++ SSG network: an extension of the reference API,
 * rooms form only (B independent one-room attacks in lockstep, B >= 1).  The attack variable delta [B][N][3] (metres) is
 * optimised directly by Adam - no tanh space, coordinates have no box -, xyz = ori_xyz + delta. */

/* The Smooth term (nontarget.py:131-135) on coordinates: the contract of psg_smooth_knn_rooms (strided rows, per-room strides
 * in floats, nb <= 16, N <= 8192, dist_sum_rooms [B] added to, grad_out [B][N][3] written) with the distance evaluated on
 * DIRECT differences, d^2 = fma(dz, dz, fma(dy, dy, dx * dx)), dx = a.x - r.x, d = sqrt(d^2): |d_fp32 - d| <= 4 * 2^-24 d,
 * where the matmul expansion of psg_smooth_knn_rooms leaves ~1e-3 m on coordinates in metres.  Neighbours by (distance,
 * index), the lower index first; the gradient sum_j (a - r_j) / d_j adds up in ascending rank order and a neighbour at
 * d_j == 0 adds exactly zero.  room_active [B] (nullable = all): an inactive room is not touched (sum, gradient, lists).
 * nn_out (nullable): int32 [B][N][nb] receives every point's neighbour indices in rank order (a room with fewer than nb
 * references leaves the missing ranks as they are). */
int psg_smooth_knn_xyz_rooms(const float *adv_xyz, int adv_stride, size_t adv_room_stride, const float *ref_xyz,
                             int ref_stride, size_t ref_room_stride, int B, int N, int nb, float *dist_sum_rooms,
                             float *grad_out, const uint8_t *room_active, int32_t *nn_out, psg_stream stream);
/* x0[b][i][0:3] = ori_xyz[b][i] + delta[b][i] for the points under mask_rooms [B][N] (nullable = all) of active rooms;
 * every other byte of x0 [B][N][9] stays. */
int psg_nu_coord_apply_rooms(const float *delta, const float *ori_xyz, const uint8_t *mask_rooms, int B, int N,
                             const uint8_t *room_active, float *x0, psg_stream stream);
/* One optimiser step on delta: g = dx0[.][0:3] + 2 coord_c delta + coord_c sgrad_xyz (nullable), then torch.optim.Adam's
 * single-tensor update (betas, eps, bias correction for `step` >= 1, step size coord_lr) of delta / m / v [B][N][3] in
 * place, on masked points of active rooms.  Adds sum(delta^2) of the delta the step started from to l2_sum_rooms [B]
 * (nullable); the slot of an inactive room is not touched. */
int psg_nu_coord_adam_step_rooms(float *delta, float *m, float *v, const uint8_t *mask_rooms, const float *dx0,
                                 const float *sgrad_xyz, float coord_c, float coord_lr, float beta1, float beta2, float eps,
                                 int step, int B, int N, const uint8_t *room_active, float *l2_sum_rooms, psg_stream stream);
/* The same step with separate weights, g = dx0[.][0:3] + 2 c_l2 delta + c_smooth sgrad_xyz (the ResGCN costs weigh the two
 * terms differently); with c_smooth == c_l2 the results of psg_nu_coord_adam_step_rooms bit for bit.  Inside a window of
 * psg_gcn_nu_field_window the step size coord_lr / (1 - beta1^t) and sqrt(1 - beta2^t) come from the window's device row
 * (slots 3 and 2) instead of the arguments - the same values. */
int psg_nu_coord_adam_step_rooms_w(float *delta, float *m, float *v, const uint8_t *mask_rooms, const float *dx0,
                                   const float *sgrad_xyz, float c_smooth, float c_l2, float coord_lr, float beta1, float beta2,
                                   float eps, int step, int B, int N, const uint8_t *room_active, float *l2_sum_rooms,
                                   psg_stream stream);
/* smooth(adv, adv) on coordinates: the ResGCN Smooth term (colper.py:115-120, tcolper.py:165-170) on channels 0:3 for G rooms
 * in lockstep - every point takes the nb nearest points of its OWN moved room, itself included, and the gradient flows
 * through both ends of every pair.  The contract of psg_smooth_knn_sym_rooms (strided rows, per-room stride in floats,
 * nb <= 16, N <= 8192, dist_sum_rooms [G] added to, grad_out [G][N][3] written, an inactive room not touched in sum,
 * gradient or lists, nn_out nullable with a scratch buffer of the call's own) with the pair values of
 * psg_smooth_knn_xyz_rooms: d = sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) on direct differences, neighbours by (distance,
 * index), u = (a_i - a_j) / d with + to the query and - to the neighbour, a pair at d == 0 adds exactly zero.  No float
 * atomics on the gradient and a FIXED order: a point's own terms in ascending rank, then the terms it receives as a
 * neighbour in ascending index of the point they come from.  Two launches for all rooms. */
int psg_smooth_knn_xyz_sym_rooms(const float *adv_xyz, int adv_stride, size_t adv_room_stride, int G, int N, int nb,
                                 float *dist_sum_rooms, float *grad_out, const uint8_t *room_active, int32_t *nn_out,
                                 psg_stream stream);

/* ONE step of NU_attack / tar_NU_attack(field = "coord" | "both") for G one-room attacks, enqueued on `stream`:
 * psg_nu_coord_apply_rooms (both: + psg_nu_tanh_color_rooms), psg_pn2_plan_build(n_forward = 1) from the moved points
 * into plan slot 0, psg_pn2_forward, psg_nu_f_loss_grad_rooms, psg_pn2_backward_full, (both: psg_smooth_knn_rooms on the
 * colours,) psg_smooth_knn_xyz_rooms, (both: psg_nu_adam_step(_rooms) on w,) psg_nu_coord_adam_step_rooms,
 * psg_nu_step_latch - whose exit snapshot therefore carries the moved coordinates and lags the optimiser by one step,
 * like the colour loop.  Cost = f + c (Smooth_rgb + L2_rgb) + coord_c (Smooth_xyz + L2_xyz), the colour terms with
 * field both only.  PSG_PN2_ARCH_SSG with the split first layers only: anything else returns PSG_ERR_ARG with a message
 * before anything is enqueued.  N must be a multiple of 64 (psg_nu_f_loss_grad_rooms). */
#define PSG_NU_FIELD_COORD 1
#define PSG_NU_FIELD_BOTH 2
typedef struct psg_nu_field_args {
    psg_pn2_model *model;
    psg_pn2_ws *ws;              /* created for G rooms of N points; plan slot 0 is rebuilt by every step */
    int step, adam_t;            /* the step's number (exit latch); optimiser steps since the optimiser was created, this one included (>= 1) */
    int G, N, mode;              /* mode: see psg_nu_step_latch */
    int use_target, target;      /* the f-loss takes `target` instead of the labels */
    int neighbour, warm;         /* Smooth terms: neighbour count; 1 = nn_state holds the previous step's colour lists */
    int field;                   /* PSG_NU_FIELD_COORD or PSG_NU_FIELD_BOTH */
    float kappa, tsign, c, lr, coord_c, coord_lr, beta1, beta2, eps;
    float *w, *m, *v;            /* [G][N][3] colour variable and moments (field both) */
    float *delta, *m_xyz, *v_xyz;   /* [G][N][3] coordinate variable and moments */
    const float *ori_xyz;        /* [G][N][3] the clean coordinates */
    const uint8_t *mask;         /* [G][N], nullable for NU_attack */
    const int32_t *n_mask;       /* [G], modes 1 and 2 */
    float *x0;                   /* [G][N][9] */
    const float *ori;            /* [G][N][3] the clean colours (field both) */
    const int32_t *labels;       /* [G][N] */
    const int32_t *starts;       /* [4][G] this step's FPS start indices */
    float *logp, *dlogp, *dx0;   /* [G][N][13], [..][13], [..][9] scratch */
    float *sgrad, *sgrad_xyz;    /* [G][N][3] each (sgrad: field both) */
    int32_t *pred;               /* [G][N] */
    float *scal;                 /* [5][G] f, Smooth_rgb, L2_rgb, Smooth_xyz, L2_xyz; zero before the first step */
    int32_t *nn_state;           /* [G][N][neighbour] (field both) */
    float *hist;                 /* this step's history row [7][G]: the latch's five entries, then Smooth_xyz, L2_xyz */
    float *out;                  /* [G][9][N] */
    uint8_t *active;             /* [G] */
    int32_t *exit_step;          /* [G] */
} psg_nu_field_args;
int psg_pn2_nu_field_step(const psg_nu_field_args *args, psg_stream stream);

/* Segmentation statistics of NB_nontarget_test_semseg.py:199-205: for every class l accumulates
 * seen[l] += #(gt==l), inter[l] += #(pred==l & gt==l), uni[l] += #(pred==l | gt==l) where
 * pred = argmax(logp) (first index on ties).  counters: int64 [3][n_cls] = seen, inter, uni.
 * pred_out (nullable) int32 [rows].  Every label must lie in [0, n_cls): the counters are indexed with it unchecked. */
int psg_seg_stats(const float *logp, const int32_t *labels, int rows, int n_cls, long long *counters,
                  int32_t *pred_out, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * Whole-scene evaluation harness.
 * ------------------------------------------------------------------------------------------ */

/* add_vote (PointNet/NB_nontarget_test_semseg.py:55-62): for every block point r with weight[r] != 0 (weight
 * nullable = all), pool[point_idx[r]][pred[r]] += 1, pred = the given labels (int32 [rows]) or, when `pred` is
 * null, argmax(logp[r]) with the first index on ties (`seg_pred.max(2)[1]`).  pool: int32 [n_points][n_cls],
 * accumulated in place.  *bad_flag (int32, device) is OR-ed with 1 if an index is out of range. */
int psg_vote_add(const float *logp, const int32_t *pred, const int32_t *point_idx, const float *weight, int rows,
                 int n_cls, int n_points, int32_t *pool, int32_t *bad_flag, psg_stream stream);

/* Per-scene statistics of NB_nontarget_test_semseg.py:219-229: pred = np.argmax(pool, 1) (first index on ties),
 * counters int64 [3][n_cls] += seen, correct, union against `labels` (int32 [n_points]).  pred_out nullable. */
int psg_vote_stats(const int32_t *pool, const int32_t *labels, int n_points, int n_cls, long long *counters,
                   int32_t *pred_out, psg_stream stream);

/* torch.dist(a, b) (p = 2) of NB_nontarget_test_semseg.py:184: out[0] = sqrt(sum (a-b)^2), accumulated in double
 * in a fixed order.  scratch256: 256 doubles of device scratch. */
int psg_l2_dist(const float *a, const float *b, size_t n, double *scratch256, float *out, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * ResGCN-28 dense DeepGCN sem-seg network (ResGCN/sem_seg_dense/architecture.py:6-68), eval mode:
 * head EdgeConv(9->64) on the xyz kNN graph, n_blocks-1 residual dynamic EdgeConv blocks (feature-space
 * kNN, k = 16, dilation 1..n_blocks-1), fusion 1x1 conv + global max, prediction MLP.  BasicConv order is
 * Conv -> ReLU -> BatchNorm (ResGCN/gcn_lib/dense/torch_nn.py:55-66).
 * ------------------------------------------------------------------------------------------ */
typedef struct psg_gcn_model psg_gcn_model;
typedef struct psg_gcn_ws psg_gcn_ws;

/* tensors: HOST fp32 pointers in the order documented in csrc/psg_resgcn.hip (per EdgeConv: conv weight
 * [64][2C], bias, BN weight/bias/running_mean/running_var; fusion_block; prediction.0/.1 with BN; prediction.3).
 * n_tensors must equal 6*n_blocks + 20.  Blocking. */
int psg_gcn_model_create(psg_ctx *ctx, const float *const *tensors, int n_tensors, int n_blocks, psg_gcn_model **out);
/* The reference's configuration switches (ResGCN/sem_seg_dense/architecture.py:26-39 `opt.block`, gcn_lib/dense/
 * torch_vertex.py:44-49 `opt.conv`): block = ResDynBlock2d / PlainDynBlock2d / DenseDynBlock2d, conv = EdgeConv2d /
 * MRConv2d.  Same tensor order as psg_gcn_model_create with the reference's shapes for that configuration (dense:
 * conv weight of block e is [64][2*64e], fusion_block [1024][64 n(n+1)/2], prediction.0 [512][1024 + 64 n(n+1)/2]). */
#define PSG_GCN_BLOCK_RES 0
#define PSG_GCN_BLOCK_PLAIN 1
#define PSG_GCN_BLOCK_DENSE 2
#define PSG_GCN_CONV_EDGE 0
#define PSG_GCN_CONV_MR 1
int psg_gcn_model_create_cfg(psg_ctx *ctx, const float *const *tensors, int n_tensors, int n_blocks, int block, int conv,
                             psg_gcn_model **out);
int psg_gcn_model_destroy(psg_gcn_model *model);
int psg_gcn_ws_create(psg_ctx *ctx, int batch, int n_point, int n_blocks, psg_gcn_ws **out);
int psg_gcn_ws_create_cfg(psg_ctx *ctx, int batch, int n_point, int n_blocks, int block, int conv, psg_gcn_ws **out);
int psg_gcn_ws_destroy(psg_gcn_ws *ws);
size_t psg_gcn_ws_bytes(const psg_gcn_ws *ws);
/* Measurement only (bench.py `roofline`): per-launch HIP-event timing on the launch stream, like psg_pn2_prof_*.  Tags:
 * 0 fused feature-space kNN kernel (torch_edge.py:32-59), 1 other kNN launches, 2 per-vertex EdgeConv GEMM, 3 edge max,
 * 4 fusion + prediction, 5 backward; flops = algorithmic FLOPs of the tagged launches.  While enabled the attack loop does
 * not use its hipGraph. */
int psg_gcn_prof_enable(psg_gcn_ws *ws, int on);
int psg_gcn_prof_read(psg_gcn_ws *ws, int n_tags, double *total_ms, int *counts, double *flops);

/* DenseDilatedKnnGraph (torch_edge.py:45-79) on point-major features x [batch][n_point][C]: neighbours at
 * ranks 0, d, 2d, ... of the ascending pairwise_distance row, k = 16; out_idx [batch][n_point][16].
 * Distances follow the reference's fp32 order (ascending-k fmaf dot, (|xi|^2 + -2 xi.xj) + |xj|^2);
 * equal distances resolve to the lowest index (torch.topk leaves that order unspecified). */
int psg_gcn_knn(psg_gcn_ws *ws, const float *x, int C, int dilation, int32_t *out_idx, psg_stream stream);
/* Measurement only: counters of the feature-space kNN kernel since the last reset, for workspaces created while the
 * environment holds PSG_GCN_KNN_STATS=1 (all zero otherwise).  The kernel decides most of a distance row on a bf16 MFMA
 * approximation with a proven error bound and evaluates the reference's fp32 distance (torch_edge.py:41-43) only for the
 * candidates that can hold a wanted rank; tiles whose bound cannot be kept take the all-fp32 path inside the same launch.
 * host_out8: [0] 32-query tiles, [1] tiles that took the exact path, [2] rows ranked on the fast path, [3] exact distances
 * evaluated there, [4] row cuts, [5] entries held at the end of the stream, [6..7] 0.  Synchronises the device. */
int psg_gcn_knn_stats(psg_gcn_ws *ws, unsigned long long *host_out8, int reset);

/* DenseDeepGCN.forward (architecture.py:58-68): x0 [batch][n_point][9] point-major -> logits [batch][n_point][13]. */
int psg_gcn_forward(psg_gcn_model *model, psg_gcn_ws *ws, const float *x0, float *logits_out, psg_stream stream);

/* Input-gradient backward of the resident forward (kNN graphs are constants, as under torch.no_grad in the
 * reference): dlogits [batch][n_point][13] -> dx0_out [batch][n_point][9]. */
int psg_gcn_backward(psg_gcn_model *model, psg_gcn_ws *ws, const float *dlogits, float *dx0_out, psg_stream stream);

/* colper.NB_attack (ResGCN/sem_seg_dense/attacks/torchattacks/attacks/colper.py:17-39): CrossEntropyLoss (mean)
 * on logits, sign ascent on colour, L-inf projection; images/adv_out [batch][9][n_point]. */
int psg_gcn_nb_attack(psg_gcn_model *model, psg_gcn_ws *ws, const float *images, const int32_t *labels, float eps,
                      float alpha, int iters, float *adv_out, psg_stream stream);

/* Teacher forcing for parity tests: nbr (device, [n_blocks][batch][n_point][16]) replaces the kNN graphs of
 * every following forward; NULL restores the dynamic graphs.  (Feature-space kNN has near-ties that no two
 * fp32 pipelines break alike, so value parity is checked on identical graphs and graph parity by overlap.) */
int psg_gcn_set_graphs(psg_gcn_ws *ws, const int32_t *nbr, psg_stream stream);

/* parity-test read-back: neighbour table of EdgeConv `block` [batch][n_point][16]; block outputs [batch][n_point][64*n_blocks] */
const int32_t *psg_gcn_edge_ptr(const psg_gcn_ws *ws, int block);
const float *psg_gcn_feats_ptr(const psg_gcn_ws *ws);

/* Read-only tap into the workspace (tests): the device pointer of a named buffer with its row and column counts.  NULL
 * with the error string set - and the counts left untouched - for a null workspace, an unknown `what`, a `block` outside
 * [0, n_blocks), a conv = mr code on an edge workspace, or a kept code while psg_gcn_debug_keep is off.  Launches nothing,
 * allocates nothing, does not synchronise.  float32 unless noted; B rooms of N points, R = B N rows, F = 64 n_blocks, C_e
 * the input width of block e (9, 64, or dense: 64 e); `block` selects e where [e] is written and is ignored elsewhere.
 *   forward state, valid from a forward call until the next forward call:
 *      0 xyz [R][3]   1 feats [R][F]   2 nbr[e] [R][16] (int32, room-local)   3 arg[e] [R][64] (uint8: winning slot, bit 0x80 =
 *      the winner's pre-activation was positive; conv = edge)   4 arg_mr[e] [R][C_e] (uint8, conv = mr)
 *      5 mask_mr[e] [R][2] (uint32 ReLU bits, conv = mr)   6 sq [R][1] and 7 xp [R][64] (the norms and the MFMA-operand copy of
 *      the LAST 64-wide kNN source whose producer or prep launch wrote them)   8 fused [R][1024]   9 mask_f [R][32] (uint32)
 *      10 fmax [B][1024]   11 farg [B][1024] (int32, room-local)   12 gb1 [B][512]   13 h1 [R][512]   14 mask1 [R][16] (uint32)
 *      15 h2 [R][256]   16 mask2 [R][8] (uint32)   17 logits [R][13]
 *      ReLU bit words: cols = words per row, bit c%32 of word c/32 = (pre-activation > 0)
 *   gradient state, valid from a backward call until the next backward call:
 *      30 g2 [R][256]   31 g1 [R][512]   32 g1part [B ceil(N/64)][512]   33 g1sum [B][512]   34 gfvec [B][1024]
 *      35 dfeats [R][F] (res / edge: prediction head + fusion transpose; other configurations: as the last block left it)
 *      36 gcur [R][64] (res / edge: G_0; conv = mr: block 0's gated gradient)
 *   kept copies (psg_gcn_debug_keep on), made on the launch stream as the loops run:
 *      50 [P | Q] of block e [R][128] (conv = mr: the gathered cat [R][2 C_e])   51 dfeats as the prediction head left it [R][F]
 *      52 dfeats after the fusion transpose [R][F]   53 [dP | dQ] of block e [R][128] (mr: dcat [R][2 C_e])
 *      54 the gated output gradient of block e [R][64] (conv = mr)   55 the state after block e's backward: gcur [R][64]
 *      (res / edge) or the whole dfeats [R][F]   56 dx0 [R][9] as block 0 wrote it */
const void *psg_gcn_debug_ptr(const psg_gcn_ws *ws, int what, int block, int *rows_out, int *cols_out);
/* on != 0: the workspace gets a second arena (allocated at the first call, freed by on = 0 and by psg_gcn_ws_destroy) and
 * psg_gcn_forward / psg_gcn_backward add device-to-device copies of the per-block buffers they overwrite (codes 50-56
 * above); no kernel and no result changes.  Off (the default), both issue exactly the launches they issue without this
 * entry point.  While on, psg_gcn_nb_attack, psg_gcn_nb_attack_field, psg_gcn_nu_window and psg_gcn_nu_field_window
 * return PSG_ERR_STATE: they replay captured forwards, which would not make the copies. */
int psg_gcn_debug_keep(psg_gcn_ws *ws, int on);

/* A WINDOW of consecutive optimiser steps of the ResGCN NU_attack / tar_NU_attack (colper.py:62-95, tcolper.py:85-132) for
 * G one-room attacks in lockstep (rooms form only: the workspace is for G rooms of N points), enqueued by ONE call.  Per
 * step: psg_nu_tanh_color_rooms, psg_gcn_forward, psg_gcn_f_loss_grad_rooms (scale c_f), psg_gcn_backward,
 * psg_smooth_knn_sym_rooms, psg_nu_adam_step_rooms (c_smooth, c_l2; psg_nu_adam_step at G = 1: the same arithmetic),
 * psg_nu_step_latch (rows = 1) - cost = c_f f + c_smooth Smooth + c_l2 L2, (c_f, c_l2) = (c, 1) for NU_attack and (1, c)
 * for tar_NU_attack.  Graphs set by psg_gcn_set_graphs are used.  The fields are those of psg_pointnet_nu_window_args;
 * `logits` / `dlogits` [G][N][13] are scratch.  The reference's host work sits between windows. */
typedef struct psg_gcn_nu_window_args {
    psg_gcn_model *model;
    psg_gcn_ws *ws;              /* created for G rooms of N points */
    int step0, n_steps;
    int G, N, mode;              /* mode: see psg_nu_step_latch */
    int use_target, target;
    int neighbour;
    int adam_t0;
    float kappa, tsign, c_f, c_smooth, c_l2, lr, beta1, beta2, eps;
    float *w, *m, *v;            /* [G][N][3] */
    const uint8_t *mask;         /* [G][N], nullable for NU_attack */
    const int32_t *n_mask;       /* [G], modes 1 and 2 */
    float *x0;                   /* [G][N][9] */
    const float *ori;            /* [G][N][3] */
    const int32_t *labels;       /* [G][N] */
    float *logits, *dlogits, *dx0; /* [G][N][13], [..][13], [..][9] scratch */
    float *sgrad;                /* [G][N][3] */
    int32_t *pred;               /* [G][N] */
    float *scal;                 /* [3][G], zero before the first window */
    int32_t *nn_state;           /* [G][N][neighbour] */
    float *hist;                 /* history rows [5][G] of the window's steps, row of step0 first */
    float *out;                  /* [G][9][N] */
    uint8_t *active;             /* [G] */
    int32_t *exit_step;          /* [G] */
} psg_gcn_nu_window_args;
/* `graph` as for psg_pn2_nu_window (first window of a shape eager, second captured, later ones replayed, the step constants
 * read from a device row); the captured sequence is a single chain on `stream`.  A failed capture is counted in
 * psg_nu_graph_stats, not retried, and the window runs eagerly; while psg_gcn_prof_enable is on no graph is used. */
int psg_gcn_nu_window(const psg_gcn_nu_window_args *args, psg_nu_graph *graph, psg_stream stream);

/* ---- ResGCN attacks on the COORDINATE field (channels 0:3): an extension of the reference API.
 * The kNN graphs are constants of the derivative, so psg_gcn_backward's dx0[.][0:3] is the exact coordinate gradient; the
 * head's xyz graph is rebuilt from the moved points by every forward (graphs set by psg_gcn_set_graphs still win). */

/* NB_attack with field = PSG_NU_FIELD_COORD | PSG_NU_FIELD_BOTH: iters x (psg_gcn_forward, psg_ce_logp_grad (mean),
 * psg_gcn_backward, psg_pgd_step_field at c0 = 0 with (coord_alpha, coord_eps) - sign ascent, eta clamped to +-coord_eps, no
 * [0, 1] clamp - and, both, at c0 = 3 with (alpha, eps)); channels 6:9 stay as given; images / adv_out [batch][9][n_point],
 * the un-projected last step is returned like psg_gcn_nb_attack's.  First and last iteration run eagerly, the interior
 * ones are captured once (a holder of the workspace's own, keyed on the model, field, both eps, both alpha and whether
 * graphs are set) and replayed; on the legacy default stream and while psg_gcn_prof_enable is on the loop stays eager.
 * Arguments are checked before anything is enqueued. */
int psg_gcn_nb_attack_field(psg_gcn_model *model, psg_gcn_ws *ws, const float *images, const int32_t *labels, int field, float eps,
                            float alpha, float coord_eps, float coord_alpha, int iters, float *adv_out, psg_stream stream);

/* A WINDOW of optimiser steps of NU_attack / tar_NU_attack with field = coord | both for G one-room attacks in lockstep.
 * The variable delta [G][N][3] (metres, zero at the start, no tanh space) is optimised by Adam, xyz = ori_xyz + delta on
 * masked points of active rooms.  Per step, in the order of psg_gcn_nu_window: psg_nu_coord_apply_rooms (both: +
 * psg_nu_tanh_color_rooms), psg_gcn_forward, psg_gcn_f_loss_grad_rooms (scale c_f), psg_gcn_backward, (both:
 * psg_smooth_knn_sym_rooms on the colours,) psg_smooth_knn_xyz_sym_rooms, (both: psg_nu_adam_step(_rooms) on w,)
 * psg_nu_coord_adam_step_rooms_w (c_smooth_xyz, c_l2_xyz, coord_lr), psg_nu_step_latch, then Smooth_xyz and L2_xyz into
 * rows 5, 6 of the step's history row.  Cost = c_f f + c_smooth_xyz Smooth_xyz + c_l2_xyz L2_xyz (+ c_smooth Smooth +
 * c_l2 L2 with both).  `graph` as for psg_gcn_nu_window; the device row's slot 3 carries coord_lr / (1 - beta1^t).
 * Refusals are psg_gcn_nu_window's; field 0 is refused too (the colour path has its own entry). */
typedef struct psg_gcn_nu_field_window_args {
    psg_gcn_model *model;
    psg_gcn_ws *ws;              /* created for G rooms of N points */
    int step0, n_steps;
    int G, N, mode;              /* mode: see psg_nu_step_latch */
    int use_target, target;
    int neighbour;
    int adam_t0;
    int field;                   /* PSG_NU_FIELD_COORD or PSG_NU_FIELD_BOTH */
    float kappa, tsign, c_f, c_smooth, c_l2, lr, c_smooth_xyz, c_l2_xyz, coord_lr, beta1, beta2, eps;
    float *w, *m, *v;            /* [G][N][3] colour variable and moments (field both) */
    float *delta, *mx, *vx;      /* [G][N][3] coordinate variable and moments */
    const float *ori_xyz;        /* [G][N][3] the clean coordinates */
    const uint8_t *mask;         /* [G][N], nullable for NU_attack */
    const int32_t *n_mask;       /* [G], modes 1 and 2 */
    float *x0;                   /* [G][N][9] */
    const float *ori;            /* [G][N][3] the clean colours (field both) */
    const int32_t *labels;       /* [G][N] */
    float *logits, *dlogits, *dx0; /* [G][N][13], [..][13], [..][9] scratch */
    float *sgrad, *sgrad_xyz;    /* [G][N][3] each (sgrad: field both) */
    int32_t *pred;               /* [G][N] */
    float *scal;                 /* [5][G] f, Smooth, L2, Smooth_xyz, L2_xyz; zero before the first window */
    int32_t *nn_state, *nn_xyz;  /* [G][N][neighbour] colour (field both) and coordinate neighbour lists */
    float *hist;                 /* history rows [7][G] of the window's steps, row of step0 first */
    float *out;                  /* [G][9][N] */
    uint8_t *active;             /* [G] */
    int32_t *exit_step;          /* [G] */
} psg_gcn_nu_field_window_args;
int psg_gcn_nu_field_window(const psg_gcn_nu_field_window_args *args, psg_nu_graph *graph, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * RandLA-Net input pipeline (first piece): exact k-nearest neighbours of 3-D points.
 * Replaces DataProcessing.knn_search (RandLA-Net/helper_tool.py:158-167) = nearest_neighbors.knn_batch(support,
 * query, k, omp=True) (utils/nearest_neighbors/knn_.cxx:103-134, nanoflann kd-tree + OpenMP on the host).
 * support [batch][n_support][3], query [batch][n_query][3] device fp32; out_idx [batch][n_query][k] int32: the k
 * support points nearest to each query in ascending (squared distance, index) order, 1 <= k <= 16.  Distances are
 * evaluated like nanoflann's L2 metric, so neighbour sets equal the reference's (order may differ among exact ties,
 * where nanoflann's order depends on its tree traversal).
 * ------------------------------------------------------------------------------------------ */
int psg_knn_points(psg_ctx *ctx, const float *support, const float *query, int batch, int n_support, int n_query, int k,
                   int32_t *out_idx, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * RandLA-Net: inference graph, colour gradient and BIM attack for ONE cloud per
 * workspace (ConfigS3DIS.val_batch_size = 1), 5 levels, k = 16, 13 classes.  Replaces Network.inference
 * (RandLA-Net/RandLANet.py:150-190 with :323-410) and the BIM loop of ares/ares/attack/bim.py:66-116,190-236.
 * PARITY UNPINNED: the reference is a TensorFlow-1 graph that cannot run in this environment; the checker is a
 * source-reading restatement (oracle/randla_net.py).
 * tensors: 6 HOST pointers per layer in forward order (pointsecguard_amd.synthetic.randla_layer_specs: fc0; per encoder
 * level mlp1, LFAmlp1, LFAatt_pooling_1fc, LFAatt_pooling_1mlp, LFAmlp2, LFAatt_pooling_2fc, LFAatt_pooling_2mlp, mlp2,
 * shortcut; decoder_0; Decoder_layer_0..4; fc1, fc2, fc): weight [cout][cin], bias or NULL, BatchNorm gamma, beta,
 * moving mean, moving variance or NULL (eps 1e-6, folded on the host).
 * ------------------------------------------------------------------------------------------ */
#define PSG_RLA_NUM_LAYERS 55
/* Possibility-based crop sampler of the RandLA-Net input pipeline (RandLA-Net/main_S3DIS.py:116-187, spatially_regular_gen):
 * one object per cloud, points [n][3] f32 and the float64 possibility of every point resident on the device.
 * argmin = np.argmin / np.min of the possibility (:134-137); query = the cloud's KDTree.query(pick, k)[1][0] (:151-156): the k
 * nearest points ascending by (float64 squared distance, index); update = possibility[idx] += (1 - d / max d)^2 with the
 * reference's float32 d (:163-166).  What the reference draws from numpy's generator stays on the host
 * (pointsecguard_amd/randla/sampler.py). */
typedef struct psg_rla_sampler psg_rla_sampler;
int psg_rla_sampler_create(psg_ctx *ctx, const float *points_host, const double *possibility_host, int n_points,
                           psg_rla_sampler **out);
int psg_rla_sampler_destroy(psg_rla_sampler *s);
int psg_rla_sampler_argmin(psg_rla_sampler *s, int *index_out, double *value_out, psg_stream stream);
int psg_rla_sampler_query(psg_rla_sampler *s, const double *pick_host3, int k, int32_t *out_idx, psg_stream stream);
int psg_rla_sampler_update(psg_rla_sampler *s, const int32_t *idx, int k, const double *pick_host3, float *scratch, psg_stream stream);
int psg_rla_sampler_possibility(psg_rla_sampler *s, double *host_out);

typedef struct psg_rla_model psg_rla_model;
typedef struct psg_rla_ws psg_rla_ws;
int psg_rla_model_create(psg_ctx *ctx, const float *const *tensors, int n_tensors, psg_rla_model **out);
int psg_rla_model_destroy(psg_rla_model *model);
int psg_rla_ws_create(psg_ctx *ctx, int n_points, psg_rla_ws **out);
/* A workspace for `batch` clouds of n_points each that are attacked together (the reference's val_batch_size is 1,
 * helper_tool.py:52, so this is a launch-coalescing device: the clouds stay independent, every neighbour / pooling /
 * interpolation index stays inside its cloud, and one launch of each kernel serves all of them).  Every [n_points][..]
 * argument of the calls below becomes [batch][n_points][..].  Both metrics: the l_2 step of psg_rla_bim_attack takes its two
 * norms per cloud (one workgroup per cloud, a fixed summation order), as bim.py:84-98 normalises per sample. */
int psg_rla_ws_create_batch(psg_ctx *ctx, int n_points, int batch, psg_rla_ws **out);
/* A cloud-batch workspace that can also differentiate the relative-position branch (psg_rla_backward_full): level 0 runs the
 * unfused chain, as under PSG_RLA_NO_FUSE16=1, and the buffers of the coordinate gradient follow everything else in the arena.
 * psg_rla_forward / psg_rla_backward behave on it as on a PSG_RLA_NO_FUSE16 workspace.  Refused under PSG_RLA_ATOMICS=1 (no
 * inverse lists).  The workspaces of the two calls above keep their layout, size and kernels. */
int psg_rla_ws_create_full(psg_ctx *ctx, int n_points, int batch, psg_rla_ws **out);
int psg_rla_ws_destroy(psg_rla_ws *ws);
size_t psg_rla_ws_bytes(const psg_rla_ws *ws);
/* Measurement only: HIP-event timing of every GEMM launch (tag 0: the 1x1 convolutions and attention scores of
 * RandLANet.py:323-410) with its algorithmic FLOPs; while enabled the BIM loop does not use its hipGraph. */
int psg_rla_prof_enable(psg_rla_ws *ws, int on);
int psg_rla_prof_read(psg_rla_ws *ws, int n_tags, double *total_ms, int *counts, double *flops);
/* The same launches split by kernel (n_tags >= 4): 0 = the 64 x 64-tile row GEMM of the point-sized layers, 1 = 128 x 128
 * tiles, 2 = 256 x 64 tiles, 3 = the row-per-thread kernel of the 8-32 channel layers; bytes = algorithmic bytes of the
 * tagged launches (input rows, output rows, addend rows, weights, mask words): these kernels are bandwidth-bound. */
int psg_rla_prof_read_kernels(psg_rla_ws *ws, int n_tags, double *total_ms, int *counts, double *flops, double *bytes);
/* xyz [n_points][3] device: builds the index pyramid of main_S3DIS.py:198-207 (psg_knn_points) and the relative
 * position encodings.  Sub-sampling is the reference's: the first n / ratio points of each level. */
int psg_rla_set_cloud(psg_rla_ws *ws, const float *xyz, psg_stream stream);
/* what: 0 neighbour idx [n_l][16], 1 up-sampling idx [n_l]; device pointers into the workspace (tests) */
const int32_t *psg_rla_index_ptr(const psg_rla_ws *ws, int what, int level);
/* Read-only tap into the workspace (tests): the device pointer of a named buffer with its row and column counts; NULL
 * with the error string set for an unknown `what` or `level`.  Launches nothing, allocates nothing, does not synchronise.
 * `level` = encoder level 0..4 for the per-level buffers, decoder layer j = 0..4 for the dec buffers, 0 otherwise.
 * float32 unless noted; n = rows of the level, d = its d_out, h = d / 2.
 *   forward state, valid from a forward call until the next backward call (which recycles agg1 / agg2 / fagg2: copy first):
 *     0 f0 [N][8]  1 dec0 [n5][1024]  2 dec_cat[j]  3 dec_out[j]  4 fc1o [N][64]  5 fc2o [N][32]  6 logits [N][13]
 *     10 fpc [n][h]  11 agg1 [n][d]  12 fagg1 [n][h]  13 agg2 [n][d]  14 fagg2 [n][d]  15 sc [n][2d]  16 enc [n][2d]
 *     17 samp [n_sub][2d]  18 arg [n_sub][2d] (bytes)  19 relpos [16n][10]  20 fxyz1 [16n][h]  21 fxyz2 [16n][h]
 *     leaky-ReLU sign bits, uint32 words, cols = words per row, bit c%32 of word c/32 = (pre-activation > 0):
 *     30 m_f0  31 m_fpc  32 m_fagg1  33 m_fagg2  34 m_enc  35 m_dec0  36 m_dec[j]  37 m_fc1  38 m_fc2
 *   gradient state, valid from a backward call until the next forward call:
 *     40 d_fc2o  41 d_fc1o  42 d_dec_out[j]  43 d_dec0  44 d_samp  45 d_enc  46 d_fagg1  47 d_fpc  51 d_f0
 *     48 g_fagg2 (lives in agg2)  49 g_agg2 (lives in fagg2)  50 g_agg1 (lives in agg1)
 *   geometry (int32), valid from the cloud call on, unless the float-atomics switch is set (never built: NULL, error set):
 *     60 inv_off [n+1]  61 inv_ent [16n]  62 invu_off [n_sub+1]  63 invu_ent [n]  64 invp_off [n+1]  65 invp_ent [16 n_sub]
 *   position-branch gradient, psg_rla_ws_create_full workspaces only (NULL, error set, on any other):
 *     sign words of the branch's two layers (uint32), valid with fxyz1 / fxyz2:  70 m_fxyz1 [16n][ceil(h/32)]  71 m_fxyz2
 *     valid from psg_rla_backward_full until the next forward call:
 *     72 G2 [16n][h]  73 G1 [16n][h] (gradients of the pre-activations of LFAmlp2 / LFAmlp1)  74 g_rp [16n][10]
 *     75 gxyz [n][3]  76 side_i [16n][4]  77 side_j [16n][4] (what edge (i, k) hands to point i / to neighbour j: x, y, z, 0)
 * The per-edge attention buffers (a1 / cat1 / a2 / cat2) change meaning with the path (T and S2 on the split path, scores
 * and the concatenation on the unfused one, unused on the fused one) and are not exposed. */
const void *psg_rla_debug_ptr(const psg_rla_ws *ws, int what, int level, int *rows_out, int *cols_out);
/* features [n_points][6] = (xyz, rgb) -> logits [n_points][13] */
int psg_rla_forward(psg_rla_model *model, psg_rla_ws *ws, const float *features, float *logits_out, psg_stream stream);
/* d loss / d logits -> d loss / d features [n_points][6] (through the feature path only: the relative-position branch
 * is constant for a colour attack); consumes the resident forward */
int psg_rla_backward(psg_rla_model *model, psg_rla_ws *ws, const float *dlogits, float *dfeatures_out, psg_stream stream);
/* The same on a psg_rla_ws_create_full workspace, plus dxyz_out [n_points][3] = d loss / d xyz of psg_rla_set_cloud through the
 * relative-position branch (RandLANet.py:347-353 and the two LFA MLPs), with the neighbour, sub-sampling and up-sampling
 * indices constant.  Geometric paths only: a caller whose features carry the same positions adds dfeatures[:, 0:3].  Where
 * dist == 0 (self edges, coincident points) the distance column contributes exactly zero.  dfeatures_out holds the bytes
 * psg_rla_backward writes on the same workspace.  No float atomics: two runs give the same bits.  PSG_ERR_ARG, before
 * anything is enqueued, on a workspace that is not full and on null arguments. */
int psg_rla_backward_full(psg_rla_model *model, psg_rla_ws *ws, const float *dlogits, float *dfeatures_out, float *dxyz_out,
                          psg_stream stream);
/* the attack's loss (bim.py:110-116) and its gradient w.r.t. the logits; loss_out (nullable) device scalar */
int psg_rla_colper_grad(const float *logits, const int32_t *labels, int n, float *dlogits, float *loss_out, psg_stream stream);
/* The same with the targeted attacks' mask and sign (TBIM bim.py:393-397 / :350-351, tar_NUattack.py:105-110): ys = the
 * labels the hinge is taken against (the target class on the origin points), mask [n] bytes or NULL = which points
 * contribute, sign = -1 for goal 't' (grad = -grad). */
int psg_rla_colper_grad_masked(const float *logits, const int32_t *ys, const uint8_t *mask, float sign, int n, float *dlogits,
                               float *loss_out, psg_stream stream);
/* One BIM update (bim.py:84-98) of the colour half of feat [n][6] from dfeat [n][6]; ori [n][3] the clean colours; l_2:
 * norms = 2 floats and delta = [n][3] floats of scratch.  psg_rla_bim_attack's step as its own entry, for the attacks whose
 * loop reads an accuracy back every iteration (TBIM.batch_attack, bim.py:484-505). */
int psg_rla_bim_step(float *feat, const float *dfeat, const float *ori, int n, float eps, float alpha, int l2_metric, float *norms,
                     float *delta, psg_stream stream);
/* The same update (bim.py:84-96) on the coordinate columns 0:3 of feat [n][6] of ONE cloud, with the gradient
 * g = dfeat[:, 0:3] + dxyz (one fp32 add; dxyz [n][3] from psg_rla_backward_full) and ori_xyz [n][3] the clean positions.  No
 * clip to a box: coordinates have none.  l_2: norms = 2 floats and delta = [n][3] floats of scratch, the norms in
 * psg_rla_bim_step's order (one workgroup, double accumulation, a fixed tree). */
int psg_rla_bim_step_field(float *feat, const float *dfeat, const float *dxyz, const float *ori_xyz, int n, float eps, float alpha,
                           int l2_metric, float *norms, float *delta, psg_stream stream);
/* NUattack / tar_NUattack (ares/ares/attack/NUattack.py:12-74, tar_NUattack.py:12-84): adversarial colours of the tanh-space
 * variable d_ws into feat [n][6] columns 3..5 (mask: only those points move) and dist2[0] = |adv - x|_2^2; then one TF1-Adam
 * step (t = 1, 2, ..) on d_ws of loss = |adv - x|_2 + c * score from dfeat = d score / d features. */
int psg_rla_nu_color(const float *xs, const float *dws, const uint8_t *mask, int n, float *feat, float *dist2, psg_stream stream);
int psg_rla_nu_adam_step(const float *xs, float *dws, float *m, float *v, const uint8_t *mask, const float *feat,
                         const float *dfeat, const float *dist2, int n, float c, float lr, int t, psg_stream stream);
/* `iters` BIM updates (goal 'ut') of the colour half of `features`; l2_metric 0: l_inf, 1: l_2 (bim.py:84-98);
 * builds the cloud's geometry itself.  adv_features_out [n_points][6]. */
int psg_rla_bim_attack(psg_rla_model *model, psg_rla_ws *ws, const float *features, const int32_t *labels, float eps,
                       float alpha, int iters, int l2_metric, float *adv_features_out, psg_stream stream);

/* NUattack / tar_NUattack on G clouds of n points in lockstep.  Every buffer is cloud-major; `active` [G] is a byte per cloud
 * (NULL: every cloud is active) and an inactive cloud is not touched by any of these calls.  No float atomics: two runs give
 * the same bits, and a cloud's results do not depend on which other clouds are active.
 *
 * psg_rla_nu_color_clouds: feat [G][n][6] columns 3..5 = adv(d_ws) with psg_rla_nu_color's arithmetic (mask [G][n] or NULL:
 * only those points move) and dist2[g] = |adv - x|_2^2, summed in double in a fixed order by PSG_RLA_NU_PARTS workgroups per
 * cloud (partials: [G][PSG_RLA_NU_PARTS] doubles of scratch) and rounded to float once. */
#define PSG_RLA_NU_PARTS 32
int psg_rla_nu_color_clouds(const float *xs, const float *dws, const uint8_t *mask, const uint8_t *active, int G, int n, float *feat,
                            float *dist2, double *partials, psg_stream stream);
/* psg_rla_nu_adam_step's update of every active cloud with its own dist2[g].  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) is computed
 * in double on the host; inside a replayed window it is read from the window's step-constant device row instead. */
int psg_rla_nu_adam_clouds(const float *xs, float *dws, float *m, float *v, const uint8_t *mask, const uint8_t *active,
                           const float *feat, const float *dfeat, const float *dist2, int G, int n, float c, float lr, int t,
                           psg_stream stream);
/* The evaluation the reference makes after every optimiser step (NUattack.py:190-213, tar_NUattack.py:235), for every active
 * cloud: pred [G][n] = the first maximum of logits [G][n][13], n_correct = #(pred == labels), n_hits = #(mask & pred == ys)
 * (0 without a mask); hist_row [G][3] = {n_correct, n_hits, dist2[g]}.  The exit test is in integers: mode 0
 * den * n_correct < num * n, mode 1 den * n_hits > num * n_mask[g].  When it fires, can_exit != 0 and step >= 1 (the
 * unperturbed start is never tested), the cloud is snapshot - out_adv [G][n][3] = the colours of feat, out_pred [G][n],
 * out_stats [G][3] = the history row - exit_step[g] = step and active[g] = 0; final != 0 snapshots every active cloud
 * without marking an exit.  scratch: [G][2 * PSG_RLA_NU_PARTS + 1] int32.  active and exit_step are required here. */
int psg_rla_nu_latch_clouds(const float *logits, const int32_t *labels, const int32_t *ys, const uint8_t *mask, const int32_t *n_mask,
                            const float *feat, const float *dist2, int G, int n, int mode, int num, int den, int step, int can_exit,
                            int final, float *hist_row, int32_t *pred, float *out_adv, int32_t *out_pred, float *out_stats,
                            uint8_t *active, int32_t *exit_step, int32_t *scratch, psg_stream stream);

/* One window of the lockstep attack: for each of n_steps optimiser steps with Adam index t = adam_t0 + i (adam_t0 >= 1):
 * colour, psg_rla_forward, latch of evaluation index t - 1 (history row i; exits from index 1 on), the masked hinge gradient
 * against ys (psg_rla_colper_grad_masked, sign +1), psg_rla_backward, Adam.  tail_eval != 0 appends colour, forward and a
 * latch with final = 1 of the last step (history row n_steps).  Nothing returns to the host inside a window.  `graph` as for
 * the other windows (first window of a shape eager, second captured, later ones replayed; a single chain on `stream`); no
 * graph is used while psg_rla_prof_enable is on, before the first psg_rla_forward of (cloud, model), or when n_steps plus
 * the tail exceed PSG_NU_GRAPH_MAX_STEPS.  ws: a workspace of
 * G clouds of N points with the clouds set. */
typedef struct psg_rla_nu_window_args {
    psg_rla_model *model;
    psg_rla_ws *ws;
    int n_steps, G, N, mode;
    int num, den;                /* the exit threshold num / den */
    int adam_t0, tail_eval;
    float cs, lr;
    const float *xs;             /* [G][N][3] clean colours */
    float *dws, *m, *v;          /* [G][N][3] */
    const uint8_t *mask;         /* [G][N], nullable (required in mode 1) */
    const int32_t *n_mask;       /* [G], mode 1 */
    const int32_t *labels, *ys;  /* [G][N]: the true labels, the labels the hinge is taken against */
    float *feat;                 /* [G][N][6], xyz in columns 0..2 */
    float *logits, *dlogits;     /* [G][N][13] */
    float *dfeat;                /* [G][N][6] */
    float *dist2;                /* [G] */
    double *partials;            /* [G][PSG_RLA_NU_PARTS] */
    int32_t *pred;               /* [G][N] */
    int32_t *scratch;            /* [G][2 * PSG_RLA_NU_PARTS + 1] */
    float *hist;                 /* [n_steps + (tail_eval != 0)][G][3] */
    float *out_adv;              /* [G][N][3] */
    int32_t *out_pred;           /* [G][N] */
    float *out_stats;            /* [G][3] */
    uint8_t *active;             /* [G] */
    int32_t *exit_step;          /* [G], -1 before */
} psg_rla_nu_window_args;
int psg_rla_nu_window(const psg_rla_nu_window_args *args, psg_nu_graph *graph, psg_stream stream);

/* TBIM / tar_NBattack (bim.py:277-505) on G clouds of n points in lockstep.  Buffers are cloud-major as above; a cloud whose
 * `running` / `active` byte is clear is not touched.
 *
 * psg_rla_bim_step_clouds: psg_rla_bim_step's update of every running cloud (running [G] bytes, NULL: all) with that cloud's own
 * norms: norms [2][G] = {|g|^2 of cloud g, |delta|^2 of cloud g}, delta [G][n][3] (both l_2 only).  The norms keep
 * psg_rla_bim_step's summation order (one workgroup per cloud, double accumulation, the fixed tree), so a cloud's colours are
 * bit-equal to psg_rla_bim_step on that cloud alone.  No byte of feat, delta or norms of a cloud that is not running is
 * written, whatever its dfeat holds. */
int psg_rla_bim_step_clouds(float *feat, const float *dfeat, const float *ori, const uint8_t *running, int G, int n, float eps,
                            float alpha, int l2_metric, float *norms, float *delta, psg_stream stream);
/* The evaluation TBIM.batch_attack makes in iteration `it` BEFORE that iteration's update, for every active cloud: pred [G][n] =
 * the first maximum of logits [G][n][13], n_correct = #(pred == labels), n_hits = #(mask & pred == hit_ys); hist_row [G][3] =
 * {n_correct, n_hits, 0}.  The cloud leaves when it >= 1 and den * n_hits > num * n_mask[g] (integers): out_pred [G][n] = pred,
 * out_stats [G][3] = the history row, exit_step[g] = it, leaving[g] = 1 (0 for an active cloud that stays).  final != 0 writes
 * out_pred and out_stats of every active cloud (the cap; exit_step only where the test fires).  `active` is NOT cleared and the
 * colours are not snapshot here: the leaving cloud still receives this iteration's update, then psg_rla_tbim_retire_clouds.
 * Inside a replayed window `it` is read from the window's step-constant device row.  scratch: [G][2 * PSG_RLA_NU_PARTS + 1]. */
int psg_rla_tbim_latch_clouds(const float *logits, const int32_t *labels, const int32_t *hit_ys, const uint8_t *mask,
                              const int32_t *n_mask, int G, int n, int num, int den, int it, int final, float *hist_row, int32_t *pred,
                              int32_t *out_pred, float *out_stats, const uint8_t *active, uint8_t *leaving, int32_t *exit_step,
                              int32_t *scratch, psg_stream stream);
/* After the update: every active cloud that is leaving (or, final != 0, every active cloud) gets out_adv [G][n][3] = the colours
 * of feat [G][n][6], then active[g] = 0 and leaving[g] = 0. */
int psg_rla_tbim_retire_clouds(const float *feat, int G, int n, int final, float *out_adv, uint8_t *active, uint8_t *leaving,
                               psg_stream stream);

/* One window of the lockstep TBIM: for each of n_steps iterations it = it0 + i: psg_rla_forward, psg_rla_tbim_latch_clouds
 * (history row i; final on the window's last step when `final` is set), the masked hinge gradient against loss_ys with `sign`
 * (psg_rla_colper_grad_masked), psg_rla_backward, psg_rla_bim_step_clouds on the active clouds, psg_rla_tbim_retire_clouds.
 * There is no tail forward: a cloud's snapshot is the prediction BEFORE the update of its last iteration and the colours AFTER
 * it, as in TBIM.batch_attack.  hit_ys are the labels the hits are counted against (the target on the origin points), loss_ys
 * the ones the hinge is taken against (the same for goal 't' / 'tm', the true labels for goal 'ut').  `graph` as for
 * psg_rla_nu_window: first window of a shape eager, second captured, later ones replayed, a single chain on `stream`; no graph
 * while psg_rla_prof_enable is on or before the first psg_rla_forward of (cloud, model).  The key is this block without it0. */
typedef struct psg_rla_tbim_window_args {
    psg_rla_model *model;
    psg_rla_ws *ws;
    int n_steps, G, N, it0;
    int num, den;                /* the exit threshold num / den */
    int final, l2_metric;
    float eps, alpha, sign;      /* sign: -1 for goal 't' / 'tm', +1 for goal 'ut' */
    const float *ori;            /* [G][N][3] clean colours */
    const uint8_t *mask;         /* [G][N], required */
    const int32_t *n_mask;       /* [G], required */
    const int32_t *labels, *hit_ys, *loss_ys;   /* [G][N] */
    float *feat;                 /* [G][N][6], xyz in columns 0..2 */
    float *logits, *dlogits;     /* [G][N][13] */
    float *dfeat;                /* [G][N][6] */
    float *norms;                /* [2][G] */
    float *delta;                /* [G][N][3] */
    int32_t *pred;               /* [G][N] */
    int32_t *scratch;            /* [G][2 * PSG_RLA_NU_PARTS + 1] */
    float *hist;                 /* [n_steps][G][3] */
    float *out_adv;              /* [G][N][3] */
    int32_t *out_pred;           /* [G][N] */
    float *out_stats;            /* [G][3] */
    uint8_t *active, *leaving;   /* [G] */
    int32_t *exit_step;          /* [G], -1 before */
} psg_rla_tbim_window_args;
int psg_rla_tbim_window(const psg_rla_tbim_window_args *args, psg_nu_graph *graph, psg_stream stream);

/* NUattack / tar_NUattack on the COORDINATE field of G clouds of n points in lockstep.  The optimiser
 * variable is delta [G][n][3] in metres (no tanh space: coordinates have no box).  Buffers are cloud-major, `active` [G] as
 * above (NULL: every cloud), an inactive cloud is skipped by whole workgroups; no float atomics anywhere.
 *
 * psg_rla_nu_coord_apply_clouds: positions fl(ori_xyz + delta) on the points of mask [G][n] (NULL: all points; the others keep
 * ori_xyz byte for byte) into columns 0..2 of feat [G][n][6] and into the contiguous xyz [G][n][3] (what the pyramid is
 * rebuilt from); dist2_xyz[g] = sum (xyz as written - ori_xyz)^2, the difference formed in double, summed in a fixed order by
 * PSG_RLA_NU_PARTS workgroups per cloud (partials: [G][PSG_RLA_NU_PARTS] doubles of scratch), rounded to float once. */
int psg_rla_nu_coord_apply_clouds(const float *ori_xyz, const float *delta, const uint8_t *mask, const uint8_t *active, int G, int n,
                                  float *feat, float *xyz, float *dist2_xyz, double *partials, psg_stream stream);
/* One TF1-Adam step (t = 1, 2, ..; betas 0.9 / 0.999, eps 1e-8 outside the root; psg_rla_nu_adam_clouds' operation order) on
 * delta of loss = |xyz - ori_xyz|_2 + c * score:  g = (dist > 0 ? (xyz - ori_xyz) / dist : 0) + c * (dfeat[:, 0:3] + dxyz), the
 * inner sum one fp32 add as in psg_rla_bim_step_field, g = 0 off the mask; dist = sqrt(dist2_xyz[g]); xyz [G][n][3] the
 * positions psg_rla_nu_coord_apply_clouds wrote, dfeat [G][n][6] / dxyz [G][n][3] from psg_rla_backward_full.  lr_t is
 * computed in double on the host, or read from the step-constant device row when one is set (psg_rla_nu_adam_clouds). */
int psg_rla_nu_coord_adam_clouds(const float *ori_xyz, float *delta, float *m_xyz, float *v_xyz, const uint8_t *mask,
                                 const uint8_t *active, const float *xyz, const float *dfeat, const float *dxyz, const float *dist2_xyz,
                                 int G, int n, float c, float lr, int t, psg_stream stream);
/* psg_rla_nu_latch_clouds (the same count stage, exit rules, integer thresholds, can_exit, "never the unperturbed start") with
 * a 4-column row: hist_row [G][4] = {n_correct, n_hits, dist2_rgb[g], dist2_xyz[g]} (dist2_rgb NULL: 0, the "coord" field), and
 * a snapshot that also carries the positions: out_adv_xyz [G][n][3] = columns 0..2 of feat, out_adv [G][n][3] = columns 3..5,
 * out_pred [G][n], out_stats [G][4] = the row. */
int psg_rla_nu_field_latch_clouds(const float *logits, const int32_t *labels, const int32_t *ys, const uint8_t *mask,
                                  const int32_t *n_mask, const float *feat, const float *dist2_rgb, const float *dist2_xyz, int G, int n,
                                  int mode, int num, int den, int step, int can_exit, int final, float *hist_row, int32_t *pred,
                                  float *out_adv_xyz, float *out_adv, int32_t *out_pred, float *out_stats, uint8_t *active,
                                  int32_t *exit_step, int32_t *scratch, psg_stream stream);

/* One window of the lockstep attack on the coordinate field, or on both fields.  For each of n_steps optimiser steps with Adam
 * index t = adam_t0 + i: psg_rla_nu_coord_apply_clouds (field BOTH: then psg_rla_nu_color_clouds), the index pyramid of all G
 * clouds rebuilt from `xyz` (what psg_rla_set_cloud(ws, xyz) does, stream-ordered, no read-back), psg_rla_forward, the field
 * latch of evaluation index t - 1 (history row i; exits from index 1 on), psg_rla_colper_grad_masked against ys (sign +1),
 * psg_rla_backward_full, psg_rla_nu_coord_adam_clouds with coord_lr (field BOTH: then psg_rla_nu_adam_clouds with lr, the colour
 * variable keeping its own dist2 and moments).  tail_eval != 0 appends apply, pyramid, forward and a latch with final = 1
 * (history row n_steps).  Nothing returns to the host inside a window; there is no hipGraph form (the pyramid's sorts and the
 * per-step xyz branch are not captured).  A frozen cloud's delta, moments and snapshot are not touched; its pyramid is rebuilt
 * from unchanged positions, to the same bits.  PSG_ERR_ARG, before anything is enqueued: a workspace that is not
 * psg_rla_ws_create_full's, (G, N) not the workspace's, field not COORD / BOTH, n_steps < 1, mode 1 without mask / n_mask, a
 * null required pointer (field COORD needs none of xs, dws, m, v, dist2, partials). */
typedef struct psg_rla_nu_field_window_args {
    psg_rla_model *model;
    psg_rla_ws *ws;              /* psg_rla_ws_create_full, G clouds of N points */
    int n_steps, G, N, mode;
    int num, den;                /* the exit threshold num / den */
    int adam_t0, tail_eval;
    int field;                   /* PSG_NU_FIELD_COORD or PSG_NU_FIELD_BOTH */
    float cs, lr, coord_lr;
    const float *xs;             /* [G][N][3] clean colours (BOTH) */
    float *dws, *m, *v;          /* [G][N][3] the colour variable and its moments (BOTH) */
    float *delta, *m_xyz, *v_xyz;   /* [G][N][3] the coordinate variable and its moments */
    const float *ori_xyz;        /* [G][N][3] clean positions */
    float *xyz;                  /* [G][N][3] the positions of the step, contiguous */
    float *dxyz;                 /* [G][N][3] */
    const uint8_t *mask;         /* [G][N], nullable (required in mode 1) */
    const int32_t *n_mask;       /* [G], mode 1 */
    const int32_t *labels, *ys;  /* [G][N] */
    float *feat;                 /* [G][N][6] */
    float *logits, *dlogits;     /* [G][N][13] */
    float *dfeat;                /* [G][N][6] */
    float *dist2, *dist2_xyz;    /* [G] each (dist2: BOTH) */
    double *partials, *partials_xyz;   /* [G][PSG_RLA_NU_PARTS] each (partials: BOTH) */
    int32_t *pred;               /* [G][N] */
    int32_t *scratch;            /* [G][2 * PSG_RLA_NU_PARTS + 1] */
    float *hist;                 /* [n_steps + (tail_eval != 0)][G][4] */
    float *out_adv, *out_adv_xyz;   /* [G][N][3] each */
    int32_t *out_pred;           /* [G][N] */
    float *out_stats;            /* [G][4] */
    uint8_t *active;             /* [G] */
    int32_t *exit_step;          /* [G], -1 before */
} psg_rla_nu_field_window_args;
int psg_rla_nu_field_window(const psg_rla_nu_field_window_args *args, psg_stream stream);

/* BIM / NBattack and TBIM / tar_NBattack on the COORDINATE field of G clouds of n points in lockstep.
 *
 * psg_rla_bim_step_field_clouds: psg_rla_bim_step_field's update of every running cloud (running [G] bytes, NULL: all) of
 * feat [G][n][6] with that cloud's own norms: norms [2][G] = {|g|^2, |delta|^2} of cloud g, delta [G][n][3] (both l_2 only),
 * g = dfeat[:, 0:3] + dxyz as one fp32 add, no box.  The same kernels serve psg_rla_bim_step_field (G = 1) and keep its
 * summation order (one workgroup per cloud, double accumulation, the fixed tree), so a cloud's positions are bit-equal to
 * psg_rla_bim_step_field on that cloud alone.  xyz_out [G][n][3] (nullable): the new positions, contiguous - the bytes of
 * feat's columns 0..2 - for the pyramid rebuild.  No byte of feat, delta, norms or xyz_out of a cloud that is not running is
 * written, whatever its gradients hold. */
int psg_rla_bim_step_field_clouds(float *feat, const float *dfeat, const float *dxyz, const float *ori_xyz, const uint8_t *running,
                                  int G, int n, float eps, float alpha, int l2_metric, float *norms, float *delta, float *xyz_out,
                                  psg_stream stream);
/* psg_rla_tbim_retire_clouds with both halves of feat snapshot: every active cloud that is leaving (or, final != 0, every
 * active cloud) gets out_adv_xyz [G][n][3] = columns 0..2 and out_adv [G][n][3] = columns 3..5 of feat [G][n][6], then
 * active[g] = 0 and leaving[g] = 0. */
int psg_rla_tbim_retire_field_clouds(const float *feat, int G, int n, int final, float *out_adv, float *out_adv_xyz, uint8_t *active,
                                     uint8_t *leaving, psg_stream stream);

/* One window of the lockstep BIM family on the coordinate field, or on both fields.  For each of n_steps iterations
 * it = it0 + i: the index pyramid of all G clouds rebuilt from `xyz` (what psg_rla_set_cloud(ws, xyz) does, stream-ordered, no
 * read-back; the caller puts the starting positions there), psg_rla_forward on feat, in mode 1 psg_rla_tbim_latch_clouds
 * (history row i [G][3]; final on the window's last step when `final` is set), psg_rla_colper_grad_masked against loss_ys with
 * mask and `sign` (mode 0: against labels, no mask, sign +1), psg_rla_backward_full, psg_rla_bim_step_field_clouds with
 * (coord_eps, coord_alpha) on the active clouds, writing `xyz`; field BOTH: then psg_rla_bim_step_clouds with (eps, alpha) on
 * the colours; psg_rla_tbim_retire_field_clouds.  `delta` is the scratch of both steps, one after the other.
 *   mode 1 (TBIM): psg_rla_tbim_window's semantics - the update of the exiting iteration is still applied to the leaving cloud,
 *     its snapshot is the prediction BEFORE that update and the positions and colours AFTER it, the cap is snapshot the same
 *     way under `final`, there is no tail forward.
 *   mode 0 (BIM, goal 'ut'): no latch, no exit; every active cloud takes every step; `final` on the window's last step snapshots
 *     all of them (out_adv, out_adv_xyz) and clears `active`.  hist, mask, n_mask, hit_ys, loss_ys, leaving and exit_step may be
 *     NULL; sign, num and den are not used (den > 0 is still required).
 * A retired cloud's positions, colours and snapshot are not touched; its pyramid is rebuilt from unchanged positions, to the
 * same bits.  Eager: there is no hipGraph form (the pyramid's sorts are not captured).  PSG_ERR_ARG, before anything is
 * enqueued: a workspace that is not psg_rla_ws_create_full's, (G, N) not the workspace's, field not COORD / BOTH, mode not 0 / 1,
 * n_steps < 1, it0 < 0, den <= 0, mode 1 without mask / n_mask / hit_ys / loss_ys / hist / leaving / exit_step, l_2 without
 * norms_xyz / delta (BOTH: norms), BOTH without ori, any other null pointer (COORD needs neither ori nor norms). */
typedef struct psg_rla_bim_field_window_args {
    psg_rla_model *model;
    psg_rla_ws *ws;              /* psg_rla_ws_create_full, G clouds of N points */
    int n_steps, G, N, it0;
    int num, den;                /* the exit threshold num / den (mode 1) */
    int final, l2_metric;
    int mode, field;             /* 0 BIM / 1 TBIM; PSG_NU_FIELD_COORD or PSG_NU_FIELD_BOTH */
    float eps, alpha, sign;      /* the colours' (BOTH); sign: -1 for goal 't' / 'tm', +1 for goal 'ut' (mode 1) */
    float coord_eps, coord_alpha;   /* the positions' (4 bytes of padding follow) */
    const float *ori;            /* [G][N][3] clean colours (BOTH) */
    const uint8_t *mask;         /* [G][N] (mode 1) */
    const int32_t *n_mask;       /* [G] (mode 1) */
    const int32_t *labels, *hit_ys, *loss_ys;   /* [G][N] (hit_ys, loss_ys: mode 1) */
    float *feat;                 /* [G][N][6] */
    float *logits, *dlogits;     /* [G][N][13] */
    float *dfeat;                /* [G][N][6] */
    float *norms;                /* [2][G] (l_2, BOTH) */
    float *delta;                /* [G][N][3] (l_2) */
    int32_t *pred;               /* [G][N] */
    int32_t *scratch;            /* [G][2 * PSG_RLA_NU_PARTS + 1] */
    float *hist;                 /* [n_steps][G][3] (mode 1) */
    float *out_adv;              /* [G][N][3] */
    int32_t *out_pred;           /* [G][N] */
    float *out_stats;            /* [G][3] */
    uint8_t *active, *leaving;   /* [G] (leaving: mode 1) */
    int32_t *exit_step;          /* [G], -1 before (mode 1) */
    const float *ori_xyz;        /* [G][N][3] clean positions */
    float *xyz;                  /* [G][N][3] the positions of the iteration, contiguous */
    float *dxyz;                 /* [G][N][3] */
    float *norms_xyz;            /* [2][G] (l_2) */
    float *out_adv_xyz;          /* [G][N][3] */
} psg_rla_bim_field_window_args;
int psg_rla_bim_field_window(const psg_rla_bim_field_window_args *args, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * RandLA-Net data preparation: grid sub-sampling and the projection of raw points onto the sub-cloud (psg_grid.hip).
 *
 * A.  DataProcessing.grid_sub_sampling (RandLA-Net/helper_tool.py:197-216) = cpp_subsampling.compute
 * (utils/cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:5-106): one output point per occupied cell of
 * edge grid_size - the barycentre of the cell's points, their mean feature, their most frequent label per label dimension.  All
 * arithmetic is fp32 in the reference's order (a cell's sums are sequential additions in INPUT order), so barycentres and
 * mean features are bit-equal to the reference's.  Ours: the output is in ascending cell-key order (the reference's is its hash
 * map's iteration order); of equally frequent labels the smallest (signed) wins; a cell index of -1 (the origin can exceed
 * the minimum corner by a rounding; undefined in the reference) counts as 0.  Results are the same bytes from run to run.
 *
 * One handle holds the scratch of clouds of up to max_points points (about 60 bytes per point) and the state between the
 * calls; it is used from one stream at a time.  Everything is enqueued on `stream`; psg_grid_assign and psg_grid_index
 * synchronise it.
 *
 * psg_grid_assign: points [n][3] device -> the cells, their order and *n_voxels_out = M, the number of occupied cells
 * (two small read-backs: the corners of the cloud, from which the host derives the grid, and M, which sizes the
 * caller's outputs); voxel_of_point [n] (device, or NULL) = the output row of every input point.  Refuses, before
 * anything is written: n < 1, grid_size not a positive finite number, non-finite coordinates, a grid of more than 2^20
 * cells along an axis.
 * psg_grid_reduce: the outputs of the last psg_grid_assign, from the same `points`: sub_points [M][3], sub_features [M][d]
 * from features [n][d] (d = 0: both NULL), sub_labels [M][l] from labels [n][l] int32, any values (l = 0: both NULL).
 *
 * B.  proj_idx of utils/data_prepare_s3dis.py (KDTree(sub_xyz).query(xyz, k = 1)): psg_grid_index bins sub_points [m][3]
 * by their own coordinates into cells of edge grid_size - the SMALLEST cell the table uses: the edge is doubled until the grid has
 * at most 64 cells per sub-point and 2^20 along an axis, which bounds a query's work; the answer does not depend on it - and
 * keeps them sorted by cell key in the handle (this replaces the state of psg_grid_assign);
 * psg_grid_nearest writes, for query [n_query][3], out_idx [n_query] = the index of the nearest sub-point, exactly
 * psg_knn_points(sub_points, query, k = 1): fp32 distance ((dx*dx) + dy*dy) + dz*dz, ties to the lower index - found through
 * the cell table, ring by ring, under a stopping bound that is conservative in fp32.  Queries outside the
 * cloud's box are answered too (the further out, the more of the table they read).
 * ------------------------------------------------------------------------------------------ */
typedef struct psg_grid psg_grid;
int psg_grid_create(psg_ctx *ctx, int max_points, psg_grid **out);
int psg_grid_destroy(psg_grid *g);
int psg_grid_assign(psg_grid *g, const float *points, int n, float grid_size, int32_t *voxel_of_point, int *n_voxels_out,
                    psg_stream stream);
int psg_grid_reduce(psg_grid *g, const float *points, const float *features, int d, const int32_t *labels, int l,
                    float *sub_points, float *sub_features, int32_t *sub_labels, psg_stream stream);
int psg_grid_index(psg_grid *g, const float *sub_points, int m, float grid_size, psg_stream stream);
int psg_grid_nearest(psg_grid *g, const float *query, int n_query, int32_t *out_idx, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * Whole-scene NB attack: one colour per scene point across all the overlapping blocks that hold
 * it.  A "slot" is a block row e = b * block_points + i of the scene's block arrays [rows][.]; point_idx [rows] int32
 * names the scene point of every slot.  rows must lie in 1 .. INT_MAX / 9 (slot numbers address [rows][9] floats):
 * anything else is refused with a message.  Nothing here uses float atomics; every output element has one writer.
 *
 * psg_scene_occ_build: the occurrence lists of every scene point, built once per scene: occ_off [n_scene + 1] (offsets,
 * occ_off[n_scene] = number of valid slots), occ_ent [rows] (the slots of point p at occ_off[p] .. occ_off[p + 1],
 * ASCENDING) - exactly np.argsort(point_idx, kind = "stable") with the offsets of np.bincount; the result does not
 * depend on scheduling.  scratch: int32 [n_scene + rows].  A slot whose index lies outside [0, n_scene) ORs 1 into
 * *bad_flag (int32, device: the psg_vote_add convention), joins no list and is neither read nor written through; the
 * unused tail of occ_ent then holds -1.
 * psg_scene_colour_to_blocks: x [rows][9], channels 3:6 of every slot <- scene_rgb [n_scene][3] of its point; the other
 * six floats of a row keep their bytes.  Bad index: flag, row untouched.
 * psg_scene_rows_mask: dlogp [rows][n_cls]: the rows of slots whose scene point is not under scene_mask [n_scene] (uint8)
 * are set to +0.0, the others are not touched (an index out of range counts as not masked).
 * psg_scene_pgd_step: for every scene point p (scene_mask nullable: under the mask only) with at least one slot:
 *   g = ((0 + dx0[e_0][3:6]) + dx0[e_1][3:6]) + ...   over the slots of p in list order, fp32, no contraction
 *   and then psg_pgd_step's arithmetic with scene_ori [n_scene][3] as the clean colours:
 *   stepped = c + dir*alpha*sign(g) (sign(0) = sign(NaN) = 0);  eta = clamp(stepped - ori, -eps, eps);
 *   c = last ? stepped : clamp(ori + eta, 0, 1)
 * scene_rgb [n_scene][3] in place.  A point without a slot does not move.  Every list is bounded by rows (offsets
 * clamped, entries outside [0, rows) skipped).  gsum_out (nullable) [n_scene][3]: the summed gradient (+0 for points
 * outside the mask or without a slot).
 * ------------------------------------------------------------------------------------------ */
int psg_scene_occ_build(const int32_t *point_idx, int rows, int n_scene, int32_t *occ_off, int32_t *occ_ent,
                        int32_t *scratch, int32_t *bad_flag, psg_stream stream);
int psg_scene_colour_to_blocks(const float *scene_rgb, const int32_t *point_idx, int rows, int n_scene, float *x,
                               int32_t *bad_flag, psg_stream stream);
int psg_scene_rows_mask(float *dlogp, const int32_t *point_idx, const uint8_t *scene_mask, int rows, int n_cls,
                        int n_scene, psg_stream stream);
int psg_scene_pgd_step(float *scene_rgb, const float *scene_ori, const uint8_t *scene_mask, const int32_t *occ_off,
                       const int32_t *occ_ent, const float *dx0, int rows, int n_scene, float alpha, float eps, float dir,
                       int last, float *gsum_out, psg_stream stream);

/* The coordinate field of the whole-scene attack: ONE displacement delta [n_scene][3] (metres) per
 * scene point.  Same slot / rows conventions and refusals as above; no float atomics, one writer per output element.
 *
 * psg_scene_delta_to_blocks: x [rows][9], channels 0:3 of every slot <- fl32(x_clean[e][0:3] + delta[point_idx[e]]): one
 * fp32 add onto the CLEAN block coordinates x_clean [rows][9] (channels 0:3 are read); the other six floats of a row of x
 * keep their bytes.  Bad index: flag, row neither read nor written.
 * psg_scene_field_step: for every scene point p (scene_mask nullable: under the mask only) with at least one slot:
 *   g = ((0 + dx0[e_0][0:3]) + dx0[e_1][0:3]) + ...   over the slots of p in list order, fp32, no contraction
 *   stepped = delta + fl(dir*alpha)*sign(g) (sign(0) = sign(NaN) = 0);  delta = last ? stepped : clamp(stepped, -eps, +eps)
 * delta [n_scene][3] in place; there is no box.  A point without a slot does not move.  Lists are bounded as in
 * psg_scene_pgd_step; gsum_out (nullable) [n_scene][3] as there. */
int psg_scene_delta_to_blocks(const float *delta, const int32_t *point_idx, const float *x_clean, int rows, int n_scene,
                              float *x, int32_t *bad_flag, psg_stream stream);
int psg_scene_field_step(float *delta, const uint8_t *scene_mask, const int32_t *occ_off, const int32_t *occ_ent,
                         const float *dx0, int rows, int n_scene, float alpha, float eps, float dir, int last,
                         float *gsum_out, psg_stream stream);

/* Whole-scene NU attack: Adam in tanh space on ONE colour per scene point.  w / m / v / c / c0 are
 * [n_scene][3] fp32; slots, lists (psg_scene_occ_build) and the rows guard as above; no float atomics, one writer per
 * output element.  `active` is one int32 word on the device (1 while the attack runs): while it is 0 psg_scene_nu_colour,
 * psg_scene_nu_step and psg_scene_nu_latch leave every byte alone.  A point MOVES when it is under scene_mask (nullable =
 * all points) and has at least one slot; every other point keeps the bytes of its w / m / v / c.
 *
 * psg_scene_nu_init: w = 0.5 * log((1 + x) / (1 - x)), x = 2 c0 - 1, for every point (psg_nu_inverse_tanh's formula).
 * psg_scene_nu_colour: c = 0.5 * (tanh(w) + 1) on the moving points (psg_nu_tanh_color's formula).
 * psg_scene_nu_step: for every moving point and channel, in psg_nu_adam_step's expression order, fp32, no contraction:
 *   Gf = ((0 + dx0[e_0][3:6]) + dx0[e_1][3:6]) + ...    over the slots of the point in list order (dx0 [rows][9])
 *   Gs = the same ordered sum over sgrad [rows][3]       (the per-slot Smooth gradients)
 *   g  = Gf + (cw * 2) * (c - c0);  g = g + cw * Gs;  th = tanh(w);  g = (g * 0.5) * (1 - th * th)
 *   then torch.optim.Adam's single-tensor update on w / m / v (step >= 1; lr / (1 - beta1^step) and sqrt(1 - beta2^step)
 *   computed in double on the host, as psg_nu_adam_step does).  The L2 term counts once per POINT, not once per slot.
 *   gsum_f_out / gsum_s_out (nullable) [n_scene][3]: Gf and Gs (+0 for points that do not move).
 * psg_scene_nu_latch: the exit test in integers over all slots.  Non-targeted (scene_mask == NULL): n_hits = slots with
 *   pred == labels, n_counted = rows; fires when n_hits * den < num * n_counted.  Targeted (scene_mask given; labels may be
 *   NULL): n_counted = slots whose point is under the mask (an index out of range counts as unmasked), n_hits = those with
 *   pred == target; fires when n_hits * den > num * n_counted.  64-bit products, no float arithmetic.  Two launches: the
 *   counts (integer atomics into counters [2], int32, which must be zero on entry and are left zero), then ONE workgroup
 *   whose first thread decides.  While active: hist_row [2] (int64) <- n_hits, n_counted; a firing step copies c into snap
 *   [n_scene][3], stores `step` in exit_step [1] and clears active.  num >= 0, den > 0. */
int psg_scene_nu_init(const float *c0, int n_scene, float *w_out, psg_stream stream);
int psg_scene_nu_colour(const float *w, const uint8_t *scene_mask, const int32_t *occ_off, int n_scene,
                        const int32_t *active, float *c, psg_stream stream);
int psg_scene_nu_step(float *w, float *m, float *v, const float *c, const float *c0, const uint8_t *scene_mask,
                      const int32_t *occ_off, const int32_t *occ_ent, const float *dx0, const float *sgrad, int rows,
                      int n_scene, float cw, float lr, float beta1, float beta2, float eps, int step,
                      const int32_t *active, float *gsum_f_out, float *gsum_s_out, psg_stream stream);
int psg_scene_nu_latch(const int32_t *pred, const int32_t *labels, int target, const int32_t *point_idx,
                       const uint8_t *scene_mask, int rows, int n_scene, int num, int den, int step, const float *c,
                       float *snap, int32_t *counters, long long *hist_row, int32_t *exit_step, int32_t *active,
                       psg_stream stream);

/* The coordinate field of the whole-scene NU attack: Adam on ONE displacement delta [n_scene][3]
 * (metres, no tanh space: coordinates have no box) per scene point; delta / m / v [n_scene][3] fp32 in place.  Lists, the
 * rows guard, the moving points and the `active` word as for psg_scene_nu_step; the slots are written by
 * psg_scene_delta_to_blocks.  For every moving point and channel ch = 0..2, in psg_nu_coord_adam_step_rooms' expression
 * order, fp32, no contraction:
 *   Gx = ((0 + dx0[e_0][ch]) + dx0[e_1][ch]) + ...       over the slots of the point in list order (dx0 [rows][9])
 *   Gs = the same ordered sum over sgrad_xyz [rows][3]    (the per-slot Smooth_xyz gradients, psg_smooth_knn_xyz_rooms)
 *   g  = Gx + (coord_c * 2) * delta;  g = g + coord_c * Gs
 *   then torch.optim.Adam's single-tensor update on delta / m / v (step >= 1; the step constants in double on the host).
 * The L2 term counts once per POINT.  gsum_x_out / gsum_s_out (nullable) [n_scene][3]: Gx and Gs (+0 for points that do
 * not move).  No float atomics, one writer per output element; while active[0] == 0 every byte is left alone. */
int psg_scene_nu_field_step(float *delta, float *m, float *v, const uint8_t *scene_mask, const int32_t *occ_off,
                            const int32_t *occ_ent, const float *dx0, const float *sgrad_xyz, int rows, int n_scene,
                            float coord_c, float coord_lr, float beta1, float beta2, float eps, int step,
                            const int32_t *active, float *gsum_x_out, float *gsum_s_out, psg_stream stream);

/* ------------------------------------------------------------------------------------------
 * The whole-scene block slicer on the device (psg_slice.hip): the per-cell work of
 * ScannetDatasetWholeScene.__getitem__ (PointNet/data_utils/S3DISDataLoader.py:124-175).  The random draws stay on the
 * host (harness.slice_plan: they depend on the cells' member counts only).  No handle: the caller owns every buffer.
 * Everything is enqueued on `stream`; nothing here synchronises.  No atomics; every output element has one writer; two
 * runs give the same bytes.
 *
 * Scene: n <= 2^30 points; x of point p at xy[p * stride], y at xy[p * stride + 1] (float64; stride in doubles, >= 2).
 * windows [n_cells][4] float64 = {s_x - pad, e_x + pad, s_y - pad, e_y + pad} in the slicer's cell order (iy outer, ix
 * inner), computed by the host; point p is a member of cell c when x >= w[0] && x <= w[1] && y >= w[2] && y <= w[3] (IEEE
 * double compares; a NaN is in no cell).  1 <= n_cells <= PSG_SLICE_MAX_CELLS (the windows sit in LDS), anything else is
 * PSG_ERR_ARG.  tile_off: int32 scratch of tile_items >= n_cells * ceil(n / PSG_SLICE_TILE) + 1 items (a product beyond
 * 2^30 is refused), written by psg_slice_count and read by psg_slice_members.
 *
 * psg_slice_count: counts [n_cells] = the members of every cell; cell_off [n_cells + 1] = their exclusive prefix sums
 * modulo 2^32 (the caller sums counts in 64 bits and goes no further when the total exceeds INT_MAX).
 * psg_slice_members: inside [inside_len], inside_len = the total: the members of cell c in ASCENDING point index
 * (np.where's order) at cell_off[c] .. cell_off[c + 1].  Same xy / windows as the count; a position outside inside_len
 * is not written.
 * psg_slice_gather: one output slot e = b * bp + i of nb blocks of bp points (nb * bp <= INT_MAX / 9): cell =
 * block_cell[b], p = inside[cell_off[cell] + src_pos[e]];
 *   data [nb][bp][9] float32 = x - centres[cell][0], y - centres[cell][1], z, r / 255.0, g / 255.0, b / 255.0, x / cmax_x,
 *     y / cmax_y, z / cmax_z: each ONE float64 operation (a true division) rounded once to float32;
 *   label [nb][bp] = labels[p];  smpw = labelweights[label] (float32 table of PSG_SLICE_CLASSES entries; +0 for a label
 *   outside it);  index = p.
 * xyz [n] rows of xyz_stride doubles, rgb [n] rows of rgb_stride doubles (both >= 3), centres [n_cells][2] float64.  A slot
 * whose cell, position or point is out of range reads nothing through it: data 0, label 0, smpw 0, index -1.
 * ------------------------------------------------------------------------------------------ */
#define PSG_SLICE_MAX_CELLS 1024
#define PSG_SLICE_TILE 256
#define PSG_SLICE_CLASSES 13
int psg_slice_count(const double *xy, int stride, int n, const double *windows, int n_cells, int32_t *tile_off,
                    long long tile_items, int32_t *counts, int32_t *cell_off, psg_stream stream);
int psg_slice_members(const double *xy, int stride, int n, const double *windows, int n_cells, const int32_t *tile_off,
                      long long tile_items, int32_t *inside, int inside_len, psg_stream stream);
int psg_slice_gather(const double *xyz, int xyz_stride, const double *rgb, int rgb_stride, const int32_t *labels, int n,
                     const int32_t *inside, int inside_len, const int32_t *cell_off, const int32_t *block_cell,
                     const double *centres, int n_cells, const int32_t *src_pos, int nb, int bp, double cmax_x, double cmax_y,
                     double cmax_z, const float *labelweights, float *data, int32_t *label, float *smpw, int32_t *index,
                     psg_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PSG_H */
