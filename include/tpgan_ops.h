/*
 * tpgan_ops.h -- C-ABI of libtpgan_hip.so: the MI355X (gfx950) neighbourhood
 * ops under TPU-GAN's generator, discriminators and losses.
 *
 * The reference (zijieli-Jlee/Temporal-Pointcloud-Upsampling-GAN) is pure
 * Python and never binds a C symbol itself: it calls four third-party CUDA
 * extensions through their Python APIs.  Each entry point below is what those
 * Python APIs bind underneath, restated as a plain C function; the comment on
 * each one cites the reference call site(s) it serves.  The ctypes binding the
 * reference side would add is shown in INTEGRATION.md and implemented in
 * temporal-pointcloud-upsampling-gan_amd/_lib.py.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM), row-major contiguous, fp32 /
 *     int32 / int64 as named; the caller owns every buffer, the library never
 *     allocates, never synchronises and holds no state;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - returns 0 on success, <0 on error (tpg_status); never throws;
 *   - canonical arithmetic: sqdist(a,b) = sum_d (a_d-b_d)^2 accumulated in d
 *     order in fp32 without FMA; neighbour order ascending (dist, idx).
 */
#ifndef TPGAN_OPS_H
#define TPGAN_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    TPG_OK = 0,
    TPG_ERR_ARG = -1,         /* bad shape / null pointer / size out of range   */
    TPG_ERR_LAUNCH = -2,      /* hipGetLastError() != hipSuccess after launch   */
    TPG_ERR_UNSUPPORTED = -3  /* e.g. K > TPG_MAX_K                             */
} tpg_status;

#define TPG_MAX_K 64 /* neighbours per query held one-per-lane in a wave64 */

/* library / device identification; safe to call without a GPU */
const char *tpg_version(void);
const char *tpg_target_arch(void); /* "gfx950" */

/* K nearest neighbours in D-dim space, optional radius cut.
 * Replaces pytorch3d.ops.knn_points -- gcn_lib/pointnet/gcn.py:16-21,38,258;
 * discriminator.py:15-20,33-38 -- and frnn.frnn_grid_points --
 * discriminator.py:27-32; loss.py:105,142,229,256-265;
 * gcn_lib/interpolation.py:20,33.
 * p1 (B,P1,D), p2 (B,P2,D); len1/len2 (B) int64 or NULL (= full).
 * r2 < 0: plain kNN, missing slots dist 0 / idx 0.
 * r2 >= 0: only d < r2 (strict); missing slots dist -1 / idx -1.
 * dist (B,P1,K) f32, idx (B,P1,K) i64, sorted ascending (dist, idx). */
int tpg_knn_f32(const float *p1, const float *p2, const int64_t *len1,
                const int64_t *len2, int B, int P1, int P2, int D, int K,
                float r2, float *dist, int64_t *idx, void *stream);

/* Plain 3-D kNN (r2 < 0 form of tpg_knn_f32, D = 3, K <= 64) on the uniform grid of tpg_frnn_grid_f32 with cells of
 * ~K/2 points: the (2R+1)^3 cells around the query's cell, R grown until the K-th distance lies inside the
 * covered region.  For the first EdgeConv's search on large clouds (gcn_lib/pointnet/gcn.py:38 at cfg5 /
 * rollout sizes) and the Chamfer nearest neighbours (loss.py:125-127 at 16384 points).  Bit-identical to
 * tpg_knn_f32(r2 < 0) incl. the (0, 0) padding; same workspace as tpg_frnn_grid_f32. */
int tpg_knn_grid_f32(const float *p1, const float *p2, const int64_t *len1, const int64_t *len2, int B,
                     int P1, int P2, int K, float *dist, int64_t *idx, void *ws, void *stream);

/* Plain kNN (no radius) in D = 32 / 64 feature space, 2 <= K <= 24, 16-byte aligned rows: the path
 * tpg_knn_f32 takes by itself for clouds of >= 2048 points (gcn_lib/pointnet/gcn.py:38,258 at cfg5's
 * 4096-point low-resolution clouds; upsampling_network.py:159-174 rollouts).  A Gram-matrix filter on
 * the bf16 matrix cores (split operands, v_mfma_f32_32x32x16_bf16) rules candidates out with a rounding bound,
 * the survivors are re-ranked with the canonical distance, and queries the bound cannot settle are redone by
 * the exhaustive kernel: the output equals tpg_knn_f32's bit for bit.  redo = 0 (diagnostic) skips that
 * last launch and leaves idx[b][i][0] = -2 on the unsettled queries. */
int tpg_knn_mfma_f32(const float *p1, const float *p2, const int64_t *len1,
                     const int64_t *len2, int B, int P1, int P2, int D, int K,
                     float *dist, int64_t *idx, int redo, void *stream);

/* The same search on SMALL clouds (P2 <= 1024; D = 32 / 64, 2 <= K <= 24, 16-byte aligned rows): the path
 * tpg_knn_f32 takes by itself for the generator's (24, 512, 32 / 64) feature-space searches
 * (gcn_lib/pointnet/gcn.py:38,258 at cfg2 / cfg4).  One sweep of the same split-operand Gram products, every
 * approximate distance of a workgroup's 32 queries in LDS, the candidates within twice the rounding bound of the
 * K-th approximate distance re-ranked with the canonical distance; queries with more than 64 candidates, a
 * non-finite bound or a cloud of fewer than 64 valid points are redone by the exhaustive kernel.  The output
 * equals tpg_knn_f32's bit for bit.  redo = 0 (diagnostic) skips that last launch and leaves
 * idx[b][i][0] = -2 on the unsettled queries. */
int tpg_knn_small_f32(const float *p1, const float *p2, const int64_t *len1,
                      const int64_t *len2, int B, int P1, int P2, int D, int K,
                      float *dist, int64_t *idx, int redo, void *stream);

/* The same radius search (r > 0, D = 3, K <= 64) on a UNIFORM GRID, for clouds where the exhaustive
 * kernel stops being free (loss.py:256-265 at 16384 points per cloud; the 10^4..10^5-point rollout,
 * upsampling_network.py:159-174): cells of edge max(r, extent/64), points counting-sorted by cell,
 * one wave per query over its 27 neighbour cells.  Results are bit-identical to tpg_knn_f32 with
 * r2 = fp32(r)*fp32(r): same distance arithmetic, same (dist, idx) selection key, -1 / -1 padding.
 * ws: tpg_frnn_grid_workspace_bytes(B, P2) bytes, 256-byte aligned. */
size_t tpg_frnn_grid_workspace_bytes(int B, int P2);
int tpg_frnn_grid_f32(const float *p1, const float *p2, const int64_t *len1, const int64_t *len2, int B, int P1,
                      int P2, int K, float r, float *dist, int64_t *idx, void *ws, void *stream);

/* Chamfer nearest-neighbour search in both directions (D = 3).
 * Replaces chamferdist.ChamferDistance.forward -- loss.py:125-127,176-181.
 * src (B,N,3), tgt (B,M,3) -> d1,i1 (B,N), d2,i2 (B,M). */
int tpg_chamfer_fwd_f32(const float *src, const float *tgt, int B, int N, int M,
                        float *d1, int64_t *i1, float *d2, int64_t *i2,
                        void *stream);
/* Backward of chamferdist's forward (loss.py:125-127,176-181): g1 (B,N), g2 (B,M) = gradients of d1, d2;
 * gsrc (B,N,3) / gtgt (B,M,3) are overwritten.  No float atomics: each output point sums its own term and the
 * terms of the points that chose it as nearest neighbour (inverted i1 / i2, ascending point order) -- bitwise
 * reproducible and bit-identical to the oracle's two loops.  ws: tpg_chamfer_bwd_workspace_bytes(B, N, M) bytes,
 * 4-byte aligned. */
size_t tpg_chamfer_bwd_workspace_bytes(int B, int N, int M);
int tpg_chamfer_bwd_f32(const float *src, const float *tgt, int B, int N, int M,
                        const int64_t *i1, const int64_t *i2, const float *g1,
                        const float *g2, float *gsrc, float *gtgt, void *ws, void *stream);

/* Furthest point sampling.  Replaces pointnet2_utils.furthest_point_sample --
 * discriminator.py:114.  xyz (B,N,3) -> idx (B,m) int32; temp (B,N) scratch. */
int tpg_fps_f32(const float *xyz, int B, int N, int m, float *temp, int32_t *idx,
                void *stream);

/* The same sampling with the "FPS of an FPS prefix" shortcut (round 3; csrc/fps.hip): every set-abstraction level after
 * the first samples the centres of the level before, in pick order (discriminator.py:114 on :131-137's gather), and
 * the furthest point sampling of such a prefix is 0, 1, ..., m-1 as long as the producing sampling's last maximum was
 * positive.  prefix_out (B) int32 (may be NULL): set to that condition per cloud; prefix_in (B) int32 (may be NULL):
 * the producing launch's flags -- clouds whose flag is set get 0..m-1 without a single round, the others the full
 * algorithm.  Results are identical to tpg_fps_f32 in every case. */
int tpg_fps_prefix_f32(const float *xyz, int B, int N, int m, float *temp, int32_t *idx,
                       const int32_t *prefix_in, int32_t *prefix_out, void *stream);

/* Dataset-side farthest point sampling: sampling.py:50-106 `farthest_point_sampling(pts, k,
 * initial_idx)` (used by train_utils.py:126, train_fluid/tempo_dataset.py:78,
 * train_action/msr_dataset.py:94,130 on the host, numba): start (B) int32 = first pick per cloud
 * (NULL = 0), skip_origin = 0 (every point is eligible; 1 = pointnet2's |x|^2 > 1e-3 rule).
 * Squared distances in fp32, arg-max ties to the smallest index (numpy argmax). */
int tpg_fps_start_f32(const float *xyz, const int32_t *start, int skip_origin, int B, int N, int m,
                      float *temp, int32_t *idx, void *stream);

/* gather_operation fwd/bwd -- discriminator.py:131-137.
 * feat (B,C,N), idx (B,S) -> out (B,C,S); bwd overwrites gfeat (B,C,N). */
int tpg_gather_fwd_f32(const float *feat, const int32_t *idx, int B, int C, int N,
                       int S, float *out, void *stream);
int tpg_gather_bwd_f32(const float *gout, const int32_t *idx, int B, int C, int N,
                       int S, float *gfeat, void *stream);

/* gather_operation on channels-last rows (the layout this build keeps clouds in): out[b,s,:] = rows[b,idx[b,s],:];
 * rows (B,N,C), idx (B,S) int32, out (B,S,C).  Same semantics as tpg_gather_fwd_f32 / _bwd_f32 on the transposed
 * tensors (discriminator.py:131-137), without the two transpose copies around it.  The backward overwrites grows
 * (B,N,C): a row named by several slots (FPS repeats a pick once a cloud runs out of candidates) gets 0.0f plus their
 * gradients in ascending slot order, each addition rounded -- no float atomics, the same bits from run to run. */
int tpg_gather_rows_fwd_f32(const float *rows, const int32_t *idx, int B, int N, int S, int C, float *out, void *stream);
int tpg_gather_rows_bwd_f32(const float *gout, const int32_t *idx, int B, int N, int S, int C, float *grows,
                            void *stream);

/* ball_query -- inside pointnet2_utils.QueryAndGroup, discriminator.py:190.
 * xyz (B,N,3), new_xyz (B,S,3) -> idx (B,S,nsample) int32. */
int tpg_ball_query_f32(const float *xyz, const float *new_xyz, int B, int N, int S,
                       float radius, int nsample, int32_t *idx, void *stream);

/* grouping_operation fwd/bwd -- gcn_lib/pointnet/gcn.py:207,261;
 * discriminator.py:270,273; 2x per QueryAndGroup.
 * feat (B,C,N), idx (B,S,K) -> out (B,C,S,K); bwd overwrites gfeat (B,C,N). */
int tpg_group_fwd_f32(const float *feat, const int32_t *idx, int B, int C, int N,
                      int S, int K, float *out, void *stream);
int tpg_group_bwd_f32(const float *gout, const int32_t *idx, int B, int C, int N,
                      int S, int K, float *gfeat, void *stream);

/* three_nn / three_interpolate -- pointnet2_utils API completeness (no call
 * site in the reference).  dist2 holds SQUARED distances. */
int tpg_three_nn_f32(const float *unknown, const float *known, int B, int n, int m,
                     float *dist2, int32_t *idx, void *stream);
int tpg_three_interp_fwd_f32(const float *feat, const int32_t *idx, const float *w,
                             int B, int C, int m, int n, float *out, void *stream);
int tpg_three_interp_bwd_f32(const float *gout, const int32_t *idx, const float *w,
                             int B, int C, int m, int n, float *gfeat,
                             void *stream);

/* ---- channels-last "row combine": gather the OUTPUT rows of the first MLP layer ----------
 * A 1x1 convolution commutes with a gather, so the first layer of every grouped MLP on the
 * path (EdgeConv: gcn_lib/pointnet/gcn.py:207-210; set abstraction: QueryAndGroup + mlps[0],
 * discriminator.py:141-145; FlowEmbedding: discriminator.py:270-280) is applied to the N
 * un-grouped points and its rows are gathered:
 *   mode 0 GATHER: out[b,s,k,:] = U[b,idx[b,s,k],:]
 *   mode 1 SUB   : out[b,s,k,:] = U[b,idx[b,s,k],:] - QE[b,s,:]
 *   mode 2 EDGE  : out[b,s,k,:] = U[b,idx,:] + lrelu(QE[b,idx,:] - QE[b,s,:], slope)  (S == N)
 * U (B,N,C), QE (B,S,C) of dtype_in; idx (B,S,K) int32; out (B,S,K,C) of dtype_out.  Rows
 * are channels-last; C % 4 == 0 when both types are f32, else C % 8 == 0; 16-B aligned bases.
 * Arithmetic is fp32 in registers with one rounding on store (f32 in -> bf16 out keeps the
 * difference U - QE exact before the single bf16 rounding).
 * An idx entry outside [0, N) reads row N - 1, in the forward, in tpg_invert_index and in the backward alike.
 * The LeakyReLU's derivative at a difference of exactly 0 (every point of a kNN graph is its own neighbour) is
 * `slope` on the neighbour side and on the centre side, so the two cancel; the front end's lrelu'(0) is slope_a. */
typedef enum { TPG_DTYPE_F32 = 0, TPG_DTYPE_BF16 = 1 } tpg_dtype;

int tpg_rowcombine_fwd(const void *U, const void *QE, const int32_t *idx, int mode, int dtype_in,
                       int dtype_out, int B, int N, int S, int K, int C, float slope, void *out,
                       void *stream);

/* per-cloud inverted index of idx (B,SK) with values in [0,N): offs (B,N+1), list (B,SK)
 * = flat (s,k) entry ids grouped by destination row, ASCENDING inside a group (a stable radix sort:
 * the gather-reduce backward then sums in a fixed order -- bitwise reproducible gradients).
 * tmp: B*SK ints of scratch (may be NULL when N <= 256). */
int tpg_invert_index(const int32_t *idx, int B, int N, int SK, int32_t *offs, int32_t *list,
                     int32_t *tmp, void *stream);

/* backward of tpg_rowcombine_fwd; atomics-free gather-reduce over the inverted index.
 * gout (B,S,K,C) of dtype_out; gU (B,N,C) and gQE (grad of QE: (B,S,C) for SUB and EDGE,
 * ignored for GATHER) of dtype_in.  E = the forward's QE (EDGE only, else NULL). */
int tpg_rowcombine_bwd(const void *gout, const int32_t *idx, const int32_t *offs, const int32_t *list,
                       const void *E, int mode, int dtype_in, int dtype_out, int B, int N, int S, int K,
                       int C, float slope, void *gU, void *gQE, void *stream);

/* EdgeConv front end on ONE product (gcn_lib/pointnet/gcn.py:176-180,207-210: node_affine(group(f)) +
 * edge_affine(group(f) - f_i), both 1x1 conv + LeakyReLU on the same grouped input).  With the two convolutions applied
 * BEFORE the gather, their weights stack into one GEMM: Y (B,N,2C) = f [We; Wn]^T -- columns [0,C) = E = We f, columns
 * [C,2C) = the node term before its activation -- and
 *   out[b,n,k,:] = lrelu(Y[b,idx[b,n,k],C:2C], slope_a) + lrelu(Y[b,idx[b,n,k],0:C] - Y[b,n,0:C], slope_e)
 * i.e. tpg_rowcombine_fwd(mode EDGE) reading both operands from one buffer with the node row's activation folded in.
 * Y of dtype_in, idx (B,N,K) int32, out (B,N,K,C) of dtype_out; C as in tpg_rowcombine_fwd and C*sizeof(dtype_in) % 16 == 0.
 * Backward: gY (B,N,2C) of dtype_in = [gE | gA * lrelu'(Y[:,C:2C])], atomics-free over the inverted index of idx
 * (tpg_invert_index), bitwise reproducible. */
int tpg_rowcombine_edge_fwd(const void *Y, const int32_t *idx, int dtype_in, int dtype_out, int B, int N, int K, int C,
                            float slope_a, float slope_e, void *out, void *stream);
int tpg_rowcombine_edge_bwd(const void *gout, const int32_t *idx, const int32_t *offs, const int32_t *list,
                            const void *Y, int dtype_in, int dtype_out, int B, int N, int K, int C, float slope_a,
                            float slope_e, void *gY, void *stream);

/* ---- BatchNorm1d + LeakyReLU + dropout mask of a classification head (discriminator.py:503-516,598-612) ----------
 * h (B,C) fp32 rows of a head's hidden layer, TRAINING mode: batch statistics over the B rows (biased variance, eps),
 *   z = (h - mean) * rstd * gamma + beta;  y = (z > 0 ? z : slope * z) * mask
 * mask (B,C, may be NULL) = the dropout's scaled keep mask (0 or 1 / (1 - p)), drawn by the caller; running statistics
 * (may be NULL) are updated with `momentum` and the unbiased variance, *num_batches_tracked (may be NULL) is incremented;
 * mean / rstd (C) are outputs, kept for the backward.  B == 1 is an argument error, as in nn.BatchNorm1d.
 * Backward: dh (B,C), dgamma / dbeta (C, may be NULL); the activation's sign is recomputed from h. */
int tpg_head_bn_act_fwd(const float *h, int B, int C, const float *gamma, const float *beta, float *running_mean,
                        float *running_var, long long *num_batches_tracked, float momentum, float eps, float slope,
                        const float *mask, float *y, float *mean, float *rstd, void *stream);
int tpg_head_bn_act_bwd(const float *gy, const float *h, const float *mean, const float *rstd, const float *gamma,
                        const float *beta, float slope, const float *mask, int B, int C, float *dh, float *dgamma,
                        float *dbeta, void *stream);

/* ---- fused BatchNorm + LeakyReLU (+ max over K neighbours) on channels-last rows ----------
 * The [conv -> BatchNorm2d -> (Leaky)ReLU]* -> max-over-nsample tail of every shared MLP
 * (discriminator.py:63-78,145-150,279-282) on rows x (P,C), P = B*S*ns:
 *   z = (x - mean) * gamma * rstd + beta;  y = z > 0 ? z : slope*z   (slope 0 = ReLU, 1 = none)
 *   K == 0: y (P,C).   K > 0: y (P/K,C) = max over each group of K consecutive rows, plus the
 *   arg-max row of every (group, channel) as one byte (first maximum).
 * training != 0: mean / rstd are computed from x (biased variance, eps) and written; running
 * statistics (may be NULL) are updated with `momentum` and the unbiased variance, and
 * *num_batches_tracked (may be NULL) is incremented, as nn.BatchNorm's forward does.
 * training == 0: mean / rstd are inputs (the caller derives them from the running statistics);
 * both NULL = identity statistics (mean 0, rstd 1: a pure activation [+ max]).
 * ws: tpg_rowbn_workspace_bytes(C, nseg) bytes of scratch, 16-byte aligned, not shared by launches
 * that may run concurrently.  gamma / beta may be NULL (1 / 0).
 * mean_shift (C, may be NULL): a per-channel constant the caller has LEFT OUT of x -- the bias of
 * the preceding 1x1 conv.  Training-mode BatchNorm(x + b) == BatchNorm(x), so the bias add (a full
 * pass, or a GEMM epilogue the batched GEMM does not have) is skipped; only the running mean sees
 * b: it is updated with mean(x) + mean_shift.  (Eval mode: the caller passes mean - b.)
 * nseg >= 1 SEGMENTS: the P rows are nseg equal consecutive blocks, each an independent call of
 * the same module (the T frames of a clip, the fake and the real batch -- discriminator.py runs
 * them one after the other): statistics per segment (mean / rstd are (nseg, C)), running
 * statistics and num_batches_tracked updated segment after segment in that order, dgamma / dbeta
 * summed over the segments.  K > 0 groups never straddle segments (K | P/nseg).
 * phase: TPG_BN_PHASE_ALL, or the reduction part / the streaming part alone (two calls with the
 * same arguments and workspace = one ALL call; lets a profiler time each kernel by itself). */
#define TPG_BN_PHASE_ALL 0
#define TPG_BN_PHASE_STATS 1
#define TPG_BN_PHASE_APPLY 2
size_t tpg_rowbn_workspace_bytes(int C, int nseg);
int tpg_rowbn_fwd(const void *x, int dtype_in, long long P, int K, int C, float eps, float momentum,
                  int training, float *running_mean, float *running_var, long long *num_batches_tracked,
                  const float *mean_shift, const float *gamma, const float *beta, float slope, float *mean,
                  float *rstd, void *y,
                  int dtype_out, uint8_t *argmax, void *ws, int nseg, int phase, void *stream);
/* gy: (P,C) for K == 0, (P/K,C) for K > 0, of dtype_g; dx (P,C) of dtype_in; dgamma / dbeta (C) f32
 * (may be NULL).  y / dtype_y (K > 0 only, may be NULL): the forward's output; with it the
 * per-channel sums of the max variant are taken from (gy, y) alone -- the pre-activation of the
 * arg-max row is recovered from y -- instead of gathering one element of x per (group, channel);
 * channels where that inversion is ill-conditioned (|beta| > 4|gamma|, or slope == 0 and
 * y == 0 carrying no gradient anyway) use the gather. */
int tpg_rowbn_bwd(const void *gy, int dtype_g, const void *x, int dtype_in, const uint8_t *argmax,
                  const void *y, int dtype_y, long long P, int K, int C, int training, const float *mean,
                  const float *rstd, const float *gamma, const float *beta, float slope, float *dgamma,
                  float *dbeta, void *dx, void *ws, int nseg, int phase, void *stream);

/* the reduction half of tpg_rowbn_bwd alone: c12 (nseg,2,C) = (sum gg / P | sum gg*xhat / P) per segment
 * (gg = gy * lrelu'), dgamma / dbeta as above; dx is not computed. */
int tpg_rowbn_bwd_sums(const void *gy, int dtype_g, const void *x, int dtype_in, const uint8_t *argmax,
                       const void *y, int dtype_y, long long P, int K, int C, int training, const float *mean,
                       const float *rstd, const float *gamma, const float *beta, float slope, float *dgamma,
                       float *dbeta, float *c12, void *ws, int nseg, void *stream);

/* The statistics / sums launches above with the folded per-channel constants of the fused tail (tpg_mlp_consts)
 * written by the SAME finalize launch -- a tail's first and last BatchNorm need no tpg_mlp_consts launch of their own:
 *   tpg_rowbn_stats_consts   : phase STATS of tpg_rowbn_fwd (training mode) + ci (nseg,4,C) = sc | sh | mu | rs
 *   tpg_rowbn_bwd_sums_consts: tpg_rowbn_bwd_sums + cb (nseg,4,C) = a | f*mu | e | f, and (ag non-NULL; K > 0, y given
 *                              in gy's type, else TPG_ERR_UNSUPPORTED) ag (P/K, C) = tpg_mlp_max_prep's output, written
 *                              by the reduction from the rows it reads anyway */
int tpg_rowbn_stats_consts(const void *x, int dtype_in, long long P, int C, float eps, float momentum,
                           float *running_mean, float *running_var, long long *num_batches_tracked,
                           const float *mean_shift, const float *gamma, const float *beta, float *mean, float *rstd,
                           float *ci, void *ws, int nseg, void *stream);
int tpg_rowbn_bwd_sums_consts(const void *gy, int dtype_g, const void *x, int dtype_in, const uint8_t *argmax,
                              const void *y, int dtype_y, long long P, int K, int C, int training, const float *mean,
                              const float *rstd, const float *gamma, const float *beta, float slope, float *dgamma,
                              float *dbeta, float *c12, float *cb, void *ag, void *ws, int nseg, void *stream);

/* ---- fused shared-MLP tail layer on MFMA tiles (csrc/mlp_fused.hip) --------------------------
 * The grouped-feature x MLP-weight contraction of set abstraction / flow embedding
 * (discriminator.py:63-78,140-148,276-282: conv1x1 -> BatchNorm2d -> LeakyReLU per layer) for one
 * layer of the tail, on channels-last bf16 rows:
 *     y = W . lrelu(scale * x + shift)        x (P,Cin) bf16, W (Cout,Cin) f32, y (P,Cout) bf16
 * scale | shift = the INPUT BatchNorm folded per channel (2*Cin floats at ss_in + seg*ss_stride -- the head of
 * a ci block, below -- NULL = identity), applied
 * together with the LeakyReLU in the MFMA A-operand prologue; bf16 MFMA (v_mfma_f32_16x16x32_bf16),
 * fp32 accumulation, one rounding of y; the epilogue accumulates the batch statistics of y (of the
 * ROUNDED values) and a finalize launch writes mean_out / rstd_out (nseg,Cout), updates
 * running_mean / running_var / num_batches_tracked like nn.BatchNorm (all three may be NULL;
 * mean_shift as in tpg_rowbn_fwd) and, if ci_out != NULL, the folded constants of the OUTPUT
 * BatchNorm, ci (nseg,4,Cout) = sc | sh | mu | rs (gamma_out, beta_out; NULL = 1 / 0): its head is the next
 * layer's ss_in (ss_stride = 4*Cout), the backward kernels read all four.  mean_out = rstd_out = ci_out =
 * running_mean = NULL: no statistics wanted (a tail without BatchNorm), no finalize launch.
 * nseg segments = nseg calls of the layer on equal consecutive row blocks, each with its own
 * statistics and (w_per_seg != 0) its own weight W[seg] (successive spectral-norm iterates).
 * Supported (Cin,Cout): (64,64) (64,128) (128,64) (128,128) (128,256) (256,128) (256,256);
 * ws: tpg_mlp_workspace_bytes(max(Cin,Cout), nseg) bytes, 16-byte aligned; after the call it holds the
 * per-workgroup partials (nseg, G, 3, Cout) f32 = mean | M2 | n with G = tpg_mlp_fwd_blocks(P, Cin, Cout, nseg)
 * workgroups per segment (host only, no launch; 0 for bad arguments or an unsupported shape). */
size_t tpg_mlp_workspace_bytes(int C, int nseg);
int tpg_mlp_fwd_blocks(long long P, int Cin, int Cout, int nseg);
int tpg_mlp_fwd(const void *x, long long P, int Cin, int Cout, int nseg, const float *ss_in, int ss_stride,
                float slope_in, const float *W, int w_per_seg, void *y, float eps, float momentum,
                float *running_mean, float *running_var, long long *num_batches_tracked, const float *mean_shift,
                const float *gamma_out, const float *beta_out, float *mean_out, float *rstd_out, float *ci_out,
                void *ws, void *stream);

/* Backward of such a layer, x_in (P,Cin) -> x_out (P,Cout) = W . lrelu(BN_in(x_in)), followed by
 * BN_out (+ LeakyReLU; + max over groups of K rows on a tail's last layer).  With BN_out's backward
 * sums known (c12), the gradient of x_out is elementwise in saved tensors,
 *     dx_out = a*gg - f*(x_out - mu) + e      (a, f*mu, e, f per channel: tpg_mlp_consts, cb (nseg,4,Cout))
 * and is never stored: it is rebuilt in the MFMA operand prologue of both gradient kernels.
 *   mode 0 DENSE: gg = g_out (P,Cout) bf16, the activated gradient written by the next layer's dgrad
 *   mode 1 MAX  : g_out (P/K,Cout) bf16 = a * lrelu'(y) * (gradient of the max output), one value per
 *                 (group, channel), made by tpg_mlp_max_prep from that gradient and the forward's output y;
 *                 arg = the arg-max bytes: the value belongs to row arg of its group, the others get 0
 * The MFMA operand the kernels build is the centred d = dx_out - e (one fma per element); e enters as a rank-one
 * term (e^T W per input channel in tpg_mlp_dgrad's epilogue, e (x) sum_rows a_in in tpg_mlp_wgrad).
 * tpg_mlp_dgrad: g_in (P,Cin) bf16 = (dx_out . W) * lrelu'(z_in) and BN_in's backward sums:
 *   c12_in (nseg,2,Cin), dgamma_in / dbeta_in (Cin, summed over segments) and cb_in (nseg,4,Cin) = the cb of
 *   BN_in for the NEXT tpg_mlp_dgrad / tpg_mlp_wgrad one layer down -- each may be NULL, all NULL = BN_in is
 *   the identity (no finalize launch).
 *   ci_in (nseg,4,Cin) = sc | sh | mu | rs of BN_in (tpg_mlp_consts).  ws: tpg_mlp_workspace_bytes.
 * tpg_mlp_wgrad: dW (nseg,Cout,Cin) f32 = dx_out^T . lrelu(BN_in(x_in)), both operands rebuilt from the
 *   saved rows, staged in LDS and read transposed (ds_read_b64_tr_b16); per-workgroup fp32 slabs summed
 *   in fixed order (bitwise reproducible).  ws: tpg_mlp_wgrad_workspace_bytes(P, Cin, Cout, nseg).
 * tpg_mlp_bn_bwd_apply: dx = a*(g - c1 - xhat*c2) for the tail's first BatchNorm (g already activated).
 * tpg_mlp_bn_bwd_apply_rowsum: the same, plus qneg (nseg * P/K, C) f32 = -sum over each group of K consecutive rows of
 *   the stored (bf16-rounded) dx, k ascending: what tpg_rowcombine_bwd(mode SUB) computes as gQE from those rows --
 *   pass it there as gQE_ready and the rows are not read a second time. */
int tpg_mlp_consts(const float *mean, const float *rstd, const float *gamma, const float *beta, const float *c12,
                   int C, int nseg, float *ci, float *cb, void *stream);
int tpg_mlp_max_prep(const void *gout, const void *y, const float *cb_out, float slope_out, long long rows, int C,
                     int nseg, void *ag, void *stream);
int tpg_mlp_dgrad(const void *x_out, const void *g_out, const uint8_t *arg, int K, const float *cb_out,
                  const void *x_in, const float *ci_in, float slope_in, const float *W,
                  int w_per_seg, long long P, int Cin, int Cout, int nseg, int mode, void *g_in, float *c12_in,
                  float *dgamma_in, float *dbeta_in, float *cb_in, void *ws, void *stream);
size_t tpg_mlp_wgrad_workspace_bytes(long long P, int Cin, int Cout, int nseg);
int tpg_mlp_wgrad(const void *x_out, const void *g_out, const uint8_t *arg, int K, const float *cb_out,
                  const void *x_in, const float *ci_in, float slope_in, long long P, int Cin,
                  int Cout, int nseg, int mode, float *dW, void *ws, void *stream);
int tpg_mlp_bn_bwd_apply(const void *g, const void *x, const float *ci, const float *c12, long long P, int C,
                         int nseg, void *dx, void *stream);
int tpg_mlp_bn_bwd_apply_rowsum(const void *g, const void *x, const float *ci, const float *c12, long long P, int K,
                                int C, int nseg, void *dx, float *qneg, void *stream);

/* ---- forward-only shared-MLP tail with eval-mode BatchNorm, one launch (csrc/mlp_infer.hip) ----
 * Eval-mode BatchNorm is a constant per-channel affine, so the whole tail behind the row gather runs per group:
 *   out[b,s,:] = max_{j<K} act_L(a_L * (W_L ... act_1(a_1 * (W_1 act_0(U[b,idx[b,s,j],:] - Q[b,s,:])) + c_1) ...) + c_L)
 *   act_l(z) = max(z, slope_l * z), 0 <= slope_l <= 1;  L = 1 (C2 == 0) or 2 weights.
 * U (B,N,C0), Q (B,S,C0) of dtype_in (fp32 or bf16) with the input affine already folded in: the difference is taken in
 * fp32 on their own values, so fp32 tables are not rounded before it; idx (B,S,K) int32 (clamped into [0,N));
 * a_l, c_l (C_l) f32; out (B,S,C_L) bf16.  bf16 MFMA operands, fp32 accumulation, affine and activation in fp32 on the
 * accumulators, one rounding where a value becomes the next MFMA operand and one at the store; the max is taken in
 * registers and by cross-lane moves (no atomics: bitwise reproducible, independent of B and of the grid).
 * W1p / W2p: the weights (C1,C0) / (C2,C1) as bf16 in B-fragment order, T = Cout/16, KS = Cin/32:
 *   Wp[((t*KS + s)*64 + lq*16 + li)*8 + e] = W[li*T + t][32*s + 8*lq + e]      t < T, s < KS, li < 16, lq < 4, e < 8
 * (16-byte aligned).  Chains (C0,C1,C2): (64,128,0) (128,256,0) (64,64,128) (256,128,256) (256,256,256); K a
 * multiple of 16, <= 256 -- tpg_mlp_infer_supported says 1 for these, tpg_mlp_infer_fwd TPG_ERR_UNSUPPORTED otherwise. */
int tpg_mlp_infer_supported(int C0, int C1, int C2, int K);
int tpg_mlp_infer_fwd(const void *U, const void *Q, const int32_t *idx, int dtype_in, int B, int N, int S, int K, int C0,
                      int C1, int C2, const void *W1p, const void *W2p, const float *a1, const float *c1, const float *a2,
                      const float *c2, float slope0, float slope1, float slope2, void *out, void *stream);

/* ---- fused spectral normalisation of a (R x Cn) conv / linear weight ------------------------
 * torch.nn.utils.spectral_norm's forward pre-hook (n_power_iterations = 1) on every conv and
 * linear of the discriminators (discriminator.py:66-68,246-247,351-359,...) in ONE launch:
 *   iterate != 0 (training):  v <- normalize(W^T u); u <- normalize(W v)   (u, v updated in place)
 *   sigma = u . (W v);  Wsn = W / sigma.      normalize(x) = x / max(|x|_2, eps)
 * backward, u and v constants:  dW = (G - <G, Wsn> u v^T) / sigma. */
int tpg_spectral_norm_fwd(const float *W, float *u, float *v, int R, int Cn, int iterate, float eps,
                          float *Wsn, float *sigma, void *stream);
int tpg_spectral_norm_bwd(const float *G, const float *Wsn, const float *u, const float *v,
                          const float *sigma, int R, int Cn, float *dW, void *stream);

/* Batched form: every spectrally-normalised weight of one discriminator forward in ONE launch.
 * desc: device array of M records {const float* W; float* u; float* v; int64 R, Cn, uses,
 * out_off} (7 x 8 bytes).  Weight m is used `uses` times in the forward (once per frame / per
 * flow-embedding pair); each use advances (u, v) by one power iteration (iterate != 0) and gets
 * its own W / sigma.  For use t the kernel writes at out + out_off + t * stride(R, Cn) floats:
 *   W/sigma_t (R*Cn) | u_t (R) | v_t (Cn) | sigma_t (1),  stride = tpg_spectral_norm_multi_stride.
 * max_rc = max over m of (R + Cn).  u, v are left at their final values.
 * Backward: desc of M records {int64 R, Cn, uses, out_off, g_off, dw_off} (6 x 8 bytes); the
 * gradient of use t of weight m is at g + g_off + t*R*Cn, and
 * dw + dw_off <- sum_t (G_t - <G_t, Wsn_t> u_t v_t^T) / sigma_t.  Both descriptor arrays hold
 * only sizes, offsets and the persistent parameter pointers, so they can be built once. */
long long tpg_spectral_norm_multi_stride(int R, int Cn);
int tpg_spectral_norm_multi_fwd(const void *desc, int M, int max_rc, float *out, int iterate, float eps,
                                void *stream);
/* The same forward in TRAINING mode with every weight's rows split over ceil(R / tpg_spectral_norm_split_rows())
 * workgroups that keep their rows in registers for all uses and exchange partial column sums once per use (round 3:
 * the one-workgroup form is the longest launch at the head of the temporal discriminator's update).  Same output layout.
 * desc: per weight 9 x int64 {W, u, v, R, Cn, uses, out_off, parts, x_off}; x_off = offset, in 8-byte words, of the
 * weight's 2 * parts * (Cn + 1) exchange words inside xws.  part_map: total_parts x int32[2] = (weight, part).
 * xws: xws_words 8-byte words, 16-byte aligned (the exchange words of all weights + one trailing word that is non-zero
 * after the launch if a bounded spin gave up); zeroed by the call itself.  Cn <= tpg_spectral_norm_split_max_cn(). */
int tpg_spectral_norm_multi_fwd_split(const void *desc, const void *part_map, int total_parts, int max_cn, float *out,
                                      void *xws, long long xws_words, float eps, void *stream);
int tpg_spectral_norm_split_rows(void);
int tpg_spectral_norm_split_max_cn(void);
int tpg_spectral_norm_split_max_rows(void);      /* R <= this (at most 16 workgroups per weight) */
/* backward: max_uses = max over m of uses (<= 64); scratch: tpg_spectral_norm_multi_bwd_scratch(M, max_uses)
 * floats (the partial inner products <G_t, Wsn_t> of the row chunks, summed in fixed order). */
long long tpg_spectral_norm_multi_bwd_scratch(int M, int max_uses);
int tpg_spectral_norm_multi_bwd(const void *desc, int M, int max_uses, const float *g, const float *out,
                                float *dw, float *scratch, void *stream);

/* ---- fused radius search + bicubic weighted average (the `--use_vel` advection features) ----
 * gcn_lib/interpolation.py:107-123 `cubic_interpolation(query_pos, field, pos, cutoff)` over
 * get_local_neighbor_graph (:16-75; FRNN K=32, unique, FRNN, kNN-4 padding, DGL scatter-sums),
 * called per frame and per sample by train_step_final.py:51-66.  query (B,Nq,3), pos (B,Np,3),
 * field (B,Np,F).  Per query: the <= 32 nearest field points with d^2 < cutoff^2 (ascending
 * (d^2, idx)), w = bicubic(d / cutoff) * 8 / (pi cutoff^3);
 *   out_plain = sum w f / (sum w + 1e-6)
 *   out_pad   = the same with the 4 nearest hits counted twice (the reference's padding edges)
 *   hits      = number of in-range neighbours found (<= 32)
 * The caller picks out_pad for the queries with hits < 32 of every cloud in which SOME query has
 * hits == 0 (that is when the reference adds its padding edges), out_plain otherwise. */
int tpg_cubic_interp_f32(const float *query, const float *pos, const float *field, int B, int Nq, int Np,
                         int F, float cutoff, float *out_plain, float *out_pad, int32_t *hits,
                         void *stream);

/* The EdgeConv MLP tail at the generator's small channel counts (gcn_lib/pointnet/gcn.py:207-211 inside
 * IDGCNLayer, gcn.py:229-231): out[n] = max_j lrelu_s2(W2 . lrelu_s1(W1 . h[n*K + j])), h (P*K, H) rows of edge
 * features, W1 (C1, H), W2 (C2, C1) fp32, no bias; (H, C1, C2) = (16, 16, 32) only (TPG_ERR_UNSUPPORTED
 * otherwise), 1 <= K <= 255, 0 <= slopes <= 1.  h / out / gout / gh are bf16 (is_bf16 = 1) or fp32; arithmetic
 * is fp32 on the vector ALUs (weights as scalar operands).  Forward: out (P, C2) and the arg-max byte of each
 * (point, channel) (first maximum).  Backward (recomputes the hidden layer from h): gh (P*K, H), dW1, dW2
 * (fp32, per-wave slabs in `ws` summed in a fixed order). */
size_t tpg_small_tail_workspace_bytes(long long P, int K);
int tpg_small_tail_fwd(const void *h, int is_bf16, const float *W1, const float *W2, float slope1, float slope2,
                       long long P, int K, int H, int C1, int C2, void *out, unsigned char *arg, void *stream);
int tpg_small_tail_bwd(const void *h, const void *out, const void *gout, const unsigned char *arg, int is_bf16,
                       const float *W1, const float *W2, float slope1, float slope2, long long P, int K, int H,
                       int C1, int C2, void *gh, float *dW1, float *dW2, void *ws, void *stream);

/* ---- row-wise linear layers of any small channel count (csrc/rowlinear.hip, round 3) -------------------------
 * The 1x1 convolutions that are NOT inside a fused tail: the generator's node / edge affines, bottlenecks,
 * decoders and skip layers (gcn_lib/pointnet/gcn.py:176-180,207-211,253-277; upsampling_network.py:44-104), the
 * first layer of every shared MLP of the discriminators applied to the un-grouped points
 * (discriminator.py:63-78,140-148,276-282: Cin = 3, 6, 131, 259, 515) and the heads' linears
 * (discriminator.py:503-516,598-612) -- in the reference: cuDNN / cuBLAS calls plus separate bias / activation kernels.
 *     y[p, o] = lrelu_slope( sum_c x[p, c] * W[seg(p)][o, c] + bias[o] )
 * x (P, Cin) and y (P, Cout) channels-last rows, f32 or bf16 (tpg_dtype); W (nseg, Cout, Cin) f32: nseg equal
 * consecutive row blocks with their own weights (P % nseg == 0, and (P / nseg) % 128 == 0 when nseg > 1;
 * Cin, Cout <= 1000: tpg_rowlinear_supported);
 * bias (Cout) f32 or NULL; slope in [0, 1], 1 = no activation.  fp32 products and accumulation on
 * v_mfma_f32_16x16x4_f32.  x, y, W 16-byte aligned.
 * Backward (y = the forward's output, needed when slope != 1: the activation's derivative is taken from its sign):
 *   tpg_rowlinear_dgrad: dx (P, Cin) = (gy * lrelu'(y)) . W
 *   tpg_rowlinear_wgrad: dW (nseg, Cout, Cin) f32 = (gy * lrelu'(y))^T . x per segment; db (Cout) f32 or NULL = its
 *                        column sums over all segments; row slabs summed in slab order (bitwise reproducible);
 *                        ws: tpg_rowlinear_wgrad_workspace_bytes(P, nseg, Cin, Cout, db != NULL) bytes. */
int tpg_rowlinear_supported(int Cin, int Cout, int has_bias);
size_t tpg_rowlinear_wgrad_workspace_bytes(long long P, int nseg, int Cin, int Cout, int has_bias);
int tpg_rowlinear_fwd(const void *x, int dtype_in, const float *W, const float *bias, long long P, int nseg, int Cin,
                      int Cout, float slope, void *y, int dtype_out, void *stream);
int tpg_rowlinear_dgrad(const void *gy, const void *y, int dtype_g, const float *W, long long P, int nseg, int Cin,
                        int Cout, float slope, void *dx, int dtype_x, void *stream);
int tpg_rowlinear_wgrad(const void *x, int dtype_x, const void *gy, const void *y, int dtype_g, long long P, int nseg,
                        int Cin, int Cout, float slope, float *dW, float *db, void *ws, void *stream);

/* ---- rollout: hard-masked expansion with the 25-frame running mask average (csrc/rollout.hip) ----------------
 * upsampling_network.py:159-174 (`forward_with_context`, the demo notebooks' sequence upsampling) for a chunk of T
 * consecutive frames t0 .. t0+T-1 of ONE sequence of N points per frame, upsampling ratio r (2 <= r <= 16):
 *     c_f = clamp of the raw mask to {0, 0.6} (NaN kept);  avg_t = mean of c_f over f in [max(0, t-24), t]
 *     keep_t(i) = avg_t(i) > 0.01  <=>  some f of the window has m_f(i) >= 0.6 and none has m_f(i) NaN
 *     out_t = [pos_t(i) + edge_t(i, j) * (keep_t(i) ? 1.0f : 0.0f)  for i, for j < r  if keep_t(i) or j == 0]
 * pos (T,N,3), edge (T,N*r,3), mask (T,N) f32.  state (2,N) int32, read and updated: [0] = last frame with a hit,
 * [1] = last frame with a NaN, TPG_CTX_NONE = none (a fresh sequence is all TPG_CTX_NONE); carrying it from one call
 * to the next (t0 advancing by T) gives what one call over all frames gives.  out: room for T*N*r points, packed frame
 * after frame, point-major, slot-minor; offsets (T+1) int64: frame t is out[offsets[t] .. offsets[t+1]).
 * Deterministic, bit-identical to the formula (no FMA).  ws: tpg_context_expand_workspace_bytes(T, N) bytes, 8-byte
 * aligned.  T <= 65535. */
#define TPG_CTX_NONE (-2147483647 - 1)
size_t tpg_context_expand_workspace_bytes(int T, int N);
int tpg_context_expand_f32(const float *pos, const float *edge, const float *mask, int T, int N, int r, int t0,
                           int32_t *state, float *out, int64_t *offsets, void *ws, void *stream);

/* ---- uncapped neighbourhood sums: particle density, neighbour counts (csrc/radius_reduce.hip) ----------------
 * train_fluid/analysis_helper.py:143-161,291-294 (get_particle_density, get_particle_density_of_two_pcd,
 * particle_dns2grid_dns) and train_utils.py:269-286 (fixed_radius_neighbor_num, get_free_surface_particles), which
 * the reference computes on the host with a scipy KD-tree.  query (B,Nq,3), pos (B,Np,3); lenq / lenp (B) int64 or
 * NULL (= full), as in tpg_frnn_grid_f32.  Per query i, over EVERY stored point j of its cloud (no cap on their number)
 * with d2 <= r2 -- INCLUSIVE, unlike the strict d2 < r2 of the K-nearest searches above, because scipy's
 * query_ball_point / query_ball_tree are -- where d2 is the canonical fp32 distance (t = q - p per axis;
 * d2 = t0*t0; d2 = d2 + t1*t1; d2 = d2 + t2*t2; no FMA) and r2 = fp32(r) * fp32(r):
 *     count (B,Nq) int32 = the number of such points
 *     sum   (B,Nq) f32   = the sum over them of w(sqrt(d2), r)
 *     kernel 0: the cubic kernel of analysis_helper.py:102-113 with coefficient 1
 *               (q = d / r;  q <= 0.5: 6 (q^3 - q^2) + 1;  q <= 1: 2 (1 - q)^3)
 *     kernel 1: train_utils.linear_kernel (r / d - 1, and 0 for d < 1e-8)
 * Either output may be NULL (counts only / sums only), not both.  Queries at or beyond lenq[b] get 0 / 0; Np = 0 or
 * lenp[b] = 0 gives 0 / 0; a query far outside the stored cloud gets 0 / 0.  TPG_ERR_UNSUPPORTED for another kernel
 * number and for B > 65535.
 * Deterministic: the sum is accumulated in 64-bit fixed point (cubic: units of 2^-32, each term truncated; linear:
 * units of 2^-23, in which every fp32 term is exact; saturating at 2^64 units), so it does not depend on the order in
 * which the neighbours are met: the same bits on every run, at every batch position and from both entries below.
 *   tpg_radius_reduce_f32             on the uniform grid of tpg_frnn_grid_f32 (four build launches + one wave per
 *                                     query over its 27 cells); ws: tpg_frnn_grid_workspace_bytes(B, Np) bytes,
 *                                     256-byte aligned
 *   tpg_radius_reduce_exhaustive_f32  the same kernel body over the whole stored cloud, for small clouds */
int tpg_radius_reduce_f32(const float *query, const float *pos, const int64_t *lenq, const int64_t *lenp, int B,
                          int Nq, int Np, float r, int kernel, int32_t *count, float *sum, void *ws, void *stream);
int tpg_radius_reduce_exhaustive_f32(const float *query, const float *pos, const int64_t *lenq, const int64_t *lenp,
                                     int B, int Nq, int Np, float r, int kernel, int32_t *count, float *sum,
                                     void *stream);

/* ---- earth mover's distance: auction matching of equal-size clouds (csrc/emd.hip) ------------------------------
 * Replaces the `emd` auction extension behind emdModule -- train_fluid/analysis_helper.py:14-64,224,255;
 * train_action/analysis_helper.py:11-49,67; loss.py:311.  xyz1 (B,n,3) are the persons, xyz2 (B,n,3) the objects;
 * every person gets one object and every object one person.  The rule, which the kernels follow bit for bit:
 *   cost    c_ij = the canonical fp32 squared distance;  value v_ij = (-c_ij) - p_j in fp32;  prices p start at 0
 *   phases  k = phases, phases-1, .., 0 with eps_k = eps * scaling^k, rounded to fp32 at each multiplication; a phase
 *           starts with every person unassigned and every owner cleared, keeps the prices, and ends when no person
 *           is unassigned
 *   round   every unassigned person i finds the best value v1 at j1 (ties: lowest j) and the best value v2 over
 *           j != j1, and bids p' = p_j1 + ((v1 - v2) + eps_k) in fp32, or nextafter(p_j1, +inf) where p' <= p_j1;
 *           every object with bids takes the highest p' (ties: lowest i): its previous owner becomes unassigned and
 *           its price p'.  All bids of a round see the prices of the round's start.
 *   rounds  counted per cloud over all phases; a cloud with persons unassigned when the count reaches `iters` is
 *           CAPPED and takes no further rounds.  n = 1 is assigned directly, in 0 rounds.
 * A cloud's results depend on that cloud alone: not on the batch, not on wide_rounds / narrow_rounds / narrow_at.
 * The caller drives three steps over one workspace of tpg_emd_workspace_bytes(B, n) bytes, 256-byte aligned:
 *   tpg_emd_init_f32    objects and prices into the workspace, assignment = -1 (m must equal n: TPG_ERR_ARG)
 *   tpg_emd_rounds_f32  `wide_rounds` rounds of two launches each (a wave per unassigned person bids; a workgroup
 *                       per cloud assigns) for clouds with more than `narrow_at` persons unassigned, then ONE launch
 *                       that runs up to `narrow_rounds` rounds, a workgroup per cloud between workgroup barriers,
 *                       for clouds with at most `narrow_at`.  Launches for a cloud that is done, capped or on the
 *                       other path do nothing.  The call must be able to advance every cloud: narrow_rounds >= 1
 *                       when narrow_at > 0, wide_rounds >= 1 (and <= 4096) when narrow_at < n.  eps > 0,
 *                       scaling >= 1, 0 <= phases <= 64, iters >= 1.
 *                       Afterwards the workspace starts with B records of 8 int32:
 *                       {phase, rounds, unassigned persons, status (0 active, 1 done, 2 capped), 4 unused};
 *                       the caller reads them and calls again while a cloud is active.
 *   tpg_emd_finish_f32  dist (B,n) = c of every person to its object, price (B,n), rounds (B).
 * TPG_ERR_UNSUPPORTED for B > 65535. */
size_t tpg_emd_workspace_bytes(int B, int n);
int tpg_emd_init_f32(const float *xyz2, int B, int n, int m, int phases, int32_t *assignment, void *ws, void *stream);
int tpg_emd_rounds_f32(const float *xyz1, int B, int n, float eps, float scaling, int phases, int iters,
                       int wide_rounds, int narrow_rounds, int narrow_at, int32_t *assignment, void *ws,
                       void *stream);
int tpg_emd_finish_f32(const float *xyz1, int B, int n, const int32_t *assignment, void *ws, float *dist, float *price,
                       int32_t *rounds, void *stream);

/* ---- Gaussian row sums, the building block of the Gaussian MMD (csrc/gauss_sum.hip) -----------------------------
 * geomloss.SamplesLoss('gaussian', blur) of train_fluid/analysis_helper.py:226-227,256-260.  a (B,N,3), b (B,M,3);
 * lena / lenb (B) int64 or NULL (= full).  out (B,N) FLOAT64: out[i] = sum over the points j of b of
 * expf(-(c_ij * s)), c the canonical fp32 squared distance, s = fp32(1 / (2 sigma^2)) with the division in double.
 * Rows at or beyond lena[b] get 0.  Every term is truncated to a multiple of 2^-32 and the terms are added as 64-bit
 * integers: the same bits whatever the order, the batch and the run, and an exact float64.  sigma <= 0: TPG_ERR_ARG;
 * M >= 2^17 or B > 65535: TPG_ERR_UNSUPPORTED. */
int tpg_gaussian_row_sums_f32(const float *a, const float *b, const int64_t *lena, const int64_t *lenb, int B, int N,
                              int M, float sigma, double *out, void *stream);

/* ---- training clips from device-resident sequences (csrc/clip_sample.hip) -------------------------------------
 * train_fluid/tempo_dataset.py:58-105 (SiamData.__getitem__) with train_utils.py:98-139 (sample_patch_with_fps) and
 * :214-221 (normalize_point_cloud), which the reference runs per clip on host workers (np.load, a scipy KD-tree, a
 * numba FPS, a pinned upload of 13 arrays).  Here every frame stays on the device and a batch is four calls:
 * tpg_patch_select_f32, tpg_clip_gather_high_f32, tpg_fps_start_f32 on the centre frame's patch,
 * tpg_clip_gather_low_f32.
 * EXCEPTION to the pointer convention above: the arrays marked HOST below are small per-clip tables in HOST memory (the
 * sampler draws them on the host); they are checked before anything is launched and travel as kernel arguments, so a
 * bad clip is an error status with nothing written, and a batch costs no host-to-device copy.
 *
 * tpg_patch_select_f32: the K nearest stored points of ONE seed point per scene (KDTree(pos).query(pos[seed], K),
 * train_utils.py:118-123), for B scenes of different sizes.  points (P,3) f32; scene b is points[first[b] ..
 * first[b]+count[b]) and its seed point is row seed[b] of that slice (first, count, seed: HOST, B ints each).
 * idx (B,K) int32, scene-local.  Rule: d2 = (dx*dx + dy*dy) + dz*dz in fp32, each operation rounded (no FMA); the
 * result is the K candidates smallest in (d2, index), in ascending lexicographic (d2, index) order -- idx[b][0] is the
 * seed or a lower-indexed exact duplicate of it.  A non-finite d2 ranks by its bit pattern (+inf after every finite
 * value), a NaN d2 as the single pattern 0x7FC00000: after +inf, all NaNs tied, by index.  Bit-exact, identical from
 * run to run and at every batch position (integer atomics and a final sort of unique keys only).
 * K <= 0, K > count[b], seed[b] outside [0, count[b]), a slice outside [0, P): TPG_ERR_ARG;
 * K > tpg_patch_select_max_k() (the K keys of a scene are ordered in LDS): TPG_ERR_UNSUPPORTED.
 * ws: tpg_patch_select_workspace_bytes(B, max_b count[b], K) bytes, 8-byte aligned; zeroed by the call itself. */
#define TPG_PATCH_SELECT_MAX_K 16384
int tpg_patch_select_max_k(void);
size_t tpg_patch_select_workspace_bytes(int B, int max_count, int K);
int tpg_patch_select_f32(const float *points, long long P, const int32_t *first, const int32_t *count,
                         const int32_t *seed, int B, int K, int32_t *idx, void *ws, void *stream);

/* All high-resolution arrays of a batch of B clips of T <= 8 frames (tempo_dataset.py:69-87):
 *     high_pos[t,b,k,:] = pos[frame_first[t,b] + patch[b,k], :] - centroids[centroid_row[b], :]     (one fp32 subtraction)
 *     high_vel[t,b,k,:] = vel[frame_first[t,b] + patch[b,k], :]                                     (vel, high_vel: both or neither)
 * pos / vel (P,3) f32: every frame back to back; frame_first (T,B) HOST: first point of clip b's frame t; count (B)
 * HOST: particles of clip b's scene (patch entries are clamped into [0, count[b])); centroids (F,3) f32: one row per
 * stored frame, centroid_row (B) HOST: the row of clip b's CENTRE frame (normalize_point_cloud of the centre frame, applied
 * to all T frames; its scale is the constant 1).  patch (B,K) int32 from tpg_patch_select_f32.  Outputs are frame-major
 * (T,B,K,3): frame t is the contiguous (B,K,3) cloud batch the networks and tpg_fps_start_f32 take. */
int tpg_clip_gather_high_f32(const float *pos, const float *vel, long long P, const int32_t *frame_first,
                             const int32_t *count, const float *centroids, int F, const int32_t *centroid_row,
                             const int32_t *patch, int T, int B, int K, float *high_pos, float *high_vel, void *stream);

/* All low-resolution arrays of the batch (tempo_dataset.py:89-100), fps (B,M) int32 = the centre patch's sampling:
 *     low_pos[t,b,j,:] = high_pos[t,b,fps[b,j],:] + noise[t,b,j,:] * jitter     (multiply, then add: two roundings)
 *     low_vel[t,b,j,:] = vel[frame_first[t,b] + fps[b,j], :]                    (vel, low_vel: both or neither)
 * noise (T,B,M,3) f32 drawn by the caller, or NULL: low_pos is then the plain gather.  The velocities are the
 * reference's, quirk included: tempo_dataset.py:98-100 indexes the WHOLE scene's velocities with the patch-local
 * sampling (`vel_center[fps_idx]`, not `highres_vel[fps_idx]`), so low_vel are the velocities of scene particles
 * fps[b,j], not of the low-resolution points; pos-only training (--in_node_feats 3) never reads them.  vel (P,3),
 * frame_first (T,B) HOST, count (B) HOST as in tpg_clip_gather_high_f32 (unused when vel is NULL).  fps entries are
 * clamped into [0, K) for the positions and into [0, count[b]) for the velocities. */
int tpg_clip_gather_low_f32(const float *high_pos, const int32_t *fps, const float *noise, float jitter,
                            const float *vel, long long P, const int32_t *frame_first, const int32_t *count, int T,
                            int B, int K, int M, float *low_pos, float *low_vel, void *stream);

/* ---- action clips from device-resident depth videos (csrc/action_sample.hip) ----------------------------------
 * train_action/msr_dataset.py:60-135 (MSRAction3D.__getitem__), which the reference runs per clip on host workers (per
 * frame an np.random.choice, a numpy gather and a numba FPS from 2048 down to 128 points).  The frames of a depth video
 * are RAGGED: every frame has its own point count.  Here every frame stays on the device and a batch is four calls:
 * tpg_frame_subset, tpg_action_gather_f32, ONE tpg_fps_start_f32 over all T*B clouds, tpg_clip_gather_low_f32 with the
 * batch viewed as (1, T*B, K, 3).  The arrays marked HOST follow the exception stated for the clip sampler above.
 *
 * tpg_frame_subset: a uniformly random ordered subset of K points of each of F frames (np.random.choice(n, K,
 * replace=False), msr_dataset.py:69-74).  count (F) HOST: points per frame; seed (F) HOST: one 64-bit seed per frame,
 * seed_lo / seed_hi its low / high 32 bits.  idx (F,K) int32, frame-local.  Key of point j, uint32 arithmetic, wrapping:
 *     mix(h):  h ^= h>>16; h *= 0x7FEB352D; h ^= h>>15; h *= 0x846CA68B; h ^= h>>16
 *     key(j) = mix( mix(j * 0x9E3779B1 + seed_lo) ^ seed_hi )
 * (a bijection of uint32: the keys of a frame are distinct).  Candidates are ordered by ascending (key, j).
 *     n >  K: the K smallest, in that order;
 *     n <= K: 0..n-1 repeated K / n times, then the K % n smallest in that order (n = K: the identity).
 * A pure function of (count, seed, K): bit-identical from run to run and at every batch position (integer atomics on LDS
 * histograms and a final sort of unique keys only).  One workgroup per frame selects and orders in LDS, so there is
 * no workspace; the frame's keys are recomputed in each of its four passes, which suits depth frames (10^3..10^5 points).
 * count[f] < 1 or K < 1: TPG_ERR_ARG, nothing written; K > TPG_PATCH_SELECT_MAX_K: TPG_ERR_UNSUPPORTED. */
int tpg_frame_subset(const int32_t *count, const uint64_t *seed, int F, int K, int32_t *idx, void *stream);

/* All high-resolution clouds of a batch of B clips of T <= 8 frames (msr_dataset.py:67-91 train, :105-127 test).
 * points (P,3) f32: every stored frame back to back; frame_first (T,B) HOST, count (T,B) HOST: clip b's frame t is
 * points[frame_first[t,b] .. + count[t,b]); idx (T,B,K) int32 from tpg_frame_subset (entries are clamped into the
 * frame); scale (B,3) f64 HOST or NULL (= ones).  With q = (double)p, y negated, and v = (q * scale[b]) / 300.0 in
 * fp64, in this operation order:
 *     TPG_ACTION_TRAIN  c[b] = fp64 mean of v over the K rows of frame T/2;  high[t,b,k,:] = (float)(v - c[b]);
 *                       centre must be NULL
 *     TPG_ACTION_TEST   c[t,b] = fp64 mean of v over the K rows of frame t;  high[t,b,k,:] = (float)(v - c[t,b]);
 *                       scale must be NULL; centre (T,B,3) f32 receives (float)c
 * The mean is summed in a fixed order (no floating-point atomics): bit-identical from run to run.  high (T,B,K,3) is
 * frame-major like tpg_clip_gather_high_f32's.  A frame outside [0, P), count < 1, a non-finite scale: TPG_ERR_ARG. */
#define TPG_ACTION_TRAIN 0
#define TPG_ACTION_TEST 1
int tpg_action_gather_f32(const float *points, long long P, const int32_t *frame_first, const int32_t *count,
                          const int32_t *idx, const double *scale, int mode, int T, int B, int K, float *high,
                          float *centre, void *stream);

/* ---- dummy-centre replacement on the device (csrc/dummy_centres.hip) --------------------------------------------
 * discriminator.py:115-130: FPS picks that landed on a 999-padded point are swapped for other points of the cloud.  The
 * reference finds them on the host and draws with np.random.choice; this entry does the same job with no host
 * involvement, so a captured step can replay it.  xyz (B,N,3) f32; centres (B,S) int32 (entries are clamped into the
 * cloud; S > N is what FPS gives for a cloud smaller than npoint, with repeated picks); draw_key: 2 int64 words ON THE DEVICE, [seed, n_iter], read by the kernel; site >= 0: the ordinal of the
 * call within a step, a launch argument.  out (B,S) int32, not centres itself.  For cloud b, all integer:
 *     hit[s] = fabsf(xyz[b, centres[b,s], 0] - 999.0f) < 1e-4f;  k = the number of hits
 *     k == 0:     out[b] = centres[b]; prefix_flag[b] is left alone
 *     pool      = every j in [0,N) that is not a hit SLOT POSITION (j < S && hit[j]) -- the reference's quirk: slot
 *                 positions are excluded, not point ids, so a pick may itself be a dummy; N - k members while S <= N
 *     pool < k:   (the reference's choice() raises; N - k < k while S <= N) out[b] = centres[b], *short_flag = 1
 *     otherwise:  out[b] = the surviving centres in slot order, then the k pool members smallest in (key(j), j),
 *                 ascending; prefix_flag[b] = 0 (the centres are no longer in pick order: the level after must not take
 *                 tpg_fps_prefix_f32's shortcut)
 * key(j) is tpg_frame_subset's, with mix as stated there and a seed per cloud, uint32 arithmetic, wrapping:
 *     seed_lo = mix( lo32(seed) ^ mix(lo32(n_iter) * 0x9E3779B1 + site) )
 *     seed_hi = mix( hi32(seed) ^ mix(b * 0x85EBCA6B + site) )                  (b: the cloud's index within the call)
 *     key(j)  = mix( mix(j * 0x9E3779B1 + seed_lo) ^ seed_hi )
 * short_flag (1) int32 is zeroed by the call and set if any cloud was short; prefix_flag (B) int32 or NULL.
 * A pure function of its inputs: bit-identical from run to run (integer LDS atomics and a sort of unique keys only).
 * One workgroup per cloud; a cloud without a hit costs one gather of S rows.  No workspace.
 * Negative B, N, S or site: TPG_ERR_ARG.  B == 0 or S == 0: TPG_OK, nothing written.  Then N == 0, a NULL xyz, centres,
 * draw_key, out or short_flag, out == centres: TPG_ERR_ARG; S > tpg_patch_select_max_k(): TPG_ERR_UNSUPPORTED.  All of
 * it is decided before anything is launched. */
int tpg_replace_dummy_centres(const float *xyz, const int32_t *centres, const int64_t *draw_key, int site, int B, int N,
                              int S, int32_t *out, int32_t *prefix_flag, int32_t *short_flag, void *stream);

/* ---- point-cloud pictures (csrc/render.hip) --------------------------------------------------------------------
 * A z-buffered square splat of F clouds, one picture each (the reference looks at its results through an Open3D
 * window, train_utils.py:224-238; the look here is this project's own).  points (F,N,3) f32; lengths (F) int64 or
 * NULL: rows at or beyond lengths[f] are never read; scalar (F,N) f32 or NULL: the value a point is coloured by
 * (NULL: its depth t).  cams: a HOST table (the exception stated for the clip sampler above) of ncam = 1 (shared by
 * all frames) or ncam = F cameras of TPG_RENDER_CAM_FLOATS floats each:
 *     [0..2] eye   [3..5] r   [6..8] d   [9..11] f   (orthonormal rows: image-right, image-DOWN, forward)
 *     [12] scale   [13] cx   [14] cy   [15] near   [16] far   [17] mode (0 = ortho, 1 = pinhole)
 * Everything is fp32, each operation rounded on its own (no FMA), dot products as (a.x*b.x + a.y*b.y) + a.z*b.z:
 *     q = p - eye;  xv = q.r;  yv = q.d;  zv = q.f
 *     ortho:    u = xv*scale + cx;         v = yv*scale + cy
 *     pinhole:  u = (xv/zv)*scale + cx;    v = (yv/zv)*scale + cy
 *     t = zv - near;  the point is dropped unless
 *         t >= 0 && zv <= far && u >= -S && u < W+S && v >= -S && v < H+S           (S = size)
 *     which a NaN or an infinity anywhere fails; the test comes BEFORE any conversion to an integer.
 * With px = (int)floorf(u), py = (int)floorf(v) the point covers columns px - S/2 .. px - S/2 + S - 1 (integer
 * division) and rows likewise, clipped to the image.  Per covered pixel the smallest 64-bit key
 * (bits(t) << 32) | index wins (a non-negative fp32 orders like its bit pattern; equal depths: the lower index; t = -0.0,
 * which only zv = -0.0 with near = 0 gives, ranks by its pattern, behind every other depth): a 64-bit atomic min on
 * `keys`, (F,H,W) uint64, 8-byte aligned, set to all ones by the call itself.  The result does not depend on the order
 * of execution: bit-identical from run to run and at every batch position.
 * winner (F,H,W) int32: the visible point's index, -1 for background.  image (F,H,W,3) uint8: background (3) uint8
 * where winner is -1, else lut[level] (lut (256,3) uint8) with s = scalar[f][winner] (or t), inv = 255/(hi - lo)
 * rounded to fp32 once, c = (s - lo)*inv and level = 0 unless c > 0 (so NaN gives 0), 255 if c >= 255, else
 * (int)(c + 0.5f).
 * NULL image / winner, size outside 1..TPG_RENDER_MAX_SIZE, W or H < 1, hi <= lo: TPG_ERR_ARG.  F == 0 or N == 0:
 * TPG_OK, nothing written.  Then: another NULL pointer, ncam not 1 or F, a non-finite camera entry, lo or inv, a mode
 * other than 0 / 1, a pinhole camera with near <= 0: TPG_ERR_ARG; W or H > TPG_RENDER_MAX_EXTENT, F > 65535 or more than
 * 2^31 pixels in all: TPG_ERR_UNSUPPORTED.  All of it is decided before anything is launched. */
#define TPG_RENDER_CAM_FLOATS 18
#define TPG_RENDER_MAX_SIZE 16
#define TPG_RENDER_MAX_EXTENT 16384
int tpg_render_points_f32(const float *points, const int64_t *lengths, const float *scalar, int F, int N,
                          const float *cams, int ncam, int W, int H, int size, float lo, float hi, const uint8_t *lut,
                          const uint8_t *background, void *keys, uint8_t *image, int32_t *winner, void *stream);

/* ---- fluid surface pictures (csrc/surface.hip) ------------------------------------------------------------------
 * Screen-space fluid rendering in three entries: every particle is a sphere of radius rad (world units), the nearest
 * sphere front per pixel is kept (a), that depth image is smoothed without crossing silhouettes (b, called as often as
 * wanted), normals are taken from it and it is shaded (c).  (The reference's demo notebooks write .bgeo files for an
 * external tool to do this; the look here is this project's own.)  points, lengths, cams, ncam, keys and the projection
 * of a point to u, v, zv, t = zv - near are tpg_render_points_f32's, word for word; everything is fp32, each operation
 * rounded on its own, dot products as (a.x*b.x + a.y*b.y) + a.z*b.z.
 *
 * (a) tpg_render_spheres_f32 -> depth (F,H,W) f32, winner (F,H,W) int32.  Per point:
 *     rp = rad*scale (ortho) or (rad/zv)*scale (pinhole), then rp = fminf(rp, (float)TPG_SURFACE_MAX_RADIUS): a nearer
 *     or larger sphere is drawn as a disc of 64 pixels radius with its true bulge (stated, not an error).
 *     The point is dropped unless
 *         t >= 0 && zv <= far && rp > 0 && u >= -rp && u < W+rp && v >= -rp && v < H+rp
 *     which a NaN or an infinity anywhere fails; the test comes BEFORE any conversion to an integer.
 *     Candidate pixels: columns (int)floorf(u - rp) .. (int)floorf(u + rp), rows likewise with v, clipped to the image.
 *     For a candidate (x, y): dx = (((float)x + 0.5f) - u) / rp, dy = (((float)y + 0.5f) - v) / rp, s = dx*dx + dy*dy;
 *     it is covered iff s < 1.0f.  Then h = sqrtf(1.0f - s), tp = t - rad*h, and tp is replaced by 0.0f unless tp > 0
 *     (the front is clamped at the near plane).  Key (bits(tp) << 32) | index, 64-bit atomic min on `keys`, (F,H,W)
 *     uint64, 8-byte aligned, set to all ones by the call itself.
 *   winner: the key's low word, -1 where the key is still all ones; depth: the float whose bits are the key's high
 *   word, +inf for background.  Equal fronts show the lower index; the result does not depend on the order of execution
 *   nor on how the discs are spread over the lanes: bit-identical from run to run and at every batch position.
 *
 * (b) tpg_surface_smooth_f32: in (F,H,W) -> out (F,H,W), out != in; half-width k = 1..TPG_SURFACE_MAX_HALF, delta > 0.
 *   bw is the binomial row of order 2k in integers (1 2 1; 1 4 6 4 1; ...; every product <= 70*70, exact in fp32).
 *   A pixel whose `in` zi is not finite is copied unchanged.  Otherwise acc = 0, ws = 0, and for oy = -k..k (outer),
 *   ox = -k..k (inner): the neighbour (x+ox, y+oy) contributes if it is inside the image, its depth zj is finite and
 *   fabsf(zj - zi) <= delta, with w = (float)(bw[oy+k]*bw[ox+k]), acc = acc + w*zj, ws = ws + w; out = acc / ws.  The
 *   summation order is part of the rule.  The centre always contributes: background never becomes surface, surface
 *   never background, and a step larger than delta is not smeared.
 *
 * (c) tpg_surface_shade_f32: depth (F,H,W) (smoothed), winner (F,H,W), scalar (F,N) or NULL, lo, hi, lut, background
 *   as for tpg_render_points_f32 -> image (F,H,W,3) uint8.  shade: a HOST table of TPG_SURFACE_SHADE_FLOATS floats:
 *     [0..2] L (unit, towards the light)   [3..5] Hh (unit half vector of L and V = (0,0,-1), computed by the host)
 *     [6] ka   [7] kd   [8] ks   [9] kf   [10] p (an integer 0..8 stored as a float)
 *   in view coordinates: x right, y down, z forward.  A pixel is surface iff its depth z is finite; every other pixel
 *   gets `background`.  The view-space point of a surface pixel (x, y):
 *     Zv = z + near;  a = (((float)x + 0.5f) - cx) / scale;  b = (((float)y + 0.5f) - cy) / scale
 *     ortho: P = (a, b, Zv);   pinhole: P = (a*Zv, b*Zv, Zv)
 *   ddx: the forward candidate P(x+1,y) - P(x,y) if that pixel exists and is surface, the backward candidate
 *   P(x,y) - P(x-1,y) likewise; the one with the smaller fabsf of its z component, forward on equality or if it is the
 *   only one; if neither exists (1/scale, 0, 0) for ortho, (Zv/scale, 0, 0) for pinhole.  ddy: the same with rows, down
 *   being forward, and (0, 1/scale, 0) / (0, Zv/scale, 0).  n = cross(ddy, ddx), each component a*b - c*d:
 *     nx = ddy.y*ddx.z - ddy.z*ddx.y;  ny = ddy.z*ddx.x - ddy.x*ddx.z;  nz = ddy.x*ddx.y - ddy.y*ddx.x
 *   (a plane facing the camera gives (0,0,-1)); len = sqrtf((nx*nx + ny*ny) + nz*nz); n = n / len componentwise if
 *   len > 0, else (0,0,-1).  dif = fmaxf(n.L, 0); sp = fmaxf(n.Hh, 0), then sp = sp*sp p times; c = fmaxf(-nz, 0),
 *   m = 1 - c, m2 = m*m, fr = (m2*m2)*m.  Base colour: lut[level] by tpg_render_points_f32's level rule with
 *   s = scalar[f][winner] (winner is read at surface pixels only and only with a scalar, taken into 0..N-1), or s = z
 *   when scalar is NULL.  Per channel val = (float)base*(ka + kd*dif) + 255.0f*(ks*sp + kf*fr), stored as 0 unless
 *   val > 0, 255 if val >= 255, else (int)(val + 0.5f).
 *
 * Checks, all before anything is launched.  TPG_ERR_ARG: negative F or N, a NULL output, W or H < 1, rad or delta not
 * positive and finite, k outside 1..TPG_SURFACE_MAX_HALF, out == in, hi <= lo, a NULL or non-finite shade table, p not
 * an integer 0..8.  Then F == 0 (and for (a), (c): N == 0): TPG_OK, nothing written.  Then another NULL pointer, keys
 * not 8-byte aligned, and the camera and lo / inv conditions of tpg_render_points_f32: TPG_ERR_ARG; its limits on W, H,
 * F and the pixels in all: TPG_ERR_UNSUPPORTED. */
#define TPG_SURFACE_MAX_RADIUS 64
#define TPG_SURFACE_MAX_HALF 4
#define TPG_SURFACE_SHADE_FLOATS 11
int tpg_render_spheres_f32(const float *points, const int64_t *lengths, int F, int N, const float *cams, int ncam, int W,
                           int H, float rad, void *keys, float *depth, int32_t *winner, void *stream);
int tpg_surface_smooth_f32(const float *in, int F, int W, int H, int k, float delta, float *out, void *stream);
int tpg_surface_shade_f32(const float *depth, const int32_t *winner, const float *scalar, int F, int N, const float *cams,
                          int ncam, int W, int H, float lo, float hi, const uint8_t *lut, const uint8_t *background,
                          const float *shade, uint8_t *image, void *stream);

/* ---- fluid thickness and absorption (csrc/surface.hip) ------------------------------------------------------------
 * The second half of screen-space fluid rendering: how much fluid a pixel looks through up to the first solid (a), and
 * the shaded surface mixed with what lies behind it by a transmittance that falls with that thickness (c).  Between the
 * two the thickness is blurred (b).  Everything is fp32, each operation rounded on its own.
 *
 * (a) tpg_render_thickness_f32 -> thickness (F,H,W) f32.  points, lengths, F, N, cams, ncam, W, H, rad as for
 *   tpg_render_spheres_f32.  limit (F,H,W) f32 or NULL: the opaque scene's depth (distance from the near plane, +inf
 *   where there is nothing); fluid beyond it is not counted.  acc (F,H,W) uint64, 8-byte aligned, zeroed by the call
 *   itself.  Per point the projection, rp (with the 64-pixel cap), the drop test, the candidate box and the coverage
 *   test s < 1.0f are those of entry (a) of "fluid surface pictures", word for word.  For a covered pixel (x, y):
 *       h = sqrtf(1.0f - s);  half = rad*h;  tp = t - half;  tb = t + half
 *       a = tp > 0 ? tp : 0.0f                       (the near-plane clamp of the fronts)
 *       b = (limit && lim < tb) ? lim : tb            (lim = limit[f][y][x]; a NaN lim leaves the whole chord)
 *       term = b - a
 *   The pixel contributes iff term > 0, and then q = (long long)(term * 16777216.0f): units of 2^-24, truncated; a
 *   64-bit integer atomic add on acc.  Then per pixel thickness = (float)acc * 2^-24f, the uint64 -> fp32 conversion
 *   rounding to nearest even.  Integer sums: the result does not depend on the order of execution nor on how the discs
 *   are spread over the lanes; bit-identical from run to run, at every batch position and under every chunking.
 *   rad <= TPG_THICKNESS_MAX_RAD keeps a term at or below 2^35 units, N <= TPG_THICKNESS_MAX_N the sum below 2^63.
 *
 * (b) Smoothing the thickness needs no entry of its own: tpg_surface_smooth_f32 with delta = FLT_MAX is a plain binomial
 *   blur whose window leaves out the pixels outside the image and nothing else (every finite difference passes the
 *   test).  Zeros are finite and take part: the fluid's outline fades out, it is not kept sharp.
 *
 * (c) tpg_surface_absorb_u8: fluid (F,H,W,3) uint8, fdepth (F,H,W) f32, thickness (F,H,W) f32: the shaded fluid layer,
 *   its depth and (a)'s image; behind (F,H,W,3) uint8, bdepth (F,H,W) f32: the solids over the background (no solid:
 *   the background colour with +inf); th_max > 0; table: a HOST table of 256 x 3 f32 transmittances, each finite and in
 *   [0,1] (a table, not expf, so that kernel, torch and numpy agree bit for bit)
 *   -> image (F,H,W,3) uint8, depth (F,H,W) f32.  Per pixel: if fdepth is not finite or bdepth < fdepth, image = behind
 *   and depth = bdepth (on equality the fluid wins, as the earlier layer does when layers are composed).  Otherwise
 *   level by tpg_render_points_f32's level rule with s = thickness, lo = 0, inv = 255/th_max rounded to fp32 once; per
 *   channel T = table[level][c], val = (float)fluid_c*(1.0f - T) + (float)behind_c*T, stored as
 *   tpg_surface_shade_f32 stores: 0 unless val > 0, 255 if val >= 255, else (int)(val + 0.5f); depth = fdepth.
 *
 * Checks, all before anything is launched.  (a): those of tpg_render_spheres_f32 (thickness the output, acc the 8-byte
 * aligned buffer), and rad > TPG_THICKNESS_MAX_RAD: TPG_ERR_ARG, N > TPG_THICKNESS_MAX_N: TPG_ERR_UNSUPPORTED.
 * (c): negative F, a NULL output or table, a table entry that is not finite or outside [0,1], th_max not positive and
 * finite, W or H < 1: TPG_ERR_ARG.  Then F == 0: TPG_OK, nothing written.  Then another NULL pointer or a th_max so
 * small that inv is not finite: TPG_ERR_ARG; the limits on W, H, F and the pixels in all: TPG_ERR_UNSUPPORTED. */
#define TPG_THICKNESS_MAX_RAD 1024
#define TPG_THICKNESS_MAX_N 134217728
int tpg_render_thickness_f32(const float *points, const int64_t *lengths, int F, int N, const float *cams, int ncam, int W,
                             int H, float rad, const float *limit, void *acc, float *thickness, void *stream);
int tpg_surface_absorb_u8(const uint8_t *fluid, const float *fdepth, const float *thickness, const uint8_t *behind,
                          const float *bdepth, int F, int W, int H, float th_max, const float *table, uint8_t *image,
                          float *depth, void *stream);

/* ---- mesh pictures (csrc/mesh_render.hip) -----------------------------------------------------------------------
 * A z-buffered rasteriser of indexed triangle meshes in two entries: the nearest face per pixel (a), then deferred
 * shading of that face (b).  (The reference hands its geometry to an external renderer; the look here is this
 * project's own.)  vertices (M,V,3) f32; vlengths (M) int64 or NULL: vlen = vlengths[m] taken into 0..V (NULL: V), rows
 * at or beyond it are never read; faces (M,T,3) int32; flengths (M) int64 or NULL: tlen likewise, faces at or beyond it
 * are never read.  M = 1: one mesh drawn in all F frames (an obstacle); M = F: mesh f in frame f.  cams, ncam, W, H,
 * keys and the projection of a vertex to u, v, zv, t = zv - near are tpg_render_points_f32's, word for word (fp32, each
 * operation rounded on its own, dot products as (a.x*b.x + a.y*b.y) + a.z*b.z).  The depth is perspective-correct;
 * every other attribute is interpolated linearly in SCREEN space, also under a pinhole camera (stated, not an error).
 *
 * Per face j < tlen with the indices i0, i1, i2:
 *   dropped unless all three lie in 0..vlen-1 (such a face never addresses memory; neither clamped nor an error);
 *   dropped unless every vertex passes  t >= 0 && zv <= far && fabsf(u) < 32768 && fabsf(v) < 32768  (TPG_MESH_GUARD),
 *     which a NaN or an infinity anywhere fails; the test comes BEFORE any conversion to an integer.  There is NO
 *     clipping: a triangle that crosses the near plane or leaves the guard band is not drawn.
 *   Snap, 8 subpixel bits: X = (int)floorf(u*256.0f + 0.5f), Y = (int)floorf(v*256.0f + 0.5f); below the guard band the
 *     product and the sum are exact.  The centre of pixel (x, y) is (256x+128, 256y+128).
 *   Edge function, int64 and exact (differences < 2^25): E(a, b, p) = (bx-ax)*(py-ay) - (by-ay)*(px-ax).
 *     A = E(v0, v1, v2); the face is dropped if A == 0.  s = the sign of A.  At a pixel centre p
 *       w0 = s*E(v1, v2, p),  w1 = s*E(v2, v0, p),  w2 = s*E(v0, v1, p)          (w0 + w1 + w2 = |A|)
 *     and the edge a -> b of w_i has the direction (dx, dy) = s*(b - a).  The pixel is covered iff for every i
 *       w_i > 0  ||  (w_i == 0 && (dy < 0 || (dy == 0 && dx > 0)))
 *     With y pointing down and the inside where E > 0 the owning edges are the left ones and the horizontal top ones:
 *     the rule depends on the edge's direction only and opposite directions get opposite answers, so a centre exactly on
 *     an edge shared by two triangles on opposite sides of it belongs to exactly one of them, and a centre on the shared
 *     vertex of a closed fan to exactly one triangle of the fan.  Both sides are drawn; there is no culling.
 *   Candidate pixels: those whose centres lie in the snapped bounding box, columns (Xmin + 127) >> 8 .. (Xmax - 128) >> 8
 *     (>> rounding down), rows likewise, clipped to the image.  Every covered pixel is a candidate.
 *   Depth of a covered pixel, in float64, every operation rounded on its own (the library is built with contraction
 *     off): l_i = (double)w_i / (double)|A|;
 *       ortho:    t = (float)((l0*t0 + l1*t1) + l2*t2)
 *       pinhole:  Z = 1.0 / ((l0/zv0 + l1/zv1) + l2/zv2);  t = (float)(Z - (double)near)
 *     and t is replaced by 0.0f unless t > 0, as the sphere fronts are.  Key (bits(t) << 32) | j, 64-bit atomic min on
 *     `keys`, (F,H,W) uint64, 8-byte aligned, set to all ones by the call itself.
 * (a) tpg_render_mesh_f32 -> depth (F,H,W) f32: the float whose bits are the key's high word, +inf for background;
 *   winner (F,H,W) int32: the key's low word, -1 for background.  Equal depths show the lower face index; the result
 *   does not depend on the order of execution nor on which lane draws which pixel (faces whose clipped box holds at most
 *   TPG_MESH_SMALL pixels are drawn by one lane, the others by a whole wave, and those of more than TPG_MESH_HUGE
 *   pixels by a second launch over 32 x 32 tiles from a list of TPG_MESH_LIST faces per frame, a face that finds the
 *   list full being drawn by a wave; tuning values, not part of the rule).  list: (F * (1 + TPG_MESH_LIST)) int32, a
 *   workspace the call itself initialises.
 * (b) tpg_mesh_shade_f32: depth, winner as (a) wrote them, the mesh, normals (M,V,3) f32 or NULL, scalar (M,V) f32 or
 *   NULL, lo, hi, lut, background as for tpg_render_points_f32, base (3) uint8 on the device or NULL, shade: the HOST
 *   table of tpg_surface_shade_f32 -> image (F,H,W,3) uint8.  A pixel whose winner j is outside 0..tlen-1, or names a
 *   face that (a) drops, gets `background`.  Otherwise l0..l2 of face j at the pixel's centre are computed exactly as in
 *   (a) and the view-space normal is
 *     with normals:  nw_k = (float)((l0*(double)n0_k + l1*(double)n1_k) + l2*(double)n2_k) per component k (n_i the
 *       normal of vertex i_i), then n = (nw.r, nw.d, nw.f) with the camera's rows, fp32 dot products;
 *     without: with P_i = (xv, yv, zv) of vertex i in fp32, a = P1 - P0, b = P2 - P0, n = cross(a, b), each component
 *       a*b - c*d:  nx = a.y*b.z - a.z*b.y;  ny = a.z*b.x - a.x*b.z;  nz = a.x*b.y - a.y*b.x.
 *   len = sqrtf((nx*nx + ny*ny) + nz*nz); n = n / len componentwise if len > 0, else (0,0,-1); then n = -n if nz > 0, so
 *   both sides are lit.  Base colour: `base` if given; else lut[level] by tpg_render_points_f32's level rule with
 *   s = (float)((l0*(double)s0 + l1*(double)s1) + l2*(double)s2) of the vertices' scalars, or s = depth at the pixel
 *   when scalar is NULL.  dif, sp, fr, val and the final rounding are tpg_surface_shade_f32's, word for word.
 *
 * Checks, all before anything is launched.  TPG_ERR_ARG: negative F, M, V or T, a NULL output, W or H < 1; for (b) also
 * hi <= lo and the shade table's conditions.  Then F == 0, T == 0 or V == 0: TPG_OK, nothing written (the caller's
 * outputs stay what they were: the Python layer sets them to background).  Then another NULL pointer (lut may be NULL
 * with a base), a NULL list, keys not 8-byte aligned, M not 1 or F, and the camera and lo / inv conditions of tpg_render_points_f32:
 * TPG_ERR_ARG; its limits on W, H, F and the pixels in all, and T or V above TPG_MESH_MAX_ROWS (2^31 / 3):
 * TPG_ERR_UNSUPPORTED. */
#define TPG_MESH_GUARD 32768
#ifndef TPG_MESH_SMALL             /* tools/mesh_render_time.py builds the library with other values to time them */
#define TPG_MESH_SMALL 16
#endif
#define TPG_MESH_HUGE 2048
#define TPG_MESH_LIST 256
#define TPG_MESH_MAX_ROWS 715827882
int tpg_render_mesh_f32(const float *vertices, const int64_t *vlengths, const int32_t *faces, const int64_t *flengths,
                        int M, int V, int T, int F, const float *cams, int ncam, int W, int H, void *keys, int32_t *list,
                        float *depth, int32_t *winner, void *stream);
int tpg_mesh_shade_f32(const float *depth, const int32_t *winner, const float *vertices, const int64_t *vlengths,
                       const int32_t *faces, const int64_t *flengths, const float *normals, const float *scalar, int M,
                       int V, int T, int F, const float *cams, int ncam, int W, int H, float lo, float hi,
                       const uint8_t *lut, const uint8_t *base, const uint8_t *background, const float *shade,
                       uint8_t *image, void *stream);

/* ---- particle fluid simulator (csrc/pbf.hip) ---------------------------------------------------------------------
 * Position Based Fluids (Macklin and Mueller 2013) with Jacobi iterations in gather form: the simulator that writes the
 * training sequences (the reference drives an external DFSPH solver, fluid_data_generation/; look and statistics here
 * are this project's own).  A batch holds B scenes of up to N particles: x, v, p (B,N,3) f32, lengths (B) int64 or NULL
 * (rows at or beyond lengths[b] are never read and never written), box a HOST table (B,6) f32 (the exception stated
 * for the clip sampler above): lo xyz, hi xyz of the scene's axis-aligned box; gravity: 3 HOST floats.
 *
 * Constants, computed by the host in fp64 and rounded to fp32 once: particle radius a, support h (= 4a), h2 = h*h in
 * fp32, and with the lattice sum S0 = sum over z in Z^3, |z| < 2, of (1 - |z|^2/4)^3 (a cubic lattice of spacing
 * s = h/2, self included; 5.15625):  wq = (1 - 0.2^2)^3 (the weight at d = 0.2 h),  dp_scale = -7 h S0 / 64,
 * cs = c / S0.  Everything below is fp32, each operation rounded on its own (no FMA), only + - * / and sqrtf;
 * comparisons and selections are exact.  clamp(p, l, u) per axis: p = p < l ? l : p; p = p > u ? u : p, with
 * l = lo + a, u = hi - a.
 *
 * Weights of a pair at the canonical distance d2 = ((dx*dx) + dy*dy) + dz*dz, dx = p_i.x - p_j.x ...; a pair counts iff
 * d2 < h2, STRICT (both weights vanish at the rim, so membership there cannot matter):
 *     u = (h2 - d2) / h2;  W = (u*u)*u                       (the density weight (h^2 - d^2)^3 over h^6: <= 1, and far
 *                                                            from the denormals the unscaled h^6 ~ 1e-8 form would meet)
 *     d = sqrtf(d2);  t = (h - d) / h;  t2 = t*t             (the gradient weight (h - d)^2 over h^2)
 *     G = (t2*(dx/d), t2*(dy/d), t2*(dz/d))                  (none for d2 == 0: duplicates and the particle itself add
 *                                                            to n and have no gradient)
 * The gradient of C_i = n_i/S0 - 1 with the spiky gradient, in these units, is g_ij = G_ij / dp_scale (poly6 over spiky
 * normalisation: 64 / (7 h S0), pointing from i to j); the rule carries the factor outside the sums:
 *     lambda_i (in units of dp_scale^2) = -C_i / (sum |G|^2 + |sum G|^2 + eps)
 *     dp_i = dp_scale * sum_j (lambda_i + lambda_j + s_ij) G_ij
 *
 * One substep of dt = 1 / (40 * substeps), as entries:
 *   tpg_pbf_predict_f32   v' = v + dt*gravity;  p = clamp(x + dt*v')                          -> p_out, v_out
 *   then `iters` times, each on a grid built from the current p so that every neighbour set is exact:
 *   tpg_pbf_grid_f32      the uniform grid of the grid searches with cell edge >= h * 1.0001, into ws
 *   tpg_pbf_lambda_f32    n = sum W (self included);  C = n / S0 - 1;  C = C > 0 ? C : 0;
 *                         lambda = -(C / ((sum |G|^2 + ((Sx*Sx + Sy*Sy) + Sz*Sz)) + eps)),  S = sum G,
 *                         |G|^2 = (Gx*Gx + Gy*Gy) + Gz*Gz per pair                            -> lam, C_out (or NULL)
 *   tpg_pbf_dp_f32        per pair r = W / wq;  r2 = r*r;  co = (lambda_i + lambda_j) + -(k*(r2*r2));  term = co * G;
 *                         dp = dp_scale * sum term;  p_out = clamp(p + dp)  (p_out may be p; dp_out or NULL).  Reads the
 *                         lambda of the launch before: Jacobi.
 *   and once more tpg_pbf_grid_f32 on the final p, then
 *   tpg_pbf_finish_f32    v_i = (p_i - x_i) / dt per axis;  per pair (self included, its term is 0)
 *                         term = (v_j - v_i) * W;  v_out = v_i + cs * sum term;  x_out = p    (x_out != x)
 *
 * Sums.  The grid's order inside a cell is not fixed from run to run, so every sum is taken in 64-bit fixed point: each
 * term converted on its own by truncation, integers added, one conversion back (round to nearest) and one multiply:
 *     n, sum |G|^2     (uint64)(term * 2^32),  result (float)acc * 2^-32
 *     sum G            (int64)(term * 2^32) per axis, result (float)acc * 2^-32
 *     dp, XSPH         term clamped into [-1024, 1024] first, (int64)(term * 2^30), result (float)acc * 2^-30
 * Terms of the first two lie within 1 + 2^-20, N <= 2^22 is checked, so no sum can wrap (csrc/pbf.hip has the
 * arithmetic).  The results do not depend on the order of execution, the batch position or the rest of the batch.
 *
 * Checks, all before anything is launched.  TPG_ERR_ARG: negative B or N, h, dt, a, S0 or wq not positive and finite,
 * eps, k or cs negative or not finite, a NULL output, x_out == x, a workspace that is NULL or not 256-byte aligned
 * (when B, N > 0).  Then B == 0 or N == 0: TPG_OK, nothing written.  Then B > 65535 or N > 2^22: TPG_ERR_UNSUPPORTED;
 * another NULL pointer, a box that is not finite or has lo >= hi on an axis: TPG_ERR_ARG.  ws: tpg_pbf_workspace_bytes(B,
 * N) bytes; lambda, dp and finish read the grid the last tpg_pbf_grid_f32 with the same B, N left there.
 * lengths are device values and are NOT checked (that would be a host read): every entry, the grid build included, takes
 * lengths[b] as min(max(lengths[b], 0), N) computed on the 64-bit value, before any narrowing -- N + 7 and 2^32 + 5 are
 * N, -3 is 0 -- so that all launches of a substep agree on a scene's particle count; NULL is N everywhere.  Rows that
 * such a length brings in are read like any other: finite values there are the caller's business. */
size_t tpg_pbf_workspace_bytes(int B, int N);
int tpg_pbf_predict_f32(const float *x, const float *v, const int64_t *lengths, const float *box, int B, int N, float dt,
                        float a, const float *gravity, float *p_out, float *v_out, void *stream);
int tpg_pbf_grid_f32(const float *p, const int64_t *lengths, int B, int N, float h, void *ws, void *stream);
int tpg_pbf_lambda_f32(const float *p, const int64_t *lengths, int B, int N, float h, float S0, float eps, const void *ws,
                       float *lam, float *C_out, void *stream);
int tpg_pbf_dp_f32(const float *p, const float *lam, const int64_t *lengths, const float *box, int B, int N, float h,
                   float a, float wq, float k, float dp_scale, const void *ws, float *p_out, float *dp_out, void *stream);
int tpg_pbf_finish_f32(const float *p, const float *x, const int64_t *lengths, int B, int N, float h, float dt, float cs,
                       const void *ws, float *x_out, float *v_out, void *stream);

/* ---- vorticity confinement and per-particle viscosity in the particle fluid simulator (csrc/pbf.hip) ----------------
 * The third velocity stage of Macklin and Mueller's solver, and an XSPH coefficient per particle instead of one per
 * batch.  Both live in the tail of the substep, on the grid of the final p that finish walks, and both use finish's pair
 * quantity u = v_j - v_i: together they cost ONE more neighbourhood walk.  With either in use a substep ends
 *     grid | finish_ex | vorticity          (vorticity only when its strength is > 0)
 * Notation, pair membership (d2 < h2; gradient pairs also d2 != 0), W, t2, G_ij = t2 * (p_i - p_j) / d per axis and the
 * fixed-point sums are those of the section above; fix30(t) is the clamp of t into [-1024, 1024] followed by
 * (int64)(t * 2^30).  Every fp32 operation is rounded on its own; only + - * / and sqrtf are used.
 *
 * tpg_pbf_finish_ex_f32: finish with two options, each switched on by a pointer.  v_i = (p_i - x_i) / dt and, per pair,
 * u = (c_j - x_j) / dt - v_i per axis (c_j: the neighbour's position in the grid's copy), exactly as in finish.
 *   cs_tab == NULL      v_out = v_i + cs * sum fix30(u * W)                                     (finish itself)
 *   cs_tab (B,N) f32    cij = 0.5f * (cs_tab[i] + cs_tab[j]);  term = fix30(cij * (u * W));  v_out = v_i + sum term, no
 *                       outer factor, cs unused.  cij and u * W are symmetric resp. antisymmetric in (i, j) bit for bit,
 *                       so term_ij = -term_ji in integers: the table moves momentum between particles, it makes none.
 *   omega_out (B,N,4)   over gradient pairs, on the velocities BEFORE XSPH (the u of this walk):
 *                           omega_i = sum u x G_ij:  x: fix30(u_y*G_z - u_z*G_y),  y: fix30(u_z*G_x - u_x*G_z),
 *                                                    z: fix30(u_x*G_y - u_y*G_x)   (two products, one subtraction)
 *                       stored as (omega_x, omega_y, omega_z, m), m = sqrtf((omega_x^2 + omega_y^2) + omega_z^2).
 *                       Right-handed: a rigid rotation Omega about +y gives omega_y > 0.
 *   With both pointers NULL the launch is finish's, bit for bit.
 *
 * tpg_pbf_vorticity_f32: a second walk on the same grid (no new build), p the final positions (finish's x_out):
 *     eta_i = sum over gradient pairs of fix30((m_i - m_j) * G_ij) per axis     m_j = omega[index_j].w, one 16-byte load;
 *                                                                                the difference form: uniform m -> eta = 0
 *     len = sqrtf((eta_x^2 + eta_y^2) + eta_z^2);  N = eta / (len + delta) per axis;  f = N x omega_i
 *         f_x = N_y*omega_z - N_z*omega_y,  f_y = N_z*omega_x - N_x*omega_z,  f_z = N_x*omega_y - N_y*omega_x
 *     v_out = v_i + (dt * vs) * f per axis
 * A wave reads only its own row of v, so v_out may be v.  Rows at or beyond lengths[b] are never read or written.
 *
 * Normalisation, in the manner of S0: R0 = (1/3) * sum over z in Z^3, 0 < |z| < 2, of ((2 - |z|)/2)^2 |z| (26 points,
 * 1.06818514...).  In a cubic lattice of spacing s = h/2 that rotates rigidly at Omega the curl above is s * R0 * 2 Omega,
 * so omega in 1/s is omega / (s * R0), and the host passes vs = fp32(strength / (s * R0)) with the strength in m/s.
 * delta > 0 keeps N finite where eta is rounding noise (ops.PBF_VORT_DELTA).
 *
 * Checks, in the order of the section above.  TPG_ERR_ARG: h, dt (and delta) not positive and finite, cs (vs) negative or
 * not finite, a NULL x_out or v_out, x_out == x, a bad workspace (when B, N > 0), negative B or N.  Then B == 0 or
 * N == 0: TPG_OK before any other pointer is looked at.  Then B > 65535 or N > 2^22: TPG_ERR_UNSUPPORTED; a NULL p, x,
 * omega or v: TPG_ERR_ARG. */
int tpg_pbf_finish_ex_f32(const float *p, const float *x, const int64_t *lengths, int B, int N, float h, float dt, float cs,
                          const float *cs_tab, const void *ws, float *x_out, float *v_out, float *omega_out, void *stream);
int tpg_pbf_vorticity_f32(const float *p, const float *omega, const float *v, const int64_t *lengths, int B, int N, float h,
                          float dt, float vs, float delta, const void *ws, float *v_out, void *stream);

/* ---- solid obstacles in the particle fluid simulator (csrc/pbf.hip) ----------------------------------------------
 * Static solids in the way of the fluid: the three shapes the fluid bodies use, each in a rotated frame of its own.  A
 * scene has up to PBF_MAX_OBSTACLES = 8 of them, in a DEVICE table obstacles (B,M,16) f32, one row per obstacle:
 *     kind, cx, cy, cz, R00 R01 R02 R10 R11 R12 R20 R21 R22 (row-major), s0, s1, s2
 *     kind 1  ball      radius s0
 *     kind 2  box       half extents s0, s1, s2
 *     kind 3  cylinder  along the local y axis: radius s0, half height s1
 * The world position of a local point q is c + R q.  A row is SKIPPED when its kind is none of 1.0f, 2.0f, 3.0f (padding
 * rows have kind 0) or when any of its 15 other values is not finite (|v| <= FLT_MAX is false: NaN, +-inf), so a row with
 * a non-finite number never tests "inside".  Like lengths, the table's values sit on the device and are not checked by
 * the entry; no address depends on a table value, so a bad row cannot fault.  (ops.pbf_obstacles validates on the host:
 * finite values, positive sizes, R orthonormal.)
 *
 * collide(p), per particle, over the obstacles o = 0 .. M-1 IN INDEX ORDER, each acting on the position the previous one
 * left.  fp32, only + - * / and sqrtf, each operation rounded on its own (no FMA); comparisons, |.| and selections are
 * exact.  With a the particle radius:
 *   local frame   dx = px - cx, dy = py - cy, dz = pz - cz;  q_k = (dx*R[0][k] + dy*R[1][k]) + dz*R[2][k],  k = x, y, z
 *   ball          E = s0 + a;  d2 = (qx*qx + qy*qy) + qz*qz;  inside iff d2 < E*E (STRICT).
 *                 d2 == 0: q = (0, E, 0);  otherwise d = sqrtf(d2), q_k = (q_k / d) * E
 *   box           E_k = s_k + a;  inside iff |q_k| < E_k on all three axes.  pen_k = E_k - |q_k|; the axis with the
 *                 smallest pen, ties to the lowest k (k = 0; pen_1 < pen_0: k = 1; pen_2 < pen_k: k = 2); on that axis
 *                 q_k = q_k < 0 ? -E_k : E_k
 *   cylinder      Er = s0 + a, Eh = s1 + a, r2 = qx*qx + qz*qz;  inside iff r2 < Er*Er and |qy| < Eh.
 *                 r = sqrtf(r2);  pen_r = Er - r;  pen_h = Eh - |qy|.
 *                 pen_h <= pen_r: onto the cap, qy = qy < 0 ? -Eh : Eh;
 *                 otherwise radially: (qx, qz) = ((qx / r) * Er, (qz / r) * Er), or (Er, 0) when r2 == 0
 *   back          ONLY a particle that was inside is written back: p_k = c_k + ((R[k][0]*qx + R[k][1]*qy) + R[k][2]*qz).
 *                 A particle that was not inside keeps its bits for that obstacle: no round trip through the local frame.
 *   at the end    the scene's box clamp of the rule above, clamp(p, lo + a, hi - a): the clamp wins over an obstacle
 *                 that leans on a wall.
 * One substep with obstacles is the substep above with collide applied once to the output of predict and once to the
 * output of every dp pass (each of which has already been clamped: the clamp is idempotent).  Velocities need nothing
 * more: finish takes v = (p - x) / dt.  The solid is a position constraint only, exactly as the walls are: no boundary
 * particles, no friction.  Consequences:
 *   - density is deficient at an obstacle's skin, as at a wall (nothing fills the solid's side of the neighbourhood);
 *   - a particle that moves more than an obstacle's half thickness in one substep can come out on the far side (it is
 *     projected to the nearest face, or is never seen inside): keep obstacles several particle spacings thick;
 *   - an obstacle that overlaps a wall can pin particles in the wedge: the obstacle pushes them through the wall, the
 *     clamp puts them back inside the obstacle.
 *
 * tpg_pbf_collide_f32: p_out = collide(p) for every scene; p_out may be p (a thread touches its own row only).  hit_out
 * (B,N) int32 or NULL: bit o is set iff obstacle o moved the particle (it tested inside).  box is the HOST table of
 * tpg_pbf_predict_f32.  One thread per particle, scenes in chunks of 64 per launch like predict.  Rows at or beyond
 * lengths[b] are never read and never written.  Checks, all before anything is launched.  TPG_ERR_ARG: negative B, N or
 * M, a not positive and finite, a NULL p_out.  Then B == 0 or N == 0: TPG_OK, nothing written.  Then B > 65535, N > 2^22
 * or M > PBF_MAX_OBSTACLES: TPG_ERR_UNSUPPORTED.  Then a NULL p or box, a box that is not finite or has lo >= hi on an
 * axis, a NULL obstacles with M > 0: TPG_ERR_ARG.  M == 0 is legal and applies the clamp alone. */
#define PBF_MAX_OBSTACLES 8
int tpg_pbf_collide_f32(const float *p, const int64_t *lengths, const float *box, const float *obstacles, int B, int N,
                        int M, float a, float *p_out, int32_t *hit_out, void *stream);

/* ---- isosurfaces (csrc/isosurface.hip) ------------------------------------------------------------------------------
 * The surface field >= iso of a scalar field on a regular lattice as an indexed triangle mesh: marching tetrahedra on
 * the Kuhn (Freudenthal) split of every lattice cube into six tetrahedra.  (The reference ends its demo by handing
 * every frame to an external tool that reconstructs the fluid's surface; this mesher is this project's own and no parity
 * with any such tool is claimed.)  Everything is fp32, each operation rounded on its own (no FMA), only + - * / and
 * sqrtf; comparisons and selections are exact.
 *
 * Lattice: nx x ny x nz nodes, origin 3 HOST floats, step s > 0; field a contiguous (nx,ny,nz) array, node (i,j,k) has
 * the id n = (i*ny + j)*nz + k and the position origin[a] + (float)index_a * s on axis a.
 * Inside: a node is inside iff field[n] >= iso (NaN is outside).
 * Edges: seven per node, to the node at offset D[d], d = 0..6,
 *     D = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (0,1,1), (1,0,1), (1,1,1),
 * where that node is in the lattice; an edge is ACTIVE iff exactly one of its ends is inside.
 * Vertices: one per active edge, numbered in ascending order of 7*n + d.  With a the owning node, b the far one, fa, fb
 * their values and pa, pb their positions:  t = (iso - fa) / (fb - fa);  x = pa + t * (pb - pa) per axis.
 * Normals: at a node g_a = field[index_a + 1] - field[index_a - 1] on each axis a, both indices clamped into the
 * lattice;  G = ga + t * (gb - ga) per axis;  len = sqrtf((Gx*Gx + Gy*Gy) + Gz*Gz);  normal = (-Gx/len, -Gy/len,
 * -Gz/len), outward (towards lower values), and (0,0,0) for len == 0.
 * Cells: addressed by their base node, whose id is the cell's id.  The six tetrahedra come from the permutations of the
 * axes in the order xyz, xzy, yxz, yzx, zxy, zyx: for a permutation pi the path v0 = base, v1 = v0 + e_pi1,
 * v2 = v1 + e_pi2, v3 = v2 + e_pi3.  All six share the cube's main diagonal, and every edge (va, vb), a < b, of a
 * tetrahedron is the edge of direction vb - va of the node va.
 * Triangles of a tetrahedron, by the inside flags of v0..v3:
 *     one corner s alone on its side (one inside or one outside): one triangle on the three edges at s, the other
 *     corners in ascending path position;
 *     two inside a < b, two outside c < d (path positions): (ac, ad, bd) and (ac, bd, bc).
 * Winding: every triangle's geometric normal points from the inside corners to the outside corners.  Whether the listed
 * order is kept or its last two vertices are exchanged is a table of 16 cases x 6 tetrahedra that the host GENERATES in
 * exact integer arithmetic: every edge vertex at its midpoint in doubled lattice coordinates, the sign of
 * (q-p) x (r-p) . (sum of the outside corners - sum of the inside corners).  No tetrahedron is degenerate, so the sign
 * does not depend on t in (0,1).
 * Faces: in ascending order of (cell id, tetrahedron, triangle), int32 vertex numbers.  Zero-area triangles occur where
 * t is 0 (a value equal to iso) and are kept: the surface stays closed with them.  Where every boundary node of the
 * lattice is outside, the mesh is a closed, consistently oriented 2-manifold (the Kuhn split is invariant under
 * translation and compatible across cube faces).
 * Non-finite values are the caller's business: they may give non-finite vertices, never an index out of range, since
 * every index depends on the values only through the inside flags.
 *
 * tpg_iso_count_f32: per node the 7-bit mask of its active edges and per cell its number of triangles (0..12) into ws,
 * their exclusive prefix sums over the G = nx*ny*nz ids, the totals [V, F] into counts (device, int64).
 * tpg_iso_emit_f32: reads what tpg_iso_count_f32 left in ws for the same field, dimensions and iso and writes vertices
 * (V,3), normals (V,3) or NULL, faces (F,3); nothing is written at or beyond V_cap vertices / F_cap faces (a short
 * buffer is truncated, never overrun).  The same bits, order included, on every run.
 *
 * Checks, all before anything is launched.  TPG_ERR_ARG: a negative dimension or cap, iso not finite, step not positive
 * and finite, a NULL counts / origin or an origin that is not finite, NULL vertices with V_cap > 0 or NULL faces with
 * F_cap > 0, a workspace that is NULL or not 256-byte aligned (when every dimension is >= 2).  Then a dimension below 2
 * (no cells): TPG_OK with V = F = 0, nothing else written.  Then G > 2^27: TPG_ERR_UNSUPPORTED; a NULL field:
 * TPG_ERR_ARG.  ws: tpg_iso_workspace_bytes(nx, ny, nz) bytes (0 where there are no cells or G > 2^27). */
size_t tpg_iso_workspace_bytes(int nx, int ny, int nz);
int tpg_iso_count_f32(const float *field, int nx, int ny, int nz, float iso, void *ws, int64_t *counts, void *stream);
int tpg_iso_emit_f32(const float *field, int nx, int ny, int nz, const float *origin, float step, float iso,
                     const void *ws, long long V_cap, long long F_cap, float *vertices, float *normals, int32_t *faces,
                     void *stream);

/* ---- anisotropic kernels (csrc/aniso.hip) -------------------------------------------------------------------------
 * The density field of tpgan_amd.mesh with one ellipsoidal kernel per particle, fitted to the particle's neighbourhood
 * (Yu and Turk, "Reconstructing surfaces of particle-based fluids using anisotropic kernels"), in place of one ball per
 * particle: flat regions come out flat and thin sheets stay sheets.  (The reference hands its frames to an external
 * tool for this; the mesher is this project's own and no parity with any such tool is claimed.)  Two stages.
 *
 * Parameters, each an fp32 value: rc (neighbourhood radius), lambda in [0,1] (centre smoothing), ks (scale of the
 * extents), kr >= 1 (largest ratio between a particle's extents), 0 < s_min <= s_max (clamp on the extents), kn (extent
 * of a particle with few neighbours), n_eps >= 0 (the count at or below which kn applies), R (support of the density
 * kernel), reach (= fp32(s_max) * fp32(R) as the Python layer calls it).  The host layer's defaults: rc = 2 R,
 * lambda = 0.9, kr = 4, s_min = 0.125, s_max = 2, kn = 0.5, n_eps = 25, ks = 1 / (the per-axis weighted variance, in
 * units of rc^2, of a full cubic lattice of the particles' spacing: mesh.lattice_covariance), which makes the kernel of
 * a particle inside a full lattice the isotropic one.
 *
 * Stage A, tpg_aniso_kernels_f32.  pos (B,N,3) f32, lengths (B) int64 or NULL, taken as min(max(lengths[b], 0), N) on
 * the 64-bit value.  Per particle i < lengths[b] of cloud b:
 *   members   the rows j < lengths[b] with d2 <= rc*rc (fp32 product), INCLUSIVE, i itself included, d2 the canonical
 *             fp32 distance of the searches: t = x_i - x_j per axis; d2 = t0*t0; d2 = d2 + t1*t1; d2 = d2 + t2*t2
 *             (a non-finite coordinate makes d2 NaN: no member)
 *   per member, fp32, each operation rounded on its own (no FMA):
 *             d = sqrtf(d2);  rho = fminf(d / rc, 1);  w = 1 - (rho*rho)*rho;  u_a = (x_j[a] - x_i[a]) / rc;
 *             wu_a = w*u_a;  the ten terms  w | wu_x, wu_y, wu_z | wu_x*u_x, wu_x*u_y, wu_x*u_z, wu_y*u_y, wu_y*u_z,
 *             wu_z*u_z,  each within [-1, 1], each converted on its own as (int64)(term * 2^32) (truncation towards
 *             zero, the scaling is exact) and added as integers: S0 | S1_a | S2_ab.  n_i = the number of members.
 *             Integer sums do not depend on the order of the members, the lane, the batch position or the launch shape.
 *   finish, float64 (+ - * / sqrt and comparisons only; each int64 sum converted to float64 once):
 *             m_a = S1_a / S0;  C_ab = S2_ab / S0 - m_a*m_b   (a <= b; n_i = 0, which only a non-finite x_i gives,
 *             has S0 = 0: m and C are 0 then)
 *             centre_i[a] = (float)((double)x_i[a] + (lambda*rc) * m_a),  lambda*rc the exact float64 product of the
 *             two fp32 parameters
 *   eigen-decomposition of C: A = C, V = I, then 5 sweeps of the rotations (p,q) = (0,1), (0,2), (1,2), r the third
 *             index, every rotation with the values the one before left:
 *                 zero = (A_pq == 0);  theta = (A_qq - A_pp) / (zero ? 1 : 2*A_pq);  sg = theta >= 0 ? 1 : -1
 *                 t = sg / (|theta| + sqrt(theta*theta + 1));  t = zero ? 0 : t       (an overflowing theta gives t = 0)
 *                 c = 1 / sqrt(t*t + 1);  s = t*c;  h = t*A_pq
 *                 A_pp = A_pp - h;  A_qq = A_qq + h;  A_pq = 0
 *                 (A_rp, A_rq) = (c*A_rp - s*A_rq,  s*A_rp + c*A_rq)
 *                 (V_kp, V_kq) = (c*V_kp - s*V_kq,  s*V_kp + c*V_kq)      for k = 0, 1, 2
 *             A zero off-diagonal element gives the identity rotation (c = 1, s = 0), carried out like any other.
 *             sigma_k = A_kk, its eigenvector the column k of V.  With S0 > 0 every quantity is a quotient or a bounded
 *             combination of finite numbers: nothing non-finite can arise, and S0 = 0 takes the kn branch below.
 *   extents   top = max(max(sigma_0, sigma_1), sigma_2) (a > b ? a : b).  If n_i <= n_eps or not top > 0:
 *             G_i = diag(1 / kn), det_i = 1 / ((kn*kn)*kn).  Otherwise
 *                 e_k = max(sigma_k, top / kr);  e_k = ks*e_k;  e_k = e_k < s_min ? s_min : e_k;
 *                 e_k = e_k > s_max ? s_max : e_k;  inv_k = 1 / e_k
 *                 G_ab = ((V_a0*inv_0)*V_b0 + (V_a1*inv_1)*V_b1) + (V_a2*inv_2)*V_b2;  det = 1 / ((e_0*e_1)*e_2)
 *   outputs   centres (B,N,3) f32, G (B,N,6) f32 in the order xx, xy, xz, yy, yz, zz, det (B,N) f32 (each the float64
 *             value rounded once), count (B,N) int32 = n_i.  Rows at or beyond lengths[b] get zeros in all four.
 * Launches: the walk (one wave per particle, the ten sums into ws) and the finish (one lane per particle); `stages`
 * selects them: 1 the walk, 2 the finish of the sums an earlier walk with the same B, N left in ws, 3 both (what the
 * host layer calls; 1 and 2 exist so that a timing can tell them apart).  tpg_aniso_kernels_exhaustive_f32: the same with
 * the lanes striding over the whole cloud instead of the uniform grid; the same bits.
 *
 * Stage B, tpg_aniso_field_f32.  query (B,Nq,3), centres (B,Np,3), G (B,Np,6), det (B,Np), lenq, lenp as above.  Per
 * query x < lenq[b] (others get 0):
 *   members   the centres j < lenp[b] with canonical fp32 |x - c_j|^2 <= reach*reach (t = x - c_j), inclusive
 *   per member, fp32, no FMA:
 *             t = x - c_j;  y_0 = (Gxx*t0 + Gxy*t1) + Gxz*t2;  y_1 = (Gxy*t0 + Gyy*t1) + Gyz*t2;
 *             y_2 = (Gxz*t0 + Gyz*t1) + Gzz*t2;  q = fminf(sqrtf((y_0*y_0 + y_1*y_1) + y_2*y_2) / R, 1)
 *             W = q <= 0.5 ? 6*((q*q)*q - q*q) + 1 : 2*((v*v)*v) with v = 1 - q; W = fmaxf(W, 0)   (the cubic of
 *             tpg_radius_reduce_f32: exactly 0 at q = 1)
 *             dw = fminf(fmaxf(det_j * W, 0), 512);  term = (uint64)(dw * 2^22)
 *   result    (float)(sum of the terms) * 2^-22.
 * Overflow: stage A's det is at most s_min^-3 (512 at the default 0.125) and the clamp holds for any det (a NaN det
 * or G gives dw = 0 or q = 1): a term is at most 2^31 units, and fewer than 2^31 of them cannot overflow 64 bits.
 * Membership at the rim does not matter: |G t| >= |t| / s_max, so the ellipsoid q < 1 lies inside the reach ball, and
 * the term vanishes at the ellipsoid's rim; both launch shapes apply the same test and return the same bits.
 * tpg_aniso_field_f32 builds the uniform grid over the centres with radius reach in ws (a second build: stage A's is
 * over the particles, with rc); tpg_aniso_field_exhaustive_f32 needs no workspace.
 *
 * Checks, all before anything is launched.  TPG_ERR_ARG: a negative B, N, Nq or Np; rc, ks, s_min, s_max, kn, R or reach
 * not positive and finite; kr not finite or below 1; lambda outside [0,1]; s_min > s_max; n_eps < 0; stages outside
 * 1..3; a NULL output; a workspace that is NULL or not 256-byte aligned where one is taken and no size is 0.  Then a
 * size of 0 among B, N / B, Nq: TPG_OK, nothing written.  Then B > 65535: TPG_ERR_UNSUPPORTED; a NULL pos / query:
 * TPG_ERR_ARG; Np == 0: zeros, TPG_OK; NULL centres, G or det: TPG_ERR_ARG.  ws: tpg_aniso_workspace_bytes(B, N) bytes
 * (stage B: of B, Np; it uses the grid's part). */
size_t tpg_aniso_workspace_bytes(int B, int N);
int tpg_aniso_kernels_f32(const float *pos, const int64_t *lengths, int B, int N, float rc, float lambda, float ks,
                          float kr, float s_min, float s_max, float kn, int n_eps, int stages, float *centres, float *G,
                          float *det, int32_t *count, void *ws, void *stream);
int tpg_aniso_kernels_exhaustive_f32(const float *pos, const int64_t *lengths, int B, int N, float rc, float lambda,
                                     float ks, float kr, float s_min, float s_max, float kn, int n_eps, int stages,
                                     float *centres, float *G, float *det, int32_t *count, void *ws, void *stream);
int tpg_aniso_field_f32(const float *query, const float *centres, const float *G, const float *det, const int64_t *lenq,
                        const int64_t *lenp, int B, int Nq, int Np, float support, float reach, float *sum, void *ws,
                        void *stream);
int tpg_aniso_field_exhaustive_f32(const float *query, const float *centres, const float *G, const float *det,
                                   const int64_t *lenq, const int64_t *lenp, int B, int Nq, int Np, float support,
                                   float reach, float *sum, void *stream);

/* ---- signed distance to a triangle mesh (csrc/mesh_sdf.hip) -------------------------------------------------------
 * query (Q,3) f32, vertices (V,3) f32, faces (F,3) int32 -> dist (Q) f32, negative inside, and face (Q) int32, the
 * nearest triangle.  Brute force over all triangles; no acceleration structure.  box: 6 HOST floats, lo xyz then hi xyz
 * of the vertices' bounding box; inv_unit: 1 / unit, unit a power of two with unit >= (largest extent of the box) / 2^16
 * (ops.mesh_sdf computes both from the vertices; the smallest such unit, 1 for a box of no extent).
 * Every vertex index is clamped into [0, V-1] before use (faces are device values the entry cannot check).
 *
 * Skipped triangles.  With u = b - a, v = c - a per axis in fp32, a triangle whose fp32 normal
 * (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx) is exactly (0, 0, 0) is skipped, for the magnitude and for the sign.
 *
 * Magnitude.  fp32, each operation rounded on its own (no FMA), only + - * / and sqrtf; comparisons and selections are
 * exact; dot(s, t) = (sx*tx + sy*ty) + sz*tz.  Per triangle (a, b, c) and query p, the closest point in region form:
 *     ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c
 *     d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
 *     vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4, e43 = d4 - d3, e56 = d5 - d6
 *   the closest point is a + v*ab + w*ac with (v, w) from the FIRST of these that holds:
 *     vertex a   d1 <= 0 and d2 <= 0                      (0, 0)
 *     vertex b   d3 >= 0 and d4 <= d3                     (1, 0)
 *     edge ab    vc <= 0 and d1 >= 0 and d3 <= 0          (d1 / (d1 - d3), 0)
 *     vertex c   d6 >= 0 and d5 <= d6                     (0, 1)
 *     edge ac    vb <= 0 and d2 >= 0 and d6 <= 0          (0, d2 / (d2 - d6))
 *     edge bc    va <= 0 and e43 >= 0 and e56 >= 0        t = e43 / (e43 + e56): (1 - t, t)
 *     face       otherwise                                s = (va + vb) + vc: (vb / s, vc / s)
 *   r_k = ap_k - (v*ab_k + w*ac_k) per axis;  dd = (rx*rx + ry*ry) + rz*rz.
 * The result takes the smallest dd over the triangles that are not skipped, ties to the LOWEST face index (a NaN dd is
 * never smaller), and dist = sqrtf(dd) once.  A (value, index) minimum does not depend on the order of execution: the
 * same bits for any tiling.  No such triangle (all skipped, or every dd NaN): dist = +inf, face = -1.
 *
 * Sign, in exact integer arithmetic.  snap(x, axis) = floor((x - lo[axis]) * inv_unit + 0.5) in fp32, then clamped into
 * [0, 2^16] (NaN: 0; the clamp changes nothing when box is the vertices' box), converted to an integer.
 *   - A query is IN THE BOX iff lo <= p <= hi on every axis (a NaN coordinate is not); a query not in the box is outside.
 *   - Otherwise Q = snap(p) and, per triangle that is not skipped, A, B, C = snap of its corners.
 *     area = (By-Ay)*(Cz-Az) - (Bz-Az)*(Cy-Ay), the doubled area of the projection on the yz plane.  area == 0: the
 *     triangle counts nothing.  area < 0: B and C are exchanged (the integer corners only), so that area > 0 below.
 *     edge(U, V) = (Vy-Uy)*(Qz-Uz) - (Vz-Uz)*(Qy-Uy) for the edges (B,C), (C,A), (A,B).  The projection COVERS the query
 *     iff for each edge:  edge > 0,  or edge == 0 and the edge owns its points: Vy-Uy > 0, or Vy-Uy == 0 and Vz-Uz > 0
 *     (a half-open rule: of two triangles on opposite sides of a shared edge exactly one owns a point on it, two on the
 *     same side both or neither; it is the coverage of the query moved by an infinitesimal (-eps^2, +eps) in (y, z)).
 *     n = (B-A) x (C-A) in integers (nx = area);  det = (nx*(Qx-Ax) + ny*(Qy-Ay)) + nz*(Qz-Az).  The crossing lies strictly
 *     AHEAD of the query in +x iff det < 0.
 *     The triangle counts one iff it covers the query and lies ahead.  Coordinates are within [0, 2^16], so an edge
 *     function is below 2^33 and det below 6 * 2^48: 64-bit integers (or float64) are exact.
 *   - inside iff the count is odd;  dist = inside ? -sqrtf(dd) : sqrtf(dd).
 * The sign is that of the SNAPPED query against the SNAPPED mesh and is meaningful for a closed mesh (every edge shared
 * by two triangles; the orientation does not matter: parity).  Within about a unit of the surface it may differ from the
 * sign in real coordinates; a query exactly on the surface gets whatever the rule above gives.
 *
 * Launch: one thread per query, 256 per workgroup, the triangles staged through LDS in tiles of 256.  Checks, all before
 * the launch.  TPG_ERR_ARG: a NULL pointer, a negative Q, V or F, inv_unit not positive and finite, a box that is not
 * finite or has lo > hi on an axis.  Then Q == 0: TPG_OK, nothing written.  Then F == 0, V == 0, or Q, V or F above
 * 2^30: TPG_ERR_UNSUPPORTED. */
int tpg_mesh_sdf_f32(const float *query, const float *vertices, const int32_t *faces, int Q, int V, int F,
                     const float *box, float inv_unit, float *dist, int32_t *face, void *stream);

/* ---- mesh obstacles in the particle fluid simulator (csrc/pbf.hip) --------------------------------------------------
 * A static solid of any shape as a SAMPLED DISTANCE FIELD in the obstacle's own frame: a lattice of nx x ny x nz nodes,
 * node (i,j,k) at origin + (i,j,k) * step, its value (signed distance, negative inside) at fields[offset +
 * (i*ny + j)*nz + k].  One device buffer `fields` of fields_len floats holds every field; rows of any scene may share
 * one at different poses.  A scene has up to PBF_MAX_SDF_OBSTACLES = 4 rows in a DEVICE table (B,M,24) of 32-bit words:
 *     words 0..16   f32: kind (4.0f), cx, cy, cz, R00 .. R22 (row-major), ox, oy, oz (lattice origin), step
 *     words 17..19  int32: nx, ny, nz
 *     words 20..21  int64 (low word first): offset
 *     words 22..23  unused
 * The world position of a local point q is c + R q.  A row is SKIPPED unless ALL of these hold: kind == 4.0f; words
 * 1..16 finite (|v| <= FLT_MAX); step > 0; 2 <= nx, ny, nz <= PBF_SDF_MAX_DIM = 4096; offset >= 0; offset + nx*ny*nz <=
 * fields_len, evaluated in 64 bits as offset <= fields_len and nx*ny*nz <= fields_len - offset (nothing can wrap).  The
 * table sits on the device and is not checked by the entry; every address derived from a table value is checked in the
 * kernel before use, and the test is uniform over a workgroup.  (ops.pbf_sdf_obstacles validates on the host.)
 *
 * collide_sdf(p), per particle, the rows o = 0 .. M-1 IN INDEX ORDER, each on the position the one before left.  fp32,
 * only + - * / and sqrtf, each rounded on its own (no FMA); with a the particle radius:
 *   local frame   as collide: d = p - c;  q_k = (dx*R[0][k] + dy*R[1][k]) + dz*R[2][k]
 *   lattice       g_k = (q_k - o_k) / step.  Unless 0 <= g_k <= (float)(n_k - 1) on all three axes the particle keeps
 *                 its bits for this row (NaN included).
 *   cell          i_k = min((int)floor(g_k), n_k - 2);  t_k = g_k - (float)i_k  (in [0, 1]; 1 on the last face)
 *   trilinear     f_abc the value at node (ix+a, iy+b, iz+c):
 *                 x_bc = f_1bc - f_0bc;  c_bc = f_0bc + tx*x_bc                      (bc = 00, 10, 01, 11)
 *                 y_c = c_1c - c_0c;     c_c = c_0c + ty*y_c                         (c = 0, 1)
 *                 gz = c_1 - c_0;        phi = c_0 + tz*gz
 *   gradient      of the interpolant, in lattice units:
 *                 gx_c = x_0c + ty*(x_1c - x_0c);  gx = gx_0 + tz*(gx_1 - gx_0);  gy = y_0 + tz*(y_1 - y_0)
 *                 n2 = (gx*gx + gy*gy) + gz*gz
 *   moved         iff phi < a (STRICT) and 0 < n2 <= FLT_MAX (a zero gradient leaves the particle):
 *                 len = sqrtf(n2);  s = a - phi;  q_k = q_k + s*(g_k / len)     (g the gradient)
 *   back          only a particle that moved: p_k = c_k + ((R[k][0]*qx + R[k][1]*qy) + R[k][2]*qz); bit o of hit.
 *   at the end    the scene's box clamp, clamp(p, lo + a, hi - a), as collide.
 * In a substep it is applied where collide is (after predict and after every dp), behind collide when both are given.
 * Consequences: one Newton step on an interpolated field leaves a particle within the interpolation error of the skin
 * phi = a, not on it; a particle outside the lattice is not seen, so the lattice must reach a beyond the surface; the
 * thinness and wedge caveats of collide apply unchanged.
 *
 * tpg_pbf_collide_sdf_f32: p_out = collide_sdf(p); p_out may be p.  hit_out (B,N) int32 or NULL.  box: the HOST table of
 * tpg_pbf_predict_f32.  One thread per particle, scenes in chunks of 64 per launch.  Rows at or beyond lengths[b] (taken
 * as everywhere: min(max(lengths[b], 0), N)) are never read and never written.  Checks, all before anything is launched.
 * TPG_ERR_ARG: negative B, N, M or fields_len, a not positive and finite, a NULL p_out.  Then B == 0 or N == 0: TPG_OK.
 * Then B > 65535, N > 2^22 or M > PBF_MAX_SDF_OBSTACLES: TPG_ERR_UNSUPPORTED.  Then a NULL p or box, a bad box, a NULL
 * table with M > 0, NULL fields with fields_len > 0: TPG_ERR_ARG.  M == 0 applies the clamp alone. */
#define PBF_MAX_SDF_OBSTACLES 4
#define PBF_SDF_MAX_DIM 4096
int tpg_pbf_collide_sdf_f32(const float *p, const int64_t *lengths, const float *box, const float *table,
                            const float *fields, long long fields_len, int B, int N, int M, float a, float *p_out,
                            int32_t *hit_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TPGAN_OPS_H */
