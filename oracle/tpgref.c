/*
 * oracle/tpgref.c -- CPU restatement of the TPU-GAN neighbourhood ops.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product path:
 * only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * this library, and only as the checker / reported CPU baseline.
 *
 * PARITY UNPINNED at op level: the arithmetic restated here lives upstream in
 * four un-vendored, un-pinned third-party CUDA packages named only in
 * /root/reference/README.md:5-8 (pointnet2_ops, pytorch3d, FRNN, chamferdist).
 * None of them is present in the build container and the reference holds no
 * tests, fixtures or golden vectors for them.  The
 * semantics below are therefore the published algorithms restated from their
 * documented behaviour and anchored on the reference's own call sites; the
 * tie/ordering rules that upstream leaves undefined are fixed here ("canonical
 * rules") and the HIP kernels are held bit-exact to THIS
 * file.  Model-level parity (reference Python running over these ops) is
 * pinned separately by tests/golden/.
 *
 * Canonical arithmetic (both here and in the csrc HIP sources, compiled -ffp-contract=off):
 *   sqdist(a,b,D) = sum_d (a_d - b_d)^2, accumulated in d order, every
 *   operation rounded to fp32, no FMA.
 *   neighbour order = ascending lexicographic (dist, idx).
 *
 * Build: gcc -O2 -fopenmp -ffp-contract=off -fno-fast-math -shared -fPIC
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TPG_OK 0
#define TPG_ERR_ARG (-1)
#define TPG_ERR_UNSUPPORTED (-3)

/* the neighbour order on distances: a before b.  A NaN distance ranks after every other (as its bits do in
 * the kernels' unsigned (dist_bits << 32 | idx) keys), NaN among themselves by index like any tie. */
static inline int dist_before(float a, float b) { return a < b || (b != b && a == a); }

static inline float sqdist(const float *a, const float *b, int D) {
    float acc = 0.0f;
    for (int d = 0; d < D; ++d) {
        float t = a[d] - b[d];
        float tt = t * t;
        acc = acc + tt;
    }
    return acc;
}

/* ------------------------------------------------------------------------ */
/* kNN / fixed-radius NN.                                                    */
/* Replaces pytorch3d.ops.knn_points  (gcn_lib/pointnet/gcn.py:16-21,38;      */
/*          discriminator.py:15,33) and frnn.frnn_grid_points                 */
/*          (discriminator.py:27-32; loss.py:256-265).                        */
/* r2 < 0  : plain kNN; slots beyond len2 get dist 0 / idx 0 (pytorch3d pad). */
/* r2 >= 0 : keep only d < r2 (strict); unfilled slots dist -1 / idx -1.      */
/* Rows of p1 beyond len1 are written as the pad value of the mode.           */
/* ------------------------------------------------------------------------ */
int tpgref_knn_f32(const float *p1, const float *p2, const int64_t *len1,
                   const int64_t *len2, int B, int P1, int P2, int D, int K,
                   float r2, float *dist, int64_t *idx) {
    if (B < 0 || P1 < 0 || P2 < 0 || D <= 0 || K <= 0) return TPG_ERR_ARG;
    const int radius = r2 >= 0.0f;
    const float pad_d = radius ? -1.0f : 0.0f;
    const int64_t pad_i = radius ? -1 : 0;
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < P1; ++i) {
            float *od = dist + ((size_t)b * P1 + i) * K;
            int64_t *oi = idx + ((size_t)b * P1 + i) * K;
            for (int k = 0; k < K; ++k) { od[k] = pad_d; oi[k] = pad_i; }
            const int n1 = len1 ? (int)len1[b] : P1;
            const int n2 = len2 ? (int)len2[b] : P2;
            if (i >= n1) continue;
            const float *q = p1 + ((size_t)b * P1 + i) * D;
            int cnt = 0; /* sorted prefix od[0..cnt) */
            for (int j = 0; j < n2; ++j) {
                const float d = sqdist(q, p2 + ((size_t)b * P2 + j) * D, D);
                if (radius && !(d < r2)) continue;
                if (cnt == K && !dist_before(d, od[K - 1])) continue; /* ties keep lower idx */
                int pos = cnt < K ? cnt : K - 1;
                while (pos > 0 && dist_before(d, od[pos - 1])) { /* strict: equal stays behind */
                    od[pos] = od[pos - 1]; oi[pos] = oi[pos - 1]; --pos;
                }
                od[pos] = d; oi[pos] = j;
                if (cnt < K) ++cnt;
            }
        }
    }
    return TPG_OK;
}

/* ------------------------------------------------------------------------ */
/* Chamfer nearest-neighbour search, both directions.                        */
/* Replaces chamferdist.ChamferDistance (loss.py:125-127,176-181).           */
/* d1[b,i] = min_j |s_i - t_j|^2, i1 = arg-min (lowest j on ties); d2/i2     */
/* the same from t to s.                                                      */
/* ------------------------------------------------------------------------ */
int tpgref_chamfer_fwd_f32(const float *src, const float *tgt, int B, int N,
                           int M, float *d1, int64_t *i1, float *d2, int64_t *i2) {
    if (B < 0 || N <= 0 || M <= 0) return TPG_ERR_ARG;
    int rc = tpgref_knn_f32(src, tgt, NULL, NULL, B, N, M, 3, 1, -1.0f, d1, i1);
    if (rc) return rc;
    return tpgref_knn_f32(tgt, src, NULL, NULL, B, M, N, 3, 1, -1.0f, d2, i2);
}

/* grad wrt both clouds given upstream grads of d1 (B,N) and d2 (B,M).       */
/* Deterministic order: direct term first, then scatter terms in index order. */
int tpgref_chamfer_bwd_f32(const float *src, const float *tgt, int B, int N, int M,
                           const int64_t *i1, const int64_t *i2, const float *g1,
                           const float *g2, float *gsrc, float *gtgt) {
    if (B < 0 || N <= 0 || M <= 0) return TPG_ERR_ARG;
    memset(gsrc, 0, sizeof(float) * (size_t)B * N * 3);
    memset(gtgt, 0, sizeof(float) * (size_t)B * M * 3);
#pragma omp parallel for schedule(static)
    for (int b = 0; b < B; ++b) {
        const float *s = src + (size_t)b * N * 3, *t = tgt + (size_t)b * M * 3;
        float *gs = gsrc + (size_t)b * N * 3, *gt = gtgt + (size_t)b * M * 3;
        for (int i = 0; i < N; ++i) {
            const int64_t j = i1[(size_t)b * N + i];
            const float g = 2.0f * g1[(size_t)b * N + i];
            for (int c = 0; c < 3; ++c) {
                const float v = g * (s[i * 3 + c] - t[j * 3 + c]);
                gs[i * 3 + c] += v; gt[j * 3 + c] -= v;
            }
        }
        for (int j = 0; j < M; ++j) {
            const int64_t i = i2[(size_t)b * M + j];
            const float g = 2.0f * g2[(size_t)b * M + j];
            for (int c = 0; c < 3; ++c) {
                const float v = g * (t[j * 3 + c] - s[i * 3 + c]);
                gt[j * 3 + c] += v; gs[i * 3 + c] -= v;
            }
        }
    }
    return TPG_OK;
}

/* ------------------------------------------------------------------------ */
/* Furthest point sampling.  Replaces pointnet2_utils.furthest_point_sample  */
/* (discriminator.py:114).  idx[0]=0, temp=1e10, points with |x|^2 <= 1e-3    */
/* are never updated nor eligible; arg-max ties -> smallest index (canonical */
/* deviation from upstream's block-size dependent tree order).    */
/* temp is caller-provided scratch (B,N).                                    */
/* ------------------------------------------------------------------------ */
int tpgref_fps_start_f32(const float *xyz, const int32_t *start, int skip_origin, int B, int N, int m,
                         float *temp, int32_t *idx);
int tpgref_fps_f32(const float *xyz, int B, int N, int m, float *temp, int32_t *idx) {
    return tpgref_fps_start_f32(xyz, NULL, 1, B, N, m, temp, idx);
}

/* start (B) = first pick per cloud (NULL: 0); skip_origin = 0: every point eligible -- the  */
/* dataset-side sampler, sampling.py:50-106 (squared distances, numpy argmax = first maximum) */
int tpgref_fps_start_f32(const float *xyz, const int32_t *start, int skip_origin, int B, int N, int m,
                         float *temp, int32_t *idx) {
    if (B < 0 || N <= 0 || m <= 0) return TPG_ERR_ARG;
#pragma omp parallel for schedule(static)
    for (int b = 0; b < B; ++b) {
        const float *x = xyz + (size_t)b * N * 3;
        float *tp = temp + (size_t)b * N;
        int32_t *o = idx + (size_t)b * m;
        for (int k = 0; k < N; ++k) tp[k] = 1e10f;
        int old = start ? (start[b] < 0 ? 0 : (start[b] >= N ? N - 1 : start[b])) : 0;
        o[0] = old;
        for (int j = 1; j < m; ++j) {
            int besti = 0;
            float best = -1.0f;
            const float *xo = x + (size_t)old * 3;
            for (int k = 0; k < N; ++k) {
                const float *xk = x + (size_t)k * 3;
                float mag = xk[0] * xk[0];
                mag = mag + xk[1] * xk[1];
                mag = mag + xk[2] * xk[2];
                if (skip_origin && mag <= 1e-3f) continue;
                const float d = sqdist(xk, xo, 3);
                const float d2 = d < tp[k] ? d : tp[k];
                tp[k] = d2;
                if (d2 > best) { best = d2; besti = k; }
            }
            old = besti;
            o[j] = old;
        }
    }
    return TPG_OK;
}

/* ------------------------------------------------------------------------ */
/* gather_operation fwd/bwd (discriminator.py:131-137).                      */
/* ------------------------------------------------------------------------ */
int tpgref_gather_fwd_f32(const float *feat, const int32_t *idx, int B, int C,
                          int N, int S, float *out) {
    if (B < 0 || C < 0 || N <= 0 || S < 0) return TPG_ERR_ARG;
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
            for (int s = 0; s < S; ++s)
                out[((size_t)b * C + c) * S + s] =
                    feat[((size_t)b * C + c) * N + idx[(size_t)b * S + s]];
    return TPG_OK;
}

int tpgref_gather_bwd_f32(const float *gout, const int32_t *idx, int B, int C,
                          int N, int S, float *gfeat) {
    if (B < 0 || C < 0 || N <= 0 || S < 0) return TPG_ERR_ARG;
    memset(gfeat, 0, sizeof(float) * (size_t)B * C * N);
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
            for (int s = 0; s < S; ++s)
                gfeat[((size_t)b * C + c) * N + idx[(size_t)b * S + s]] +=
                    gout[((size_t)b * C + c) * S + s];
    return TPG_OK;
}

/* ------------------------------------------------------------------------ */
/* ball_query (inside QueryAndGroup, discriminator.py:190).  Scan k in index */
/* order, keep the first nsample with d < r^2; first hit pre-fills the row;   */
/* no hit leaves the row at 0.                                                */
/* ------------------------------------------------------------------------ */
int tpgref_ball_query_f32(const float *xyz, const float *new_xyz, int B, int N,
                          int S, float radius, int nsample, int32_t *idx) {
    if (B < 0 || N <= 0 || S < 0 || nsample <= 0) return TPG_ERR_ARG;
    const float r2 = radius * radius;
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b) {
        for (int s = 0; s < S; ++s) {
            int32_t *o = idx + ((size_t)b * S + s) * nsample;
            for (int l = 0; l < nsample; ++l) o[l] = 0;
            const float *q = new_xyz + ((size_t)b * S + s) * 3;
            int cnt = 0;
            for (int k = 0; k < N && cnt < nsample; ++k) {
                const float d = sqdist(q, xyz + ((size_t)b * N + k) * 3, 3);
                if (d < r2) {
                    if (cnt == 0)
                        for (int l = 0; l < nsample; ++l) o[l] = k;
                    o[cnt] = k;
                    ++cnt;
                }
            }
        }
    }
    return TPG_OK;
}

/* ------------------------------------------------------------------------ */
/* grouping_operation fwd/bwd (gcn_lib/pointnet/gcn.py:207,261;              */
/* discriminator.py:270,273).  bwd sums in (s,k) order.                       */
/* ------------------------------------------------------------------------ */
int tpgref_group_fwd_f32(const float *feat, const int32_t *idx, int B, int C,
                         int N, int S, int K, float *out) {
    if (B < 0 || C < 0 || N <= 0 || S < 0 || K < 0) return TPG_ERR_ARG;
    const size_t SK = (size_t)S * K;
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            const float *f = feat + ((size_t)b * C + c) * N;
            const int32_t *id = idx + (size_t)b * SK;
            float *o = out + ((size_t)b * C + c) * SK;
            for (size_t e = 0; e < SK; ++e) o[e] = f[id[e]];
        }
    return TPG_OK;
}

int tpgref_group_bwd_f32(const float *gout, const int32_t *idx, int B, int C,
                         int N, int S, int K, float *gfeat) {
    if (B < 0 || C < 0 || N <= 0 || S < 0 || K < 0) return TPG_ERR_ARG;
    const size_t SK = (size_t)S * K;
    memset(gfeat, 0, sizeof(float) * (size_t)B * C * N);
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            float *g = gfeat + ((size_t)b * C + c) * N;
            const int32_t *id = idx + (size_t)b * SK;
            const float *o = gout + ((size_t)b * C + c) * SK;
            for (size_t e = 0; e < SK; ++e) g[id[e]] += o[e];
        }
    return TPG_OK;
}

/* ------------------------------------------------------------------------ */
/* three_nn / three_interpolate (no call sites in the reference; exported     */
/* for pointnet2_utils API completeness).  three_nn returns SQUARED distance  */
/* here; the Python layer applies sqrt like upstream's wrapper.               */
/* ------------------------------------------------------------------------ */
int tpgref_three_nn_f32(const float *unknown, const float *known, int B, int n,
                        int m, float *dist2, int32_t *idx) {
    if (B < 0 || n < 0 || m <= 0) return TPG_ERR_ARG;
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < n; ++i) {
            const float *q = unknown + ((size_t)b * n + i) * 3;
            float bd[3] = {INFINITY, INFINITY, INFINITY};
            int32_t bi[3] = {0, 0, 0};
            for (int k = 0; k < m; ++k) {
                const float d = sqdist(q, known + ((size_t)b * m + k) * 3, 3);
                if (d < bd[0]) {
                    bd[2] = bd[1]; bi[2] = bi[1]; bd[1] = bd[0]; bi[1] = bi[0];
                    bd[0] = d; bi[0] = k;
                } else if (d < bd[1]) {
                    bd[2] = bd[1]; bi[2] = bi[1]; bd[1] = d; bi[1] = k;
                } else if (d < bd[2]) {
                    bd[2] = d; bi[2] = k;
                }
            }
            for (int l = 0; l < 3; ++l) {
                dist2[((size_t)b * n + i) * 3 + l] = bd[l];
                idx[((size_t)b * n + i) * 3 + l] = bi[l];
            }
        }
    return TPG_OK;
}

int tpgref_three_interp_fwd_f32(const float *feat, const int32_t *idx,
                                const float *w, int B, int C, int m, int n,
                                float *out) {
    if (B < 0 || C < 0 || m <= 0 || n < 0) return TPG_ERR_ARG;
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            const float *f = feat + ((size_t)b * C + c) * m;
            for (int i = 0; i < n; ++i) {
                const int32_t *id = idx + ((size_t)b * n + i) * 3;
                const float *ww = w + ((size_t)b * n + i) * 3;
                float acc = ww[0] * f[id[0]];
                acc = acc + ww[1] * f[id[1]];
                acc = acc + ww[2] * f[id[2]];
                out[((size_t)b * C + c) * n + i] = acc;
            }
        }
    return TPG_OK;
}

int tpgref_three_interp_bwd_f32(const float *gout, const int32_t *idx,
                                const float *w, int B, int C, int m, int n,
                                float *gfeat) {
    if (B < 0 || C < 0 || m <= 0 || n < 0) return TPG_ERR_ARG;
    memset(gfeat, 0, sizeof(float) * (size_t)B * C * m);
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            float *g = gfeat + ((size_t)b * C + c) * m;
            for (int i = 0; i < n; ++i) {
                const int32_t *id = idx + ((size_t)b * n + i) * 3;
                const float *ww = w + ((size_t)b * n + i) * 3;
                const float go = gout[((size_t)b * C + c) * n + i];
                for (int l = 0; l < 3; ++l) g[id[l]] += go * ww[l];
            }
        }
    return TPG_OK;
}

/* ------------------------------------------------------------------------ */
/* Row combine (channels-last) -- restates the build's OWN fused form of      */
/* "group -> first 1x1 conv" (include/tpgan_ops.h, tpg_rowcombine_*).  The    */
/* reference computes conv(group(x)) (gcn_lib/pointnet/gcn.py:207-210,        */
/* discriminator.py:141-145,270-280); equality of the two forms up to fp32    */
/* rounding is pinned at model level by tests/golden/.  fp32 only; bf16 is     */
/* emulated in the tests by rounding inputs/outputs.                           */
/* ------------------------------------------------------------------------ */
static inline float lrelu(float d, float slope) { return d > 0.0f ? d : d * slope; }

int tpgref_rowcombine_fwd_f32(const float *U, const float *QE, const int32_t *idx, int mode, int B,
                              int N, int S, int K, int C, float slope, float *out) {
    if (B < 0 || N <= 0 || S < 0 || K < 0 || C <= 0 || mode < 0 || mode > 2) return TPG_ERR_ARG;
    if (mode == 2 && S != N) return TPG_ERR_ARG;
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < K; ++k) {
                const size_t row = ((size_t)b * S + s) * K + k;
                const int n = idx[row];
                const float *u = U + ((size_t)b * N + n) * C;
                float *o = out + row * C;
                for (int c = 0; c < C; ++c) {
                    if (mode == 0) o[c] = u[c];
                    else if (mode == 1) o[c] = u[c] - QE[((size_t)b * S + s) * C + c];
                    else {
                        const float d = QE[((size_t)b * N + n) * C + c] - QE[((size_t)b * S + s) * C + c];
                        o[c] = u[c] + lrelu(d, slope);
                    }
                }
            }
    return TPG_OK;
}

/* sums run in (s,k) order per destination; the HIP order is unspecified, so the kernels are judged per element
 * against the float64 twin: depth * 2^-24 * sum |term| (oracle/ref_ops.py rowcombine_bound, tests/rowgather_rule.py).
 * idx is NOT clamped here: callers pass indices inside [0, N). */
int tpgref_rowcombine_bwd_f32(const float *gout, const int32_t *idx, const float *E, int mode, int B,
                              int N, int S, int K, int C, float slope, float *gU, float *gQE) {
    if (B < 0 || N <= 0 || S < 0 || K < 0 || C <= 0 || mode < 0 || mode > 2) return TPG_ERR_ARG;
    memset(gU, 0, sizeof(float) * (size_t)B * N * C);
    if (mode != 0) memset(gQE, 0, sizeof(float) * (size_t)B * S * C);
#pragma omp parallel for schedule(static)
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < K; ++k) {
                const size_t row = ((size_t)b * S + s) * K + k;
                const int n = idx[row];
                const float *g = gout + row * C;
                for (int c = 0; c < C; ++c) {
                    gU[((size_t)b * N + n) * C + c] += g[c];
                    if (mode == 1) gQE[((size_t)b * S + s) * C + c] -= g[c];
                    if (mode == 2) {
                        const float d = E[((size_t)b * N + n) * C + c] - E[((size_t)b * S + s) * C + c];
                        const float ge = d > 0.0f ? g[c] : g[c] * slope;
                        gQE[((size_t)b * N + n) * C + c] += ge;
                        gQE[((size_t)b * S + s) * C + c] -= ge;
                    }
                }
            }
    return TPG_OK;
}

/* ------------------------------------------------------------------------ */
/* Bicubic radius interpolation: gcn_lib/interpolation.py:107-123            */
/* (cubic_interpolation) over get_local_neighbor_graph :16-75, as called by  */
/* train_step_final.py:51-66.  See include/tpgan_ops.h for the reduction of  */
/* the DGL graph to per-query sums; sums here run sequentially over the      */
/* neighbours in ascending (d^2, idx) order.                                 */
/* ------------------------------------------------------------------------ */
static float bicubic_w(float r, float cutoff, float coeff) {
    const float q = r / cutoff;
    float ker = 0.0f;
    if (q >= 0.0f && q <= 0.5f) ker = 6.0f * (q * q * q - q * q) + 1.0f;
    else if (q > 0.5f && q <= 1.0f) { const float t = 1.0f - q; ker = 2.0f * (t * t * t); }
    return ker * coeff;
}

int tpgref_cubic_interp_f32(const float *query, const float *pos, const float *field, int B, int Nq,
                            int Np, int F, float cutoff, float *out_plain, float *out_pad,
                            int32_t *hits) {
    if (B < 0 || Nq < 0 || Np < 0 || F <= 0 || !(cutoff > 0.0f)) return TPG_ERR_ARG;
    enum { K = 32 };
    const float r2 = cutoff * cutoff;
    const float coeff = (float)(8.0 / (3.14159265358979323846 * (double)cutoff * (double)cutoff * (double)cutoff));
    const size_t nq = (size_t)B * Nq;
    float *dist = (float *)malloc(sizeof(float) * (nq * K + 1));
    int64_t *idx = (int64_t *)malloc(sizeof(int64_t) * (nq * K + 1));
    if (!dist || !idx) { free(dist); free(idx); return TPG_ERR_ARG; }
    int rc = tpgref_knn_f32(query, pos, NULL, NULL, B, Nq, Np, 3, K, r2, dist, idx);
    if (rc == TPG_OK) {
#pragma omp parallel for schedule(static)
        for (long long t = 0; t < (long long)nq; ++t) {
            const int b = (int)(t / Nq);
            const float *fb = field + (size_t)b * Np * F;
            int nh = 0;
            double den = 0.0, denp = 0.0;
            for (int f = 0; f < F; ++f) { out_plain[t * F + f] = 0.0f; out_pad[t * F + f] = 0.0f; }
            /* two passes keep the sums in double: the kernel's tree order differs anyway */
            double num[16], nump[16];
            const int FF = F < 16 ? F : 16;
            for (int f = 0; f < FF; ++f) { num[f] = 0.0; nump[f] = 0.0; }
            for (int k = 0; k < K; ++k) {
                const int64_t j = idx[t * K + k];
                if (j < 0) break;
                float d2 = dist[t * K + k];
                if (d2 < 1e-8f) d2 = 0.0f;
                const float w = bicubic_w(sqrtf(d2), cutoff, coeff);
                const float wp = k < 4 ? 2.0f * w : w;
                den += w; denp += wp;
                for (int f = 0; f < FF; ++f) {
                    num[f] += (double)(w * fb[(size_t)j * F + f]);
                    nump[f] += (double)(wp * fb[(size_t)j * F + f]);
                }
                ++nh;
            }
            for (int f = 0; f < FF; ++f) {
                out_plain[t * F + f] = (float)(num[f] / (den + 1e-6));
                out_pad[t * F + f] = (float)(nump[f] / (denp + 1e-6));
            }
            hits[t] = nh;
        }
    }
    free(dist); free(idx);
    return rc;
}
