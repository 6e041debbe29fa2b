// Anisotropic kernels for surface reconstruction (Yu and Turk, "Reconstructing surfaces of particle-based fluids using
// anisotropic kernels"): every particle gets a smoothed centre and an ellipsoidal kernel fitted to the weighted
// covariance of its neighbourhood (stage A), and the density field is the sum of those kernels (stage B).  The rule in
// full, operation by operation: include/tpgan_ops.h, "anisotropic kernels".  The mesher that uses it is this project's
// own (tpgan_amd.mesh); the reference hands its frames to an external reconstruction tool.
//
// Both stages follow radius_reduce.hip: one wave per particle / query, its candidates from fg_candidates of
// frnn_grid_build.hpp (the walk over the 27 cells of the uniform grid around it or, exhaustive shape, the lanes stride
// over the whole cloud), every sum in 64-bit fixed point with tpg_wave_add_u64 for the wave totals, so that the result
// does not depend on the order in which the grid hands out the neighbours nor on the launch shape.
//
// Stage A is TWO launches.  The walk leaves the ten sums of a particle in the workspace (ten planes of int64, one value
// per particle) and its member count in `count`; the finish takes ONE LANE per particle and runs the float64 part: the
// mean, the covariance, five Jacobi sweeps (15 rotations, each two divisions and two square roots deep: several hundred
// dependent operations) and the extents.  Behind the walk on lane 0 that chain would run with 63 lanes idle on every
// wave; as a launch of its own it fills every lane, costs 80 bytes of traffic per particle each way and no
// synchronisation but the stream's order.
//
// Stage B walks a grid built over the SMOOTHED centres with radius reach = s_max * support; the cell-sorted copy
// carries the source row in .w, which is where G and det of a member are gathered from (28 bytes, members only).
#include "frnn_grid_build.hpp"
#include "tpg_common.hpp"

namespace {

struct AnParams {
    float rc, lambda, ks, kr, s_min, s_max, kn;
    int n_eps;
};

__device__ __forceinline__ long long an_fix32(float term) { return (long long)(term * 4294967296.0f); }

// ---- stage A, the walk: sums[k][b*N + i], k = 0..9 (w | w u_x, w u_y, w u_z | xx, xy, xz, yy, yz, zz), count[b*N + i]
template <bool GRID>
__global__ __launch_bounds__(FG_WAVES * 64) void an_sums_kernel(
    const float *__restrict__ pos, const int64_t *__restrict__ lengths, int N, const GridParams *__restrict__ gp,
    int cstride, const int *__restrict__ start, const float4 *__restrict__ sorted, float rc, float rc2,
    long long *__restrict__ sums, int32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int i = blockIdx.x * FG_WAVES + wave;
    if (i >= N) return;
    const size_t q = (size_t)b * N + i;
    const size_t plane = (size_t)gridDim.y * N;
    const int n = fg_len(lengths, b, N);
    int cnt = 0;
    long long s[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) s[k] = 0;
    if (i < n) {
        const float qx = pos[q * 3], qy = pos[q * 3 + 1], qz = pos[q * 3 + 2];
        fg_candidates<GRID>(qx, qy, qz, gp, b, cstride, start, sorted, pos, n, N, lane,
                            [&](float px, float py, float pz, int) {
                                const float d2 = tpg_sq3(qx, qy, qz, px, py, pz);
                                if (d2 <= rc2) {
                                    ++cnt;
                                    const float d = sqrtf(d2);
                                    const float rho = fminf(d / rc, 1.0f);
                                    const float w = 1.0f - (rho * rho) * rho;
                                    const float ux = (px - qx) / rc, uy = (py - qy) / rc, uz = (pz - qz) / rc;
                                    const float wx = w * ux, wy = w * uy, wz = w * uz;
                                    s[0] += an_fix32(w);
                                    s[1] += an_fix32(wx);
                                    s[2] += an_fix32(wy);
                                    s[3] += an_fix32(wz);
                                    s[4] += an_fix32(wx * ux);
                                    s[5] += an_fix32(wx * uy);
                                    s[6] += an_fix32(wx * uz);
                                    s[7] += an_fix32(wy * uy);
                                    s[8] += an_fix32(wy * uz);
                                    s[9] += an_fix32(wz * uz);
                                }
                            });
    }
    // wave totals (the whole wave is here: every branch above is wave-uniform)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
#pragma unroll
    for (int k = 0; k < 10; ++k) s[k] = tpg_wave_add_u64(s[k]);
    if (lane == 0) {
        count[q] = cnt;
#pragma unroll
        for (int k = 0; k < 10; ++k) sums[(size_t)k * plane + q] = s[k];
    }
}

// one Jacobi rotation in the (p, q) plane of the symmetric matrix; r is the third index.  arp = A[r][p], arq = A[r][q];
// vXp / vXq the columns p and q of V.  A zero apq gives t = 0: the identity, carried out like any other rotation.
__device__ __forceinline__ void an_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                          double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
    const bool zero = apq == 0.0;
    const double theta = (aqq - app) / (zero ? 1.0 : 2.0 * apq);
    const double sg = theta >= 0.0 ? 1.0 : -1.0;
    double t = sg / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = zero ? 0.0 : t;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    double a = v0p, e = v0q;
    v0p = c * a - s * e;
    v0q = s * a + c * e;
    a = v1p, e = v1q;
    v1p = c * a - s * e;
    v1q = s * a + c * e;
    a = v2p, e = v2q;
    v2p = c * a - s * e;
    v2q = s * a + c * e;
}

// ---- stage A, the finish: one lane per particle, float64 from the integer sums
__global__ __launch_bounds__(256) void an_finish_kernel(const float *__restrict__ pos, const int64_t *__restrict__ lengths,
                                                        int N, const long long *__restrict__ sums,
                                                        const int32_t *__restrict__ count, AnParams prm,
                                                        float *__restrict__ centres, float *__restrict__ G,
                                                        float *__restrict__ det) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const size_t q = (size_t)b * N + i;
    const size_t plane = (size_t)gridDim.y * N;
    if (i >= fg_len(lengths, b, N)) {                      // not a particle: zeros (count is 0 from the walk)
#pragma unroll
        for (int a = 0; a < 3; ++a) centres[q * 3 + a] = 0.0f;
#pragma unroll
        for (int a = 0; a < 6; ++a) G[q * 6 + a] = 0.0f;
        det[q] = 0.0f;
        return;
    }
    double S[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) S[k] = (double)sums[(size_t)k * plane + q];
    const int n = count[q];
    const bool any = S[0] > 0.0;
    const double S0 = any ? S[0] : 1.0;
    const double mx = S[1] / S0, my = S[2] / S0, mz = S[3] / S0;        // all sums are 0 when S[0] is
    const double lr = (double)prm.lambda * (double)prm.rc;
    centres[q * 3] = (float)((double)pos[q * 3] + lr * mx);
    centres[q * 3 + 1] = (float)((double)pos[q * 3 + 1] + lr * my);
    centres[q * 3 + 2] = (float)((double)pos[q * 3 + 2] + lr * mz);
    double a00 = S[4] / S0 - mx * mx, a01 = S[5] / S0 - mx * my, a02 = S[6] / S0 - mx * mz;
    double a11 = S[7] / S0 - my * my, a12 = S[8] / S0 - my * mz, a22 = S[9] / S0 - mz * mz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < 5; ++sweep) {
        an_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0,1), r = 2
        an_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0,2), r = 1
        an_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1,2), r = 0
    }
    double top = a00 > a11 ? a00 : a11;
    top = top > a22 ? top : a22;
    float g[6], dt;
    if (n <= prm.n_eps || !(top > 0.0)) {
        const double kn = (double)prm.kn, inv = 1.0 / kn;
        g[0] = g[3] = g[5] = (float)inv;
        g[1] = g[2] = g[4] = 0.0f;
        dt = (float)(1.0 / ((kn * kn) * kn));
    } else {
        const double ks = (double)prm.ks, lo = (double)prm.s_min, hi = (double)prm.s_max;
        const double fl = top / (double)prm.kr;
        double e0 = a00 > fl ? a00 : fl, e1 = a11 > fl ? a11 : fl, e2 = a22 > fl ? a22 : fl;
        e0 = ks * e0, e1 = ks * e1, e2 = ks * e2;
        e0 = e0 < lo ? lo : e0, e1 = e1 < lo ? lo : e1, e2 = e2 < lo ? lo : e2;
        e0 = e0 > hi ? hi : e0, e1 = e1 > hi ? hi : e1, e2 = e2 > hi ? hi : e2;
        const double i0 = 1.0 / e0, i1 = 1.0 / e1, i2 = 1.0 / e2;
        g[0] = (float)(((v00 * i0) * v00 + (v01 * i1) * v01) + (v02 * i2) * v02);
        g[1] = (float)(((v00 * i0) * v10 + (v01 * i1) * v11) + (v02 * i2) * v12);
        g[2] = (float)(((v00 * i0) * v20 + (v01 * i1) * v21) + (v02 * i2) * v22);
        g[3] = (float)(((v10 * i0) * v10 + (v11 * i1) * v11) + (v12 * i2) * v12);
        g[4] = (float)(((v10 * i0) * v20 + (v11 * i1) * v21) + (v12 * i2) * v22);
        g[5] = (float)(((v20 * i0) * v20 + (v21 * i1) * v21) + (v22 * i2) * v22);
        dt = (float)(1.0 / ((e0 * e1) * e2));
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) G[q * 6 + a] = g[a];
    det[q] = dt;
}

// ---- stage B: sum[b][i] = sum over the centres within reach of det_j * W(|G_j (x - xbar_j)| / R)
template <bool GRID>
__global__ __launch_bounds__(FG_WAVES * 64) void an_field_kernel(
    const float *__restrict__ query, const float *__restrict__ centres, const float *__restrict__ G,
    const float *__restrict__ det, const int64_t *__restrict__ lenq, const int64_t *__restrict__ lenp, int Nq, int Np,
    const GridParams *__restrict__ gp, int cstride, const int *__restrict__ start, const float4 *__restrict__ sorted,
    float R, float reach2, float *__restrict__ sum) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int i = blockIdx.x * FG_WAVES + wave;
    if (i >= Nq) return;
    const size_t q = (size_t)b * Nq + i;
    tpg_u64 acc = 0;
    if (i < fg_len(lenq, b, Nq)) {
        const float qx = query[q * 3], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
        const float *Gb = G + (size_t)b * Np * 6, *db = det + (size_t)b * Np;
        fg_candidates<GRID>(qx, qy, qz, gp, b, cstride, start, sorted, centres, fg_len(lenp, b, Np), Np, lane,
                            [&](float px, float py, float pz, int j) {
                                if (!(tpg_sq3(qx, qy, qz, px, py, pz) <= reach2)) return;
                                const float *g = Gb + (size_t)j * 6;
                                const float t0 = qx - px, t1 = qy - py, t2 = qz - pz;
                                const float y0 = (g[0] * t0 + g[1] * t1) + g[2] * t2;
                                const float y1 = (g[1] * t0 + g[3] * t1) + g[4] * t2;
                                const float y2 = (g[2] * t0 + g[4] * t1) + g[5] * t2;
                                const float u = fminf(sqrtf((y0 * y0 + y1 * y1) + y2 * y2) / R, 1.0f);
                                const float w = tpg_cubic_spline_w(u);
                                // clamped into [0, 512] whatever det holds (NaN -> 0): a term is at most 2^31 units
                                const float dw = fminf(fmaxf(db[j] * w, 0.0f), 512.0f);
                                acc += (tpg_u64)(dw * 4194304.0f);
                            });
    }
    acc = tpg_wave_add_u64(acc);
    if (lane == 0) sum[q] = (float)acc * 2.384185791015625e-7f;
}

bool an_pos(float v) { return v > 0.0f && v <= 3.0e38f; }

size_t an_sums_bytes(int B, int N) { return align256(sizeof(long long) * 10 * (size_t)B * N); }

int an_kernels(bool grid, const float *pos, const int64_t *lengths, int B, int N, float rc, float lambda, float ks,
               float kr, float s_min, float s_max, float kn, int n_eps, int stages, float *centres, float *G, float *det,
               int32_t *count, void *ws, void *stream) {
    hipStream_t st = tpg_stream(stream);
    if (B < 0 || N < 0 || !an_pos(rc) || !an_pos(ks) || !an_pos(s_min) || !an_pos(s_max) || !an_pos(kn) ||
        !(kr >= 1.0f && kr <= 3.0e38f) || !(lambda >= 0.0f && lambda <= 1.0f) || s_min > s_max || n_eps < 0 ||
        stages < 1 || stages > 3 || !centres || !G || !det || !count)
        return TPG_ERR_ARG;
    if (B > 0 && N > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    if (B == 0 || N == 0) return TPG_OK;
    if (B > 65535) return TPG_ERR_UNSUPPORTED;            // clouds ride on gridDim.y
    if (!pos) return TPG_ERR_ARG;
    long long *sums = reinterpret_cast<long long *>(static_cast<unsigned char *>(ws) + fg_workspace_bytes(B, N));
    if (stages & 1) {
        if (grid) {
            GridView v;
            const int rcode = fg_build(pos, lengths, B, N, rc, 0, ws, st, &v);
            if (rcode) return rcode;
            hipLaunchKernelGGL(an_sums_kernel<true>, dim3(fg_query_blocks(N), B), dim3(FG_WAVES * 64), 0, st, pos,
                               lengths, N, v.gp, FG_CELLS, v.start, v.sorted, rc, rc * rc, sums, count);
        } else {
            hipLaunchKernelGGL(an_sums_kernel<false>, dim3(fg_query_blocks(N), B), dim3(FG_WAVES * 64), 0, st, pos,
                               lengths, N, (const GridParams *)nullptr, 0, (const int *)nullptr, (const float4 *)nullptr,
                               rc, rc * rc, sums, count);
        }
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    if (stages & 2) {
        const AnParams prm = {rc, lambda, ks, kr, s_min, s_max, kn, n_eps};
        hipLaunchKernelGGL(an_finish_kernel, dim3((N + 255) / 256, B), dim3(256), 0, st, pos, lengths, N, sums, count,
                           prm, centres, G, det);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}

int an_field(bool grid, const float *query, const float *centres, const float *G, const float *det, const int64_t *lenq,
             const int64_t *lenp, int B, int Nq, int Np, float support, float reach, float *sum, void *ws, void *stream) {
    hipStream_t st = tpg_stream(stream);
    if (B < 0 || Nq < 0 || Np < 0 || !an_pos(support) || !an_pos(reach) || !sum) return TPG_ERR_ARG;
    if (grid && B > 0 && Nq > 0 && Np > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    if (B == 0 || Nq == 0) return TPG_OK;
    if (B > 65535) return TPG_ERR_UNSUPPORTED;
    if (!query) return TPG_ERR_ARG;
    if (Np == 0)                                           // nothing stored: zeros
        return hipMemsetAsync(sum, 0, sizeof(float) * (size_t)B * Nq, st) == hipSuccess ? TPG_OK : TPG_ERR_LAUNCH;
    if (!centres || !G || !det) return TPG_ERR_ARG;
    if (grid) {
        GridView v;
        const int rcode = fg_build(centres, lenp, B, Np, reach, 0, ws, st, &v);
        if (rcode) return rcode;
        hipLaunchKernelGGL(an_field_kernel<true>, dim3(fg_query_blocks(Nq), B), dim3(FG_WAVES * 64), 0, st, query,
                           centres, G, det, lenq, lenp, Nq, Np, v.gp, FG_CELLS, v.start, v.sorted, support,
                           reach * reach, sum);
    } else {
        hipLaunchKernelGGL(an_field_kernel<false>, dim3(fg_query_blocks(Nq), B), dim3(FG_WAVES * 64), 0, st, query,
                           centres, G, det, lenq, lenp, Nq, Np, (const GridParams *)nullptr, 0, (const int *)nullptr,
                           (const float4 *)nullptr, support, reach * reach, sum);
    }
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

}  // namespace

extern "C" size_t tpg_aniso_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return fg_workspace_bytes(B, N) + an_sums_bytes(B, N);
}

extern "C" int tpg_aniso_kernels_f32(const float *pos, const int64_t *lengths, int B, int N, float rc, float lambda,
                                     float ks, float kr, float s_min, float s_max, float kn, int n_eps, int stages,
                                     float *centres, float *G, float *det, int32_t *count, void *ws, void *stream) {
    return an_kernels(true, pos, lengths, B, N, rc, lambda, ks, kr, s_min, s_max, kn, n_eps, stages, centres, G, det,
                      count, ws, stream);
}

extern "C" int tpg_aniso_kernels_exhaustive_f32(const float *pos, const int64_t *lengths, int B, int N, float rc,
                                                float lambda, float ks, float kr, float s_min, float s_max, float kn,
                                                int n_eps, int stages, float *centres, float *G, float *det,
                                                int32_t *count, void *ws, void *stream) {
    return an_kernels(false, pos, lengths, B, N, rc, lambda, ks, kr, s_min, s_max, kn, n_eps, stages, centres, G, det,
                      count, ws, stream);
}

extern "C" int tpg_aniso_field_f32(const float *query, const float *centres, const float *G, const float *det,
                                   const int64_t *lenq, const int64_t *lenp, int B, int Nq, int Np, float support,
                                   float reach, float *sum, void *ws, void *stream) {
    return an_field(true, query, centres, G, det, lenq, lenp, B, Nq, Np, support, reach, sum, ws, stream);
}

extern "C" int tpg_aniso_field_exhaustive_f32(const float *query, const float *centres, const float *G, const float *det,
                                              const int64_t *lenq, const int64_t *lenp, int B, int Nq, int Np,
                                              float support, float reach, float *sum, void *stream) {
    return an_field(false, query, centres, G, det, lenq, lenp, B, Nq, Np, support, reach, sum, nullptr, stream);
}
