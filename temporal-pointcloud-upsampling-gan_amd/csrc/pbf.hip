// Position Based Fluids, Jacobi iterations in gather form (the rule in full: include/tpgan_ops.h, "particle fluid
// simulator"; the numpy statement: tests/pbf_rule.py).  One substep of every scene of a batch is
//     predict | iters x ( grid | lambda | dp ) | grid | finish
// with the scenes on gridDim.y and ragged lengths, as in the grid searches.  With a per-particle XSPH table or vorticity
// confinement the tail is grid | finish_ex | vorticity (the rule: "vorticity confinement and per-particle viscosity" in
// the header; the numpy statement: tests/pbf_vort_rule.py): one more walk of the same grid.
//
// Launch shapes.  predict is one thread per particle (streaming, 24 bytes in, 24 out).  lambda, dp and finish are
// rr_kernel's shape (csrc/radius_reduce.hip): one wave per particle, the 27 cells around it as 9 runs of 3 x-adjacent
// cells of the cell-sorted array, 64 candidates of the concatenated runs per trip, the wave totals by tpg_wave_add_u64 at
// the end, no LDS.  The walk is pbf_walk below, not fg_walk of frnn_grid_build.hpp: through the shared helper the three
// passes ran 0.7 to 1.7 % slower (profiles/refactor_grid_walk.txt).  A neighbour's position comes from the grid's
// cell-sorted COPY (x, y, z, index), its lambda or previous position through the index; a wave writes its own particle only, and only into arrays no wave of the launch
// reads a neighbour from, so the Jacobi passes have no races by construction.
//
// Summation order.  The order inside a cell follows an atomic cursor (frnn_grid_build.hpp), so every neighbourhood sum
// is taken in 64-bit FIXED POINT, term by term a function of the pair alone, integer additions, one conversion back:
//   n, sum |g|^2   terms in [0, 1 + 2^-20]; unit 2^-32, unsigned.  Fewer than 2^22 terms (N is checked) of less than 2^33
//                  units stay below 2^55.
//   sum g          components in [-(1 + 2^-20), 1 + 2^-20]; unit 2^-32, signed: |sum| < 2^55.
//   dp, XSPH       a term is clamped into [-1024, 1024] (far outside anything a fluid at this scale produces: 1024
//                  supports per pair, 1024 m/s), unit 2^-30, signed: |term| <= 2^40 units, |sum| < 2^62.
// None can wrap, so no saturation is needed.  Truncation towards zero loses < 2^-30 per term against terms whose own
// fp32 rounding is 2^-24 relative.
//
// fp32 operations are + - * / and sqrtf only, each rounded on its own (-ffp-contract=off, no fast-math); comparisons
// and selections are exact.  Finite inputs are the caller's business: a NaN coordinate contributes unspecified
// (but in-bounds, fault-free) values to its neighbours' sums.
#include "frnn_grid_build.hpp"
#include "tpg_common.hpp"

namespace {

constexpr int PBF_MAX_N = 1 << 22;          // terms per sum: the overflow argument above
constexpr int PBF_BOX_CHUNK = 64;           // scenes per launch of the kernels that clamp (boxes ride in the arguments)
constexpr float PBF_U32 = 4294967296.0f, PBF_INV_U32 = 2.3283064365386963e-10f;      // 2^32, 2^-32
constexpr float PBF_U30 = 1073741824.0f, PBF_INV_U30 = 9.313225746154785e-10f;       // 2^30, 2^-30
constexpr float PBF_TERM_MAX = 1024.0f;

struct PbfBoxes { float c[PBF_BOX_CHUNK][6]; };      // lo xyz, hi xyz per scene of the chunk

// the grid build's own clamp (64-bit, into [0, N]): every launch kind and the grid agree on a scene's particle count
__device__ __forceinline__ int pbf_len(const int64_t *lengths, int b, int N) { return fg_len(lengths, b, N); }

__device__ __forceinline__ float pbf_clamp(float p, float lo, float hi) {
    p = p < lo ? lo : p;
    return p > hi ? hi : p;
}

__device__ __forceinline__ long long pbf_fix30(float t) {
    t = t < -PBF_TERM_MAX ? -PBF_TERM_MAX : t;
    t = t > PBF_TERM_MAX ? PBF_TERM_MAX : t;
    return (long long)(t * PBF_U30);
}

// W = ((h2 - d2) / h2)^3, the density weight over h^6
__device__ __forceinline__ float pbf_w(float d2, float h2) {
    const float u = (h2 - d2) / h2;
    return (u * u) * u;
}

// every candidate of the 27 cells around (px, py, pz), 64 per trip: f(candidate) on the lane that holds it.  fg_walk
// of frnn_grid_build.hpp around the particle's own cell, clamped into the grid, written out: see the note above
template <class F>
__device__ __forceinline__ void pbf_walk(const GridParams &g, const int *__restrict__ st, const float4 *__restrict__ pts,
                                         float px, float py, float pz, int lane, F &&f) {
    int cx = cell_axis(px, g.lo[0], g.inv_h), cy = cell_axis(py, g.lo[1], g.inv_h), cz = cell_axis(pz, g.lo[2], g.inv_h);
    cx = min(max(cx, 0), g.dim[0] - 1);
    cy = min(max(cy, 0), g.dim[1] - 1);
    cz = min(max(cz, 0), g.dim[2] - 1);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
    int rb[9], re[9], total = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int zz = cz + t / 3 - 1, yy = cy + t % 3 - 1;
        int bgn = 0, end = 0;
        if (zz >= 0 && zz < g.dim[2] && yy >= 0 && yy < g.dim[1]) {
            const int row = (zz * g.dim[1] + yy) * g.dim[0];
            bgn = st[row + x0];
            end = st[row + x1 + 1];
        }
        rb[t] = bgn;
        re[t] = end;
        total += end - bgn;
    }
    for (int base = 0; base < total; base += 64) {
        int c = base + lane, at = -1;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int n = re[t] - rb[t];
            if (at < 0 && c < n) at = rb[t] + c;
            c -= (at < 0) ? n : 0;
        }
        if (at >= 0 && base + lane < total) f(pts[at]);
    }
}

// step 1: v += dt g; p = clamp(x + dt v)                 grid (ceil(N/256), chunk of scenes)
__global__ __launch_bounds__(256) void pbf_predict_kernel(const float *__restrict__ x, const float *__restrict__ v,
                                                          const int64_t *__restrict__ lengths, PbfBoxes box, int b0, int N,
                                                          float dt, float a, float gx, float gy, float gz,
                                                          float *__restrict__ p_out, float *__restrict__ v_out) {
    const int b = b0 + blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pbf_len(lengths, b, N)) return;
    const size_t q = ((size_t)b * N + i) * 3;
    const float g[3] = {gx, gy, gz};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float vv = v[q + d] + dt * g[d];
        v_out[q + d] = vv;
        p_out[q + d] = pbf_clamp(x[q + d] + dt * vv, box.c[blockIdx.y][d] + a, box.c[blockIdx.y][3 + d] - a);
    }
}

// lambda pass: n, C, lambda of every particle               grid (ceil(N/FG_WAVES), B)
__global__ __launch_bounds__(FG_WAVES * 64) void pbf_lambda_kernel(
    const float *__restrict__ p, const int64_t *__restrict__ lengths, int N, const GridParams *__restrict__ gp,
    const int *__restrict__ start, const float4 *__restrict__ sorted, float h, float h2, float S0, float eps,
    float *__restrict__ lam, float *__restrict__ C_out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, i = blockIdx.x * FG_WAVES + wave;
    if (i >= pbf_len(lengths, b, N)) return;
    const size_t q = (size_t)b * N + i;
    const float px = p[q * 3], py = p[q * 3 + 1], pz = p[q * 3 + 2];
    tpg_u64 an = 0, ag2 = 0;
    long long ax = 0, ay = 0, az = 0;
    pbf_walk(gp[b], start + (size_t)b * (FG_CELLS + 1), sorted + (size_t)b * N, px, py, pz, lane, [&](const float4 c) {
        const float d2 = tpg_sq3(px, py, pz, c.x, c.y, c.z);
        if (!(d2 < h2)) return;
        an += (tpg_u64)(pbf_w(d2, h2) * PBF_U32);
        if (d2 == 0.0f) return;
        const float d = sqrtf(d2), t = (h - d) / h, t2 = t * t;
        const float gx = t2 * ((px - c.x) / d), gy = t2 * ((py - c.y) / d), gz = t2 * ((pz - c.z) / d);
        ag2 += (tpg_u64)(((gx * gx + gy * gy) + gz * gz) * PBF_U32);
        ax += (long long)(gx * PBF_U32);
        ay += (long long)(gy * PBF_U32);
        az += (long long)(gz * PBF_U32);
    });
    an = tpg_wave_add_u64(an);
    ag2 = tpg_wave_add_u64(ag2);
    ax = tpg_wave_add_u64(ax);
    ay = tpg_wave_add_u64(ay);
    az = tpg_wave_add_u64(az);
    if (lane == 0) {
        const float n = (float)an * PBF_INV_U32, sg2 = (float)ag2 * PBF_INV_U32;
        const float sx = (float)ax * PBF_INV_U32, sy = (float)ay * PBF_INV_U32, sz = (float)az * PBF_INV_U32;
        float C = n / S0 - 1.0f;
        C = C > 0.0f ? C : 0.0f;
        lam[q] = -(C / ((sg2 + ((sx * sx + sy * sy) + sz * sz)) + eps));
        if (C_out) C_out[q] = C;
    }
}

// dp pass: p_out = clamp(p + dp); p_out may be p itself (a wave reads only its own row of p, the neighbours' positions
// come from the grid's copy), hence no __restrict__ on the two        grid (ceil(N/FG_WAVES), chunk of scenes)
__global__ __launch_bounds__(FG_WAVES * 64) void pbf_dp_kernel(
    const float *p, const float *__restrict__ lam, const int64_t *__restrict__ lengths, PbfBoxes box, int b0,
    int N, const GridParams *__restrict__ gp, const int *__restrict__ start, const float4 *__restrict__ sorted, float h,
    float h2, float a, float wq, float k, float dp_scale, float *p_out, float *__restrict__ dp_out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = b0 + blockIdx.y, i = blockIdx.x * FG_WAVES + wave;
    const int n = pbf_len(lengths, b, N);
    if (i >= n) return;
    const size_t q = (size_t)b * N + i;
    const float px = p[q * 3], py = p[q * 3 + 1], pz = p[q * 3 + 2];
    const float li = lam[q];
    const float *lb = lam + (size_t)b * N;
    long long ax = 0, ay = 0, az = 0;
    pbf_walk(gp[b], start + (size_t)b * (FG_CELLS + 1), sorted + (size_t)b * N, px, py, pz, lane, [&](const float4 c) {
        const float d2 = tpg_sq3(px, py, pz, c.x, c.y, c.z);
        if (!(d2 < h2) || d2 == 0.0f) return;
        const float r = pbf_w(d2, h2) / wq, r2 = r * r;
        const float co = (li + lb[tpg_clamp_idx(__float_as_int(c.w), n)]) + -(k * (r2 * r2));
        const float d = sqrtf(d2), t = (h - d) / h, t2 = t * t;
        ax += pbf_fix30(co * (t2 * ((px - c.x) / d)));
        ay += pbf_fix30(co * (t2 * ((py - c.y) / d)));
        az += pbf_fix30(co * (t2 * ((pz - c.z) / d)));
    });
    ax = tpg_wave_add_u64(ax);
    ay = tpg_wave_add_u64(ay);
    az = tpg_wave_add_u64(az);
    if (lane == 0) {
        const float dp[3] = {dp_scale * ((float)ax * PBF_INV_U30), dp_scale * ((float)ay * PBF_INV_U30),
                             dp_scale * ((float)az * PBF_INV_U30)};
        const float pi[3] = {px, py, pz};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            p_out[q * 3 + d] = pbf_clamp(pi[d] + dp[d], box.c[blockIdx.y][d] + a, box.c[blockIdx.y][3 + d] - a);
            if (dp_out) dp_out[q * 3 + d] = dp[d];
        }
    }
}

// step 3: v = (p - x) / dt, XSPH, x = p                     grid (ceil(N/FG_WAVES), B)
// TABLE: the XSPH coefficient of a pair is the mean of the two particles' entries of cs_tab (B,N), inside the term, so
// that term_ij = -term_ji in integers; CURL: omega_i = sum u x G over the gradient pairs, on the velocities BEFORE XSPH
// (the ones this walk has), stored as (x, y, z, |omega|).  <false, false> is the pass of tpg_pbf_finish_f32: h, cs_tab and
// omega_out are not looked at there.
template <bool TABLE, bool CURL>
__global__ __launch_bounds__(FG_WAVES * 64) void pbf_finish_kernel(
    const float *__restrict__ p, const float *__restrict__ x, const int64_t *__restrict__ lengths, int N,
    const GridParams *__restrict__ gp, const int *__restrict__ start, const float4 *__restrict__ sorted, float h, float h2,
    float dt, float cs, const float *__restrict__ cs_tab, float *__restrict__ x_out, float *__restrict__ v_out,
    float4 *__restrict__ omega_out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, i = blockIdx.x * FG_WAVES + wave;
    const int n = pbf_len(lengths, b, N);
    if (i >= n) return;
    const size_t q = (size_t)b * N + i;
    const float px = p[q * 3], py = p[q * 3 + 1], pz = p[q * 3 + 2];
    const float vx = (px - x[q * 3]) / dt, vy = (py - x[q * 3 + 1]) / dt, vz = (pz - x[q * 3 + 2]) / dt;
    const float *xb = x + (size_t)b * N * 3;
    float ci = 0.0f;
    const float *cb = nullptr;
    if constexpr (TABLE) {
        cb = cs_tab + (size_t)b * N;
        ci = cb[i];
    }
    long long ax = 0, ay = 0, az = 0, wx = 0, wy = 0, wz = 0;
    pbf_walk(gp[b], start + (size_t)b * (FG_CELLS + 1), sorted + (size_t)b * N, px, py, pz, lane, [&](const float4 c) {
        const float d2 = tpg_sq3(px, py, pz, c.x, c.y, c.z);
        if (!(d2 < h2)) return;
        const float w = pbf_w(d2, h2);
        const int j = tpg_clamp_idx(__float_as_int(c.w), n);
        const float *xj = xb + (size_t)j * 3;
        const float ux = (c.x - xj[0]) / dt - vx, uy = (c.y - xj[1]) / dt - vy, uz = (c.z - xj[2]) / dt - vz;
        if constexpr (TABLE) {
            const float cij = 0.5f * (ci + cb[j]);
            ax += pbf_fix30(cij * (ux * w));
            ay += pbf_fix30(cij * (uy * w));
            az += pbf_fix30(cij * (uz * w));
        } else {
            ax += pbf_fix30(ux * w);
            ay += pbf_fix30(uy * w);
            az += pbf_fix30(uz * w);
        }
        if constexpr (CURL) {
            if (d2 == 0.0f) return;
            const float d = sqrtf(d2), t = (h - d) / h, t2 = t * t;
            const float gx = t2 * ((px - c.x) / d), gy = t2 * ((py - c.y) / d), gz = t2 * ((pz - c.z) / d);
            wx += pbf_fix30(uy * gz - uz * gy);
            wy += pbf_fix30(uz * gx - ux * gz);
            wz += pbf_fix30(ux * gy - uy * gx);
        }
    });
    ax = tpg_wave_add_u64(ax);
    ay = tpg_wave_add_u64(ay);
    az = tpg_wave_add_u64(az);
    if constexpr (CURL) {
        wx = tpg_wave_add_u64(wx);
        wy = tpg_wave_add_u64(wy);
        wz = tpg_wave_add_u64(wz);
    }
    if (lane == 0) {
        if constexpr (TABLE) {
            v_out[q * 3] = vx + (float)ax * PBF_INV_U30;
            v_out[q * 3 + 1] = vy + (float)ay * PBF_INV_U30;
            v_out[q * 3 + 2] = vz + (float)az * PBF_INV_U30;
        } else {
            v_out[q * 3] = vx + cs * ((float)ax * PBF_INV_U30);
            v_out[q * 3 + 1] = vy + cs * ((float)ay * PBF_INV_U30);
            v_out[q * 3 + 2] = vz + cs * ((float)az * PBF_INV_U30);
        }
        x_out[q * 3] = px;
        x_out[q * 3 + 1] = py;
        x_out[q * 3 + 2] = pz;
        if constexpr (CURL) {
            const float ox = (float)wx * PBF_INV_U30, oy = (float)wy * PBF_INV_U30, oz = (float)wz * PBF_INV_U30;
            omega_out[q] = make_float4(ox, oy, oz, sqrtf((ox * ox + oy * oy) + oz * oz));
        }
    }
}

// vorticity confinement: eta_i = sum (m_i - m_j) G_ij over the gradient pairs, m = |omega| of the finish pass (the
// difference form: a uniform |omega| gives eta = 0 exactly); N = eta / (|eta| + delta); v_out = v + (dt * vs) * (N x omega_i).
// v_out may be v (a wave reads only its own row of v; a neighbour's m comes from omega, which no wave writes), hence
// no __restrict__ on the two                                  grid (ceil(N/FG_WAVES), B)
__global__ __launch_bounds__(FG_WAVES * 64) void pbf_vorticity_kernel(
    const float *__restrict__ p, const float4 *__restrict__ omega, const float *v, const int64_t *__restrict__ lengths,
    int N, const GridParams *__restrict__ gp, const int *__restrict__ start, const float4 *__restrict__ sorted, float h,
    float h2, float dt, float vs, float delta, float *v_out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, i = blockIdx.x * FG_WAVES + wave;
    const int n = pbf_len(lengths, b, N);
    if (i >= n) return;
    const size_t q = (size_t)b * N + i;
    const float px = p[q * 3], py = p[q * 3 + 1], pz = p[q * 3 + 2];
    const float4 *ob = omega + (size_t)b * N;
    const float4 oi = ob[i];
    long long ax = 0, ay = 0, az = 0;
    pbf_walk(gp[b], start + (size_t)b * (FG_CELLS + 1), sorted + (size_t)b * N, px, py, pz, lane, [&](const float4 c) {
        const float d2 = tpg_sq3(px, py, pz, c.x, c.y, c.z);
        if (!(d2 < h2) || d2 == 0.0f) return;
        const float dm = oi.w - ob[tpg_clamp_idx(__float_as_int(c.w), n)].w;
        const float d = sqrtf(d2), t = (h - d) / h, t2 = t * t;
        ax += pbf_fix30(dm * (t2 * ((px - c.x) / d)));
        ay += pbf_fix30(dm * (t2 * ((py - c.y) / d)));
        az += pbf_fix30(dm * (t2 * ((pz - c.z) / d)));
    });
    ax = tpg_wave_add_u64(ax);
    ay = tpg_wave_add_u64(ay);
    az = tpg_wave_add_u64(az);
    if (lane == 0) {
        const float ex = (float)ax * PBF_INV_U30, ey = (float)ay * PBF_INV_U30, ez = (float)az * PBF_INV_U30;
        const float den = sqrtf((ex * ex + ey * ey) + ez * ez) + delta;
        const float nx = ex / den, ny = ey / den, nz = ez / den;
        const float s = dt * vs;
        v_out[q * 3] = v[q * 3] + s * (ny * oi.z - nz * oi.y);
        v_out[q * 3 + 1] = v[q * 3 + 1] + s * (nz * oi.x - nx * oi.z);
        v_out[q * 3 + 2] = v[q * 3 + 2] + s * (nx * oi.y - ny * oi.x);
    }
}

// the shape checks every entry shares; > 0: nothing to do (TPG_OK), < 0: the status to return
int pbf_shape(int B, int N) {
    if (B < 0 || N < 0) return TPG_ERR_ARG;
    if (B == 0 || N == 0) return 1;
    if (B > 65535 || N > PBF_MAX_N) return TPG_ERR_UNSUPPORTED;       // scenes ride on gridDim.y; the sums' headroom
    return 0;
}

bool pbf_pos(float v) { return v > 0.0f && v <= 3.0e38f; }            // positive and finite

// box (B,6) host floats: finite, lo < hi on every axis
bool pbf_box_ok(const float *box, int B) {
    for (int b = 0; b < B; ++b)
        for (int d = 0; d < 3; ++d) {
            const float lo = box[b * 6 + d], hi = box[b * 6 + 3 + d];
            if (!(lo < hi) || !(lo >= -3.0e38f) || !(hi <= 3.0e38f)) return false;
        }
    return true;
}

void pbf_fill_boxes(PbfBoxes &out, const float *box, int b0, int nb) {
    for (int j = 0; j < PBF_BOX_CHUNK; ++j)
        for (int d = 0; d < 6; ++d) out.c[j][d] = j < nb ? box[(size_t)(b0 + j) * 6 + d] : 0.0f;
}

}  // namespace

extern "C" size_t tpg_pbf_workspace_bytes(int B, int N) { return fg_workspace_bytes(B, N); }

extern "C" int tpg_pbf_predict_f32(const float *x, const float *v, const int64_t *lengths, const float *box, int B, int N,
                                   float dt, float a, const float *gravity, float *p_out, float *v_out, void *stream) {
    if (!pbf_pos(dt) || !pbf_pos(a) || !p_out || !v_out) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!x || !v || !box || !gravity || !pbf_box_ok(box, B)) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    for (int b0 = 0; b0 < B; b0 += PBF_BOX_CHUNK) {
        const int nb = min(PBF_BOX_CHUNK, B - b0);
        PbfBoxes bx;
        pbf_fill_boxes(bx, box, b0, nb);
        hipLaunchKernelGGL(pbf_predict_kernel, dim3((N + 255) / 256, nb), dim3(256), 0, st, x, v, lengths, bx, b0, N, dt,
                           a, gravity[0], gravity[1], gravity[2], p_out, v_out);
    }
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_pbf_grid_f32(const float *p, const int64_t *lengths, int B, int N, float h, void *ws, void *stream) {
    if (!pbf_pos(h)) return TPG_ERR_ARG;
    if (B > 0 && N > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!p) return TPG_ERR_ARG;
    GridView v;
    const int rc = fg_build(p, lengths, B, N, h, 0, ws, tpg_stream(stream), &v);
    if (rc) return rc;
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_pbf_lambda_f32(const float *p, const int64_t *lengths, int B, int N, float h, float S0, float eps,
                                  const void *ws, float *lam, float *C_out, void *stream) {
    if (!pbf_pos(h) || !pbf_pos(S0) || !(eps >= 0.0f) || !(eps <= 3.0e38f) || !lam) return TPG_ERR_ARG;
    if (B > 0 && N > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!p) return TPG_ERR_ARG;
    const GridView v = fg_view(ws, B, N);
    hipLaunchKernelGGL(pbf_lambda_kernel, dim3(fg_query_blocks(N), B), dim3(FG_WAVES * 64), 0, tpg_stream(stream), p,
                       lengths, N, v.gp, v.start, v.sorted, h, h * h, S0, eps, lam, C_out);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_pbf_dp_f32(const float *p, const float *lam, const int64_t *lengths, const float *box, int B, int N,
                              float h, float a, float wq, float k, float dp_scale, const void *ws, float *p_out,
                              float *dp_out, void *stream) {
    if (!pbf_pos(h) || !pbf_pos(a) || !pbf_pos(wq) || !(k >= 0.0f) || !(k <= 3.0e38f) || !(dp_scale >= -3.0e38f) ||
        !(dp_scale <= 3.0e38f) || !p_out)
        return TPG_ERR_ARG;
    if (B > 0 && N > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!p || !lam || !box || !pbf_box_ok(box, B)) return TPG_ERR_ARG;
    const GridView v = fg_view(ws, B, N);
    for (int b0 = 0; b0 < B; b0 += PBF_BOX_CHUNK) {
        const int nb = min(PBF_BOX_CHUNK, B - b0);
        PbfBoxes bx;
        pbf_fill_boxes(bx, box, b0, nb);
        hipLaunchKernelGGL(pbf_dp_kernel, dim3(fg_query_blocks(N), nb), dim3(FG_WAVES * 64), 0, tpg_stream(stream), p, lam,
                           lengths, bx, b0, N, v.gp, v.start, v.sorted, h, h * h, a, wq, k, dp_scale, p_out, dp_out);
    }
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_pbf_finish_f32(const float *p, const float *x, const int64_t *lengths, int B, int N, float h, float dt,
                                  float cs, const void *ws, float *x_out, float *v_out, void *stream) {
    if (!pbf_pos(h) || !pbf_pos(dt) || !(cs >= 0.0f) || !(cs <= 3.0e38f) || !x_out || !v_out || x_out == x) return TPG_ERR_ARG;
    if (B > 0 && N > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!p || !x) return TPG_ERR_ARG;
    const GridView v = fg_view(ws, B, N);
    hipLaunchKernelGGL((pbf_finish_kernel<false, false>), dim3(fg_query_blocks(N), B), dim3(FG_WAVES * 64), 0,
                       tpg_stream(stream), p, x, lengths, N, v.gp, v.start, v.sorted, h, h * h, dt, cs,
                       (const float *)nullptr, x_out, v_out, (float4 *)nullptr);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

// finish with a per-particle XSPH table and / or the curl (the rule: include/tpgan_ops.h, "vorticity confinement and
// per-particle viscosity"); with neither it is tpg_pbf_finish_f32
extern "C" int tpg_pbf_finish_ex_f32(const float *p, const float *x, const int64_t *lengths, int B, int N, float h, float dt,
                                     float cs, const float *cs_tab, const void *ws, float *x_out, float *v_out,
                                     float *omega_out, void *stream) {
    if (!pbf_pos(h) || !pbf_pos(dt) || !(cs >= 0.0f) || !(cs <= 3.0e38f) || !x_out || !v_out || x_out == x) return TPG_ERR_ARG;
    if (B > 0 && N > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!p || !x) return TPG_ERR_ARG;
    const GridView v = fg_view(ws, B, N);
    const dim3 grid(fg_query_blocks(N), B), block(FG_WAVES * 64);
    hipStream_t st = tpg_stream(stream);
    float4 *om = reinterpret_cast<float4 *>(omega_out);
#define PBF_FINISH(TABLE, CURL)                                                                                        \
    hipLaunchKernelGGL((pbf_finish_kernel<TABLE, CURL>), grid, block, 0, st, p, x, lengths, N, v.gp, v.start, v.sorted, h, \
                       h * h, dt, cs, cs_tab, x_out, v_out, om)
    if (cs_tab && om) PBF_FINISH(true, true);
    else if (cs_tab) PBF_FINISH(true, false);
    else if (om) PBF_FINISH(false, true);
    else PBF_FINISH(false, false);
#undef PBF_FINISH
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_pbf_vorticity_f32(const float *p, const float *omega, const float *v, const int64_t *lengths, int B,
                                     int N, float h, float dt, float vs, float delta, const void *ws, float *v_out,
                                     void *stream) {
    if (!pbf_pos(h) || !pbf_pos(dt) || !(vs >= 0.0f) || !(vs <= 3.0e38f) || !pbf_pos(delta) || !v_out) return TPG_ERR_ARG;
    if (B > 0 && N > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!p || !omega || !v) return TPG_ERR_ARG;
    const GridView g = fg_view(ws, B, N);
    hipLaunchKernelGGL(pbf_vorticity_kernel, dim3(fg_query_blocks(N), B), dim3(FG_WAVES * 64), 0, tpg_stream(stream), p,
                       reinterpret_cast<const float4 *>(omega), v, lengths, N, g.gp, g.start, g.sorted, h, h * h, dt, vs,
                       delta, v_out);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

// ---- static solid obstacles (the rule in full: include/tpgan_ops.h, "solid obstacles"; the numpy statement:
// tests/pbf_obstacle_rule.py).  collide is a launch kind of its own, after predict and after every dp: one thread per
// particle, streaming like predict (12 bytes in, 12 or 16 out).  The M rows of a scene sit at an address that depends on
// blockIdx.y alone and are read before the kernel's only stores, so they travel through the scalar cache into scalar
// registers, and every branch on a row's kind or on its finiteness is uniform over the workgroup.  No address depends on a
// table value.  No LDS, no atomics.
namespace {

constexpr int PBF_OBSTACLE_FLOATS = 16;     // PBF_MAX_OBSTACLES: include/tpgan_ops.h

__device__ __forceinline__ bool pbf_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for NaN

// p = collide(p): the obstacles in index order, then the box clamp         grid (ceil(N/256), chunk of scenes)
// p_out may be p (a thread reads and writes its own row only), hence no __restrict__ on the two
__global__ __launch_bounds__(256) void pbf_collide_kernel(const float *p, const int64_t *__restrict__ lengths, PbfBoxes box,
                                                          const float *__restrict__ obstacles, int b0, int N, int M,
                                                          float a, float *p_out, int32_t *__restrict__ hit_out) {
    const int b = b0 + blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pbf_len(lengths, b, N)) return;
    const size_t at = (size_t)b * N + i;
    float px = p[at * 3], py = p[at * 3 + 1], pz = p[at * 3 + 2];
    const float *__restrict__ row = obstacles + (size_t)b * M * PBF_OBSTACLE_FLOATS;
    int hit = 0;
    for (int o = 0; o < M; ++o, row += PBF_OBSTACLE_FLOATS) {
        float t[PBF_OBSTACLE_FLOATS];
#pragma unroll
        for (int j = 0; j < PBF_OBSTACLE_FLOATS; ++j) t[j] = row[j];
        const float kind = t[0];
        bool ok = kind == 1.0f || kind == 2.0f || kind == 3.0f;
#pragma unroll
        for (int j = 1; j < PBF_OBSTACLE_FLOATS; ++j) ok = ok && pbf_finite(t[j]);
        if (!ok) continue;
        const float dx = px - t[1], dy = py - t[2], dz = pz - t[3];
        float qx = (dx * t[4] + dy * t[7]) + dz * t[10];
        float qy = (dx * t[5] + dy * t[8]) + dz * t[11];
        float qz = (dx * t[6] + dy * t[9]) + dz * t[12];
        bool inside;
        if (kind == 1.0f) {
            const float E = t[13] + a, d2 = (qx * qx + qy * qy) + qz * qz;
            inside = d2 < E * E;
            if (d2 == 0.0f) {
                qx = 0.0f, qy = E, qz = 0.0f;
            } else {
                const float d = sqrtf(d2);
                qx = (qx / d) * E, qy = (qy / d) * E, qz = (qz / d) * E;
            }
        } else if (kind == 2.0f) {
            const float Ex = t[13] + a, Ey = t[14] + a, Ez = t[15] + a;
            const float ax = fabsf(qx), ay = fabsf(qy), az = fabsf(qz);
            inside = ax < Ex && ay < Ey && az < Ez;
            const float p0 = Ex - ax, p1 = Ey - ay, p2 = Ez - az;
            int k = 0;
            float pk = p0;
            if (p1 < pk) k = 1, pk = p1;
            if (p2 < pk) k = 2;
            if (k == 0) qx = qx < 0.0f ? -Ex : Ex;
            if (k == 1) qy = qy < 0.0f ? -Ey : Ey;
            if (k == 2) qz = qz < 0.0f ? -Ez : Ez;
        } else {
            const float Er = t[13] + a, Eh = t[14] + a, r2 = qx * qx + qz * qz;
            inside = r2 < Er * Er && fabsf(qy) < Eh;
            const float r = sqrtf(r2), pen_r = Er - r, pen_h = Eh - fabsf(qy);
            if (pen_h <= pen_r) {
                qy = qy < 0.0f ? -Eh : Eh;
            } else if (r2 == 0.0f) {
                qx = Er, qz = 0.0f;
            } else {
                qx = (qx / r) * Er, qz = (qz / r) * Er;
            }
        }
        if (inside) {
            px = t[1] + ((t[4] * qx + t[5] * qy) + t[6] * qz);
            py = t[2] + ((t[7] * qx + t[8] * qy) + t[9] * qz);
            pz = t[3] + ((t[10] * qx + t[11] * qy) + t[12] * qz);
            hit |= 1 << o;
        }
    }
    p_out[at * 3] = pbf_clamp(px, box.c[blockIdx.y][0] + a, box.c[blockIdx.y][3] - a);
    p_out[at * 3 + 1] = pbf_clamp(py, box.c[blockIdx.y][1] + a, box.c[blockIdx.y][4] - a);
    p_out[at * 3 + 2] = pbf_clamp(pz, box.c[blockIdx.y][2] + a, box.c[blockIdx.y][5] - a);
    if (hit_out) hit_out[at] = hit;
}

}  // namespace

extern "C" int tpg_pbf_collide_f32(const float *p, const int64_t *lengths, const float *box, const float *obstacles, int B,
                                   int N, int M, float a, float *p_out, int32_t *hit_out, void *stream) {
    if (M < 0 || !pbf_pos(a) || !p_out) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk && chk != TPG_ERR_UNSUPPORTED) return chk > 0 ? TPG_OK : chk;
    if (chk || M > PBF_MAX_OBSTACLES) return TPG_ERR_UNSUPPORTED;
    if (!p || !box || !pbf_box_ok(box, B) || (M > 0 && !obstacles)) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    for (int b0 = 0; b0 < B; b0 += PBF_BOX_CHUNK) {
        const int nb = min(PBF_BOX_CHUNK, B - b0);
        PbfBoxes bx;
        pbf_fill_boxes(bx, box, b0, nb);
        hipLaunchKernelGGL(pbf_collide_kernel, dim3((N + 255) / 256, nb), dim3(256), 0, st, p, lengths, bx, obstacles, b0, N,
                           M, a, p_out, hit_out);
    }
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

// ---- mesh obstacles: sampled distance fields (the rule in full: include/tpgan_ops.h, "mesh obstacles"; the numpy
// statement: tests/pbf_sdf_rule.py).  A launch kind of its own with collide's shape: one thread per particle, the M rows
// of a scene at an address that depends on blockIdx.y alone, read before the kernel's only stores, so every branch on a
// row is uniform over the workgroup.  Unlike collide, addresses DO depend on table values here (the field's offset and
// dims): a row is used only after offset >= 0 and offset + nx*ny*nz <= fields_len have been checked in 64 bits, and a
// particle reads its cell only after it has tested inside the lattice, so every index lies in [offset, offset + nx*ny*nz).
// Eight gathered loads per particle and obstacle; no LDS, no atomics.
namespace {

constexpr int PBF_SDF_WORDS = 24;           // PBF_MAX_SDF_OBSTACLES, PBF_SDF_MAX_DIM: include/tpgan_ops.h

__global__ __launch_bounds__(256) void pbf_collide_sdf_kernel(const float *p, const int64_t *__restrict__ lengths,
                                                              PbfBoxes box, const float *__restrict__ table,
                                                              const float *__restrict__ fields, long long fields_len,
                                                              int b0, int N, int M, float a, float *p_out,
                                                              int32_t *__restrict__ hit_out) {
    const int b = b0 + blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pbf_len(lengths, b, N)) return;
    const size_t at = (size_t)b * N + i;
    float px = p[at * 3], py = p[at * 3 + 1], pz = p[at * 3 + 2];
    const float *__restrict__ row = table + (size_t)b * M * PBF_SDF_WORDS;
    int hit = 0;
    for (int o = 0; o < M; ++o, row += PBF_SDF_WORDS) {
        float t[17];
#pragma unroll
        for (int j = 0; j < 17; ++j) t[j] = row[j];
        const int nx = __float_as_int(row[17]), ny = __float_as_int(row[18]), nz = __float_as_int(row[19]);
        const long long off = (long long)(((tpg_u64)(unsigned)__float_as_int(row[21]) << 32) |
                                          (unsigned)__float_as_int(row[20]));
        bool ok = t[0] == 4.0f && t[16] > 0.0f;
#pragma unroll
        for (int j = 1; j < 17; ++j) ok = ok && pbf_finite(t[j]);
        ok = ok && nx >= 2 && ny >= 2 && nz >= 2 && nx <= PBF_SDF_MAX_DIM && ny <= PBF_SDF_MAX_DIM && nz <= PBF_SDF_MAX_DIM;
        const long long cells = ok ? ((long long)nx * ny) * nz : 0;          // <= 2^36
        ok = ok && off >= 0 && off <= fields_len && cells <= fields_len - off;
        if (!ok) continue;
        const float dx = px - t[1], dy = py - t[2], dz = pz - t[3];
        float qx = (dx * t[4] + dy * t[7]) + dz * t[10];
        float qy = (dx * t[5] + dy * t[8]) + dz * t[11];
        float qz = (dx * t[6] + dy * t[9]) + dz * t[12];
        const float gx = (qx - t[13]) / t[16], gy = (qy - t[14]) / t[16], gz = (qz - t[15]) / t[16];
        const bool in = gx >= 0.0f && gx <= (float)(nx - 1) && gy >= 0.0f && gy <= (float)(ny - 1) && gz >= 0.0f &&
                        gz <= (float)(nz - 1);
        if (!in) continue;
        const int ix = min((int)floorf(gx), nx - 2), iy = min((int)floorf(gy), ny - 2), iz = min((int)floorf(gz), nz - 2);
        const float tx = gx - (float)ix, ty = gy - (float)iy, tz = gz - (float)iz;
        const float *__restrict__ f = fields + off + ((long long)ix * ny + iy) * nz + iz;
        const long long sx = (long long)ny * nz;
        const float f000 = f[0], f001 = f[1], f010 = f[nz], f011 = f[nz + 1];
        const float f100 = f[sx], f101 = f[sx + 1], f110 = f[sx + nz], f111 = f[sx + nz + 1];
        const float x00 = f100 - f000, x10 = f110 - f010, x01 = f101 - f001, x11 = f111 - f011;
        const float c00 = f000 + tx * x00, c10 = f010 + tx * x10, c01 = f001 + tx * x01, c11 = f011 + tx * x11;
        const float y0 = c10 - c00, y1 = c11 - c01;
        const float c0 = c00 + ty * y0, c1 = c01 + ty * y1;
        const float gradz = c1 - c0;
        const float phi = c0 + tz * gradz;
        const float gradx0 = x00 + ty * (x10 - x00), gradx1 = x01 + ty * (x11 - x01);
        const float gradx = gradx0 + tz * (gradx1 - gradx0);
        const float grady = y0 + tz * (y1 - y0);
        const float n2 = (gradx * gradx + grady * grady) + gradz * gradz;
        const bool moved = phi < a && n2 > 0.0f && pbf_finite(n2);
        if (moved) {
            const float len = sqrtf(n2), s = a - phi;
            qx = qx + s * (gradx / len), qy = qy + s * (grady / len), qz = qz + s * (gradz / len);
            px = t[1] + ((t[4] * qx + t[5] * qy) + t[6] * qz);
            py = t[2] + ((t[7] * qx + t[8] * qy) + t[9] * qz);
            pz = t[3] + ((t[10] * qx + t[11] * qy) + t[12] * qz);
            hit |= 1 << o;
        }
    }
    p_out[at * 3] = pbf_clamp(px, box.c[blockIdx.y][0] + a, box.c[blockIdx.y][3] - a);
    p_out[at * 3 + 1] = pbf_clamp(py, box.c[blockIdx.y][1] + a, box.c[blockIdx.y][4] - a);
    p_out[at * 3 + 2] = pbf_clamp(pz, box.c[blockIdx.y][2] + a, box.c[blockIdx.y][5] - a);
    if (hit_out) hit_out[at] = hit;
}

}  // namespace

extern "C" int tpg_pbf_collide_sdf_f32(const float *p, const int64_t *lengths, const float *box, const float *table,
                                       const float *fields, long long fields_len, int B, int N, int M, float a,
                                       float *p_out, int32_t *hit_out, void *stream) {
    if (M < 0 || fields_len < 0 || !pbf_pos(a) || !p_out) return TPG_ERR_ARG;
    const int chk = pbf_shape(B, N);
    if (chk && chk != TPG_ERR_UNSUPPORTED) return chk > 0 ? TPG_OK : chk;
    if (chk || M > PBF_MAX_SDF_OBSTACLES) return TPG_ERR_UNSUPPORTED;
    if (!p || !box || !pbf_box_ok(box, B) || (M > 0 && !table) || (fields_len > 0 && !fields)) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    for (int b0 = 0; b0 < B; b0 += PBF_BOX_CHUNK) {
        const int nb = min(PBF_BOX_CHUNK, B - b0);
        PbfBoxes bx;
        pbf_fill_boxes(bx, box, b0, nb);
        hipLaunchKernelGGL(pbf_collide_sdf_kernel, dim3((N + 255) / 256, nb), dim3(256), 0, st, p, lengths, bx, table, fields,
                           fields_len, b0, N, M, a, p_out, hit_out);
    }
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
