// Uncapped neighbourhood sums: per query, the NUMBER of stored points within r and the SUM of a radial kernel over
// them -- every point in range, however many (reference call sites, all on the host through a scipy KD-tree:
// train_fluid/analysis_helper.py:143-161 get_particle_density / get_particle_density_of_two_pcd, :291-294
// particle_dns2grid_dns; train_utils.py:269-286 fixed_radius_neighbor_num / get_free_surface_particles).  The
// K-nearest searches of knn.hip / frnn_grid.hip keep at most 64 neighbours by design; at the fluid clips' particle
// spacing a cutoff of 2-3 spacings holds 40-120 and the count is the result itself.
//
// Membership: d2 <= r2, INCLUSIVE (scipy's query_ball_point / query_ball_tree are), with the project's canonical fp32
// distance (t = q - p per axis; d = t0*t0; d = d + t1*t1; d = d + t2*t2; no FMA) and r2 = fp32(r) * fp32(r).
//
// Two launch shapes of one kernel body, one wave per query, no LDS (fg_candidates of frnn_grid_build.hpp hands out the
// candidates of either):
//   grid        the uniform grid (cell edge >= r * 1.0001, so no pair within r sits more than one cell apart): the walk
//               over the 27 cells around the query's cell, 64 candidates per trip
//   exhaustive  the lanes stride over the whole stored cloud (small clouds: no build launches)
//
// Summation order.  The grid's fill places the points of a cell through an atomic cursor, so the order in which a
// query meets its neighbours changes from run to run, and a float sum that follows it would not be reproducible.
// The sum is therefore taken in 64-bit FIXED POINT: every term is converted on its own (a function of the pair
// alone), integer addition is associative and commutative, and one conversion back to fp32 ends it.  The result is
// independent of the candidate order, of the lane a candidate lands on, of the batch position and of which of the two
// launch shapes ran: the two entries return the same bits.
//   cubic   terms lie in [0, 1]; unit 2^-32 (truncation error < 2^-32 per term against the fp32 term's own 2^-24);
//           fewer than 2^31 terms of at most 2^32 units cannot overflow
//   linear  fp32(r / d) - 1 is a multiple of 2^-23 whenever it is not 0 (r / d >= 1 has an ulp of at least 2^-23), so
//           with the unit 2^-23 the conversion is EXACT and the result is the correctly rounded sum of the fp32 terms;
//           a term is clamped at 2^40 and the addition saturates (still order-independent) instead of wrapping
#include "frnn_grid_build.hpp"
#include "tpg_common.hpp"

namespace {

constexpr int RR_CUBIC = 0, RR_LINEAR = 1;

// one neighbour's term in fixed point; d2 <= r2 already holds
__device__ __forceinline__ tpg_u64 rr_term(float d2, float r, int kernel) {
    const float d = sqrtf(d2);
    if (kernel == RR_CUBIC) {
        // analysis_helper.py:102-113 with coefficient 1; sqrt(d2) / r may exceed 1 by an ulp at the rim
        return (tpg_u64)(tpg_cubic_spline_w(fminf(d / r, 1.0f)) * 4294967296.0f);
    }
    // train_utils.py:258-266
    if (d < 1.0e-8f) return 0;
    const float w = fminf(fmaxf(r / d - 1.0f, 0.0f), 1099511627776.0f);
    return (tpg_u64)(w * 8388608.0f);
}

__device__ __forceinline__ tpg_u64 rr_sat_add(tpg_u64 a, tpg_u64 b) {
    const tpg_u64 s = a + b;
    return s < a ? ~0ull : s;
}

// count[b][i] = #{j : d2(i, j) <= r2}, sum[b][i] = sum over them of w(sqrt(d2), r); either may be NULL
template <bool GRID>
__global__ __launch_bounds__(FG_WAVES * 64) void rr_kernel(
    const float *__restrict__ query, const float *__restrict__ pos, const int64_t *__restrict__ lenq,
    const int64_t *__restrict__ lenp, int Nq, int Np, const GridParams *__restrict__ gp, int cstride,
    const int *__restrict__ start, const float4 *__restrict__ sorted, float r, float r2, int kernel,
    int32_t *__restrict__ count, float *__restrict__ sum) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int i = blockIdx.x * FG_WAVES + wave;
    if (i >= Nq) return;
    const size_t q = (size_t)b * Nq + i;
    const int nq = lenq ? (int)lenq[b] : Nq;
    int cnt = 0;
    tpg_u64 acc = 0;
    if (i < nq) {
        const float qx = query[q * 3], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
        // the exhaustive shape reads lenp itself (the grid's own count is fg_build's business)
        const int np = GRID ? 0 : (lenp ? min(max((int)lenp[b], 0), Np) : Np);
        fg_candidates<GRID>(qx, qy, qz, gp, b, cstride, start, sorted, pos, np, Np, lane,
                            [&](float px, float py, float pz, int) {
                                const float d = tpg_sq3(qx, qy, qz, px, py, pz);
                                if (d <= r2) {
                                    ++cnt;
                                    if (sum) acc = rr_sat_add(acc, rr_term(d, r, kernel));
                                }
                            });
    }
    // wave totals: xor butterfly of integer additions (the whole wave is here: every branch above is wave-uniform)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        cnt += __shfl_xor(cnt, s);
        acc = rr_sat_add(acc, __shfl_xor(acc, s));
    }
    if (lane == 0) {
        if (count) count[q] = cnt;
        if (sum) sum[q] = (float)acc * (kernel == RR_CUBIC ? 2.3283064365386963e-10f : 1.1920928955078125e-7f);
    }
}

// argument checks of both entries; > 0: nothing left to do (TPG_OK), < 0: the status to return
int rr_check(const float *query, const float *pos, int B, int Nq, int Np, float r, int kernel, int32_t *count,
             float *sum, hipStream_t st) {
    if (B < 0 || Nq < 0 || Np < 0 || !(r > 0.0f) || (!count && !sum)) return TPG_ERR_ARG;
    if (kernel != RR_CUBIC && kernel != RR_LINEAR) return TPG_ERR_UNSUPPORTED;
    if (B == 0 || Nq == 0) return 1;
    if (!query) return TPG_ERR_ARG;
    if (B > 65535) return TPG_ERR_UNSUPPORTED;           // clouds ride on gridDim.y
    if (Np == 0) {                                       // nothing stored: zeros
        if (count && hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)B * Nq, st) != hipSuccess) return TPG_ERR_LAUNCH;
        if (sum && hipMemsetAsync(sum, 0, sizeof(float) * (size_t)B * Nq, st) != hipSuccess) return TPG_ERR_LAUNCH;
        return 1;
    }
    if (!pos) return TPG_ERR_ARG;
    return 0;
}

}  // namespace

extern "C" int tpg_radius_reduce_f32(const float *query, const float *pos, const int64_t *lenq, const int64_t *lenp,
                                     int B, int Nq, int Np, float r, int kernel, int32_t *count, float *sum, void *ws,
                                     void *stream) {
    hipStream_t st = tpg_stream(stream);
    if (B > 0 && Nq > 0 && Np > 0 && !fg_workspace_ok(ws)) return TPG_ERR_ARG;
    const int chk = rr_check(query, pos, B, Nq, Np, r, kernel, count, sum, st);
    if (chk) return chk > 0 ? TPG_OK : chk;
    GridView v;
    const int rc = fg_build(pos, lenp, B, Np, r, 0, ws, st, &v);
    if (rc) return rc;
    hipLaunchKernelGGL(rr_kernel<true>, dim3(fg_query_blocks(Nq), B), dim3(FG_WAVES * 64), 0, st, query, pos,
                       lenq, lenp, Nq, Np, v.gp, FG_CELLS, v.start, v.sorted, r, r * r, kernel, count, sum);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_radius_reduce_exhaustive_f32(const float *query, const float *pos, const int64_t *lenq,
                                                const int64_t *lenp, int B, int Nq, int Np, float r, int kernel,
                                                int32_t *count, float *sum, void *stream) {
    hipStream_t st = tpg_stream(stream);
    const int chk = rr_check(query, pos, B, Nq, Np, r, kernel, count, sum, st);
    if (chk) return chk > 0 ? TPG_OK : chk;
    hipLaunchKernelGGL(rr_kernel<false>, dim3(fg_query_blocks(Nq), B), dim3(FG_WAVES * 64), 0, st, query, pos,
                       lenq, lenp, Nq, Np, (const GridParams *)nullptr, 0, (const int *)nullptr,
                       (const float4 *)nullptr, r, r * r, kernel, count, sum);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
