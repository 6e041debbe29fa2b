// Gaussian row sums: out[b][i] = sum_j exp(-c_ij / (2 sigma^2)) over every point j of cloud b, the building block of the
// Gaussian MMD between two clouds (reference: geomloss.SamplesLoss('gaussian', blur) in
// train_fluid/analysis_helper.py:226-227,256-260; tpgan_amd/metrics.py states the estimator).
//
// Exhaustive, one wave per row, the launch shape of rr_kernel<false> (csrc/radius_reduce.hip) -- the Gaussian has no
// cutoff, so there is no grid to walk.  c is the canonical fp32 squared distance, the exponent the fp32 product
// c * s with s = fp32(1 / (2 sigma^2)), the term expf(-(c * s)).
//
// Summation.  As radius_reduce.hip does for the cubic kernel: every term lies in [0, 1] and is converted ON ITS OWN to
// 64-bit fixed point with unit 2^-32 (truncated: an error below 2^-32 per term), and the terms are added as integers.
// The result does not depend on the order of the terms, the lane a term lands on, or the batch position.  A cloud has
// fewer than 2^17 points here (the entry refuses more), so a row sum is below 2^49 units and converts to float64
// exactly: the output is float64.
#include "tpg_common.hpp"

namespace {

constexpr int GS_WAVES = 4;
constexpr int GS_MAX_POINTS = (1 << 17) - 1;

__global__ __launch_bounds__(GS_WAVES * 64) void gs_kernel(const float *__restrict__ a, const float *__restrict__ bp,
                                                           const int64_t *__restrict__ lena,
                                                           const int64_t *__restrict__ lenb, int N, int M, float s,
                                                           double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int i = blockIdx.x * GS_WAVES + wave;
    if (i >= N) return;
    const size_t q = (size_t)b * N + i;
    const int na = lena ? (int)lena[b] : N;
    tpg_u64 acc = 0;
    if (i < na) {
        const float qx = a[q * 3], qy = a[q * 3 + 1], qz = a[q * 3 + 2];
        const int nb = lenb ? min(max((int)lenb[b], 0), M) : M;
        const float *x = bp + (size_t)b * M * 3;
        for (int j = lane; j < nb; j += 64) {
            const float c = tpg_sq3(qx, qy, qz, x[(size_t)j * 3], x[(size_t)j * 3 + 1], x[(size_t)j * 3 + 2]);
            const float w = fminf(expf(-(c * s)), 1.0f);
            acc += (tpg_u64)(w * 4294967296.0f);
        }
    }
    acc = tpg_wave_add_u64(acc);
    if (lane == 0) out[q] = (double)acc * 2.3283064365386963e-10;
}

}  // namespace

extern "C" int tpg_gaussian_row_sums_f32(const float *a, const float *b, const int64_t *lena, const int64_t *lenb,
                                         int B, int N, int M, float sigma, double *out, void *stream) {
    if (B < 0 || N < 0 || M < 0 || !(sigma > 0.0f)) return TPG_ERR_ARG;
    if (B == 0 || N == 0) return TPG_OK;
    if (!a || !out) return TPG_ERR_ARG;
    if (B > 65535 || M > GS_MAX_POINTS) return TPG_ERR_UNSUPPORTED;
    hipStream_t st = tpg_stream(stream);
    if (M == 0) {
        if (hipMemsetAsync(out, 0, sizeof(double) * (size_t)B * N, st) != hipSuccess) return TPG_ERR_LAUNCH;
        return TPG_OK;
    }
    if (!b) return TPG_ERR_ARG;
    const float s = (float)(1.0 / (2.0 * (double)sigma * (double)sigma));
    hipLaunchKernelGGL(gs_kernel, dim3((N + GS_WAVES - 1) / GS_WAVES, B), dim3(GS_WAVES * 64), 0, st, a, b, lena, lenb,
                       N, M, s, out);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
