// Hard-masked position expansion of a chunk of rollout frames with the 25-frame running mask average
// (upsampling_network.py:159-174, `forward_with_context`), fused for T frames of one sequence.
//
// The reference clamps each raw mask to {0, 0.6} (NaN passes through), averages the last <= 25 clamped masks and keeps
// a point when the average exceeds 0.01.  Since 0.6f / 25 > 0.01 in any summation order and a NaN poisons the mean,
//     keep_t(i)  <=>  some frame f of the window has m_f(i) >= 0.6  and  no frame f of the window has m_f(i) NaN,
// so the history of a point is two int32: the last frame with a hit and the last frame with a NaN (TPG_CTX_NONE:
// never).  Three launches, no atomics, no cross-workgroup waits:
//   1. ctx_keep:   thread per point walks the T frames, updates its state; per (frame, 64-point tile) the keep bits
//                  (one 64-bit ballot) and the tile's output count (valid lanes + (r-1) * kept lanes);
//   2. ctx_scan:   one workgroup: exclusive scan of the counts in (frame, tile) order -> tile offsets + offsets (T+1);
//   3. ctx_write:  wave per (frame, tile): the lane's output start = tile offset + lanes before it + (r-1) * kept lanes
//                  before it (mbcnt of the keep bits); writes pos + edge * (keep ? 1 : 0) for slot 0 and, when kept,
//                  slots 1..r-1 -- the reference's arithmetic (multiply then add, no FMA), point-major, slot-minor.
#include "tpg_common.hpp"


namespace {

constexpr int CTX_WINDOW = 25;      // frames in the running average (upsampling_network.py:166-169)
constexpr int CTX_BLOCK = 256;      // 4 tiles of 64 points per workgroup in launches 1 and 3
constexpr int CTX_SCAN = 1024;

__device__ __forceinline__ unsigned ctx_lanes_below(tpg_u64 m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__global__ __launch_bounds__(CTX_BLOCK) void ctx_keep_kernel(const float *__restrict__ mask, int T, int N, int r, int t0,
                                                            int ntiles, int32_t *__restrict__ state,
                                                            tpg_u64 *__restrict__ bits, int32_t *__restrict__ counts) {
    const int tile = blockIdx.x * (CTX_BLOCK / TPG_WAVE) + threadIdx.x / TPG_WAVE;
    if (tile >= ntiles) return;                                   // whole waves only: the ballots below stay full
    const int lane = threadIdx.x % TPG_WAVE;
    const int i = tile * TPG_WAVE + lane;
    const bool valid = i < N;
    const int nvalid = min(N - tile * TPG_WAVE, TPG_WAVE);
    int last_hit = valid ? state[i] : TPG_CTX_NONE;
    int last_nan = valid ? state[N + i] : TPG_CTX_NONE;
    for (int k = 0; k < T; ++k) {
        const int t = t0 + k;
        const float m = valid ? mask[(size_t)k * N + i] : 0.0f;
        if (m >= 0.6f) last_hit = t;
        if (m != m) last_nan = t;
        const int lo = t - (CTX_WINDOW - 1);                      // window [max(0, lo), t]; frames are >= 0
        const bool keep = valid && last_hit >= lo && last_nan < lo;
        const tpg_u64 b = __ballot(keep);
        if (lane == 0) {
            bits[(size_t)k * ntiles + tile] = b;
            counts[(size_t)k * ntiles + tile] = nvalid + (r - 1) * __popcll(b);
        }
    }
    if (valid) {
        state[i] = last_hit;
        state[N + i] = last_nan;
    }
}

// Exclusive scan of M = T * ntiles counts, frame-major: thread j owns the contiguous run [j*L, (j+1)*L).
__global__ __launch_bounds__(CTX_SCAN) void ctx_scan_kernel(const int32_t *__restrict__ counts, long long M, int ntiles,
                                                           int T, int64_t *__restrict__ tile_off,
                                                           int64_t *__restrict__ offsets) {
    __shared__ long long part[CTX_SCAN];
    const int j = threadIdx.x;
    const long long L = (M + CTX_SCAN - 1) / CTX_SCAN;
    const long long b = min((long long)j * L, M), e = min(b + L, M);
    long long s = 0;
    for (long long q = b; q < e; ++q) s += counts[q];
    part[j] = s;
    __syncthreads();
    for (int d = 1; d < CTX_SCAN; d <<= 1) {                      // inclusive Hillis-Steele scan of the run sums
        const long long add = j >= d ? part[j - d] : 0;
        __syncthreads();
        part[j] += add;
        __syncthreads();
    }
    long long run = part[j] - s;                                  // exclusive
    int frame = (int)(b / ntiles), tile = (int)(b - (long long)frame * ntiles);
    for (long long q = b; q < e; ++q) {
        tile_off[q] = run;
        if (tile == 0) offsets[frame] = run;
        run += counts[q];
        if (++tile == ntiles) tile = 0, ++frame;
    }
    if (j == CTX_SCAN - 1) offsets[T] = part[j];
}

__global__ __launch_bounds__(CTX_BLOCK) void ctx_write_kernel(const float *__restrict__ pos,
                                                             const float *__restrict__ edge, int N, int r, int ntiles,
                                                             const tpg_u64 *__restrict__ bits,
                                                             const int64_t *__restrict__ tile_off,
                                                             float *__restrict__ out) {
    const int tile = blockIdx.x * (CTX_BLOCK / TPG_WAVE) + threadIdx.x / TPG_WAVE;
    const int k = blockIdx.y;
    if (tile >= ntiles) return;
    const int lane = threadIdx.x % TPG_WAVE;
    const int i = tile * TPG_WAVE + lane;
    if (i >= N) return;
    const tpg_u64 b = bits[(size_t)k * ntiles + tile];
    const bool keep = (b >> lane) & 1ull;
    const size_t o = (size_t)tile_off[(size_t)k * ntiles + tile] + lane + (size_t)(r - 1) * ctx_lanes_below(b);
    const size_t p = (size_t)k * N + i;
    const float px = pos[p * 3], py = pos[p * 3 + 1], pz = pos[p * 3 + 2];
    const float kf = keep ? 1.0f : 0.0f;
    const float *e = edge + p * r * 3;
    float *y = out + o * 3;
    const int slots = keep ? r : 1;
    // scalar fp32 multiply / add per coordinate (no packed v_pk_*_f32: see build.py on -fno-slp-vectorize)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int s = 0; s < slots; ++s) {
        y[s * 3] = px + e[s * 3] * kf;
        y[s * 3 + 1] = py + e[s * 3 + 1] * kf;
        y[s * 3 + 2] = pz + e[s * 3 + 2] * kf;
    }
}

size_t ctx_tiles(int N) { return ((size_t)N + TPG_WAVE - 1) / TPG_WAVE; }

}  // namespace

extern "C" size_t tpg_context_expand_workspace_bytes(int T, int N) {
    if (T <= 0 || N <= 0) return 0;
    const size_t M = (size_t)T * ctx_tiles(N);
    return M * (sizeof(tpg_u64) + sizeof(int64_t) + sizeof(int32_t));
}

extern "C" int tpg_context_expand_f32(const float *pos, const float *edge, const float *mask, int T, int N, int r,
                                      int t0, int32_t *state, float *out, int64_t *offsets, void *ws, void *stream) {
    if (T < 0 || N < 0 || t0 < 0 || T > 65535 || t0 > 2147483647 - T) return TPG_ERR_ARG;
    if (r < 2 || r > 16) return TPG_ERR_UNSUPPORTED;
    if (T == 0) return TPG_OK;
    if (!offsets) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    if (N == 0) {
        if (hipMemsetAsync(offsets, 0, sizeof(int64_t) * ((size_t)T + 1), st) != hipSuccess) return TPG_ERR_LAUNCH;
        return TPG_OK;
    }
    if (!pos || !edge || !mask || !state || !out || !ws) return TPG_ERR_ARG;
    if (((uintptr_t)ws & 7) != 0) return TPG_ERR_ARG;
    const int ntiles = (int)ctx_tiles(N);
    const long long M = (long long)T * ntiles;
    tpg_u64 *bits = reinterpret_cast<tpg_u64 *>(ws);
    int64_t *tile_off = reinterpret_cast<int64_t *>(bits + M);
    int32_t *counts = reinterpret_cast<int32_t *>(tile_off + M);
    const int blocks = (ntiles + CTX_BLOCK / TPG_WAVE - 1) / (CTX_BLOCK / TPG_WAVE);
    hipLaunchKernelGGL(ctx_keep_kernel, dim3(blocks), dim3(CTX_BLOCK), 0, st, mask, T, N, r, t0, ntiles, state, bits,
                       counts);
    TPG_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(ctx_scan_kernel, dim3(1), dim3(CTX_SCAN), 0, st, counts, M, ntiles, T, tile_off, offsets);
    TPG_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(ctx_write_kernel, dim3(blocks, T), dim3(CTX_BLOCK), 0, st, pos, edge, N, r, ntiles, bits,
                       tile_off, out);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
