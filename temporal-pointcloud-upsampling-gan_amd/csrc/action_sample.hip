// Batched action-clip sampler (train_action/msr_dataset.py:60-135 on the device): the two steps of a batch that
// csrc/clip_sample.hip and csrc/fps.hip do not already cover.
//
// tpg_frame_subset: a uniformly random ordered subset of K points per frame, for a ragged batch of frames -- what the
// reference asks np.random.choice(n, K, replace=False) for, frame by frame on the host.  Point j of a frame gets the
// 32-bit key
//     mix(h):  h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16        (uint32, wrapping)
//     key(j) = mix(mix(j * 0x9E3779B1 + seed_lo) ^ seed_hi)
// and the candidates are ordered by ascending (key, j).  Every step of key() is a bijection of uint32 (an odd
// multiplier, an add, xor-shifts, xors), so the keys of one frame are DISTINCT and the order is that of the keys alone.
// n > K: the K smallest in that order; n <= K: 0..n-1 repeated K / n times, then the K % n smallest in that order.
//
// ONE workgroup per frame does the whole selection: a depth frame has 10^3..10^5 points and a key costs a dozen integer
// instructions, so the frame's keys are simply recomputed in each of the four passes (three 11 + 11 + 10-bit histogram
// passes of a radix select in LDS for the ksel-th smallest key, one pass that collects the keys up to it) and the
// survivors are ordered by a bitonic sort in LDS, as sel_sort_kernel orders a patch (key, digits, block scan and sort
// are tpg_select.hpp's, shared with clip_sample.hip and dummy_centres.hip; the two-bin resolve is written out here).
// LDS atomics on integers and a sort of unique keys only: the result is a pure function of (count, seed, K), and nothing
// but idx is written to memory.
//
// tpg_action_gather_f32: all high-resolution clouds of the batch and their centroid in one launch, one workgroup per
// frame.  The centroid is an fp64 sum in a FIXED order (thread t adds rows t, t + 256, ... in that order; the 256
// partial sums are folded by a fixed tree), recomputed by every workgroup that needs it: no floating-point atomics, no
// workspace, no second launch, the same bits wherever and whenever it runs.
#include <math.h>

#include "tpg_select.hpp"

namespace {

constexpr int FS_THREADS = 1024;
constexpr int FS_GROUP = 32;                             // frames per launch (their rows travel as kernel arguments)

struct FsFrames {                                        // host arrays of one group of frames, passed by value
    int count[FS_GROUP];
    unsigned seed_lo[FS_GROUP], seed_hi[FS_GROUP];
};

// Points of the frame selected by the K % n (n <= K) or K (n > K) smallest keys.
__host__ __device__ inline int fs_selected(int n, int K) { return n > K ? K : K % n; }

// Digit PASS of the ksel-th smallest key of the frame: prefix = the digits found so far, krem = the rank left.
template <int PASS>
__device__ __forceinline__ void fs_digit(int n, unsigned lo, unsigned hi, unsigned *h, unsigned *s_scan, unsigned *s_out,
                                         unsigned *prefix, unsigned *krem) {
    const int t = threadIdx.x;
    for (int i = t; i < TPG_SEL_BINS; i += FS_THREADS) h[i] = 0;
    __syncthreads();
    for (int j = t; j < n; j += FS_THREADS) {
        const unsigned key = tpg_subset_key((unsigned)j, lo, hi);
        if (tpg_sel_matches<PASS>(key, *prefix)) atomicAdd(&h[tpg_sel_digit<PASS>(key)], 1u);
    }
    __syncthreads();
    // the bin that holds the krem-th smallest entry (the histogram's total is >= krem >= 1): two bins per thread,
    // written out by hand -- tpg_sel_resolve<FS_THREADS> gives the same bin but other code, not yet timed in this kernel
    const unsigned v0 = h[2 * t], v1 = h[2 * t + 1];
    const unsigned excl = tpg_block_excl_scan<FS_THREADS>(v0 + v1, s_scan, nullptr);
    if (excl < *krem && *krem <= excl + (v0 + v1)) {     // exactly one thread
        const bool first = *krem <= excl + v0;
        s_out[0] = (unsigned)(2 * t) + (first ? 0u : 1u);
        s_out[1] = *krem - excl - (first ? 0u : v0);
    }
    __syncthreads();
    *prefix |= tpg_sel_place<PASS>(s_out[0]);
    *krem = s_out[1];
    __syncthreads();
}

__global__ __launch_bounds__(FS_THREADS) void frame_subset_kernel(FsFrames fr, int f0, int K, int n2,
                                                                 int32_t *__restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) tpg_u64 fs_keys[];    // n2 slots
    __shared__ unsigned h[TPG_SEL_BINS];
    __shared__ unsigned s_scan[FS_THREADS];
    __shared__ unsigned s_out[3];                                        // bin, rank left, slot counter
    const int g = blockIdx.x, t = threadIdx.x;
    const int n = fr.count[g];
    const unsigned lo = fr.seed_lo[g], hi = fr.seed_hi[g];
    int32_t *out = idx + (size_t)(f0 + g) * K;
    const int ksel = fs_selected(n, K);
    const int lead = K - ksel;                           // n <= K: (K / n) * n entries that repeat 0..n-1
    for (int i = t; i < lead; i += FS_THREADS) out[i] = i % n;
    if (ksel == 0) return;                               // (uniform over the workgroup)

    // the ksel-th smallest key, digit by digit
    unsigned prefix = 0, krem = (unsigned)ksel;
    fs_digit<0>(n, lo, hi, h, s_scan, s_out, &prefix, &krem);
    fs_digit<1>(n, lo, hi, h, s_scan, s_out, &prefix, &krem);
    fs_digit<2>(n, lo, hi, h, s_scan, s_out, &prefix, &krem);
    const unsigned kth = prefix;                         // keys are distinct: exactly ksel of them are <= kth

    if (t == 0) s_out[2] = 0;
    for (int i = t; i < n2; i += FS_THREADS) fs_keys[i] = ~0ull;
    __syncthreads();
    for (int j = t; j < n; j += FS_THREADS) {
        const unsigned key = tpg_subset_key((unsigned)j, lo, hi);
        if (key <= kth) {
            const unsigned slot = atomicAdd(&s_out[2], 1u);              // any slot: the sort below fixes the order
            if (slot < (unsigned)n2) fs_keys[slot] = ((tpg_u64)key << 32) | (unsigned)j;
        }
    }
    __syncthreads();
    tpg_lds_bitonic_sort<FS_THREADS>(fs_keys, n2);
    for (int i = t; i < ksel; i += FS_THREADS) out[lead + i] = tpg_clamp_idx((int32_t)(unsigned)fs_keys[i], n);
}

// ---- gather + scale + centre ------------------------------------------------------------------------------------------
struct AgFrames {                                        // host arrays of one group of clips, passed by value
    TpgClipTable first, count;                           // first point of clip g's frame t, and its point count
    double scale[TPG_CLIP_GROUP * 3];
};

// Row k of frame (t,b): the stored point, y negated, times the clip's scale, over 300 -- fp64, in this order.
__device__ __forceinline__ void ag_row(const float *__restrict__ points, const int32_t *__restrict__ idx, int first,
                                       int count, int k, double sx, double sy, double sz, double v[3]) {
    const size_t src = ((size_t)first + (size_t)tpg_clamp_idx(idx[k], count)) * 3;
    v[0] = ((double)points[src] * sx) / 300.0;
    v[1] = ((double)(-points[src + 1]) * sy) / 300.0;
    v[2] = ((double)points[src + 2] * sz) / 300.0;
}

__global__ __launch_bounds__(TPG_CLIP_THREADS) void action_gather_kernel(const float *__restrict__ points, AgFrames fr,
                                                                        const int32_t *__restrict__ idx, int b0, int T,
                                                                        int B, int K, int per_frame,
                                                                        float *__restrict__ high,
                                                                        float *__restrict__ centre) {
    __shared__ double s_sum[3][TPG_CLIP_THREADS];
    const int g = blockIdx.x, t = blockIdx.y, b = b0 + g, tid = threadIdx.x;
    const double sx = fr.scale[g * 3], sy = fr.scale[g * 3 + 1], sz = fr.scale[g * 3 + 2];
    // the centroid: of this frame (test split) or of the clip's middle frame (train split)
    const int tc = per_frame ? t : T / 2;
    {
        const int32_t *ci = idx + ((size_t)tc * B + b) * K;
        const int cfirst = fr.first.at[tc * TPG_CLIP_GROUP + g], ccount = fr.count.at[tc * TPG_CLIP_GROUP + g];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, v[3];
        for (int k = tid; k < K; k += TPG_CLIP_THREADS) {
            ag_row(points, ci, cfirst, ccount, k, sx, sy, sz, v);
            a0 += v[0];
            a1 += v[1];
            a2 += v[2];
        }
        s_sum[0][tid] = a0;
        s_sum[1][tid] = a1;
        s_sum[2][tid] = a2;
        __syncthreads();
        for (int d = TPG_CLIP_THREADS / 2; d > 0; d >>= 1) {
            if (tid < d) {
                s_sum[0][tid] += s_sum[0][tid + d];
                s_sum[1][tid] += s_sum[1][tid + d];
                s_sum[2][tid] += s_sum[2][tid + d];
            }
            __syncthreads();
        }
    }
    const double c0 = s_sum[0][0] / (double)K, c1 = s_sum[1][0] / (double)K, c2 = s_sum[2][0] / (double)K;
    if (centre && tid == 0) {
        float *c = centre + ((size_t)t * B + b) * 3;
        c[0] = (float)c0;
        c[1] = (float)c1;
        c[2] = (float)c2;
    }
    const int32_t *fi = idx + ((size_t)t * B + b) * K;
    const int first = fr.first.at[t * TPG_CLIP_GROUP + g], count = fr.count.at[t * TPG_CLIP_GROUP + g];
    float *dst = high + ((size_t)t * B + b) * K * 3;
    for (int k = tid; k < K; k += TPG_CLIP_THREADS) {
        double v[3];
        ag_row(points, fi, first, count, k, sx, sy, sz, v);
        dst[(size_t)k * 3] = (float)(v[0] - c0);
        dst[(size_t)k * 3 + 1] = (float)(v[1] - c1);
        dst[(size_t)k * 3 + 2] = (float)(v[2] - c2);
    }
}

}  // namespace

extern "C" int tpg_frame_subset(const int32_t *count, const uint64_t *seed, int F, int K, int32_t *idx, void *stream) {
    if (F < 0) return TPG_ERR_ARG;
    if (F == 0) return TPG_OK;
    if (K < 1 || !count || !seed || !idx) return TPG_ERR_ARG;
    for (int f = 0; f < F; ++f)                          // host arrays: every frame is checked before anything is launched
        if (count[f] < 1) return TPG_ERR_ARG;
    if (K > TPG_PATCH_SELECT_MAX_K) return TPG_ERR_UNSUPPORTED;
    if (!tpg_allow_dynamic_lds<&frame_subset_kernel>((int)(TPG_PATCH_SELECT_MAX_K * sizeof(tpg_u64)))) return TPG_ERR_UNSUPPORTED;
    hipStream_t st = tpg_stream(stream);
    for (int f0 = 0; f0 < F; f0 += FS_GROUP) {
        const int nf = F - f0 < FS_GROUP ? F - f0 : FS_GROUP;
        FsFrames fr;
        int most = 1;
        for (int g = 0; g < FS_GROUP; ++g) {
            fr.count[g] = g < nf ? count[f0 + g] : 1;
            fr.seed_lo[g] = g < nf ? (unsigned)(seed[f0 + g] & 0xFFFFFFFFull) : 0u;
            fr.seed_hi[g] = g < nf ? (unsigned)(seed[f0 + g] >> 32) : 0u;
            if (g < nf && fs_selected(fr.count[g], K) > most) most = fs_selected(fr.count[g], K);
        }
        int n2 = 2;
        while (n2 < most) n2 <<= 1;
        hipLaunchKernelGGL(frame_subset_kernel, dim3(nf), dim3(FS_THREADS), (size_t)n2 * sizeof(tpg_u64), st, fr, f0, K, n2,
                           idx);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}

extern "C" int tpg_action_gather_f32(const float *points, long long P, const int32_t *frame_first, const int32_t *count,
                                     const int32_t *idx, const double *scale, int mode, int T, int B, int K, float *high,
                                     float *centre, void *stream) {
    if (T < 0 || B < 0 || K < 0 || P < 0) return TPG_ERR_ARG;
    if (mode != TPG_ACTION_TRAIN && mode != TPG_ACTION_TEST) return TPG_ERR_ARG;
    if (T == 0 || B == 0 || K == 0) return TPG_OK;
    if (T > TPG_CLIP_MAX_T) return TPG_ERR_UNSUPPORTED;
    if (!points || !frame_first || !count || !idx || !high) return TPG_ERR_ARG;
    if (mode == TPG_ACTION_TEST ? (scale != nullptr || centre == nullptr) : centre != nullptr) return TPG_ERR_ARG;
    for (int i = 0; i < T * B; ++i)
        if (count[i] < 1 || frame_first[i] < 0 || (long long)frame_first[i] + count[i] > P) return TPG_ERR_ARG;
    if (scale)
        for (int i = 0; i < B * 3; ++i)
            if (!isfinite(scale[i])) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    for (int b0 = 0; b0 < B; b0 += TPG_CLIP_GROUP) {
        const int nb = B - b0 < TPG_CLIP_GROUP ? B - b0 : TPG_CLIP_GROUP;
        AgFrames fr;
        fr.first = tpg_clip_table(frame_first, T, B, b0, 0);
        fr.count = tpg_clip_table(count, T, B, b0, 1);
        for (int i = 0; i < TPG_CLIP_GROUP * 3; ++i) fr.scale[i] = (scale && i < nb * 3) ? scale[b0 * 3 + i] : 1.0;
        hipLaunchKernelGGL(action_gather_kernel, dim3(nb, T), dim3(TPG_CLIP_THREADS), 0, st, points, fr, idx, b0, T, B,
                           K, mode == TPG_ACTION_TEST ? 1 : 0, high, centre);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}
