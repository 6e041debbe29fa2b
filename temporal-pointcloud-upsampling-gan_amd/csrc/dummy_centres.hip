// Dummy-centre replacement of the discriminators' set-abstraction levels (discriminator.py:115-130) on the device.
//
// tpg_replace_dummy_centres: FPS picks that landed on a 999-padded point are swapped for other points of the cloud.
// The reference finds the hits on the host and draws the replacements with np.random.choice; here the draw is the
// keyed order of tpg_frame_subset (tpg_subset_key, tpg_select.hpp) with a seed per (draw_key, site, cloud), so a
// captured step replays it with no host involvement.  The rule is stated in include/tpgan_ops.h.
//
// ONE workgroup per cloud.  Thread t owns the slots t*per .. t*per + per - 1, so a block scan of the survivors per
// thread is the stable compaction.  A cloud without a hit leaves after the hit scan (one gather of S rows and the copy
// of its row): that is all an all-keep step pays.  Otherwise the k-th smallest key of the pool is found digit by digit
// on an LDS histogram (three passes over the N keys, a dozen integer instructions each), the k keys up to it are
// collected and ordered by a bitonic sort in LDS as (key << 32) | j.  LDS atomics on integers and a sort of unique
// keys only: the result is a pure function of the inputs.
#include <math.h>

#include "tpg_select.hpp"

namespace {

constexpr int DC_THREADS = 1024;

__device__ __forceinline__ bool dc_in_pool(int j, int S, const unsigned char *s_hit) { return !(j < S && s_hit[j]); }

// Digit PASS of the krem-th smallest key of the pool: prefix = the digits found so far, krem = the rank left.
template <int PASS>
__device__ __forceinline__ void dc_digit(int N, int S, const unsigned char *s_hit, unsigned lo, unsigned hi, unsigned *h,
                                         unsigned *s_scan, unsigned *s_out, unsigned *prefix, unsigned *krem) {
    for (int i = threadIdx.x; i < TPG_SEL_BINS; i += DC_THREADS) h[i] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < N; j += DC_THREADS) {
        if (!dc_in_pool(j, S, s_hit)) continue;
        const unsigned key = tpg_subset_key((unsigned)j, lo, hi);
        if (tpg_sel_matches<PASS>(key, *prefix)) atomicAdd(&h[tpg_sel_digit<PASS>(key)], 1u);
    }
    __syncthreads();
    unsigned bin;
    tpg_sel_resolve<DC_THREADS>(h, *krem, s_scan, s_out, &bin, krem);
    *prefix |= tpg_sel_place<PASS>(bin);
}

__global__ __launch_bounds__(DC_THREADS) void dummy_centres_kernel(const float *__restrict__ xyz,
                                                                  const int32_t *__restrict__ centres,
                                                                  const int64_t *__restrict__ draw_key, unsigned site,
                                                                  int N, int S, int per, int n2cap,
                                                                  int32_t *__restrict__ out,
                                                                  int32_t *__restrict__ prefix_flag,
                                                                  int32_t *__restrict__ short_flag) {
    extern __shared__ __attribute__((aligned(16))) tpg_u64 dc_keys[];    // n2cap keys, then the S hit bytes
    __shared__ unsigned h[TPG_SEL_BINS];
    __shared__ unsigned s_scan[DC_THREADS];
    __shared__ unsigned s_out[3];                                        // bin, rank left, slot counter
    unsigned char *s_hit = reinterpret_cast<unsigned char *>(dc_keys + n2cap);
    const int b = blockIdx.x, t = threadIdx.x;
    const float *pts = xyz + (size_t)b * N * 3;
    const int32_t *row = centres + (size_t)b * S;
    int32_t *dst = out + (size_t)b * S;
    const int s0 = t * per < S ? t * per : S, s1 = s0 + per < S ? s0 + per : S;

    // survivors of this thread's slots (low half) and its hit slots that are pool positions, s < N (high half): one
    // scan serves both, S <= 16384 keeps the halves apart
    unsigned kept = 0, barred = 0;
    for (int s = s0; s < s1; ++s) {
        const bool hit = fabsf(pts[(size_t)tpg_clamp_idx(row[s], N) * 3] - 999.0f) < 1e-4f;
        s_hit[s] = hit ? 1 : 0;
        kept += hit ? 0u : 1u;
        barred += (hit && s < N) ? 1u : 0u;
    }
    if (!__syncthreads_or(kept != (unsigned)(s1 - s0))) {                // k == 0: the row as it is
        for (int s = s0; s < s1; ++s) dst[s] = row[s];
        return;
    }
    unsigned total;
    unsigned at = tpg_block_excl_scan<DC_THREADS>(kept | (barred << 16), s_scan, &total) & 0xFFFFu;
    const unsigned survivors = total & 0xFFFFu;
    const int k = S - (int)survivors, pool = N - (int)(total >> 16);
    if (pool < k) {                                                      // the reference's choice() raises here
        for (int s = s0; s < s1; ++s) dst[s] = row[s];
        if (t == 0) *short_flag = 1;
        return;
    }
    for (int s = s0; s < s1; ++s)
        if (!s_hit[s]) dst[at++] = row[s];
    if (t == 0 && prefix_flag) prefix_flag[b] = 0;                       // no longer in pick order

    const tpg_u64 seed = (tpg_u64)draw_key[0], iter = (tpg_u64)draw_key[1];
    const unsigned lo = tpg_mix32((unsigned)seed ^ tpg_mix32((unsigned)iter * 0x9E3779B1u + site));
    const unsigned hi = tpg_mix32((unsigned)(seed >> 32) ^ tpg_mix32((unsigned)b * 0x85EBCA6Bu + site));

    // the k-th smallest key of the pool (pool >= k >= 1 members), digit by digit
    unsigned prefix = 0, krem = (unsigned)k;
    dc_digit<0>(N, S, s_hit, lo, hi, h, s_scan, s_out, &prefix, &krem);
    dc_digit<1>(N, S, s_hit, lo, hi, h, s_scan, s_out, &prefix, &krem);
    dc_digit<2>(N, S, s_hit, lo, hi, h, s_scan, s_out, &prefix, &krem);
    const unsigned kth = prefix;                         // keys are distinct: exactly k pool members are <= kth

    int n2 = 2;
    while (n2 < k) n2 <<= 1;                             // k <= the host's bound <= n2cap
    if (t == 0) s_out[2] = 0;
    for (int i = t; i < n2; i += DC_THREADS) dc_keys[i] = ~0ull;
    __syncthreads();
    for (int j = t; j < N; j += DC_THREADS) {
        if (!dc_in_pool(j, S, s_hit)) continue;
        const unsigned key = tpg_subset_key((unsigned)j, lo, hi);
        if (key <= kth) {
            const unsigned slot = atomicAdd(&s_out[2], 1u);              // any slot: the sort below fixes the order
            if (slot < (unsigned)n2) dc_keys[slot] = ((tpg_u64)key << 32) | (unsigned)j;
        }
    }
    __syncthreads();
    tpg_lds_bitonic_sort<DC_THREADS>(dc_keys, n2);
    for (int i = t; i < k; i += DC_THREADS) dst[survivors + i] = tpg_clamp_idx((int32_t)(unsigned)dc_keys[i], N);
}

size_t dc_lds_bytes(int n2cap, int S) { return (size_t)n2cap * sizeof(tpg_u64) + (((size_t)S + 7) & ~(size_t)7); }

}  // namespace

extern "C" int tpg_replace_dummy_centres(const float *xyz, const int32_t *centres, const int64_t *draw_key, int site,
                                         int B, int N, int S, int32_t *out, int32_t *prefix_flag, int32_t *short_flag,
                                         void *stream) {
    if (B < 0 || N < 0 || S < 0 || site < 0) return TPG_ERR_ARG;
    if (B == 0 || S == 0) return TPG_OK;
    if (N == 0 || !xyz || !centres || !draw_key || !out || !short_flag || out == centres) return TPG_ERR_ARG;
    if (S > TPG_PATCH_SELECT_MAX_K) return TPG_ERR_UNSUPPORTED;
    if (!tpg_allow_dynamic_lds<&dummy_centres_kernel>((int)dc_lds_bytes(TPG_PATCH_SELECT_MAX_K, TPG_PATCH_SELECT_MAX_K)))
        return TPG_ERR_UNSUPPORTED;
    // a served cloud has k <= S hits and a pool of at least k: of N - k members while S <= N, of at most N beyond
    const int bound = S <= N ? N / 2 : N, most = S < bound ? S : bound;
    int n2cap = 2;
    while (n2cap < most) n2cap <<= 1;
    hipStream_t st = tpg_stream(stream);
    if (hipMemsetAsync(short_flag, 0, sizeof(int32_t), st) != hipSuccess) return TPG_ERR_LAUNCH;
    hipLaunchKernelGGL(dummy_centres_kernel, dim3(B), dim3(DC_THREADS), dc_lds_bytes(n2cap, S), st, xyz, centres,
                       draw_key, (unsigned)site, N, S, (S + DC_THREADS - 1) / DC_THREADS, n2cap, out, prefix_flag,
                       short_flag);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
