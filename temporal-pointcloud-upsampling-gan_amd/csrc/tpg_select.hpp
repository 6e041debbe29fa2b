// What the two clip samplers (clip_sample.hip, action_sample.hip) and dummy_centres.hip share: the subset key, the
// radix select of the k-th smallest 32-bit key, the LDS sort of the survivors, and the per-launch tables of a group of
// clips.
//
// ONE definition of "the k-th smallest key is found digit by digit (bits 31..21, 20..10, 9..0) from a 2048-bin histogram
// of the keys that match the digits found so far; the survivors are ordered as (key << 32) | index": patch select walks
// global histograms with 256 threads, frame subset an LDS histogram with 1024.  Every piece is called by ALL `THREADS`
// threads of a 1-D workgroup.
#pragma once
#include "tpg_common.hpp"

// ---- the keyed order of tpg_frame_subset and tpg_replace_dummy_centres (include/tpgan_ops.h) ---------------------------
// Every step is a bijection of uint32 (an odd multiplier, an add, xor-shifts, xors): the keys of one seed are distinct.
__host__ __device__ inline unsigned tpg_mix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}
__host__ __device__ inline unsigned tpg_subset_key(unsigned j, unsigned seed_lo, unsigned seed_hi) {
    return tpg_mix32(tpg_mix32(j * 0x9E3779B1u + seed_lo) ^ seed_hi);
}

// ---- digits ---------------------------------------------------------------------------------------------------------
constexpr int TPG_SEL_BINS = 2048;
constexpr int TPG_SEL_SHIFT0 = 21, TPG_SEL_SHIFT1 = 10;  // digits: bits 31..21, 20..10, 9..0

template <int PASS>
__device__ __forceinline__ unsigned tpg_sel_digit(unsigned key) {
    if (PASS == 0) return key >> TPG_SEL_SHIFT0;
    if (PASS == 1) return (key >> TPG_SEL_SHIFT1) & (TPG_SEL_BINS - 1);
    return key & ((1u << TPG_SEL_SHIFT1) - 1);
}
// digit PASS, back in its place in the key
template <int PASS>
__device__ __forceinline__ unsigned tpg_sel_place(unsigned digit) {
    return digit << (PASS == 0 ? TPG_SEL_SHIFT0 : PASS == 1 ? TPG_SEL_SHIFT1 : 0);
}
// do the digits before PASS equal the prefix's?
template <int PASS>
__device__ __forceinline__ bool tpg_sel_matches(unsigned key, unsigned prefix) {
    if (PASS == 0) return true;
    if (PASS == 1) return (key >> TPG_SEL_SHIFT0) == (prefix >> TPG_SEL_SHIFT0);
    return (key >> TPG_SEL_SHIFT1) == (prefix >> TPG_SEL_SHIFT1);
}

// ---- scan, resolve ----------------------------------------------------------------------------------------------------
// Exclusive scan of one value per thread over the workgroup, through `s` (THREADS words of LDS); total: the sum, or null.
template <int THREADS>
__device__ __forceinline__ unsigned tpg_block_excl_scan(unsigned v, unsigned *s, unsigned *total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const unsigned add = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const unsigned incl = s[t];
    if (total) *total = s[THREADS - 1];
    __syncthreads();
    return incl - v;
}

// The bin of a finished histogram (TPG_SEL_BINS bins, total >= krem >= 1) that holds the krem-th smallest entry, and that
// entry's rank (1-based) inside the bin.  Uniform over the workgroup; LDS: s_scan[THREADS], s_out[2].  Patch select's
// use; frame_subset_kernel writes its two bins per thread out by hand (action_sample.hip).
template <int THREADS>
__device__ __forceinline__ void tpg_sel_resolve(const unsigned *hist, unsigned krem, unsigned *s_scan, unsigned *s_out,
                                                unsigned *bin, unsigned *krem_out) {
    constexpr int PER = TPG_SEL_BINS / THREADS;
    static_assert(PER * THREADS == TPG_SEL_BINS, "the threads share the bins evenly");
    const int t = threadIdx.x;
    unsigned v[PER], sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        v[i] = hist[t * PER + i];
        sum += v[i];
    }
    const unsigned excl = tpg_block_excl_scan<THREADS>(sum, s_scan, nullptr);
    if (excl < krem && krem <= excl + sum) {             // exactly one thread
        unsigned run = excl;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (krem <= run + v[i]) {
                s_out[0] = (unsigned)(t * PER + i);
                s_out[1] = krem - run;
                break;
            }
            run += v[i];
        }
    }
    __syncthreads();
    *bin = s_out[0];
    *krem_out = s_out[1];
    __syncthreads();
}

// ---- sort -------------------------------------------------------------------------------------------------------------
// Bitonic sort, ascending, of keys[0 .. n2) in LDS, n2 a power of two; a barrier after the fill before, one at the end.
template <int THREADS>
__device__ __forceinline__ void tpg_lds_bitonic_sort(tpg_u64 *keys, int n2) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const tpg_u64 a = keys[i], c = keys[p];
                    if ((a > c) == ((i & k) == 0)) {
                        keys[i] = c;
                        keys[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---- a group of clips' tables, passed to the gathers by value -----------------------------------------------------------
constexpr int TPG_CLIP_MAX_T = 8;                        // frames per clip; ops.py's CLIP_MAX_T says the same
constexpr int TPG_CLIP_GROUP = 32;                       // clips per launch (their rows travel as kernel arguments)
constexpr int TPG_CLIP_THREADS = 256;                    // workgroup of the three gathers

struct TpgClipTable {
    int at[TPG_CLIP_MAX_T * TPG_CLIP_GROUP];             // [t * TPG_CLIP_GROUP + g]: the entry of clip g's frame t
};

// The group of clips b0 .. b0 + TPG_CLIP_GROUP - 1 of a (T,B) host array (null: none); `pad` wherever there is no frame.
static inline TpgClipTable tpg_clip_table(const int32_t *src, int T, int B, int b0, int pad) {
    TpgClipTable tab;
    for (int t = 0; t < TPG_CLIP_MAX_T; ++t)
        for (int g = 0; g < TPG_CLIP_GROUP; ++g)
            tab.at[t * TPG_CLIP_GROUP + g] = (src && t < T && b0 + g < B) ? src[t * B + b0 + g] : pad;
    return tab;
}
