// Batched training-clip sampler (train_fluid/tempo_dataset.py:58-105 + train_utils.py:98-139,214-221 on the device).
//
// tpg_patch_select_f32: the K nearest stored points of ONE seed point per scene, K in the thousands, for a ragged batch
// of scenes -- what the reference asks a KD-tree for.  Selection key of candidate j: (bits of d2_j, j) with the canonical
// d2 = (dx*dx + dy*dy) + dz*dz in fp32 (tpg_sq3); a non-negative fp32 orders like its bit pattern, a NaN d2 counts as
// 0x7FC00000 (after +inf).  Result = the K smallest keys in ascending order.  A radix select on the 32 distance bits
// (11 + 11 + 10) finds the K-th key, the survivors are compacted and one workgroup per scene orders them in LDS (digits,
// block scan, resolve and bitonic sort: tpg_select.hpp, shared with action_sample.hip):
//
//   sel_hist<0,1,2>  (chunks, scenes) workgroups of SEL_CHUNK candidates: LDS histogram of the pass's digit over the
//                    candidates that match the digits found so far, added to the scene's global histogram (integer
//                    atomics: order-independent).  Every workgroup re-derives the earlier digits from the finished
//                    histograms itself (a 2048-bin scan: ~2 us, no extra launch, no cross-workgroup wait).
//   sel_ties         per chunk, the number of candidates whose distance EQUALS the K-th: ties are taken by ascending
//                    index, and a chunk's first tie has rank = the ties of the chunks before it.
//   sel_compact      keys below the K-th distance go to an arbitrary free slot (one slot counter per scene, one atomic
//                    per workgroup); the first `krem` ties go to slot K - krem + rank.  The slots' order is irrelevant:
//   sel_sort         bitonic sort of the scene's K keys (unique: the index is part of the key) in LDS, indices out.
// The result is therefore a pure function of the input: bit-identical from run to run and at every batch position.
//
// tpg_clip_gather_high_f32 / tpg_clip_gather_low_f32: every high- / low-resolution array of a batch in one launch each.
#include "tpg_select.hpp"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_PER_THREAD = 4;                        // consecutive candidates per thread (index order = thread order)
constexpr int SEL_CHUNK = SEL_THREADS * SEL_PER_THREAD;  // candidates per workgroup
constexpr int SEL_SORT_THREADS = 1024;
constexpr int SEL_GROUP = 32;                            // scenes per launch (their slices travel as kernel arguments)
constexpr unsigned SEL_NAN_KEY = 0x7FC00000u;

struct SelScenes {                                       // host arrays of one group of scenes, passed by value
    int first[SEL_GROUP], count[SEL_GROUP], seed[SEL_GROUP];
};

// per-scene workspace: 3 histograms | slot counter (+ 3 pad words) | tie count per chunk | K keys
struct SelWs {
    unsigned *hist;     // [3][TPG_SEL_BINS]
    unsigned *counter;  // [4]
    unsigned *ties;     // [chunks]
    tpg_u64 *keys;      // [K]
};

__host__ __device__ inline size_t sel_head_words(int chunks) {
    const size_t w = 3 * (size_t)TPG_SEL_BINS + 4 + (size_t)chunks;
    return (w + 1) & ~(size_t)1;                         // keys start 8-byte aligned
}
__host__ __device__ inline size_t sel_scene_bytes(int chunks, int K) { return sel_head_words(chunks) * 4 + (size_t)K * 8; }

__device__ __forceinline__ SelWs sel_ws(void *ws, int scene, int chunks, int K) {
    unsigned char *base = reinterpret_cast<unsigned char *>(ws) + (size_t)scene * sel_scene_bytes(chunks, K);
    SelWs w;
    w.hist = reinterpret_cast<unsigned *>(base);
    w.counter = w.hist + 3 * TPG_SEL_BINS;
    w.ties = w.counter + 4;
    w.keys = reinterpret_cast<tpg_u64 *>(base + sel_head_words(chunks) * 4);
    return w;
}

__device__ __forceinline__ unsigned sel_key(const float *__restrict__ pts, size_t j, float sx, float sy, float sz) {
    const float d2 = tpg_sq3(pts[j * 3], pts[j * 3 + 1], pts[j * 3 + 2], sx, sy, sz);
    return d2 != d2 ? SEL_NAN_KEY : __float_as_uint(d2);
}

// Digits 0 .. NP-1 of the K-th key from the finished histograms: prefix = those digits in place, krem = rank left.
template <int NP>
__device__ __forceinline__ void sel_prefix(const SelWs &w, int K, unsigned *s_scan, unsigned *s_out, unsigned *prefix,
                                           unsigned *krem) {
    unsigned p = 0, k = (unsigned)K, bin;
    if (NP >= 1) {
        tpg_sel_resolve<SEL_THREADS>(w.hist, k, s_scan, s_out, &bin, &k);
        p = tpg_sel_place<0>(bin);
    }
    if (NP >= 2) {
        tpg_sel_resolve<SEL_THREADS>(w.hist + TPG_SEL_BINS, k, s_scan, s_out, &bin, &k);
        p |= tpg_sel_place<1>(bin);
    }
    if (NP >= 3) {
        tpg_sel_resolve<SEL_THREADS>(w.hist + 2 * TPG_SEL_BINS, k, s_scan, s_out, &bin, &k);
        p |= tpg_sel_place<2>(bin);
    }
    *prefix = p;
    *krem = k;
}

template <int PASS>
__global__ __launch_bounds__(SEL_THREADS) void sel_hist_kernel(const float *__restrict__ points, SelScenes sc, int b0,
                                                              int K, int chunks, void *ws) {
    __shared__ unsigned h[TPG_SEL_BINS];
    __shared__ unsigned s_scan[SEL_THREADS];
    __shared__ unsigned s_out[2];
    const int g = blockIdx.y, n = sc.count[g];
    const int base = blockIdx.x * SEL_CHUNK;
    if (base >= n) return;
    const SelWs w = sel_ws(ws, b0 + g, chunks, K);
    for (int i = threadIdx.x; i < TPG_SEL_BINS; i += SEL_THREADS) h[i] = 0;
    unsigned prefix, krem;
    sel_prefix<PASS>(w, K, s_scan, s_out, &prefix, &krem);
    __syncthreads();
    const float *pts = points + (size_t)sc.first[g] * 3;
    const float sx = pts[(size_t)sc.seed[g] * 3], sy = pts[(size_t)sc.seed[g] * 3 + 1], sz = pts[(size_t)sc.seed[g] * 3 + 2];
#pragma unroll
    for (int i = 0; i < SEL_PER_THREAD; ++i) {
        const int j = base + threadIdx.x * SEL_PER_THREAD + i;
        if (j < n) {
            const unsigned key = sel_key(pts, (size_t)j, sx, sy, sz);
            if (tpg_sel_matches<PASS>(key, prefix)) atomicAdd(&h[tpg_sel_digit<PASS>(key)], 1u);
        }
    }
    __syncthreads();
    unsigned *gh = w.hist + PASS * TPG_SEL_BINS;
    for (int i = threadIdx.x; i < TPG_SEL_BINS; i += SEL_THREADS)
        if (h[i]) atomicAdd(&gh[i], h[i]);
}

__global__ __launch_bounds__(SEL_THREADS) void sel_ties_kernel(const float *__restrict__ points, SelScenes sc, int b0,
                                                              int K, int chunks, void *ws) {
    __shared__ unsigned s_scan[SEL_THREADS];
    __shared__ unsigned s_out[2];
    const int g = blockIdx.y, n = sc.count[g];
    const int base = blockIdx.x * SEL_CHUNK;
    if (base >= n) return;
    const SelWs w = sel_ws(ws, b0 + g, chunks, K);
    unsigned kth, krem;
    sel_prefix<3>(w, K, s_scan, s_out, &kth, &krem);
    const float *pts = points + (size_t)sc.first[g] * 3;
    const float sx = pts[(size_t)sc.seed[g] * 3], sy = pts[(size_t)sc.seed[g] * 3 + 1], sz = pts[(size_t)sc.seed[g] * 3 + 2];
    unsigned c = 0;
#pragma unroll
    for (int i = 0; i < SEL_PER_THREAD; ++i) {
        const int j = base + threadIdx.x * SEL_PER_THREAD + i;
        if (j < n && sel_key(pts, (size_t)j, sx, sy, sz) == kth) ++c;
    }
    unsigned total;
    tpg_block_excl_scan<SEL_THREADS>(c, s_scan, &total);
    if (threadIdx.x == 0) w.ties[blockIdx.x] = total;
}

__global__ __launch_bounds__(SEL_THREADS) void sel_compact_kernel(const float *__restrict__ points, SelScenes sc, int b0,
                                                                 int K, int chunks, void *ws) {
    __shared__ unsigned s_scan[SEL_THREADS];
    __shared__ unsigned s_out[2];
    const int g = blockIdx.y, n = sc.count[g];
    const int base = blockIdx.x * SEL_CHUNK;
    if (base >= n) return;
    const SelWs w = sel_ws(ws, b0 + g, chunks, K);
    unsigned kth, krem;
    sel_prefix<3>(w, K, s_scan, s_out, &kth, &krem);
    const unsigned below = (unsigned)K - krem;           // keys strictly below the K-th distance
    // ties in the chunks before this one
    unsigned part = 0, ties_before;
    for (int cidx = threadIdx.x; cidx < (int)blockIdx.x; cidx += SEL_THREADS) part += w.ties[cidx];
    tpg_block_excl_scan<SEL_THREADS>(part, s_scan, &ties_before);

    const float *pts = points + (size_t)sc.first[g] * 3;
    const float sx = pts[(size_t)sc.seed[g] * 3], sy = pts[(size_t)sc.seed[g] * 3 + 1], sz = pts[(size_t)sc.seed[g] * 3 + 2];
    unsigned key[SEL_PER_THREAD];
    unsigned nless = 0, ntie = 0;
#pragma unroll
    for (int i = 0; i < SEL_PER_THREAD; ++i) {
        const int j = base + threadIdx.x * SEL_PER_THREAD + i;
        key[i] = j < n ? sel_key(pts, (size_t)j, sx, sy, sz) : 0xFFFFFFFFu;
        if (j < n) {
            nless += key[i] < kth;
            ntie += key[i] == kth;
        }
    }
    // slots of the keys below: one counter bump per workgroup, order inside by thread (any order would do)
    unsigned less_total;
    const unsigned less_excl = tpg_block_excl_scan<SEL_THREADS>(nless, s_scan, &less_total);
    if (threadIdx.x == 0) s_out[0] = less_total ? atomicAdd(w.counter, less_total) : 0u;
    __syncthreads();
    unsigned slot = s_out[0] + less_excl;
    __syncthreads();
    unsigned rank = ties_before + tpg_block_excl_scan<SEL_THREADS>(ntie, s_scan, nullptr);
#pragma unroll
    for (int i = 0; i < SEL_PER_THREAD; ++i) {
        const int j = base + threadIdx.x * SEL_PER_THREAD + i;
        if (j >= n) continue;
        const tpg_u64 full = ((tpg_u64)key[i] << 32) | (unsigned)j;
        if (key[i] < kth) {
            if (slot < below) w.keys[slot] = full;       // (always true; the guard keeps a bad input inside the buffer)
            ++slot;
        } else if (key[i] == kth) {
            if (rank < krem) w.keys[below + rank] = full;
            ++rank;
        }
    }
}

__global__ __launch_bounds__(SEL_SORT_THREADS) void sel_sort_kernel(int b0, int K, int n2, int chunks, void *ws,
                                                                   int32_t *__restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) tpg_u64 sel_keys[];
    const int b = b0 + blockIdx.x;
    const SelWs w = sel_ws(ws, b, chunks, K);
    for (int i = threadIdx.x; i < n2; i += SEL_SORT_THREADS) sel_keys[i] = i < K ? w.keys[i] : ~0ull;
    __syncthreads();
    tpg_lds_bitonic_sort<SEL_SORT_THREADS>(sel_keys, n2);
    for (int i = threadIdx.x; i < K; i += SEL_SORT_THREADS) idx[(size_t)b * K + i] = (int32_t)(unsigned)sel_keys[i];
}

int sel_chunks(int max_count) { return (max_count + SEL_CHUNK - 1) / SEL_CHUNK; }

// ---- gathers ------------------------------------------------------------------------------------------------------
struct ClipFrames {                                      // host arrays of one group of clips, passed by value
    TpgClipTable first;                                  // first point of clip g's frame t
    int count[TPG_CLIP_GROUP];                           // particles of the clip's scene
    int crow[TPG_CLIP_GROUP];                            // row of the centre frame's centroid
};

__global__ __launch_bounds__(TPG_CLIP_THREADS) void clip_gather_high_kernel(const float *__restrict__ pos,
                                                                           const float *__restrict__ vel, ClipFrames cf,
                                                                           const float *__restrict__ centroids,
                                                                           const int32_t *__restrict__ patch, int b0,
                                                                           int B, int K, float *__restrict__ high_pos,
                                                                           float *__restrict__ high_vel) {
    const int k = blockIdx.x * TPG_CLIP_THREADS + threadIdx.x;
    const int g = blockIdx.y, t = blockIdx.z;
    if (k >= K) return;
    const int b = b0 + g;
    const int p = tpg_clamp_idx(patch[(size_t)b * K + k], cf.count[g]);
    const size_t src = ((size_t)cf.first.at[t * TPG_CLIP_GROUP + g] + (size_t)p) * 3;
    const size_t dst = (((size_t)t * B + b) * K + k) * 3;
    const float *c = centroids + (size_t)cf.crow[g] * 3;
    high_pos[dst] = pos[src] - c[0];
    high_pos[dst + 1] = pos[src + 1] - c[1];
    high_pos[dst + 2] = pos[src + 2] - c[2];
    if (vel) {
        high_vel[dst] = vel[src];
        high_vel[dst + 1] = vel[src + 1];
        high_vel[dst + 2] = vel[src + 2];
    }
}

__global__ __launch_bounds__(TPG_CLIP_THREADS) void clip_gather_low_kernel(const float *__restrict__ high_pos,
                                                                          const float *__restrict__ vel, ClipFrames cf,
                                                                          const int32_t *__restrict__ fps,
                                                                          const float *__restrict__ noise, float jitter,
                                                                          int b0, int B, int K, int M,
                                                                          float *__restrict__ low_pos,
                                                                          float *__restrict__ low_vel) {
    const int j = blockIdx.x * TPG_CLIP_THREADS + threadIdx.x;
    const int g = blockIdx.y, t = blockIdx.z;
    if (j >= M) return;
    const int b = b0 + g;
    const int f = fps[(size_t)b * M + j];
    const size_t src = (((size_t)t * B + b) * K + tpg_clamp_idx(f, K)) * 3;
    const size_t dst = (((size_t)t * B + b) * M + j) * 3;
    if (noise) {                                         // multiply, then add: two roundings (no FMA in this library)
        low_pos[dst] = high_pos[src] + noise[dst] * jitter;
        low_pos[dst + 1] = high_pos[src + 1] + noise[dst + 1] * jitter;
        low_pos[dst + 2] = high_pos[src + 2] + noise[dst + 2] * jitter;
    } else {
        low_pos[dst] = high_pos[src];
        low_pos[dst + 1] = high_pos[src + 1];
        low_pos[dst + 2] = high_pos[src + 2];
    }
    if (vel) {                                           // the reference's rows: fps[b,j] taken as a SCENE index
        const size_t v = ((size_t)cf.first.at[t * TPG_CLIP_GROUP + g] + (size_t)tpg_clamp_idx(f, cf.count[g])) * 3;
        low_vel[dst] = vel[v];
        low_vel[dst + 1] = vel[v + 1];
        low_vel[dst + 2] = vel[v + 2];
    }
}

}  // namespace

extern "C" int tpg_patch_select_max_k(void) { return TPG_PATCH_SELECT_MAX_K; }

extern "C" size_t tpg_patch_select_workspace_bytes(int B, int max_count, int K) {
    if (B <= 0 || max_count <= 0 || K <= 0) return 0;
    return (size_t)B * sel_scene_bytes(sel_chunks(max_count), K);
}

extern "C" int tpg_patch_select_f32(const float *points, long long P, const int32_t *first, const int32_t *count,
                                    const int32_t *seed, int B, int K, int32_t *idx, void *ws, void *stream) {
    if (B < 0 || P < 0) return TPG_ERR_ARG;
    if (B == 0) return TPG_OK;
    if (K <= 0 || !points || !first || !count || !seed || !idx || !ws) return TPG_ERR_ARG;
    if (((uintptr_t)ws & 7) != 0) return TPG_ERR_ARG;
    int max_count = 0;
    for (int b = 0; b < B; ++b) {                        // host arrays: every scene is checked before anything is launched
        if (first[b] < 0 || count[b] <= 0 || (long long)first[b] + count[b] > P) return TPG_ERR_ARG;
        if (K > count[b] || seed[b] < 0 || seed[b] >= count[b]) return TPG_ERR_ARG;
        if (count[b] > max_count) max_count = count[b];
    }
    if (K > TPG_PATCH_SELECT_MAX_K) return TPG_ERR_UNSUPPORTED;
    int n2 = 1;
    while (n2 < K) n2 <<= 1;
    const size_t smem = (size_t)n2 * sizeof(tpg_u64);
    hipStream_t st = tpg_stream(stream);
    if (!tpg_allow_dynamic_lds<&sel_sort_kernel>((int)(TPG_PATCH_SELECT_MAX_K * sizeof(tpg_u64)))) return TPG_ERR_UNSUPPORTED;
    const int chunks = sel_chunks(max_count);
    // histograms, slot counters (and the rest of the head) start at zero
    if (hipMemsetAsync(ws, 0, (size_t)B * sel_scene_bytes(chunks, K), st) != hipSuccess) return TPG_ERR_LAUNCH;
    for (int b0 = 0; b0 < B; b0 += SEL_GROUP) {
        const int nb = B - b0 < SEL_GROUP ? B - b0 : SEL_GROUP;
        SelScenes sc;
        int group_max = 0;
        for (int g = 0; g < SEL_GROUP; ++g) {
            sc.first[g] = g < nb ? first[b0 + g] : 0;
            sc.count[g] = g < nb ? count[b0 + g] : 0;
            sc.seed[g] = g < nb ? seed[b0 + g] : 0;
            if (sc.count[g] > group_max) group_max = sc.count[g];
        }
        const dim3 grid(sel_chunks(group_max), nb), block(SEL_THREADS);
        hipLaunchKernelGGL(sel_hist_kernel<0>, grid, block, 0, st, points, sc, b0, K, chunks, ws);
        TPG_RETURN_IF_LAUNCH_FAILED();
        hipLaunchKernelGGL(sel_hist_kernel<1>, grid, block, 0, st, points, sc, b0, K, chunks, ws);
        TPG_RETURN_IF_LAUNCH_FAILED();
        hipLaunchKernelGGL(sel_hist_kernel<2>, grid, block, 0, st, points, sc, b0, K, chunks, ws);
        TPG_RETURN_IF_LAUNCH_FAILED();
        hipLaunchKernelGGL(sel_ties_kernel, grid, block, 0, st, points, sc, b0, K, chunks, ws);
        TPG_RETURN_IF_LAUNCH_FAILED();
        hipLaunchKernelGGL(sel_compact_kernel, grid, block, 0, st, points, sc, b0, K, chunks, ws);
        TPG_RETURN_IF_LAUNCH_FAILED();
        hipLaunchKernelGGL(sel_sort_kernel, dim3(nb), dim3(SEL_SORT_THREADS), smem, st, b0, K, n2, chunks, ws, idx);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}

extern "C" int tpg_clip_gather_high_f32(const float *pos, const float *vel, long long P, const int32_t *frame_first,
                                        const int32_t *count, const float *centroids, int F, const int32_t *centroid_row,
                                        const int32_t *patch, int T, int B, int K, float *high_pos, float *high_vel,
                                        void *stream) {
    if (T < 0 || B < 0 || K < 0 || P < 0 || F < 0) return TPG_ERR_ARG;
    if (T == 0 || B == 0 || K == 0) return TPG_OK;
    if (T > TPG_CLIP_MAX_T) return TPG_ERR_UNSUPPORTED;
    if (!pos || !frame_first || !count || !centroids || !centroid_row || !patch || !high_pos) return TPG_ERR_ARG;
    if ((vel != nullptr) != (high_vel != nullptr)) return TPG_ERR_ARG;
    for (int b = 0; b < B; ++b) {
        if (count[b] <= 0 || centroid_row[b] < 0 || centroid_row[b] >= F) return TPG_ERR_ARG;
        for (int t = 0; t < T; ++t)
            if (frame_first[t * B + b] < 0 || (long long)frame_first[t * B + b] + count[b] > P) return TPG_ERR_ARG;
    }
    hipStream_t st = tpg_stream(stream);
    for (int b0 = 0; b0 < B; b0 += TPG_CLIP_GROUP) {
        const int nb = B - b0 < TPG_CLIP_GROUP ? B - b0 : TPG_CLIP_GROUP;
        ClipFrames cf;
        cf.first = tpg_clip_table(frame_first, T, B, b0, 0);
        for (int g = 0; g < TPG_CLIP_GROUP; ++g) {
            cf.count[g] = g < nb ? count[b0 + g] : 1;
            cf.crow[g] = g < nb ? centroid_row[b0 + g] : 0;
        }
        const dim3 grid((K + TPG_CLIP_THREADS - 1) / TPG_CLIP_THREADS, nb, T);
        hipLaunchKernelGGL(clip_gather_high_kernel, grid, dim3(TPG_CLIP_THREADS), 0, st, pos, vel, cf, centroids, patch, b0,
                           B, K, high_pos, high_vel);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}

extern "C" int tpg_clip_gather_low_f32(const float *high_pos, const int32_t *fps, const float *noise, float jitter,
                                       const float *vel, long long P, const int32_t *frame_first, const int32_t *count,
                                       int T, int B, int K, int M, float *low_pos, float *low_vel, void *stream) {
    if (T < 0 || B < 0 || K < 0 || M < 0 || P < 0) return TPG_ERR_ARG;
    if (T == 0 || B == 0 || M == 0) return TPG_OK;
    if (T > TPG_CLIP_MAX_T) return TPG_ERR_UNSUPPORTED;
    if (K == 0 || !high_pos || !fps || !low_pos) return TPG_ERR_ARG;
    if ((vel != nullptr) != (low_vel != nullptr)) return TPG_ERR_ARG;
    if (vel) {
        if (!frame_first || !count) return TPG_ERR_ARG;
        for (int b = 0; b < B; ++b) {
            if (count[b] <= 0) return TPG_ERR_ARG;
            for (int t = 0; t < T; ++t)
                if (frame_first[t * B + b] < 0 || (long long)frame_first[t * B + b] + count[b] > P) return TPG_ERR_ARG;
        }
    }
    hipStream_t st = tpg_stream(stream);
    for (int b0 = 0; b0 < B; b0 += TPG_CLIP_GROUP) {
        const int nb = B - b0 < TPG_CLIP_GROUP ? B - b0 : TPG_CLIP_GROUP;
        ClipFrames cf;
        cf.first = tpg_clip_table(vel ? frame_first : nullptr, T, B, b0, 0);
        for (int g = 0; g < TPG_CLIP_GROUP; ++g) {
            cf.count[g] = (vel && g < nb) ? count[b0 + g] : 1;
            cf.crow[g] = 0;
        }
        const dim3 grid((M + TPG_CLIP_THREADS - 1) / TPG_CLIP_THREADS, nb, T);
        hipLaunchKernelGGL(clip_gather_low_kernel, grid, dim3(TPG_CLIP_THREADS), 0, st, high_pos, vel, cf, fps, noise,
                           jitter, b0, B, K, M, low_pos, low_vel);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}
