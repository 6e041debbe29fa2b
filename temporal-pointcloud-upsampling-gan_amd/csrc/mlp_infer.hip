// Forward-only shared-MLP tail with eval-mode BatchNorm, one launch per tail:
//
//     out[b,s,:] = max_{j<K} act_L(a_L * (W_L ... act_1(a_1 * (W_1 act_0(U[b,idx[b,s,j],:] - Q[b,s,:])) + c_1) ...) + c_L)
//     act_l(z) = max(z, slope_l * z)
//
// Eval-mode BatchNorm is a constant per-channel affine (a_l, c_l), so nothing couples the rows of a tail and nothing
// forces a launch boundary between its layers: the grouped rows (B*S*K, C_0) that ops.row_combine writes and every
// per-layer intermediate stay in registers / LDS.  The launch reads the N-row table U, the S-row table Q and the
// index list and writes S rows per cloud.  The input affine (a_0, c_0) is folded into U and Q by the caller.
//
// Work split: a WAVE owns a group (b,s) and walks its K/16 strips of 16 neighbours, STRIPS at a time; no workgroup
// barrier after the weights are staged.
//   layer 1   A fragment = the lane's 8 consecutive channels of the gathered row (fp32 or bf16 table) minus the centre
//             row in fp32 -- fp32 tables are NOT rounded before the subtraction --, activation in fp32, packed to bf16; v_mfma_f32_16x16x32_bf16 against W_1.
//   hand-off  affine + activation in fp32 on the accumulators (4 rows x T channels per lane), rounded to bf16 and
//             written to a per-wave LDS scratch of 16 rows x C_1 (16-byte chunks XOR-swizzled by the row: no padding,
//             two-way conflicts at worst), read back as the A fragments of layer 2 (row li, channels 32 s + 8 lq ..).
//   max       affine + activation in fp32, max over the lane's 4 accumulator rows, over the strips in registers,
//             over the lane quarters by two cross-lane moves at the end; one bf16 rounding at the store.  No atomics:
//             the same input gives the same bits, whatever the grid.
// Weights are bf16 in MFMA B-fragment order (packed by the caller, ops.pack_infer_weight): fragment (t, s) is 64
// consecutive 16-byte vectors, lane (li, lq) holding W[li*T + t][32 s + 8 lq .. + 8] -- the channel-order trick of
// mlp_fused.hip (tile t, column j = channel j*T + t), so a lane's T accumulators of a row are T consecutive channels.
// They are staged in LDS by a plain copy when they fit next to the scratch in 160 KB; (256,256,256) keeps W_1 there
// and reads W_2's fragments from global memory (128 KB, L2-resident, coalesced 1 KB per fragment), a k-step ahead of
// their MFMAs (measured at 128 clouds x 256 x 32 rows: 1.14 ms with four fragments in flight, 0.93 ms a k-step ahead).
#include "tpg_rows.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;   // one MFMA A / B fragment (4 VGPRs)

constexpr int MI_THREADS = 256;
constexpr int MI_WAVES = MI_THREADS / 64;
constexpr int MI_LDS_MAX = 160 * 1024;

template <int C0, int C1, int C2> struct mi_plan {
    static constexpr int CH = C2 ? C1 : 0;                       // width of the hand-off rows (none for one weight)
    static constexpr int W1B = C1 * C0 * 2, W2B = C2 * C1 * 2;   // bytes of the packed weights
    static constexpr int SCR = MI_WAVES * 16 * CH * 2;
    static constexpr bool W2L = C2 != 0 && W1B + W2B + SCR <= MI_LDS_MAX;
    static constexpr bool W1L = W1B + SCR + (W2L ? W2B : 0) <= MI_LDS_MAX;
    static constexpr int SMEM = (W1L ? W1B : 0) + (W2L ? W2B : 0) + SCR;
};

__device__ __forceinline__ bf16x8 mi_frag(const uint4 v) {
    union { uint4 u; bf16x8 f; } cv;
    cv.u = v;
    return cv.f;
}

// affine + activation + max over the lane's 4 rows of one strip, folded into the running maxima
template <int T>
__device__ __forceinline__ void mi_fold_max(const tpg_f32x4 (&acc)[T], const float *__restrict__ a,
                                            const float *__restrict__ c, float slope, int li, float (&rmax)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float av = a[li * T + t], cv = c[li * T + t];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float z = __builtin_fmaf(acc[t][r], av, cv);
            z = fmaxf(z, z * slope);
            rmax[t] = fmaxf(rmax[t], z);
        }
    }
}

// grid (G); U (B,N,C0), Q (B,S,C0) of TU = fp32 or bf16; idx (B*S, K) int32; W1p / W2p packed bf16 fragments; a / c per-channel fp32;
// out (B*S, CL) bf16.  groups = B*S.
template <typename TU, int C0, int C1, int C2, int STRIPS>
__global__ __launch_bounds__(MI_THREADS) void mlp_infer_kernel(
    const TU *__restrict__ U, const TU *__restrict__ Q, const int *__restrict__ idx, int N, int S,
    int K, long long groups, const uint4 *__restrict__ W1p, const uint4 *__restrict__ W2p, const float *__restrict__ a1,
    const float *__restrict__ c1, const float *__restrict__ a2, const float *__restrict__ c2, float slope0, float slope1,
    float slope2, __hip_bfloat16 *__restrict__ out) {
    using P = mi_plan<C0, C1, C2>;
    constexpr int KS0 = C0 / 32, T1 = C1 / 16, KS1 = C1 / 32, T2 = C2 / 16;
    constexpr int CL = C2 ? C2 : C1, TL = CL / 16;
    static_assert(T1 == 4 || T1 % 8 == 0, "hand-off stores are 8 or 16 bytes");
    static_assert(TL % 8 == 0, "the output row store is 16-byte vectors");
    extern __shared__ __attribute__((aligned(16))) unsigned char mi_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    uint4 *w1l = reinterpret_cast<uint4 *>(mi_smem);
    uint4 *w2l = reinterpret_cast<uint4 *>(mi_smem + (P::W1L ? P::W1B : 0));
    unsigned char *scr = mi_smem + (P::W1L ? P::W1B : 0) + (P::W2L ? P::W2B : 0) + wave * 16 * P::CH * 2;
    if constexpr (P::W1L)
        for (int e = tid; e < P::W1B / 16; e += MI_THREADS) w1l[e] = W1p[e];
    if constexpr (P::W2L)
        for (int e = tid; e < P::W2B / 16; e += MI_THREADS) w2l[e] = W2p[e];
    __syncthreads();

    for (long long g = (long long)blockIdx.x * MI_WAVES + wave; g < groups; g += (long long)gridDim.x * MI_WAVES) {
        const int *gi = idx + (size_t)g * K;
        const TU *Ub = U + (size_t)(g / S) * N * C0 + 8 * lq;
        const TU *Qg = Q + (size_t)g * C0 + 8 * lq;
        float rmax[TL];
#pragma unroll
        for (int t = 0; t < TL; ++t) rmax[t] = -INFINITY;

        for (int j0 = 0; j0 < K; j0 += 16 * STRIPS) {
            // ---- gather: the lane's 8 channels per k-step of neighbour row li of every strip, minus the centre row.
            // The difference is taken in fp32 on the tables' own values (fp32 tables: no rounding before it) and
            // rounded ONCE, after the activation, where it becomes the A operand.
            bf16x8 afr[STRIPS][KS0];
            {
                const TU *pu[STRIPS];
#pragma unroll
                for (int st = 0; st < STRIPS; ++st) pu[st] = Ub + (size_t)tpg_clamp_idx(gi[j0 + st * 16 + li], N) * C0;
#pragma unroll
                for (int s = 0; s < KS0; ++s) {
                    float q[8];
                    tpg_load_row<TU, 8>(Qg + 32 * s, q);
#pragma unroll
                    for (int st = 0; st < STRIPS; ++st) {
                        float u[8];
                        tpg_load_row<TU, 8>(pu[st] + 32 * s, u);
                        union { unsigned w[4]; bf16x8 v; } cv;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float a = u[2 * i] - q[2 * i], b = u[2 * i + 1] - q[2 * i + 1];
                            a = fmaxf(a, a * slope0);
                            b = fmaxf(b, b * slope0);
                            cv.w[i] = tpg_pack_bf16x2(a, b);
                        }
                        afr[st][s] = cv.v;
                    }
                }
            }
            // the global weight pointers are re-read as opaque values per chunk: W1p / W2p are read-only and not aliased,
            // so the compiler would otherwise lift EVERY fragment load out of both loops (T*KS*4 registers, spilled)
            const uint4 *w1g = W1p, *w2g = W2p;
            asm volatile("" : "+s"(w1g), "+s"(w2g));
            // ---- layer 1
            tpg_f32x4 acc1[STRIPS][T1];
#pragma unroll
            for (int st = 0; st < STRIPS; ++st)
#pragma unroll
                for (int t = 0; t < T1; ++t) acc1[st][t] = tpg_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < KS0; ++s) {
#pragma unroll
                for (int t = 0; t < T1; ++t) {
                    bf16x8 b;
                    if constexpr (P::W1L) b = mi_frag(w1l[(t * KS0 + s) * 64 + lane]);
                    else b = mi_frag(w1g[(t * KS0 + s) * 64 + lane]);
#pragma unroll
                    for (int st = 0; st < STRIPS; ++st)
                        acc1[st][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[st][s], b, acc1[st][t], 0, 0, 0);
                    if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // as mlp_fwd_kernel: no hoisting of every B read
                }
            }
            if constexpr (C2 == 0) {
#pragma unroll
                for (int st = 0; st < STRIPS; ++st) mi_fold_max<T1>(acc1[st], a1, c1, slope1, li, rmax);
            } else {
                // ---- hand-off: accumulator layout (rows 4 lq + r, channels li*T1 ..) -> A fragments (row li)
                bf16x8 a2f[STRIPS][KS1];
#pragma unroll
                for (int st = 0; st < STRIPS; ++st) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 4 * lq + r;
                        unsigned o[T1 / 2];
#pragma unroll
                        for (int t = 0; t < T1; t += 2) {
                            float z0 = __builtin_fmaf(acc1[st][t][r], a1[li * T1 + t], c1[li * T1 + t]);
                            float z1 = __builtin_fmaf(acc1[st][t + 1][r], a1[li * T1 + t + 1], c1[li * T1 + t + 1]);
                            z0 = fmaxf(z0, z0 * slope1);
                            z1 = fmaxf(z1, z1 * slope1);
                            o[t / 2] = tpg_pack_bf16x2(z0, z1);
                        }
                        unsigned char *prow = scr + row * (C1 * 2);
                        if constexpr (T1 == 4) {
                            const int chunk = (li >> 1) ^ (row & 7);
                            *reinterpret_cast<uint2 *>(prow + chunk * 16 + (li & 1) * 8) = make_uint2(o[0], o[1]);
                        } else {
#pragma unroll
                            for (int v = 0; v < T1 / 8; ++v) {
                                const int chunk = (li * (T1 / 8) + v) ^ (row & 7);
                                *reinterpret_cast<uint4 *>(prow + chunk * 16) =
                                    make_uint4(o[4 * v], o[4 * v + 1], o[4 * v + 2], o[4 * v + 3]);
                            }
                        }
                    }
                    // the scratch is this wave's own: LDS operations of a wave complete in order, the fences keep the
                    // compiler from moving the reads over the writes (and the next strip's writes over these reads)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                    for (int s = 0; s < KS1; ++s) {
                        const int chunk = (4 * s + lq) ^ (li & 7);
                        a2f[st][s] = mi_frag(*reinterpret_cast<const uint4 *>(scr + li * (C1 * 2) + chunk * 16));
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                // ---- layer 2
                constexpr int T2N = T2 ? T2 : 1;
                tpg_f32x4 acc2[STRIPS][T2N];
#pragma unroll
                for (int st = 0; st < STRIPS; ++st)
#pragma unroll
                    for (int t = 0; t < T2N; ++t) acc2[st][t] = tpg_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if constexpr (P::W2L) {
#pragma unroll
                    for (int s = 0; s < KS1; ++s) {
#pragma unroll
                        for (int t = 0; t < T2N; ++t) {
                            const bf16x8 b = mi_frag(w2l[(t * KS1 + s) * 64 + lane]);
#pragma unroll
                            for (int st = 0; st < STRIPS; ++st)
                                acc2[st][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2f[st][s], b, acc2[st][t], 0, 0, 0);
                            if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                } else {
                    // W_2 from global memory (L2): one wave per SIMD and a round trip of several hundred cycles per
                    // fragment -- the T2 fragments of k-step s + 1 are requested before the MFMAs of k-step s run
                    uint4 bq[2][T2N];
#pragma unroll
                    for (int t = 0; t < T2N; ++t) bq[0][t] = w2g[(t * KS1) * 64 + lane];
#pragma unroll
                    for (int s = 0; s < KS1; ++s) {
                        if (s + 1 < KS1) {
#pragma unroll
                            for (int t = 0; t < T2N; ++t) bq[(s + 1) & 1][t] = w2g[(t * KS1 + s + 1) * 64 + lane];
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int t = 0; t < T2N; ++t)
#pragma unroll
                            for (int st = 0; st < STRIPS; ++st)
                                acc2[st][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2f[st][s], mi_frag(bq[s & 1][t]),
                                                                                      acc2[st][t], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
#pragma unroll
                for (int st = 0; st < STRIPS; ++st) mi_fold_max<T2N>(acc2[st], a2, c2, slope2, li, rmax);
            }
        }
        // ---- max over the lane quarters (rows 4 lq + r of every strip), one rounding, 16 lanes write the row
#pragma unroll
        for (int t = 0; t < TL; ++t) {
            rmax[t] = fmaxf(rmax[t], __shfl_xor(rmax[t], 16, 64));
            rmax[t] = fmaxf(rmax[t], __shfl_xor(rmax[t], 32, 64));
        }
        if (lq == 0) {
            __hip_bfloat16 *po = out + (size_t)g * CL + li * TL;
#pragma unroll
            for (int v = 0; v < TL / 8; ++v)
                reinterpret_cast<uint4 *>(po)[v] =
                    make_uint4(tpg_pack_bf16x2(rmax[8 * v], rmax[8 * v + 1]), tpg_pack_bf16x2(rmax[8 * v + 2], rmax[8 * v + 3]),
                               tpg_pack_bf16x2(rmax[8 * v + 4], rmax[8 * v + 5]), tpg_pack_bf16x2(rmax[8 * v + 6], rmax[8 * v + 7]));
        }
    }
}

template <typename TU, int C0, int C1, int C2, int STRIPS>
int mi_launch(const void *U, const void *Q, const int32_t *idx, int N, int S, int K, long long groups, const void *W1p,
              const void *W2p, const float *a1, const float *c1, const float *a2, const float *c2, float s0, float s1,
              float s2, void *out, hipStream_t stream) {
    using P = mi_plan<C0, C1, C2>;
    constexpr auto kern = mlp_infer_kernel<TU, C0, C1, C2, STRIPS>;
    if (P::SMEM > 64 * 1024 && !tpg_allow_dynamic_lds<kern>(P::SMEM)) return TPG_ERR_UNSUPPORTED;
    // one wave per group; the weights are staged once per workgroup, so no more workgroups than the 256 CUs hold at once
    const int per_cu = P::SMEM > 80 * 1024 ? 1 : (P::SMEM > 40 * 1024 ? 2 : 4);
    const long long want = (groups + MI_WAVES - 1) / MI_WAVES;
    const int grid = (int)(want < 256 * per_cu ? want : 256 * per_cu);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(MI_THREADS), P::SMEM, stream,
                       reinterpret_cast<const TU *>(U), reinterpret_cast<const TU *>(Q), idx, N, S, K,
                       groups, reinterpret_cast<const uint4 *>(W1p), reinterpret_cast<const uint4 *>(W2p), a1, c1, a2, c2,
                       s0, s1, s2, reinterpret_cast<__hip_bfloat16 *>(out));
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

}  // namespace

// channel chains (C0, C1, C2), C2 = 0: one weight
#define TPG_MI_CHAINS(X) X(64, 128, 0) X(128, 256, 0) X(64, 64, 128) X(256, 128, 256) X(256, 256, 256)

extern "C" int tpg_mlp_infer_supported(int C0, int C1, int C2, int K) {
    if (K < 16 || K > 256 || K % 16) return 0;
#define TPG_MI_SUP(A, B, C) \
    if (C0 == A && C1 == B && C2 == C) return 1;
    TPG_MI_CHAINS(TPG_MI_SUP)
#undef TPG_MI_SUP
    return 0;
}

template <int C0, int C1, int C2, int STRIPS, typename... Args> int mi_launch_dtype(int dtype_in, Args... args) {
    return dtype_in == TPG_DTYPE_F32 ? mi_launch<float, C0, C1, C2, STRIPS>(args...)
                                     : mi_launch<__hip_bfloat16, C0, C1, C2, STRIPS>(args...);
}

extern "C" int tpg_mlp_infer_fwd(const void *U, const void *Q, const int32_t *idx, int dtype_in, int B, int N, int S, int K,
                                 int C0, int C1, int C2, const void *W1p, const void *W2p, const float *a1, const float *c1,
                                 const float *a2, const float *c2, float slope0, float slope1, float slope2, void *out,
                                 void *stream) {
    if (B < 0 || N < 0 || S < 0 || K <= 0 || C0 <= 0 || C1 <= 0 || C2 < 0) return TPG_ERR_ARG;
    if (dtype_in != TPG_DTYPE_F32 && dtype_in != TPG_DTYPE_BF16) return TPG_ERR_ARG;
    if (!(slope0 >= 0.0f && slope0 <= 1.0f && slope1 >= 0.0f && slope1 <= 1.0f && slope2 >= 0.0f && slope2 <= 1.0f))
        return TPG_ERR_ARG;
    if (!tpg_mlp_infer_supported(C0, C1, C2, K)) return TPG_ERR_UNSUPPORTED;
    if (B == 0 || S == 0) return TPG_OK;
    if (N == 0) return TPG_ERR_ARG;
    if (!U || !Q || !idx || !W1p || !a1 || !c1 || !out || (C2 && (!W2p || !a2 || !c2))) return TPG_ERR_ARG;
    const long long groups = (long long)B * S;
    hipStream_t st = tpg_stream(stream);
#define TPG_MI_FWD(A, Bc, C)                                                                                         \
    if (C0 == A && C1 == Bc && C2 == C)                                                                              \
        return K % 32 == 0 ? mi_launch_dtype<A, Bc, C, 2>(dtype_in, U, Q, idx, N, S, K, groups, W1p, W2p, a1, c1, a2, c2,   \
                                                          slope0, slope1, slope2, out, st)                           \
                           : mi_launch_dtype<A, Bc, C, 1>(dtype_in, U, Q, idx, N, S, K, groups, W1p, W2p, a1, c1, a2, c2,   \
                                                          slope0, slope1, slope2, out, st);
    TPG_MI_CHAINS(TPG_MI_FWD)
#undef TPG_MI_FWD
    return TPG_ERR_UNSUPPORTED;
}
