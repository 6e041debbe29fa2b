// The split-operand bf16 Gram filter of the feature-space searches (D = 32 / 64): the approximation, its error bound and
// the key of the exact re-ranking tail, stated once for knn_mfma.hpp (large clouds, two sweeps) and knn_small.hpp (small
// clouds, one sweep).  Included by knn.hip (inside its anonymous namespace, after knn_dist_row) before those two.
//
// The neighbour LIST is what must be bit-exact against the oracle, not the way candidates are ruled out:
//
//   approximate  d~(q,p) = |y_q|^2 + |y_p|^2 - 2 y_q.y_p ,  y = x - origin (the mean of the cloud's first tile of points)
//
// with the product on v_mfma_f32_32x32x16_bf16 from SPLIT operands: t = hi + lo + r, hi = bf16(t),
// lo = bf16(t - hi), |r| <= 2^-16 |t|; hi.hi + hi.lo + lo.hi leaves out lo.lo and the two residual terms,
// together <= 6.06 2^-16 |y_q||y_p|.  (A first form on v_mfma_f32_32x32x2_f32 -- exact fp32, five times tighter --
// was 2-3x slower: the f32 matrix instruction runs at the vector rate and does NOT co-execute with the VALU work
// of the selection, SQ_VALU_MFMA_COEXEC_CYCLES = 0; the bf16 one costs 7 x 32 cycles per 32 x 32 pairs beside it.)
// |y_p|^2 enters as a fourth product: three bf16 terms (exact) against (1, 1, 1).
//
//   |d~ - d_canonical| <= E_q := 2^-13 |y_q| max_p|y_p| + (8 D + 64) 2^-24 (|y_q| + max_p|y_p|)^2      (km_bound)
//
// A lane of the matrix instruction is (row or query c = lane & 31, half h = lane >> 5): of k-step ks it holds the
// dimensions 16 ks + 8 h .. + 8.
#pragma once

typedef float km_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 km_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int KM_CAP = 64;              // candidate slots per query
constexpr float KM_BIG = 1.0e30f;       // the norm of a padding row / an empty list entry: finite (no 0 x INF in the matrix unit), never a hit
constexpr int KM_MAX_K = 24;            // 2 M guaranteed candidates (M = 10 / 14 / 16 minima kept per lane) must exceed K with room to spare
constexpr long long KM_REDO = -2;       // first index slot of a query the filter could not settle: knn_redo_kernel (knn.hip) redoes it

// x = hi + lo + r with hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32): |r| <= 2^-16 |x|
__device__ __forceinline__ void km_split2(float a, float b, unsigned &hi, unsigned &lo) {
    const __hip_bfloat16 ha = __float2bfloat16(a), hb = __float2bfloat16(b);
    const unsigned short ua = *reinterpret_cast<const unsigned short *>(&ha), ub = *reinterpret_cast<const unsigned short *>(&hb);
    hi = (unsigned)ua | ((unsigned)ub << 16);
    const float ra = a - __uint_as_float((unsigned)ua << 16), rb = b - __uint_as_float((unsigned)ub << 16);
    const __hip_bfloat16 la = __float2bfloat16(ra), lb = __float2bfloat16(rb);
    lo = (unsigned)*reinterpret_cast<const unsigned short *>(&la) | ((unsigned)*reinterpret_cast<const unsigned short *>(&lb) << 16);
}

// One k-step of a lane's half row: centre its 8 floats x8 (read only if the row is there: y = 0 otherwise) on the
// origin's same dimensions o8, split scale * y into (hi, lo) bf16 pairs, add the squares of y to s.  scale = 1 (queries)
// or -2 (points): both products are exact.
__device__ __forceinline__ void km_centre_split(const float4 *x8, const float *o8, bool valid, float scale, uint4 &hi, uint4 &lo,
                                                float &s) {
    float y[8];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 o = *reinterpret_cast<const float4 *>(o8 + 4 * v);
        if (valid) {
            t = x8[v];
            t.x -= o.x; t.y -= o.y; t.z -= o.z; t.w -= o.w;
        }
        y[4 * v] = t.x; y[4 * v + 1] = t.y; y[4 * v + 2] = t.z; y[4 * v + 3] = t.w;
        s += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
    }
    km_split2(scale * y[0], scale * y[1], hi.x, lo.x);
    km_split2(scale * y[2], scale * y[3], hi.y, lo.y);
    km_split2(scale * y[4], scale * y[5], hi.z, lo.z);
    km_split2(scale * y[6], scale * y[7], hi.w, lo.w);
}

// |y_p|^2 (or KM_BIG on a padding row) as three bf16 terms (8 + 8 + 8 significant bits: exact), w0 = terms 0 | 1,
// w1 = term 2: one more matrix instruction against km_ones starts the accumulator at the norm, instead of four LDS
// reads and sixteen moves per lane and sub-tile
__device__ __forceinline__ void km_norm_triplet(float nv, unsigned &w0, unsigned &w1) {
    const __hip_bfloat16 n0 = __float2bfloat16(nv);
    const float r0 = nv - __bfloat162float(n0);
    const __hip_bfloat16 n1 = __float2bfloat16(r0);
    const __hip_bfloat16 n2 = __float2bfloat16(r0 - __bfloat162float(n1));
    w0 = (unsigned)*reinterpret_cast<const unsigned short *>(&n0) | ((unsigned)*reinterpret_cast<const unsigned short *>(&n1) << 16);
    w1 = (unsigned)*reinterpret_cast<const unsigned short *>(&n2);
}

// B operand of the norm step: ones at k = 0, 1, 2 (lanes of the lower half), zeros elsewhere
__device__ __forceinline__ uint4 km_ones(int h) {
    return h == 0 ? make_uint4(0x3f803f80u, 0x00003f80u, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
}

// d'(p, q) = |y_p|^2 - 2 y_p.y_q of 32 rows x 32 queries (the query's own norm is the same for a whole column: the
// kernels add it where they need it): the accumulator starts from the row norms (an x ones) and takes 3 KS matrix
// instructions, lo.hi, hi.lo, hi.hi per k-step.  The ORDER of the fp32 accumulation is part of the bound: keep it.
template <int KS>
__device__ __forceinline__ km_f32x16 km_gram(const uint4 &an, const uint4 &ones, const uint4 (&ah)[KS], const uint4 (&al)[KS],
                                             const uint4 (&bqh)[KS], const uint4 (&bql)[KS]) {
    const km_f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    km_f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(km_bf16x8, an), __builtin_bit_cast(km_bf16x8, ones), zero16, 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const km_bf16x8 Ah = __builtin_bit_cast(km_bf16x8, ah[ks]), Al = __builtin_bit_cast(km_bf16x8, al[ks]);
        const km_bf16x8 Bh = __builtin_bit_cast(km_bf16x8, bqh[ks]), Bl = __builtin_bit_cast(km_bf16x8, bql[ks]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh, acc, 0, 0, 0);
    }
    return acc;
}

// |d~ - d_canonical| <= E_q = c1 |y_q| max|y_p| + c2 (|y_q| + max|y_p|)^2 :
//   c1 = 2^-13: the three dropped cross terms of the split products, 6.06 2^-16 |y_q||y_p|, with a third to spare;
//   c2 = (8 D + 64) 2^-24: fp32 accumulation of the 3 D / 16 matrix steps (taken as 4 ulp each of the running
//        magnitude), the two norms, the centring and the canonical sum itself, doubled.
// Both terms are RELATIVE: they hold while nothing underflows.  Below the normal range the norm triplet is no longer exact
// (its terms are bf16 denormals: 2^-133 apart), the lo halves and the products are cut off, and whether the matrix unit
// keeps or flushes them is not ours to know.  Taking the worst -- every operand and product below 2^-126 lost -- the
// loss is under 2^-126 (3 D + 6 + 6 D (|y_q| + max|y_p|)), which from max|y_p| >= KM_TINY = 2^-40 on is less than 2^-20 of
// the c2 term ((8 D + 64) 2^-104 at least) and inside its doubling.  Below KM_TINY, or with a NaN norm, there is no
// bound: E_q = +Inf, which no threshold of either kernel survives (measured before this rule: a cloud scaled by 2^-70,
// distances ~2e-41, came back with wrong lists from knn_small_kernel; profiles/knn_bound.txt).
// The bare bound: how each kernel rounds and uses it is its own.
constexpr float KM_C1 = 1.220703125e-4f;                                                         // 2^-13
template <int D_T> constexpr float KM_C2 = (float)(8 * D_T + 64) * 5.9604644775390625e-8f;       // (8 D + 64) 2^-24
constexpr float KM_TINY = 9.094947017729282e-13f;                                                // 2^-40
template <int D_T>
__device__ __forceinline__ float km_bound(float sqq, float sq_pmax) {
    if (!(sq_pmax >= KM_TINY)) return __builtin_inff();
    return KM_C1 * sqq * sq_pmax + KM_C2<D_T> * (sqq + sq_pmax) * (sqq + sq_pmax);
}

// ---- the tail: exact re-ranking of a query's listed points, one wave per query, one candidate per lane.  The key is the
// canonical distance of the candidate row (in registers) to the query as given (qs: LDS) with the row's index j, or INF
// on a lane without a candidate.  The kernels rank the keys by counting, each in its own loop; a key of rank < K (not
// INF) is stored as neighbour `rank`, a query at or beyond its cloud's n1 gets the exhaustive kernels' (0, 0) padding --
// both written at their sites: as helpers they changed the kernels' registers and occupancy (profiles/knn_shared.txt).
template <int D_T>
__device__ __forceinline__ tpg_u64 km_tail_key(const float *qs, const float4 (&row)[D_T / 4], int j) {
    tpg_u64 key = TPG_KNN_INF;
    if (j >= 0) key = tpg_knn_key(knn_dist_row<D_T>(qs, row), j);
    return key;
}
