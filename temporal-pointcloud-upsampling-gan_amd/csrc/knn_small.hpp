// Feature-space kNN (D = 32 / 64) on SMALL clouds (64 .. 1024 valid points): the Gram-matrix filter of knn_gram.hpp
// in one sweep, exact re-ranking of the survivors.  Included by knn.hip after knn_gram.hpp and knn_mfma.hpp (inside its
// anonymous namespace); the approximation, its bound, the tail's key, KM_BIG, KM_CAP and KM_REDO are knn_gram.hpp's,
// the origin's tile (km_tile_rows) is knn_mfma.hpp's.
//
// The tiled exhaustive kernel spends three VALU instructions per pair and dimension (-ffp-contract=off): 24 x 512 x 512
// pairs x 192 instructions is a floor of 31-35 us per search of the generator's (24, 512, 64) clouds, 75-82 us measured,
// six searches per step.  knn_mfma.hpp cannot run here: its threshold needs 32+ entries per lane, its 128-query
// workgroups are 96 for 24 x 512 queries, and its tail ranks 32 queries per wave one after the other.  On a small cloud
// a workgroup can SEE every approximate distance of its queries at once, which makes the threshold a selection
// problem instead of a second sweep:
//
//   workgroup  8 waves, KS_Q = 32 queries of one cloud (the split queries are the B operand of EVERY wave);
//   sweep      the 32-row sub-tiles of the cloud are dealt to the waves.  A lane (row c = lane & 31, half h = lane >> 5)
//              reads the half rows it feeds the matrix unit straight from global memory / L2 (the whole cloud is
//              <= 256 KB), centres and splits them in registers -- the same work per lane as staging a tile in LDS,
//              without the round trip, and the LDS goes to the distance matrix instead -- and takes the
//              1 + 3 D / 16 v_mfma_f32_32x32x16_bf16 products per sub-tile (km_gram of knn_gram.hpp: norm triplet, lo.hi,
//              hi.lo, hi.hi).  d'(q, p) = |y_p|^2 - 2 y_p.y_q goes to the LDS matrix dm[query][point] (the query's own norm
//              is the same for every point of a row: it is never added);
//   select     one wave per query, 4 queries per wave (selection and tail are chains of LDS and L2 latencies per
//              query: with 4 waves and 8 queries each the kernel took 72 us where the tiled kernel takes 86).
//              Every lane takes the minimum of its points (j = lane mod 64),
//              T_q = the K-th smallest of the 64 lane minima (rank by counting): K DISTINCT points have d' <= T_q,
//              and about K + 1 .. K + 6 in all.  C = {p : d' <= T_q + 2 E_q} is collected into <= KM_CAP = 64 slots;
//   tail       knn_gram.hpp's: canonical distance of the listed rows (km_tail_key: knn_dist_row of knn.hip), rank by counting
//              over the 64-bit (dist, idx) keys, the first K are written; at D = 32 the rows of the next query are
//              fetched before the current one is ranked (at D = 64 a second set of rows does not fit 128 VGPRs).
//
// Why the first K of C are the answer.  |d~ - d_canonical| <= E_q for every point (km_bound of knn_gram.hpp, max|y_p| over
// the whole cloud; d~ = d' + |y_q|^2, so differences and thresholds in d' are differences and thresholds in d~):
//   * the K points with d' <= T_q have a canonical distance <= T_q + E_q, so the true K-th distance d_K <= T_q + E_q;
//   * every point of the true top K, and every point tying at d_K, has d~ <= d_K + E_q <= T_q + 2 E_q and is in C.
// So C holds every point whose (dist, idx) key is at or below the K-th key, and ranking C by key gives the exhaustive
// kernels' list bit for bit.  No verification step is needed; the threshold is rounded UP (E_q x 1.001, the sum
// + 2^-20 of itself).  A query goes to knn_redo_kernel (first index slot = KM_REDO) when C overflows its 64 slots
// (ties everywhere, all points identical), when the threshold is not finite and below the padding norm (NaN / Inf /
// huge inputs: max|y_p| is taken NaN-preserving; a cloud within 2^-40 of its origin, where products underflow and
// km_bound gives +Inf), or when the cloud has fewer than KS_MIN_VALID valid points (fewer than
// one point per lane: the lane minima would not be K distinct points).
#pragma once

constexpr int KS_Q = 32;                // queries per workgroup (the 32 columns of the matrix instruction)
constexpr int KS_WAVES = 8;             // waves per workgroup: two workgroups per CU, 4 waves per SIMD (<= 128 VGPRs)
constexpr int KS_QW = KS_Q / KS_WAVES;  // queries selected and ranked per wave
constexpr int KS_MIN_VALID = 64;        // fewer valid points than this in a cloud: no filter
constexpr int KS_MAX_P2 = 1024;         // the distance matrix of 32 queries must fit the LDS: 32 x 1028 x 4 B = 128.5 KB
static_assert(KS_Q % KS_WAVES == 0 && KS_QW % 2 == 0 && KS_MAX_P2 <= 65536, "queries per wave in pairs; 16-bit candidate slots");

constexpr int ks_ldq(int P2) { return ((P2 + 31) & ~31) + 4; }   // row of the distance matrix in floats (16-B aligned rows)
template <int D_T>
constexpr size_t ks_smem_bytes(int P2) {
    return sizeof(float) * ((size_t)KS_Q * ks_ldq(P2) + D_T + KS_Q + KS_WAVES * D_T) + sizeof(tpg_u64) * KS_WAVES * 64 +
           sizeof(int) * (KS_Q + 2) + sizeof(unsigned short) * KS_Q * KM_CAP;
}

template <int D_T>
__global__ __launch_bounds__(KS_WAVES * 64, 4) void knn_small_kernel(
    const float *__restrict__ p1, const float *__restrict__ p2, const int64_t *__restrict__ len1,
    const int64_t *__restrict__ len2, int P1, int P2, int K, int gx, float *__restrict__ dist, int64_t *__restrict__ idx) {
    constexpr int KS = D_T / 16;                   // k-steps of the 32x32x16 matrix instruction
    constexpr int NV = 2 * KS;                     // float4 a lane holds of its half row
    constexpr int G = KS_WAVES * 64 / D_T;         // row groups of the origin's sum
    constexpr int RG = km_tile_rows<D_T>() / G;    // rows per group
    constexpr int V4 = D_T / 4;
    static_assert(RG * G == km_tile_rows<D_T>() && G * D_T == KS_WAVES * 64, "origin: one (group, dim) per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char ks_smem[];
    const int LDQ = ks_ldq(P2);
    float *dm = reinterpret_cast<float *>(ks_smem);                   // [KS_Q][LDQ]  d'(query, point); first the origin's partial sums
    float *org = dm + KS_Q * LDQ;                                     // [D_T]
    float *nqs = org + D_T;                                           // [KS_Q]       |y_q|^2
    float *qrow = nqs + KS_Q;                                         // [KS_WAVES][D_T]  tail: the query as given
    tpg_u64 *keys = reinterpret_cast<tpg_u64 *>(qrow + KS_WAVES * D_T);   // [KS_WAVES][64]
    int *cnt = reinterpret_cast<int *>(keys + KS_WAVES * 64);         // [KS_Q]
    unsigned *pmax = reinterpret_cast<unsigned *>(cnt + KS_Q);        // max_p |y_p|^2 (bits of a non-negative float, or of a NaN)
    unsigned short *cbuf = reinterpret_cast<unsigned short *>(pmax + 2);  // [KS_Q][KM_CAP]  candidate rows (< 1024: 16 bits)

    const int b = blockIdx.x / gx;
    const int q0 = (blockIdx.x - b * gx) * KS_Q;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int n1 = len1 ? (int)len1[b] : P1;
    const int n2 = len2 ? min((int)len2[b], P2) : P2;
    float *od = dist + (size_t)b * P1 * K;
    int64_t *oi = idx + (size_t)b * P1 * K;
    if (n2 < KS_MIN_VALID) {                       // the exhaustive kernel handles (and pads) these
        if (tid < KS_Q && q0 + tid < P1) oi[(size_t)(q0 + tid) * K] = KM_REDO;
        return;
    }
    const float *cb = p2 + (size_t)b * P2 * D_T;

    // origin = mean of the cloud's first km_tile_rows points (knn_mfma.hpp), G partial sums per dimension in a fixed order
    {
        const int d = tid % D_T, g = tid / D_T;
        const int rows0 = min(n2, km_tile_rows<D_T>());
        float a = 0.0f;
#pragma unroll
        for (int r = 0; r < RG; ++r)
            if (g * RG + r < rows0) a += cb[(size_t)(g * RG + r) * D_T + d];
        dm[g * D_T + d] = a;
        if (tid == 0) *pmax = 0u;
        __syncthreads();
        if (tid < D_T) {
            float s = 0.0f;
#pragma unroll
            for (int gg = 0; gg < G; ++gg) s += dm[gg * D_T + tid];
            org[tid] = s / (float)rows0;
        }
        __syncthreads();
    }

    auto load_half = [&](const float *row, bool valid, float4 (&x)[NV]) {
#pragma unroll
        for (int i = 0; i < NV; ++i)
            x[i] = valid ? *reinterpret_cast<const float4 *>(row + 16 * (i >> 1) + 8 * h + 4 * (i & 1)) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    // centre, split scale * y into (hi, lo) bf16 pairs; returns the row's |y|^2 (both halves)
    auto centre_split = [&](const float4 (&x)[NV], bool valid, float scale, uint4 (&hi)[KS], uint4 (&lo)[KS]) {
        float s = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)      // (org + ...: this lane's dims of the origin)
            km_centre_split(x + 2 * ks, org + 16 * ks + 8 * h, valid, scale, hi[ks], lo[ks], s);
        return s + __shfl_xor(s, 32);
    };

    // ---- this lane's query (B operand): dims 16 ks + 8 h .. + 8 of query q0 + c, the same in every wave ----
    uint4 bqh[KS], bql[KS];
    {
        const int qi = q0 + c;
        float4 x[NV];
        load_half(p1 + ((size_t)b * P1 + (qi < P1 ? qi : 0)) * D_T, qi < P1, x);
        const float nq = centre_split(x, qi < P1, 1.0f, bqh, bql);
        if (tid < KS_Q) nqs[tid] = nq;
    }

    // ---- the sweep: sub-tile s = wave, wave + 8, ... (16 waves per CU hide the rows' way from L2) ----
    const uint4 ones = km_ones(h);
    const int NS = (n2 + 31) >> 5;
    float mymax = 0.0f;
    for (int s = wave; s < NS; s += KS_WAVES) {
        const bool valid = 32 * s + c < n2;
        float4 cur[NV];
        load_half(cb + (size_t)min(32 * s + c, n2 - 1) * D_T, valid, cur);
        uint4 ah[KS], al[KS];
        const float ss = centre_split(cur, valid, -2.0f, ah, al);
        // the accumulator starts at the row's norm triplet; KM_BIG on padding rows
        unsigned w0, w1;
        km_norm_triplet(valid ? ss : KM_BIG, w0, w1);
        const uint4 an = h == 0 ? make_uint4(w0, w1, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
        if (valid) mymax = (ss > mymax || ss != ss) ? ss : mymax;      // a NaN norm stays (fmaxf would drop it)
        const km_f32x16 acc = km_gram<KS>(an, ones, ah, al, bqh, bql);
        // acc[4 g + r] is (point 32 s + 8 g + 4 h + r, query c)
        float *drow = dm + c * LDQ + 32 * s + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4 *>(drow + 8 * g) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
    }
    atomicMax(pmax, __float_as_uint(mymax));
    __syncthreads();

    // ---- select: threshold and candidate list of this wave's KS_QW queries --------------------------------
    const float sq_pmax = sqrtf(__uint_as_float(*pmax));
    const int NT = (n2 + 63) >> 6;
    for (int qq = 0; qq < KS_QW; ++qq) {
        const int ql = wave * KS_QW + qq, i = q0 + ql;
        if (i >= P1 || i >= n1) continue;                              // (uniform over the wave)
        const float *drow = dm + ql * LDQ;
        float mn = KM_BIG;
        for (int t = 0; t < NT; t += 4) {                              // four LDS reads in flight
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int j = 64 * (t + u) + lane; v[u] = j < n2 ? drow[j] : KM_BIG; }
            mn = fminf(fminf(mn, v[0]), fminf(fminf(v[1], v[2]), v[3]));
        }
        // rank of this lane's minimum among the 64 (ties by lane: a permutation), T = the one of rank K - 1
        int rank = 0;
#pragma unroll 8
        for (int s = 0; s < 64; ++s) {
            const float o = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(mn), s));
            rank += (o < mn || (o == mn && s < lane)) ? 1 : 0;
        }
        const tpg_u64 at = __ballot(rank == K - 1);
        const float T = __uint_as_float((unsigned)__builtin_amdgcn_readlane(
            (int)__float_as_uint(mn), __builtin_amdgcn_readfirstlane(at ? __builtin_ctzll(at) : 0)));
        const float sqq = sqrtf(nqs[ql]);
        const float eq = km_bound<D_T>(sqq, sq_pmax) * 1.001f;
        float thr = T + 2.0f * eq;
        thr = thr + fabsf(thr) * 9.5367431640625e-7f;                  // + 2^-20: upwards, whatever the additions rounded
        int n = 0;
        if (at != 0 && thr < 1.0e29f) {                                // (false for a NaN)
            for (int t = 0; t < NT; t += 4) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int j = 64 * (t + u) + lane; v[u] = j < n2 ? drow[j] : KM_BIG; }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool hit = v[u] <= thr;                      // (padding: KM_BIG > thr)
                    const tpg_u64 m = __ballot(hit);
                    const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                    if (hit && pos < KM_CAP) cbuf[ql * KM_CAP + pos] = (unsigned short)(64 * (t + u) + lane);
                    n += __popcll(m);
                }
            }
        } else {
            n = KM_CAP + 1;
        }
        if (lane == 0) cnt[ql] = n;
    }
    // (cnt, cbuf, keys and qrow below are this wave's own: LDS operations of one wave complete in order, no barrier)

    // ---- tail: exact re-ranking, one query at a time, the next query's candidate rows in flight --------------
    float *qs = qrow + wave * D_T;
    tpg_u64 *ks_ = keys + wave * 64;
    const tpg_u64 INF = TPG_KNN_INF;
    auto fetch = [&](int qq, float4 (&row)[V4], float &qx, int &j, int &n) {
        const int ql = wave * KS_QW + qq, i = q0 + ql;
        j = -1;
        n = -1;
        if (qq >= KS_QW || i >= P1 || i >= n1) return;
        if (lane < D_T) qx = p1[((size_t)b * P1 + i) * D_T + lane];
        n = cnt[ql];
        if (n <= KM_CAP && lane < n) {
            j = cbuf[ql * KM_CAP + lane];
            const float4 *c4 = reinterpret_cast<const float4 *>(cb + (size_t)j * D_T);
#pragma unroll
            for (int d = 0; d < V4; ++d) row[d] = c4[d];
        }
    };
    auto finish = [&](int qq, const float4 (&row)[V4], float qx, int j, int n) {
        const int i = q0 + wave * KS_QW + qq;
        if (qq >= KS_QW || i >= P1) return;
        if (i >= n1) {
            if (lane < K) { od[(size_t)i * K + lane] = 0.0f; oi[(size_t)i * K + lane] = 0; }
            return;
        }
        if (lane < D_T) qs[lane] = qx;
        const tpg_u64 key = km_tail_key<D_T>(qs, row, j);
        ks_[lane] = key;
        const int nk = (n >= K && n <= KM_CAP) ? n : 0;
        int rank = 0;
        for (int s = 0; s < nk; s += 8)                                // (slots from n on hold INF: never below a key)
#pragma unroll
            for (int u = 0; u < 8; ++u) rank += ks_[s + u] < key ? 1 : 0;
        if (nk > 0) {
            if (rank < K && key != INF) {
                od[(size_t)i * K + rank] = tpg_knn_key_dist(key);
                oi[(size_t)i * K + rank] = tpg_knn_key_idx(key);
            }
        } else if (lane == 0) {
            oi[(size_t)i * K] = KM_REDO;
        }
    };
    float4 rowA[V4];
    float qA = 0.0f;
    int jA, nA;
    if constexpr (D_T == 32) {
        // the rows of query qq + 1 are fetched into a second register set before query qq is ranked
        float4 rowB[V4];
        float qB = 0.0f;
        int jB, nB;
        fetch(0, rowA, qA, jA, nA);
#pragma unroll 1
        for (int qq = 0; qq < KS_QW; qq += 2) {
            fetch(qq + 1, rowB, qB, jB, nB);
            finish(qq, rowA, qA, jA, nA);
            fetch(qq + 2, rowA, qA, jA, nA);
            finish(qq + 1, rowB, qB, jB, nB);
        }
    } else {
        // D = 64: two sets of candidate rows are 128 VGPRs, the whole budget of 4 waves per SIMD (95 spilled): one
        // set, and the other three waves of the SIMD cover the fetch
#pragma unroll 1
        for (int qq = 0; qq < KS_QW; ++qq) {
            fetch(qq, rowA, qA, jA, nA);
            finish(qq, rowA, qA, jA, nA);
        }
    }
}
