// Row-wise linear layers (1x1 convolutions on channels-last rows) of ANY small channel count, hand-written on the
// f32 matrix instructions -- round 3, VERDICT r2 item 4(a).
//
// What this replaces: the library GEMMs (hipBLASLt through torch: ~250 launches per cfg2 step, 17 TFLOP/s = launch
// overhead) and the elementwise launches around them (bias add, LeakyReLU forward / backward, fp32 <-> bf16 casts, the
// sums of split-K partials) for
//   * the generator's node / edge affines, bottlenecks, decoders and skip layers
//     (gcn_lib/pointnet/gcn.py:176-180,207-211,253-277; upsampling_network.py:44-104),
//   * the FIRST layer of every shared MLP of the discriminators, applied to the un-grouped points before the gather
//     (discriminator.py:63-78,140-148,276-282; Cin = 3, 6, 131, 259, 515: not multiples of anything),
//   * the heads' linears (discriminator.py:503-516,598-612).
//
//     y[p, o] = lrelu_s( sum_c x[p, c] * W[seg(p)][o, c] + b[o] )          x (P, Cin) f32 | bf16,  W (nseg, Cout, Cin) f32
//
// nseg equal consecutive row blocks with their own weights (successive spectral-norm iterates of one module called
// nseg times: frames, fake / real batch).  Arithmetic: v_mfma_f32_16x16x4_f32 -- exact fp32 products, fp32
// accumulation (bf16 inputs are widened exactly): the pre-gather layers must not be rounded to bf16 (their outputs are
// subtracted from each other after the gather), and at these sizes (<= 0.2 GFLOP per call) the f32 matrix rate is
// not what bounds a launch.
//
//   forward   a workgroup = 64 rows (4 waves x 16), the weight staged in LDS once per pass of <= 128 output columns;
//             the x fragment of 16 k's is ONE 16-byte load per lane (lane = row r, k-slot g holds k0+4g .. k0+4g+3;
//             any bijection of the 16 k's onto (slot, step) is a valid operand layout as long as W uses the same
//             one), all fragments of <= 256 k's in flight together; bias + LeakyReLU + the store's rounding in the
//             epilogue.
//   dgrad     dx = (gy * lrelu'(y)) . W : the same kernel, the weight transposed while it is staged, the activation's
//             derivative applied to the A fragment (the sign of the saved output y decides: lrelu is monotone).
//   wgrad     dW = (gy * lrelu'(y))^T . x, db = column sums: row slabs, each walked in LDS-staged chunks -> fp32
//             partial tiles -> a reduce launch that sums the slabs in a fixed order (bitwise reproducible; the bias
//             is the weight of a constant-one input).
#include "tpg_rows.hpp"

namespace {

#define RL_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

constexpr int RL_WG_CT = 16;         // wgrad: tiles per group (64 accumulator registers)

// f[s] = M[r][k + s], s = 0..3 (row-major, leading dimension ld = K): zero beyond K or when !ok.
template <typename T>
__device__ __forceinline__ void rl_load_k4(const T *M, long long r, bool ok, int K, int k, bool vec, float (&f)[4]) {
    f[0] = f[1] = f[2] = f[3] = 0.0f;
    if (!ok || k >= K) return;
    const T *p = M + r * (long long)K + k;
    if (vec && k + 3 < K) {
        tpg_load_row(p, f);
        return;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (k + s < K) f[s] = tpg_load_one(p + s);
}

// f[s] = M[k + s][c], s = 0..3 (rows k .. k+3 of a row-major (Krows x ld) matrix): zero beyond Krows or when !ok.
template <typename T>
__device__ __forceinline__ void rl_load_r4(const T *M, long long k, long long Krows, int ld, int c, bool ok, float (&f)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s] = (ok && k + s < Krows) ? tpg_load_one(M + (k + s) * (long long)ld + c) : 0.0f;
}

// ---- forward / dgrad ---------------------------------------------------------------------------------------------
// out (P, N) = [act'(Y) *] A (P, KA) . B^T [+ bias][, lrelu],  B (N, KA) staged in LDS per pass of NP output columns:
//   BT == false (forward): KA = Cin,  N = Cout, B[n][k] = W[n][k]   (straight copy)
//   BT == true  (dgrad)  : KA = Cout, N = Cin,  B[n][k] = W[k][n]   (transposed while staging: the compute loop is the
//                          forward's);  Y (P, KA) = the forward's output, slope_in its slope
// A workgroup (8 waves x 16 rows) stages B once per pass with coalesced loads -- ONE L2 round trip instead of one per
// 16 k's -- and every wave then streams its A fragments (one 16-byte load per 16 k's, the next one in flight) against
// ds_read_b128 fragments of B in a rolled loop.  Rows of B are KS = roundup16(KA) + 4 floats apart: the 16 lanes of a k-slot read
// 16-byte words 4 banks apart, conflict-free.
constexpr int RL_NP_MAX = 128;       // output columns per pass (8 tiles of 16: 32 accumulator registers)
constexpr int RL_LDS_FLOATS = 16000; // 64 KB of dynamic LDS minus slack

__host__ __device__ inline int rl_ks(int KA) { return ((KA + 15) & ~15) + 4; }
__host__ __device__ inline int rl_np(int KA, int N) {
    int np = (RL_LDS_FLOATS / rl_ks(KA)) & ~15;
    if (np > RL_NP_MAX) np = RL_NP_MAX;
    const int n16 = (N + 15) & ~15;
    return np < n16 ? np : n16;
}

constexpr int RL_WAVES = 8;                       // waves per workgroup: 8 x 16 = 128 rows share one staging of the weight
constexpr int RL_THREADS = RL_WAVES * 64;
constexpr int RL_WG_ROWS = RL_WAVES * 16;

template <typename TA, typename TO, bool BT>
__global__ __launch_bounds__(RL_THREADS) void rowlin_kernel(const TA *__restrict__ A, const TA *__restrict__ Y,
                                                            const float *__restrict__ W, const float *__restrict__ bias,
                                                            TO *__restrict__ out, long long P, long long Pseg, int Cin,
                                                            int Cout, float slope_in, float slope_out) {
    extern __shared__ __attribute__((aligned(16))) float rl_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long long wg0 = (long long)blockIdx.x * RL_WG_ROWS;         // first row of the workgroup
    const long long r0 = wg0 + wave * 16;
    const int KA = BT ? Cout : Cin, N = BT ? Cin : Cout;
    const int KS = rl_ks(KA), NP = rl_np(KA, N), K16 = (KA + 15) & ~15;
    const float *Ws = W + (wg0 / Pseg) * (long long)Cout * Cin;       // (a workgroup never straddles segments)
    const bool vecA = (KA & 3) == 0;
    const long long row = r0 + r;
    const bool rok = row < P;
    for (int n0 = 0; n0 < N; n0 += NP) {
        const int ncur = min(NP, N - n0);                            // valid columns of this pass
        const int nt = (ncur + 15) >> 4;
        __syncthreads();                                              // (the previous pass is done with the LDS)
        if (!BT) {
            // B[nn][k] = W[n0 + nn][k]: 16 threads x 16 bytes walk a row, 32 rows at a time (no divisions)
            const int tr = tid >> 4, tk = (tid & 15) * 4;
            const bool vecW = (Cin & 3) == 0;
            for (int nn = tr; nn < nt * 16; nn += RL_THREADS / 16) {
                const float *src = Ws + (long long)(n0 + nn) * Cin;
                for (int k = tk; k < K16; k += 64) {
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (nn < ncur && k < KA) {
                        if (vecW) {
                            v = *reinterpret_cast<const float4 *>(src + k);
                        } else {
                            v.x = src[k];
                            if (k + 1 < KA) v.y = src[k + 1];
                            if (k + 2 < KA) v.z = src[k + 2];
                            if (k + 3 < KA) v.w = src[k + 3];
                        }
                    }
                    *reinterpret_cast<float4 *>(rl_lds + nn * KS + k) = v;
                }
            }
        } else {
            // B[nn][k] = W[k][n0 + nn]: 16 threads x 16 bytes walk a row k of W along nn (coalesced), transposed stores
            const int tk = tid >> 4, tn = (tid & 15) * 4;
            const bool vecW = (Cin & 3) == 0 && (n0 & 3) == 0;
            for (int k = tk; k < K16; k += RL_THREADS / 16) {
                const float *src = Ws + (long long)k * Cin + n0;
                for (int nn = tn; nn < nt * 16; nn += 64) {
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (k < KA && nn < ncur) {
                        if (vecW && nn + 3 < ncur) {
                            v = *reinterpret_cast<const float4 *>(src + nn);
                        } else {
                            v.x = src[nn];
                            if (nn + 1 < ncur) v.y = src[nn + 1];
                            if (nn + 2 < ncur) v.z = src[nn + 2];
                            if (nn + 3 < ncur) v.w = src[nn + 3];
                        }
                    }
                    rl_lds[nn * KS + k] = v.x;
                    rl_lds[(nn + 1) * KS + k] = v.y;
                    rl_lds[(nn + 2) * KS + k] = v.z;
                    rl_lds[(nn + 3) * KS + k] = v.w;
                }
            }
        }
        __syncthreads();
        if (r0 >= P) continue;                                        // (the wave still takes part in the barriers)
        tpg_f32x4 acc[RL_NP_MAX / 16];
#pragma unroll
        for (int c = 0; c < RL_NP_MAX / 16; ++c) acc[c] = tpg_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // software-pipelined k loop (NOT unrolled: ~90 live registers, several waves per SIMD): the A fragment of the
        // next 16 k's is in flight while this one meets its <= 8 B fragments
        float a[4], an[4];
        rl_load_k4(A, row, rok, KA, 4 * g, vecA, a);
        if (Y != nullptr) {                                           // gz = gy * lrelu'(z): sign(y) == sign(z)
            float yv[4];
            rl_load_k4(Y, row, rok, KA, 4 * g, vecA, yv);
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = yv[s] > 0.0f ? a[s] : a[s] * slope_in;
        }
        const float *bk = rl_lds + 4 * g + r * KS;
#pragma unroll 1
        for (int k0 = 0; k0 < K16; k0 += 16) {
            rl_load_k4(A, row, rok && k0 + 16 < K16, KA, k0 + 16 + 4 * g, vecA, an);
            if (Y != nullptr) {
                float yv[4];
                rl_load_k4(Y, row, rok && k0 + 16 < K16, KA, k0 + 16 + 4 * g, vecA, yv);
#pragma unroll
                for (int s = 0; s < 4; ++s) an[s] = yv[s] > 0.0f ? an[s] : an[s] * slope_in;
            }
#pragma unroll
            for (int c = 0; c < RL_NP_MAX / 16; ++c) {
                if (c < nt) {                                         // (wave-uniform)
                    const float4 b = *reinterpret_cast<const float4 *>(bk + k0 + 16 * c * KS);
                    acc[c] = RL_MFMA(a[0], b.x, acc[c]);
                    acc[c] = RL_MFMA(a[1], b.y, acc[c]);
                    acc[c] = RL_MFMA(a[2], b.z, acc[c]);
                    acc[c] = RL_MFMA(a[3], b.w, acc[c]);
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = an[s];
        }
        // D[m = 4g + i][n = r] in register i
#pragma unroll
        for (int c = 0; c < RL_NP_MAX / 16; ++c) {
            const int n = n0 + 16 * c + r;
            if (c >= nt || n >= N) continue;
            const float bv = (!BT && bias != nullptr) ? bias[n] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long p = r0 + 4 * g + i;
                if (p < P) {
                    float v = acc[c][i] + bv;
                    if (!BT) v = v > 0.0f ? v : v * slope_out;
                    tpg_store_one(out + p * (long long)N + n, v);
                }
            }
        }
    }
}

// ---- wgrad --------------------------------------------------------------------------------------------------------
// partial dW of one row slab: ws[(seg * nslab + slab)][o][c], c < CinE = Cin + has_bias (the bias column reads x == 1).
// The slab is walked in chunks of RC rows staged in LDS with coalesced loads (gz = gy * lrelu'(y) applied while staging,
// x widened to fp32): G[p][o] (stride GS) and X[p][c] (stride XS); a wave owns groups of <= 16 output tiles and reads
// its fragments from LDS (4 consecutive rows p per k-slot, 16 consecutive columns per lane group: conflict-free).
template <typename TX, typename TG>
__global__ __launch_bounds__(256) void rowlin_wgrad_kernel(const TX *__restrict__ x, const TG *__restrict__ gy,
                                                           const TG *__restrict__ Y, float *__restrict__ ws, long long Pseg,
                                                           int nslab, long long R, int Cin, int Cout, int has_bias,
                                                           float slope, int GC, int RC) {
    extern __shared__ __attribute__((aligned(16))) float rl_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int seg = blockIdx.x / nslab, slab = blockIdx.x - seg * nslab;
    const long long p0 = (long long)seg * Pseg + (long long)slab * R;
    const long long p1 = min(p0 + R, (long long)(seg + 1) * Pseg);
    const int CinE = Cin + has_bias;
    const int OT = (Cout + 15) >> 4, CTt = (CinE + 15) >> 4;
    const int GS = OT * 16 + 4, XS = CTt * 16 + 4;                   // LDS row strides (16-column padded, +4: bank offset)
    float *Gl = rl_lds, *Xl = rl_lds + RC * GS;
    const int cgroups = (CTt + GC - 1) / GC;
    const int ngroups = OT * cgroups;
    float *out = ws + (size_t)blockIdx.x * Cout * CinE;
    // a wave keeps the accumulators of two tile groups across the chunks; more than 8 groups (Cout * Cin beyond
    // ~128 x 256) take further rounds over the slab
    for (int gb = 0; gb < ngroups; gb += 8) {
        tpg_f32x4 acc[2][RL_WG_CT];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int c = 0; c < RL_WG_CT; ++c) acc[u][c] = tpg_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (long long c0r = p0; c0r < p1; c0r += RC) {
            const int rows = (int)min((long long)RC, p1 - c0r);
            __syncthreads();
            {
                // 16 threads x 4 columns walk a row, 16 rows at a time (no divisions); lrelu' applied while staging
                const int tr = tid >> 4, tc = (tid & 15) * 4;
                for (int pr = tr; pr < RC; pr += 16) {
                    const bool rin = pr < rows;
                    const TG *gsrc = gy + (c0r + pr) * (long long)Cout;
                    const TG *ysrc = Y != nullptr ? Y + (c0r + pr) * (long long)Cout : nullptr;
                    for (int o = tc; o < OT * 16; o += 64) {
                        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (rin && o + j < Cout) {
                                v[j] = tpg_load_one(gsrc + o + j);
                                if (ysrc != nullptr) v[j] = tpg_load_one(ysrc + o + j) > 0.0f ? v[j] : v[j] * slope;
                            }
                        *reinterpret_cast<float4 *>(Gl + pr * GS + o) = make_float4(v[0], v[1], v[2], v[3]);
                    }
                    const TX *xsrc = x + (c0r + pr) * (long long)Cin;
                    for (int c = tc; c < CTt * 16; c += 64) {
                        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (rin) v[j] = c + j < Cin ? tpg_load_one(xsrc + c + j) : ((c + j == Cin && has_bias) ? 1.0f : 0.0f);
                        *reinterpret_cast<float4 *>(Xl + pr * XS + c) = make_float4(v[0], v[1], v[2], v[3]);
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int grp = gb + wave + 4 * u;
                if (grp < ngroups) {
                    const int ot = grp / cgroups, ct0 = (grp - ot * cgroups) * GC;
                    const int nt = min(GC, CTt - ct0);
                    for (int k0 = 0; k0 < rows; k0 += 16) {           // (rows beyond `rows` are zero in LDS)
                        const float *ga = Gl + (k0 + 4 * g) * GS + 16 * ot + r;
                        const float a0 = ga[0], a1 = ga[GS], a2 = ga[2 * GS], a3 = ga[3 * GS];
                        const float *xb = Xl + (k0 + 4 * g) * XS + 16 * ct0 + r;
#pragma unroll
                        for (int c = 0; c < RL_WG_CT; ++c) {
                            if (c < nt) {
                                acc[u][c] = RL_MFMA(a0, xb[16 * c], acc[u][c]);
                                acc[u][c] = RL_MFMA(a1, xb[16 * c + XS], acc[u][c]);
                                acc[u][c] = RL_MFMA(a2, xb[16 * c + 2 * XS], acc[u][c]);
                                acc[u][c] = RL_MFMA(a3, xb[16 * c + 3 * XS], acc[u][c]);
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int grp = gb + wave + 4 * u;
            if (grp >= ngroups) continue;
            const int ot = grp / cgroups, ct0 = (grp - ot * cgroups) * GC;
            const int nt = min(GC, CTt - ct0);
#pragma unroll
            for (int c = 0; c < RL_WG_CT; ++c) {
                const int cc = 16 * (ct0 + c) + r;
                if (c >= nt || cc >= CinE) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int oo = 16 * ot + 4 * g + i;
                    if (oo < Cout) out[(size_t)oo * CinE + cc] = acc[u][c][i];
                }
            }
        }
    }
}

// dW (nseg, Cout, Cin) = sum over the slabs IN ORDER; db (Cout) = the bias column summed over slabs and segments in
// order.  A workgroup = 64 consecutive elements x 4 waves; wave w sums slabs w, w+4, ... (coalesced 256-byte reads), the
// four partial sums are combined in wave order through LDS: a fixed association, bitwise reproducible.
__global__ __launch_bounds__(256) void rowlin_wgrad_reduce_kernel(const float *__restrict__ ws, int nseg, int nslab, int Cin,
                                                                  int Cout, int has_bias, float *__restrict__ dW,
                                                                  float *__restrict__ db) {
    __shared__ float part[4][64];
    const int CinE = Cin + has_bias;
    const long long per = (long long)Cout * CinE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long t = (long long)blockIdx.x * 64 + lane;
    const long long nW = (long long)nseg * Cout * Cin;
    float s = 0.0f;
    if (t < nW) {
        const int seg = (int)(t / ((long long)Cout * Cin));
        const long long rem = t - (long long)seg * Cout * Cin;
        const int o = (int)(rem / Cin), c = (int)(rem - (long long)o * Cin);
        const float *p = ws + ((size_t)seg * nslab) * per + (size_t)o * CinE + c;
        for (int k = wave; k < nslab; k += 4) s += p[(size_t)k * per];
    } else if (has_bias && t < nW + Cout) {
        const int o = (int)(t - nW);
        const int total = nseg * nslab;
        for (int k = wave; k < total; k += 4) s += ws[(size_t)k * per + (size_t)o * CinE + Cin];
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
        const float v = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        if (t < nW) dW[t] = v;
        else if (has_bias && db != nullptr && t < nW + Cout) db[t - nW] = v;
    }
}

struct WgradPlan {
    long long R;
    int nslab, GC, RC;
    size_t smem;
};

WgradPlan wgrad_plan(long long Pseg, int nseg, int Cin, int Cout, int has_bias) {
    WgradPlan w;
    const int OT = (Cout + 15) / 16, CTt = (Cin + has_bias + 15) / 16;
    // tile groups: <= 16 tiles each, at most 8 groups per workgroup (2 per wave): more output than that is rare
    // (Cout * Cin > 8 * 16 * 256 = 128 x 256) and handled by giving the groups whole column ranges anyway
    int GC = CTt < RL_WG_CT ? CTt : RL_WG_CT;
    while (OT * ((CTt + GC - 1) / GC) < 4 && GC > 1) GC = (GC + 1) / 2;      // give all four waves a tile group
    w.GC = GC;
    // rows staged per chunk: what 60 KB of LDS hold, whole 16-row steps
    const int GS = OT * 16 + 4, XS = CTt * 16 + 4;
    int RC = (15000 / (GS + XS)) & ~15;
    if (RC > 128) RC = 128;
    if (RC < 16) RC = 16;
    w.RC = RC;
    w.smem = sizeof(float) * (size_t)RC * (GS + XS);
    // ~256 workgroups over all segments, slabs of whole chunks
    long long slabs = 256 / (nseg > 0 ? nseg : 1);
    if (slabs < 1) slabs = 1;
    long long R = (Pseg + slabs - 1) / slabs;
    R = (R + RC - 1) / RC * RC;
    w.R = R;
    w.nslab = (int)((Pseg + R - 1) / R);
    return w;
}

bool rl_args_ok(long long P, int nseg, int Cin, int Cout) {
    return P >= 0 && nseg >= 1 && Cin >= 1 && Cout >= 1 && Cin <= 1000 && Cout <= 1000 && P % nseg == 0 &&
           (nseg == 1 || (P / nseg) % 128 == 0) && P < (1LL << 40);
}

bool rl_wgrad_fits(int Cin, int Cout, int has_bias) {
    return wgrad_plan(1024, 1, Cin, Cout, has_bias).smem <= 64 * 1024;
}

}  // namespace

extern "C" int tpg_rowlinear_supported(int Cin, int Cout, int has_bias) {
    return Cin >= 1 && Cout >= 1 && Cin <= 1000 && Cout <= 1000 && rl_wgrad_fits(Cin, Cout, has_bias ? 1 : 0) &&
           rl_wgrad_fits(Cin, Cout, 0);
}

extern "C" size_t tpg_rowlinear_wgrad_workspace_bytes(long long P, int nseg, int Cin, int Cout, int has_bias) {
    if (!rl_args_ok(P, nseg, Cin, Cout) || P == 0) return 16;
    const WgradPlan w = wgrad_plan(P / nseg, nseg, Cin, Cout, has_bias ? 1 : 0);
    return sizeof(float) * (size_t)nseg * w.nslab * Cout * (Cin + (has_bias ? 1 : 0)) + 16;
}

extern "C" int tpg_rowlinear_fwd(const void *x, int dtype_in, const float *W, const float *bias, long long P, int nseg,
                                 int Cin, int Cout, float slope, void *y, int dtype_out, void *stream) {
    if (!rl_args_ok(P, nseg, Cin, Cout) || slope < 0.0f || slope > 1.0f) return TPG_ERR_ARG;
    if (P == 0) return TPG_OK;
    if (!x || !W || !y) return TPG_ERR_ARG;
    if ((dtype_in != TPG_DTYPE_F32 && dtype_in != TPG_DTYPE_BF16) || (dtype_out != TPG_DTYPE_F32 && dtype_out != TPG_DTYPE_BF16))
        return TPG_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W)) & 15) return TPG_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((P + RL_WG_ROWS - 1) / RL_WG_ROWS)), blk(RL_THREADS);
    hipStream_t st = tpg_stream(stream);
    const long long Pseg = P / nseg;
    const size_t smem = sizeof(float) * (size_t)rl_np(Cin, Cout) * rl_ks(Cin);
#define RL_FWD(TA, TO)                                                                                               \
    hipLaunchKernelGGL((rowlin_kernel<TA, TO, false>), grid, blk, smem, st, static_cast<const TA *>(x),                  \
                       static_cast<const TA *>(nullptr), W, bias, static_cast<TO *>(y), P, Pseg, Cin, Cout, 1.0f, slope)
    if (dtype_in == TPG_DTYPE_F32 && dtype_out == TPG_DTYPE_F32) RL_FWD(float, float);
    else if (dtype_in == TPG_DTYPE_F32) RL_FWD(float, __hip_bfloat16);
    else if (dtype_out == TPG_DTYPE_F32) RL_FWD(__hip_bfloat16, float);
    else RL_FWD(__hip_bfloat16, __hip_bfloat16);
#undef RL_FWD
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_rowlinear_dgrad(const void *gy, const void *y, int dtype_g, const float *W, long long P, int nseg,
                                   int Cin, int Cout, float slope, void *dx, int dtype_x, void *stream) {
    if (!rl_args_ok(P, nseg, Cin, Cout) || slope < 0.0f || slope > 1.0f) return TPG_ERR_ARG;
    if (P == 0) return TPG_OK;
    if (!gy || !W || !dx || (slope != 1.0f && !y)) return TPG_ERR_ARG;
    if ((dtype_g != TPG_DTYPE_F32 && dtype_g != TPG_DTYPE_BF16) || (dtype_x != TPG_DTYPE_F32 && dtype_x != TPG_DTYPE_BF16))
        return TPG_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(W)) & 15)
        return TPG_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((P + RL_WG_ROWS - 1) / RL_WG_ROWS)), blk(RL_THREADS);
    hipStream_t st = tpg_stream(stream);
    const long long Pseg = P / nseg;
    const void *yy = slope != 1.0f ? y : nullptr;
    const size_t smem = sizeof(float) * (size_t)rl_np(Cout, Cin) * rl_ks(Cout);
#define RL_DG(TA, TO)                                                                                                \
    hipLaunchKernelGGL((rowlin_kernel<TA, TO, true>), grid, blk, smem, st, static_cast<const TA *>(gy),                  \
                       static_cast<const TA *>(yy), W, static_cast<const float *>(nullptr), static_cast<TO *>(dx), P, \
                       Pseg, Cin, Cout, slope, 1.0f)
    if (dtype_g == TPG_DTYPE_F32 && dtype_x == TPG_DTYPE_F32) RL_DG(float, float);
    else if (dtype_g == TPG_DTYPE_F32) RL_DG(float, __hip_bfloat16);
    else if (dtype_x == TPG_DTYPE_F32) RL_DG(__hip_bfloat16, float);
    else RL_DG(__hip_bfloat16, __hip_bfloat16);
#undef RL_DG
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_rowlinear_wgrad(const void *x, int dtype_x, const void *gy, const void *y, int dtype_g, long long P,
                                   int nseg, int Cin, int Cout, float slope, float *dW, float *db, void *ws,
                                   void *stream) {
    if (!rl_args_ok(P, nseg, Cin, Cout) || slope < 0.0f || slope > 1.0f || !dW) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    if (P == 0) {
        if (hipMemsetAsync(dW, 0, sizeof(float) * (size_t)nseg * Cout * Cin, st) != hipSuccess) return TPG_ERR_LAUNCH;
        if (db && hipMemsetAsync(db, 0, sizeof(float) * Cout, st) != hipSuccess) return TPG_ERR_LAUNCH;
        return TPG_OK;
    }
    if (!x || !gy || !ws || (slope != 1.0f && !y)) return TPG_ERR_ARG;
    if ((dtype_g != TPG_DTYPE_F32 && dtype_g != TPG_DTYPE_BF16) || (dtype_x != TPG_DTYPE_F32 && dtype_x != TPG_DTYPE_BF16))
        return TPG_ERR_UNSUPPORTED;
    const int has_bias = db != nullptr;
    if (!rl_wgrad_fits(Cin, Cout, has_bias)) return TPG_ERR_UNSUPPORTED;
    const long long Pseg = P / nseg;
    const WgradPlan w = wgrad_plan(Pseg, nseg, Cin, Cout, has_bias);
    const void *yy = slope != 1.0f ? y : nullptr;
    const dim3 grid((unsigned)(nseg * w.nslab)), blk(256);
    float *wsf = static_cast<float *>(ws);
#define RL_WG(TX, TG)                                                                                                \
    hipLaunchKernelGGL((rowlin_wgrad_kernel<TX, TG>), grid, blk, w.smem, st, static_cast<const TX *>(x),              \
                       static_cast<const TG *>(gy), static_cast<const TG *>(yy), wsf, Pseg, w.nslab, w.R, Cin, Cout,  \
                       has_bias, slope, w.GC, w.RC)
    if (dtype_x == TPG_DTYPE_F32 && dtype_g == TPG_DTYPE_F32) RL_WG(float, float);
    else if (dtype_x == TPG_DTYPE_F32) RL_WG(float, __hip_bfloat16);
    else if (dtype_g == TPG_DTYPE_F32) RL_WG(__hip_bfloat16, float);
    else RL_WG(__hip_bfloat16, __hip_bfloat16);
#undef RL_WG
    const long long total = (long long)nseg * Cout * Cin + (has_bias ? Cout : 0);
    hipLaunchKernelGGL(rowlin_wgrad_reduce_kernel, dim3((unsigned)((total + 63) / 64)), blk, 0, st, wsf, nseg, w.nslab, Cin,
                       Cout, has_bias, dW, db);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
