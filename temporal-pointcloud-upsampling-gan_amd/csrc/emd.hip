// Earth mover's distance between equal-size clouds: a one-to-one assignment of every point of xyz1 (the persons) to a
// point of xyz2 (the objects) that approximately minimises the sum of squared distances, by a forward auction with
// Jacobi rounds and epsilon scaling (reference call sites, all through the third-party `emd` auction extension:
// train_fluid/analysis_helper.py:14-64,224,255, train_action/analysis_helper.py:11-49,67, loss.py:311).
//
// The rule (include/tpgan_ops.h states it in full; tests/test_metrics_cpu.py restates it in numpy and the kernels
// reproduce that statement bit for bit, the round count included):
//   cost    c_ij = tpg_sq3(person i, object j), value v_ij = (-c_ij) - p_j, prices p start at 0 and only grow
//   phases  k = phases .. 0 with eps_k = eps * scaling^k (rounded per multiplication); every phase starts with nobody
//           assigned and keeps the prices; it ends when nobody is unassigned
//   round   every unassigned person finds its best object j1 (ties: lowest j) and the second best value v2 over
//           j != j1 and bids p' = p_j1 + ((v1 - v2) + eps_k), or the next float above p_j1 where that rounds to p_j1;
//           every object takes its highest bid (ties: lowest i), its previous owner becomes unassigned
// A bid is one 64-bit atomicMax on (bits of p' << 32) | (0xFFFFFFFF - i).  Prices are non-negative, so their bits order
// as integers, and every later bid for an object is above its price, hence above every earlier key: the keys are
// never cleared, and "this object took a bid in this round" is "its key's price is above its price".  All of a round's
// bids read the prices of the round's start, and the maximum does not depend on the order of the atomics, so a
// cloud's results depend on nothing but the cloud.
//
// Two paths run the same rounds; a cloud is on the narrow one while at most `narrow_at` persons are unassigned:
//   wide    two launches per round: emd_bid_kernel, one wave per person (assigned persons leave at once), and
//           emd_assign_kernel, one workgroup per cloud over the objects, which also ends the round
//   narrow  emd_narrow_kernel, one workgroup per cloud, up to `narrow_rounds` rounds per launch between workgroup
//           barriers; its 16 waves share the bidders of a compacted list that each round rewrites (losers and evicted
//           owners), so that a round with three bidders costs three scans of the objects and no launch
// A round's end (both paths, the same code) counts the round, ends the phase -- clears the assignment and steps to the
// next epsilon -- when nobody is unassigned, and sets the cloud to "capped" at `iters` rounds.  No kernel waits on
// another workgroup; every loop is bounded by n, `phases` or `narrow_rounds`; clouds that are done, capped or on the
// other path leave at once, so surplus launches are no-ops.  The host loop (ops.py) reads one 32-byte record per cloud
// between batches of launches.
#include "tpg_common.hpp"

namespace {

constexpr int EMD_ACTIVE = 0, EMD_DONE = 1, EMD_CAPPED = 2;
constexpr int EMD_BID_WAVES = 4;      // persons per workgroup of the wide bid kernel
constexpr int EMD_BLOCK = 1024;       // the one workgroup per cloud of the round ends and of the narrow path
constexpr int EMD_BLOCK_WAVES = EMD_BLOCK / 64;

struct EmdState {                     // per cloud, 32 bytes, at the start of the workspace (the host reads it)
    int phase, rounds, unassigned, status, pad[4];
};

struct EmdWs {
    EmdState *state;                  // (B)
    float4 *obj;                      // (B,n) {x, y, z, price} of the objects
    tpg_u64 *key;                     // (B,n) highest bid so far
    int *owner;                       // (B,n) object -> person, -1
    int *choice;                      // (B,n) person -> the object of its bid in this round (narrow path)
    int *list[2];                     // (B,n) the unassigned persons of this / the next round (narrow path)
};

inline size_t emd_pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

inline size_t emd_layout(void *ws, int B, int n, EmdWs *out) {
    const size_t bn = (size_t)B * n;
    char *p = static_cast<char *>(ws);
    size_t off = 0;
    EmdWs w;
    w.state = reinterpret_cast<EmdState *>(p + off); off += emd_pad(sizeof(EmdState) * (size_t)B);
    w.obj = reinterpret_cast<float4 *>(p + off); off += emd_pad(sizeof(float4) * bn);
    w.key = reinterpret_cast<tpg_u64 *>(p + off); off += emd_pad(sizeof(tpg_u64) * bn);
    w.owner = reinterpret_cast<int *>(p + off); off += emd_pad(sizeof(int) * bn);
    w.choice = reinterpret_cast<int *>(p + off); off += emd_pad(sizeof(int) * bn);
    w.list[0] = reinterpret_cast<int *>(p + off); off += emd_pad(sizeof(int) * bn);
    w.list[1] = reinterpret_cast<int *>(p + off); off += emd_pad(sizeof(int) * bn);
    if (out) *out = w;
    return off;
}

// float <-> an int that orders like the float (no NaN handling: a NaN never becomes a candidate)
__device__ __forceinline__ int emd_ord(float v) {
    const int b = __float_as_int(v);
    return b ^ ((b >> 31) & 0x7FFFFFFF);
}
__device__ __forceinline__ float emd_unord(int o) { return __int_as_float(o ^ ((o >> 31) & 0x7FFFFFFF)); }

__device__ __forceinline__ float emd_eps(float eps, float scaling, int k, int phases) {
    float e = eps;
    for (int t = 0; t < phases; ++t)
        if (t < k) e = e * scaling;
    return e;
}

// The bid of person i = (px, py, pz) over the n objects of its cloud, by one whole wave: -> the object (in every
// lane, inside [0, n)) and the bid's key.
__device__ __forceinline__ void emd_bid(const float4 *obj, int n, float px, float py, float pz, int i, float eps_k,
                                        int lane, int *j_out, tpg_u64 *key_out) {
    float v1 = -INFINITY, v2 = -INFINITY;
    int j1 = 0x7FFFFFFF;
#pragma unroll 4
    for (int j = lane; j < n; j += 64) {
        const float4 o = obj[j];
        const float c = tpg_sq3(px, py, pz, o.x, o.y, o.z);
        const float v = (-c) - o.w;
        if (v > v1) {                  // j ascends within a lane: an equal value keeps the lower j and counts as second
            v2 = v1;
            v1 = v;
            j1 = j;
        } else if (v > v2) {
            v2 = v;
        }
    }
    // best: highest value, then lowest j; second: the highest value of everything but the best
    const tpg_u64 mine = ((tpg_u64)((unsigned)emd_ord(v1) ^ 0x80000000u) << 32) | (0xFFFFFFFFu - (unsigned)j1);
    const tpg_u64 top = tpg_wave_max_u64(mine);
    const float b2 = emd_unord(tpg_wave_max_i32(emd_ord(mine == top ? v2 : v1)));
    const float b1 = emd_unord((int)((unsigned)(top >> 32) ^ 0x80000000u));
    int j = (int)(0xFFFFFFFFu - (unsigned)top);
    if ((unsigned)j >= (unsigned)n) j = 0;               // only when no value compared at all (NaN coordinates)
    const float p = obj[j].w;
    const float inc = (b1 - b2) + eps_k;
    float pn = p + inc;
    if (!(pn > p)) pn = __uint_as_float(__float_as_uint(p) + 1u);     // nextafter(p, +inf) of a non-negative float
    *j_out = j;
    *key_out = ((tpg_u64)__float_as_uint(pn) << 32) | (0xFFFFFFFFu - (unsigned)i);
}

// The end of a round in which `newly` persons took a free object.  Every thread of the cloud's workgroup calls it with
// the same arguments and keeps the same state; -> true when a new phase starts (the caller clears the assignment).
__device__ __forceinline__ bool emd_round_end(EmdState *s, int newly, int n, int iters) {
    bool reset = false;
    s->unassigned -= newly;
    s->rounds += 1;
    if (s->unassigned == 0) {
        if (s->phase == 0) {
            s->status = EMD_DONE;
        } else {
            s->phase -= 1;
            s->unassigned = n;
            reset = true;
        }
    }
    if (s->status == EMD_ACTIVE && s->rounds >= iters) s->status = EMD_CAPPED;
    return reset;
}

__global__ __launch_bounds__(256) void emd_init_kernel(const float *__restrict__ xyz2, int n, int phases,
                                                       EmdWs w, int32_t *__restrict__ assign) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t at = (size_t)b * n + j;
    w.obj[at] = make_float4(xyz2[at * 3], xyz2[at * 3 + 1], xyz2[at * 3 + 2], 0.0f);
    w.key[at] = 0;
    w.owner[at] = n == 1 ? 0 : -1;
    assign[at] = n == 1 ? 0 : -1;
    if (j == 0) {
        EmdState s = {};
        s.phase = n == 1 ? 0 : phases;
        s.unassigned = n == 1 ? 0 : n;
        s.status = n == 1 ? EMD_DONE : EMD_ACTIVE;
        w.state[b] = s;
    }
}

__global__ __launch_bounds__(EMD_BID_WAVES * 64) void emd_bid_kernel(const float *__restrict__ xyz1, int n, float eps,
                                                                     float scaling, int phases, int narrow_at, EmdWs w,
                                                                     const int32_t *assign) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int i = blockIdx.x * EMD_BID_WAVES + wave;
    if (i >= n) return;
    const EmdState s = w.state[b];
    if (s.status != EMD_ACTIVE || s.unassigned <= narrow_at) return;
    const size_t base = (size_t)b * n;
    if (assign[base + i] >= 0) return;
    const float *x = xyz1 + (base + i) * 3;
    int j;
    tpg_u64 key;
    emd_bid(w.obj + base, n, x[0], x[1], x[2], i, emd_eps(eps, scaling, s.phase, phases), lane, &j, &key);
    if (lane == 0) atomicMax(w.key + base + j, key);
}

__global__ __launch_bounds__(EMD_BLOCK) void emd_assign_kernel(int n, int iters, int narrow_at, EmdWs w,
                                                               int32_t *assign) {
    __shared__ int newly;
    const int b = blockIdx.x, tid = threadIdx.x;
    EmdState s = w.state[b];
    if (s.status != EMD_ACTIVE || s.unassigned <= narrow_at) return;      // the whole workgroup
    const size_t base = (size_t)b * n;
    float4 *obj = w.obj + base;
    const tpg_u64 *key = w.key + base;
    int *owner = w.owner + base;
    int32_t *as = assign + base;
    if (tid == 0) newly = 0;
    __syncthreads();
    int mine = 0;
    for (int j = tid; j < n; j += EMD_BLOCK) {
        const tpg_u64 k = key[j];
        const unsigned bits = (unsigned)(k >> 32);
        if (bits > __float_as_uint(obj[j].w)) {          // a bid of this round: its winner takes the object
            const int i = tpg_clamp_idx((int)(0xFFFFFFFFu - (unsigned)k), n);
            const int prev = owner[j];
            if (prev >= 0) as[tpg_clamp_idx(prev, n)] = -1;   // prev is assigned, so it is nobody's winner i
            else ++mine;
            owner[j] = i;
            as[i] = j;
            obj[j].w = __uint_as_float(bits);
        }
    }
    if (mine) atomicAdd(&newly, mine);
    __syncthreads();
    if (emd_round_end(&s, newly, n, iters)) {
        for (int j = tid; j < n; j += EMD_BLOCK) {
            owner[j] = -1;
            as[j] = -1;
        }
    }
    if (tid == 0) w.state[b] = s;
}

__global__ __launch_bounds__(EMD_BLOCK) void emd_narrow_kernel(const float *__restrict__ xyz1, int n, float eps,
                                                               float scaling, int phases, int iters, int narrow_at,
                                                               int max_rounds, EmdWs w, int32_t *assign) {
    __shared__ int cnt[2];
    __shared__ int newly;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    EmdState s = w.state[b];
    if (s.status != EMD_ACTIVE || s.unassigned > narrow_at) return;       // the whole workgroup
    const size_t base = (size_t)b * n;
    float4 *obj = w.obj + base;
    tpg_u64 *key = w.key + base;
    int *owner = w.owner + base, *choice = w.choice + base;
    int *list[2] = {w.list[0] + base, w.list[1] + base};
    int32_t *as = assign + base;
    const float *x1 = xyz1 + base * 3;
    if (tid == 0) {
        cnt[0] = 0;
        cnt[1] = 0;
        newly = 0;
    }
    __syncthreads();
    // the unassigned persons, in the order the atomics hand out: nothing below depends on it
    for (int i = tid; i < n; i += EMD_BLOCK)
        if (as[i] < 0) list[0][min(atomicAdd(&cnt[0], 1), n - 1)] = i;
    __syncthreads();
    int cur = 0;
    for (int r = 0; r < max_rounds; ++r) {
        if (s.status != EMD_ACTIVE || s.unassigned > narrow_at) break;    // the same in every thread
        const int *lst = list[cur];
        int *nxt = list[cur ^ 1];
        const int m = min(cnt[cur], n);
        const float eps_k = emd_eps(eps, scaling, s.phase, phases);
        for (int pos = wave; pos < m; pos += EMD_BLOCK_WAVES) {
            const int i = tpg_clamp_idx(lst[pos], n);
            int j;
            tpg_u64 k;
            emd_bid(obj, n, x1[(size_t)i * 3], x1[(size_t)i * 3 + 1], x1[(size_t)i * 3 + 2], i, eps_k, lane, &j, &k);
            if (lane == 0) {
                atomicMax(key + j, k);
                choice[i] = j;
            }
        }
        __syncthreads();
        for (int pos = tid; pos < m; pos += EMD_BLOCK) {
            const int i = tpg_clamp_idx(lst[pos], n);
            const int j = tpg_clamp_idx(choice[i], n);
            const tpg_u64 k = key[j];
            if ((unsigned)k == 0xFFFFFFFFu - (unsigned)i) {               // i holds the object's highest bid
                const int prev = owner[j];
                if (prev >= 0) {
                    as[tpg_clamp_idx(prev, n)] = -1;
                    nxt[min(atomicAdd(&cnt[cur ^ 1], 1), n - 1)] = prev;
                } else {
                    atomicAdd(&newly, 1);
                }
                owner[j] = i;
                as[i] = j;
                obj[j].w = __uint_as_float((unsigned)(k >> 32));
            } else {
                nxt[min(atomicAdd(&cnt[cur ^ 1], 1), n - 1)] = i;
            }
        }
        __syncthreads();
        const bool reset = emd_round_end(&s, newly, n, iters);
        if (reset) {                                                      // a new phase: everybody bids again
            for (int j = tid; j < n; j += EMD_BLOCK) {
                owner[j] = -1;
                as[j] = -1;
                nxt[j] = j;
            }
        }
        __syncthreads();                                                  // everybody has read newly and cnt
        if (tid == 0) {
            newly = 0;
            cnt[cur] = 0;
            if (reset) cnt[cur ^ 1] = n;
        }
        cur ^= 1;
        __syncthreads();
    }
    if (tid == 0) w.state[b] = s;
}

__global__ __launch_bounds__(256) void emd_finish_kernel(const float *__restrict__ xyz1, int n, EmdWs w,
                                                         const int32_t *__restrict__ assign, float *__restrict__ dist,
                                                         float *__restrict__ price, int32_t *__restrict__ rounds) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t base = (size_t)b * n;
    const float4 o = w.obj[base + tpg_clamp_idx(assign[base + i], n)];
    const float *x = xyz1 + (base + i) * 3;
    dist[base + i] = tpg_sq3(x[0], x[1], x[2], o.x, o.y, o.z);
    price[base + i] = w.obj[base + i].w;
    if (i == 0) rounds[b] = w.state[b].rounds;
}

// > 0: nothing to do (TPG_OK), < 0: the status to return, 0: go on
int emd_check(int B, int n, const void *ws) {
    if (B < 0 || n < 0) return TPG_ERR_ARG;
    if (B == 0 || n == 0) return 1;
    if (B > 65535) return TPG_ERR_UNSUPPORTED;                            // clouds ride on gridDim.y
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return TPG_ERR_ARG;
    return 0;
}

}  // namespace

extern "C" size_t tpg_emd_workspace_bytes(int B, int n) {
    if (B <= 0 || n <= 0) return 0;
    return emd_layout(nullptr, B, n, nullptr);
}

extern "C" int tpg_emd_init_f32(const float *xyz2, int B, int n, int m, int phases, int32_t *assignment, void *ws,
                                void *stream) {
    if (phases < 0 || phases > 64 || n != m) return TPG_ERR_ARG;
    const int chk = emd_check(B, n, ws);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!xyz2 || !assignment) return TPG_ERR_ARG;
    EmdWs w;
    emd_layout(ws, B, n, &w);
    hipLaunchKernelGGL(emd_init_kernel, dim3((n + 255) / 256, B), dim3(256), 0, tpg_stream(stream), xyz2, n, phases, w,
                       assignment);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_emd_rounds_f32(const float *xyz1, int B, int n, float eps, float scaling, int phases, int iters,
                                  int wide_rounds, int narrow_rounds, int narrow_at, int32_t *assignment, void *ws,
                                  void *stream) {
    if (!(eps > 0.0f) || !(scaling >= 1.0f) || phases < 0 || phases > 64 || iters < 1 || wide_rounds < 0 ||
        narrow_rounds < 0 || narrow_at < 0 || wide_rounds > 4096)
        return TPG_ERR_ARG;
    // a call that could not advance a cloud would make the host loop spin
    if ((narrow_at > 0 && narrow_rounds < 1) || (narrow_at < n && wide_rounds < 1)) return TPG_ERR_ARG;
    const int chk = emd_check(B, n, ws);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!xyz1 || !assignment) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    EmdWs w;
    emd_layout(ws, B, n, &w);
    if (narrow_at < n) {
        for (int r = 0; r < wide_rounds; ++r) {
            hipLaunchKernelGGL(emd_bid_kernel, dim3((n + EMD_BID_WAVES - 1) / EMD_BID_WAVES, B),
                               dim3(EMD_BID_WAVES * 64), 0, st, xyz1, n, eps, scaling, phases, narrow_at, w, assignment);
            hipLaunchKernelGGL(emd_assign_kernel, dim3(B), dim3(EMD_BLOCK), 0, st, n, iters, narrow_at, w, assignment);
        }
    }
    if (narrow_at > 0)
        hipLaunchKernelGGL(emd_narrow_kernel, dim3(B), dim3(EMD_BLOCK), 0, st, xyz1, n, eps, scaling, phases, iters,
                           narrow_at, narrow_rounds, w, assignment);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_emd_finish_f32(const float *xyz1, int B, int n, const int32_t *assignment, void *ws, float *dist,
                                  float *price, int32_t *rounds, void *stream) {
    const int chk = emd_check(B, n, ws);
    if (chk) return chk > 0 ? TPG_OK : chk;
    if (!xyz1 || !assignment || !dist || !price || !rounds) return TPG_ERR_ARG;
    EmdWs w;
    emd_layout(ws, B, n, &w);
    hipLaunchKernelGGL(emd_finish_kernel, dim3((n + 255) / 256, B), dim3(256), 0, tpg_stream(stream), xyz1, n, w,
                       assignment, dist, price, rounds);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
