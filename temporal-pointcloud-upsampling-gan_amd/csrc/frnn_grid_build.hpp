// The uniform grid of frnn_grid.hip and radius_reduce.hip: parameters, the four build launches and the workspace
// layout, shared by the translation units that query it (each gets its own copy of the kernels).
//
//   cell edge  h = max(r, extent / 64) * (1 + 1e-4)     (>= r with a margin far above fp32 rounding)
//   cell(p)    = floor((p - lo) / h) per axis, the same expression for stored points and queries
//
// Build (four small launches per call, all clouds at once):
//   bbox   per cloud: lo, 1/h, grid dims (<= 64 per axis)            one workgroup per cloud
//   count  cell of every point, int atomics on the cell counters     (deterministic totals)
//   scan   exclusive prefix of the counters                          one workgroup per cloud
//   fill   points copied into cell order as (x, y, z, original index); the order INSIDE a cell follows an atomic
//          cursor and is not fixed from run to run: a consumer's result must not depend on it
#pragma once
#include "tpg_common.hpp"

namespace {

constexpr int FG_MAXDIM = 64;           // cells per axis
constexpr int FG_WAVES = 4;             // queries per workgroup

struct GridParams {                     // per cloud, 8 floats / ints
    float lo[3];
    float inv_h;
    int dim[3];
    int ncell;
};

__device__ __forceinline__ int cell_axis(float p, float lo, float inv_h) {
    return (int)floorf((p - lo) * inv_h);
}

// points of cloud b that the grid holds: lengths[b] clamped into [0, P2] in 64 bits, BEFORE the narrowing (2^32 + 5 is
// P2 points, not 5), the same for every launch of the build and for whoever walks the grid with lengths of its own
__device__ __forceinline__ int fg_len(const int64_t *__restrict__ len2, int b, int P2) {
    return len2 ? (int)min(max(len2[b], (int64_t)0), (int64_t)P2) : P2;
}

__global__ __launch_bounds__(1024) void fg_bbox_kernel(const float *__restrict__ p2, const int64_t *__restrict__ len2,
                                                       int P2, float r, int knn_k, GridParams *__restrict__ gp) {
    __shared__ float red[6][16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n2 = fg_len(len2, b, P2);
    const float *x = p2 + (size_t)b * P2 * 3;
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int i = tid; i < n2; i += 1024)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = x[(size_t)i * 3 + d];
            mn[d] = fminf(mn[d], v);
            mx[d] = fmaxf(mx[d], v);
        }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            mn[d] = fminf(mn[d], __shfl_xor(mn[d], s));
            mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], s));
        }
        if (lane == 0) { red[d][wave] = mn[d]; red[3 + d][wave] = mx[d]; }
    }
    __syncthreads();
    if (tid == 0) {
        float ext = 0.0f;
        float lo[3];
        for (int d = 0; d < 3; ++d) {
            float a = red[d][0], c = red[3 + d][0];
            for (int w = 1; w < 16; ++w) { a = fminf(a, red[d][w]); c = fmaxf(c, red[3 + d][w]); }
            lo[d] = n2 > 0 ? a : 0.0f;
            ext = fmaxf(ext, n2 > 0 ? c - a : 0.0f);
        }
        float h = fmaxf(r, ext / (float)FG_MAXDIM) * 1.0001f;
        if (knn_k > 0) {
            // kNN form: ~K/2 points per cell (flat directions count as one cell edge of the coarsest grid), so that the
            // ball inscribed in the 27 cells around a query's cell holds ~2 K points and one pass usually settles it
            float vol = 1.0f;
            for (int d = 0; d < 3; ++d) {
                float a = red[d][0], c = red[3 + d][0];
                for (int w = 1; w < 16; ++w) { a = fminf(a, red[d][w]); c = fmaxf(c, red[3 + d][w]); }
                vol *= fmaxf(n2 > 0 ? c - a : 0.0f, ext / (float)FG_MAXDIM);
            }
            const float want = cbrtf(vol * 0.5f * (float)max(knn_k, 8) / (float)max(n2, 1));
            h = fmaxf(want, ext / (float)FG_MAXDIM) * 1.0001f;
            if (!(h > 0.0f)) h = 1.0f;                      // a cloud of identical points: one cell
        }
        GridParams g;
        g.inv_h = 1.0f / h;
        int nc = 1;
        for (int d = 0; d < 3; ++d) {
            g.lo[d] = lo[d];
            float c = red[3 + d][0];
            for (int w = 1; w < 16; ++w) c = fmaxf(c, red[3 + d][w]);
            int n = n2 > 0 ? cell_axis(c, lo[d], g.inv_h) + 1 : 1;
            n = n < 1 ? 1 : (n > FG_MAXDIM ? FG_MAXDIM : n);
            g.dim[d] = n;
            nc *= n;
        }
        g.ncell = nc;
        gp[b] = g;
    }
}

__device__ __forceinline__ int cell_of(const GridParams &g, float px, float py, float pz) {
    int cx = cell_axis(px, g.lo[0], g.inv_h), cy = cell_axis(py, g.lo[1], g.inv_h), cz = cell_axis(pz, g.lo[2], g.inv_h);
    cx = min(max(cx, 0), g.dim[0] - 1);
    cy = min(max(cy, 0), g.dim[1] - 1);
    cz = min(max(cz, 0), g.dim[2] - 1);
    return (cz * g.dim[1] + cy) * g.dim[0] + cx;
}

// counts[b][cell] += 1; cellid[b][i] = cell        grid (ceil(P2/256), B)
__global__ __launch_bounds__(256) void fg_count_kernel(const float *__restrict__ p2, const int64_t *__restrict__ len2,
                                                       int P2, const GridParams *__restrict__ gp, int cstride,
                                                       int *__restrict__ counts, int *__restrict__ cellid) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n2 = fg_len(len2, b, P2);
    if (i >= n2) return;
    const GridParams g = gp[b];
    const float *x = p2 + ((size_t)b * P2 + i) * 3;
    const int c = cell_of(g, x[0], x[1], x[2]);
    cellid[(size_t)b * P2 + i] = c;
    atomicAdd(&counts[(size_t)b * cstride + c], 1);
}

// start[b][c] = exclusive prefix of counts (start has ncell + 1 entries); counts are zeroed again to
// serve as the fill cursors.                          grid (B)
__global__ __launch_bounds__(1024) void fg_scan_kernel(const GridParams *__restrict__ gp, int cstride,
                                                       int *__restrict__ counts, int *__restrict__ start) {
    __shared__ int wsum[32];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nc = gp[b].ncell;
    int *cnt = counts + (size_t)b * cstride, *st = start + (size_t)b * (cstride + 1);
    const int per = (nc + 1023) / 1024;
    const int lo = min(tid * per, nc), hi = min(lo + per, nc);
    int local = 0;
    for (int c = lo; c < hi; ++c) local += cnt[c];
    int incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        int w = lane < 16 ? wsum[lane] : 0;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const int o = __shfl_up(w, d);
            if (lane >= d) w += o;
        }
        if (lane < 16) wsum[16 + lane] = w;
    }
    __syncthreads();
    int run = incl - local + (wave ? wsum[16 + wave - 1] : 0);
    for (int c = lo; c < hi; ++c) {
        const int n = cnt[c];
        st[c] = run;
        cnt[c] = 0;
        run += n;
    }
    if (tid == 0) st[nc] = wsum[16 + 15];
}

// sorted[b][start[cell] + k] = (x, y, z, bits of i)      grid (ceil(P2/256), B)
__global__ __launch_bounds__(256) void fg_fill_kernel(const float *__restrict__ p2, const int64_t *__restrict__ len2,
                                                      int P2, int cstride, const int *__restrict__ cellid,
                                                      const int *__restrict__ start, int *__restrict__ cursor,
                                                      float4 *__restrict__ sorted) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n2 = fg_len(len2, b, P2);
    if (i >= n2) return;
    const int c = cellid[(size_t)b * P2 + i];
    const int pos = start[(size_t)b * (cstride + 1) + c] + atomicAdd(&cursor[(size_t)b * cstride + c], 1);
    const float *x = p2 + ((size_t)b * P2 + i) * 3;
    sorted[(size_t)b * P2 + pos] = make_float4(x[0], x[1], x[2], __int_as_float(i));
}

constexpr int FG_CELLS = FG_MAXDIM * FG_MAXDIM * FG_MAXDIM;

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

// bytes of the workspace fg_build carves up: params | counters / cursors | starts | cell ids | cell-sorted points
static inline size_t fg_workspace_bytes(int B, int P2) {
    if (B <= 0 || P2 <= 0) return 0;
    return align256(sizeof(GridParams) * (size_t)B) + align256(sizeof(int) * (size_t)B * FG_CELLS) +
           align256(sizeof(int) * (size_t)B * (FG_CELLS + 1)) + align256(sizeof(int) * (size_t)B * P2) +
           align256(sizeof(float4) * (size_t)B * P2);
}

// what every entry that builds the grid asks of the workspace pointer
static inline bool fg_workspace_ok(const void *ws) { return ws && !(reinterpret_cast<uintptr_t>(ws) & 255); }

// workgroups along x of a one-wave-per-query launch over P1 queries (FG_WAVES * 64 threads each)
static inline unsigned fg_query_blocks(int P1) { return (unsigned)((P1 + FG_WAVES - 1) / FG_WAVES); }

// where fg_build keeps its results in the workspace: whoever queries a grid that an earlier call built asks here
static inline void fg_carve(void *ws, int B, int P2, GridParams **gp_o, int **counts_o, int **start_o, int **cellid_o,
                            float4 **sorted_o) {
    unsigned char *w = static_cast<unsigned char *>(ws);
    *gp_o = reinterpret_cast<GridParams *>(w);
    w += align256(sizeof(GridParams) * (size_t)B);
    *counts_o = reinterpret_cast<int *>(w);
    w += align256(sizeof(int) * (size_t)B * FG_CELLS);
    *start_o = reinterpret_cast<int *>(w);
    w += align256(sizeof(int) * (size_t)B * (FG_CELLS + 1));
    *cellid_o = reinterpret_cast<int *>(w);
    w += align256(sizeof(int) * (size_t)B * P2);
    *sorted_o = reinterpret_cast<float4 *>(w);
}

// grid build shared by the entries; r > 0: radius form, knn_k > 0: kNN form
static int fg_build(const float *p2, const int64_t *len2, int B, int P2, float r, int knn_k, void *ws, hipStream_t st,
                    GridParams **gp_o, int **start_o, float4 **sorted_o) {
    GridParams *gp; int *counts, *start, *cellid; float4 *sorted;
    fg_carve(ws, B, P2, &gp, &counts, &start, &cellid, &sorted);
    if (hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B * FG_CELLS, st) != hipSuccess) return TPG_ERR_LAUNCH;
    const dim3 pg((P2 + 255) / 256, B);
    hipLaunchKernelGGL(fg_bbox_kernel, dim3(B), dim3(1024), 0, st, p2, len2, P2, r, knn_k, gp);
    hipLaunchKernelGGL(fg_count_kernel, pg, dim3(256), 0, st, p2, len2, P2, gp, FG_CELLS, counts, cellid);
    hipLaunchKernelGGL(fg_scan_kernel, dim3(B), dim3(1024), 0, st, gp, FG_CELLS, counts, start);
    hipLaunchKernelGGL(fg_fill_kernel, pg, dim3(256), 0, st, p2, len2, P2, FG_CELLS, cellid, start, counts, sorted);
    *gp_o = gp; *start_o = start; *sorted_o = sorted;
    return TPG_OK;
}
