// The uniform grid that frnn_grid.hip, radius_reduce.hip, pbf.hip and aniso.hip query: its parameters and workspace
// layout, the build's entry (the four build kernels are compiled once, in frnn_grid.hip) and the walk over the 27
// cells around a query (fg_query_kernel, rr_kernel and the two anisotropic stages call it; pbf.hip keeps a copy of its
// own, for speed: see there).
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
// Walk (one wave per query): the 27 cells are 9 runs of 3 x-adjacent cells, each a contiguous range of the cell-sorted
// array; the lanes take 64 candidates of the concatenated runs per trip.
#pragma once
#include "tpg_common.hpp"

constexpr int FG_MAXDIM = 64;           // cells per axis
constexpr int FG_WAVES = 4;             // queries per workgroup
constexpr int FG_CELLS = FG_MAXDIM * FG_MAXDIM * FG_MAXDIM;

struct GridParams {                     // per cloud, 8 floats / ints
    float lo[3];
    float inv_h;
    int dim[3];
    int ncell;
};

// what a kernel that queries the grid is given: per cloud b, gp[b], the FG_CELLS + 1 cell starts from
// start + b * (FG_CELLS + 1) and the P2 cell-sorted points (x, y, z, bits of the original index) from sorted + b * P2
struct GridView {
    const GridParams *gp;
    const int *start;
    const float4 *sorted;
};

__device__ __forceinline__ int cell_axis(float p, float lo, float inv_h) {
    return (int)floorf((p - lo) * inv_h);
}

// the cell a stored point is filed under: cell_axis clamped into the grid
__device__ __forceinline__ int cell_of(const GridParams &g, float px, float py, float pz) {
    int cx = cell_axis(px, g.lo[0], g.inv_h), cy = cell_axis(py, g.lo[1], g.inv_h), cz = cell_axis(pz, g.lo[2], g.inv_h);
    cx = min(max(cx, 0), g.dim[0] - 1);
    cy = min(max(cy, 0), g.dim[1] - 1);
    cz = min(max(cz, 0), g.dim[2] - 1);
    return (cz * g.dim[1] + cy) * g.dim[0] + cx;
}

// cell_axis for a query that may lie anywhere (a lattice around the fluid, a dummy at 999, 1e30): the same value inside
// [-2, FG_MAXDIM + 2), clamped in float before the conversion outside it (and NaN -> -2), where the walk selects nothing
__device__ __forceinline__ int fg_cell_any(float p, float lo, float inv_h) {
    return (int)floorf(fminf(fmaxf((p - lo) * inv_h, -2.0f), (float)(FG_MAXDIM + 2)));
}

// points of cloud b that the grid holds: lengths[b] clamped into [0, P2] in 64 bits, BEFORE the narrowing (2^32 + 5 is
// P2 points, not 5), the same for every launch of the build and for whoever walks the grid with lengths of its own
__device__ __forceinline__ int fg_len(const int64_t *__restrict__ len2, int b, int P2) {
    return len2 ? (int)min(max(len2[b], (int64_t)0), (int64_t)P2) : P2;
}

// The walk over the 27 cells around cell (cx, cy, cz) of one cloud (st: its cell starts), 64 candidates per trip.
// Every trip calls f(at, has) on EVERY lane: has says whether the lane holds a candidate, and at is then its position in
// the cloud's cell-sorted array (without one, at is not an index).  The cell is the caller's: fg_cell_any's for a query that
// may lie anywhere, or one clamped into the grid (then x0 <= x1 always holds).
template <class F>
__device__ __forceinline__ void fg_walk_at(const GridParams &g, const int *__restrict__ st, int cx, int cy, int cz,
                                           int lane, F &&f) {
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
    // the 9 (dz, dy) runs: [begin, end) of the cell-sorted array, and their running total
    int rb[9], re[9], total = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int zz = cz + t / 3 - 1, yy = cy + t % 3 - 1;
        int bgn = 0, end = 0;
        if (x0 <= x1 && zz >= 0 && zz < g.dim[2] && yy >= 0 && yy < g.dim[1]) {
            const int row = (zz * g.dim[1] + yy) * g.dim[0];
            bgn = st[row + x0];
            end = st[row + x1 + 1];
        }
        rb[t] = bgn;
        re[t] = end;
        total += end - bgn;
    }
    for (int base = 0; base < total; base += 64) {
        // candidate number base + lane of the concatenated runs
        int c = base + lane, at = -1;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int n = re[t] - rb[t];
            if (at < 0 && c < n) at = rb[t] + c;
            c -= (at < 0) ? n : 0;
        }
        f(at, at >= 0 && base + lane < total);
    }
}

// the same walk, f(candidate) only on the lanes that hold one
template <class F>
__device__ __forceinline__ void fg_walk(const GridParams &g, const int *__restrict__ st, const float4 *__restrict__ pts,
                                        int cx, int cy, int cz, int lane, F &&f) {
    fg_walk_at(g, st, cx, cy, cz, lane, [&](int at, bool has) {
        if (has) f(pts[at]);
    });
}

// f(x, y, z, row) for every candidate of a query (qx, qy, qz) that may lie anywhere, on the lane that holds it: the
// points of the 27 cells around it (GRID), or every stored row below np of pos (exhaustive: the lanes stride over the
// whole cloud, no grid)
template <bool GRID, class F>
__device__ __forceinline__ void fg_candidates(float qx, float qy, float qz, const GridParams *__restrict__ gp, int b,
                                              int cstride, const int *__restrict__ start,
                                              const float4 *__restrict__ sorted, const float *__restrict__ pos, int np,
                                              int Np, int lane, F &&f) {
    if (GRID) {
        const GridParams g = gp[b];
        fg_walk(g, start + (size_t)b * (cstride + 1), sorted + (size_t)b * Np, fg_cell_any(qx, g.lo[0], g.inv_h),
                fg_cell_any(qy, g.lo[1], g.inv_h), fg_cell_any(qz, g.lo[2], g.inv_h), lane,
                [&](const float4 p) { f(p.x, p.y, p.z, __float_as_int(p.w)); });
    } else {
        const float *x = pos + (size_t)b * Np * 3;
        for (int j = lane; j < np; j += 64) f(x[(size_t)j * 3], x[(size_t)j * 3 + 1], x[(size_t)j * 3 + 2], j);
    }
}

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

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

// where fg_build keeps what a query needs in the workspace: whoever queries a grid that an earlier call built asks here
static inline GridView fg_view(const void *ws, int B, int P2) {
    const unsigned char *w = static_cast<const unsigned char *>(ws);
    GridView v;
    v.gp = reinterpret_cast<const GridParams *>(w);
    w += align256(sizeof(GridParams) * (size_t)B) + align256(sizeof(int) * (size_t)B * FG_CELLS);
    v.start = reinterpret_cast<const int *>(w);
    w += align256(sizeof(int) * (size_t)B * (FG_CELLS + 1)) + align256(sizeof(int) * (size_t)B * P2);
    v.sorted = reinterpret_cast<const float4 *>(w);
    return v;
}

// the grid build (frnn_grid.hip): r > 0: radius form, knn_k > 0: kNN form; *view = fg_view(ws, B, P2).  Shared by
// the library's translation units and by nobody else, hence hidden.
__attribute__((visibility("hidden"))) int fg_build(const float *p2, const int64_t *len2, int B, int P2, float r, int knn_k,
                                                   void *ws, hipStream_t st, GridView *view);
