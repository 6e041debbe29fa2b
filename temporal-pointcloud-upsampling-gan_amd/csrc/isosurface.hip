// Isosurfaces of a scalar field on a regular lattice: marching tetrahedra on the Kuhn (Freudenthal) split of every lattice
// cube into six tetrahedra, as indexed triangle meshes (vertices, normals, faces).  include/tpgan_ops.h has the rule in
// full ("isosurfaces"); the mesher is this project's own (the reference hands its frames to an external tool).  Every
// index depends on the field only through the nodes' inside flags (field >= iso), so no field value, NaN and inf
// included, can produce an index out of range; all floating point is fp32, one rounding per operation.
//
// Two entries with one host read of the two totals between them:
//   tpg_iso_count_f32
//       iso_classify   one workgroup per tile of ISO_TILE = 2048 nodes, 8 nodes per lane (coalesced: lane t takes nodes
//                      tile + 256 s + t).  Per node the 8 corners of its cube are read (where they exist), the 7-bit mask
//                      of active edges and the cell's triangle count 0..12 go to two byte arrays, and the tile's two
//                      totals, packed into one 64-bit word (faces high, vertices low: neither reaches 2^32 at G <= 2^27),
//                      to sums[tile].
//       iso_scan_sums  ONE workgroup turns sums[] into exclusive prefixes, 256 at a time with a running carry, and writes
//                      the totals [V, F].  At most 65 536 tiles: 256 rounds.
//       iso_offsets    one workgroup per tile, 8 CONSECUTIVE nodes per lane (two 8-byte loads): lane-local prefixes,
//                      a wave scan of the lane totals, the four wave totals through LDS, the tile's prefix on top; the
//                      exclusive offsets go out as 16-byte stores.
//       A reduce / scan-of-sums / add chain: no workgroup waits for another inside a launch.
//   tpg_iso_emit_f32
//       iso_vertices   one lane per node: vertex offset[n] + popcount(mask & ((1 << d) - 1)) for each active edge d.
//       iso_faces      one lane per cell: the 8 inside flags again, then per tetrahedron the case's triangles; an edge of
//                      a tetrahedron is owned by its corner that comes first on the path, the direction is the corner
//                      offsets' difference, and the vertex index follows from that node's offset and mask.
//       Nothing is written at or beyond V_cap / F_cap.
// Integer prefix sums and one writer per output element: the same bits, order included, on every run.  No atomics, no LDS
// beyond the scans' 4 words, no scratch.
#include "tpg_common.hpp"

#include <math.h>

namespace {

constexpr int ISO_THREADS = 256;
constexpr int ISO_ITEMS = 8;
constexpr int ISO_TILE = ISO_THREADS * ISO_ITEMS;
constexpr long long ISO_MAX_NODES = 1ll << 27;

// Corner codes: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Nibble d of ISO_DIR_CODE: the code of direction D[d]; nibble c of
// ISO_CODE_DIR: the direction of the code c.  Nibble p of ISO_PATH1 / ISO_PATH2: the codes of v1 and v2 of tetrahedron p
// (xyz, xzy, yxz, yzx, zxy, zyx); v0 = 0 and v3 = 7 for all six.
constexpr unsigned ISO_DIR_CODE = 0x7563421u;
constexpr unsigned ISO_CODE_DIR = 0x64523100u;
constexpr unsigned ISO_PATH1 = 0x442211u;
constexpr unsigned ISO_PATH2 = 0x656353u;

constexpr int iso_nibble(unsigned word, int at) { return (int)((word >> (4 * at)) & 7u); }
constexpr int iso_path_code(int p, int a) { return a == 0 ? 0 : (a == 1 ? iso_nibble(ISO_PATH1, p) : (a == 2 ? iso_nibble(ISO_PATH2, p) : 7)); }

constexpr bool iso_tables_ok() {
    const int D[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}, {1, 1, 1}};
    const int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int d = 0; d < 7; ++d) {
        const int code = D[d][0] | (D[d][1] << 1) | (D[d][2] << 2);
        if (iso_nibble(ISO_DIR_CODE, d) != code || iso_nibble(ISO_CODE_DIR, code) != d) return false;
    }
    for (int p = 0; p < 6; ++p) {
        const int c1 = 1 << P[p][0], c2 = c1 | (1 << P[p][1]);
        if (iso_path_code(p, 1) != c1 || iso_path_code(p, 2) != c2 || (c2 | (1 << P[p][2])) != 7) return false;
    }
    return true;
}
static_assert(iso_tables_ok(), "the packed direction / path tables disagree with D and the permutations");

struct IsoDims {
    int nx, ny, nz, G;
};

struct IsoOrigin {
    float o[3];
};

// bit `case` of flip[p]: the triangles of that case of tetrahedron p are listed with their last two vertices exchanged
struct IsoWinding {
    unsigned short flip[6];
};

// The winding table in exact integer arithmetic (the rule's recipe): every edge vertex at its midpoint in doubled lattice
// coordinates, the sign of (q-p) x (r-p) . (sum of outside corners - sum of inside corners).  No tetrahedron is
// degenerate, so the sign is never 0 and does not depend on where in (0,1) the vertices sit.
IsoWinding iso_winding() {
    IsoWinding w;
    for (int p = 0; p < 6; ++p) {
        int corner[4][3];
        for (int a = 0; a < 4; ++a)
            for (int x = 0; x < 3; ++x) corner[a][x] = (iso_path_code(p, a) >> x) & 1;
        unsigned short bits = 0;
        for (int cs = 1; cs < 15; ++cs) {
            int in[4], out[4], ni = 0, no = 0;
            for (int a = 0; a < 4; ++a) {
                if ((cs >> a) & 1) in[ni++] = a;
                else out[no++] = a;
            }
            int e[3][2];                                   // the first triangle's edges, as pairs of path positions
            if (ni == 2) {
                e[0][0] = in[0], e[0][1] = out[0];
                e[1][0] = in[0], e[1][1] = out[1];
                e[2][0] = in[1], e[2][1] = out[1];
            } else {
                const int s = ni == 1 ? in[0] : out[0];
                for (int a = 0, k = 0; a < 4; ++a)
                    if (a != s) e[k][0] = s, e[k][1] = a, ++k;
            }
            long long m[3][3], dir[3];
            for (int x = 0; x < 3; ++x) {
                for (int k = 0; k < 3; ++k) m[k][x] = corner[e[k][0]][x] + corner[e[k][1]][x];
                dir[x] = 0;
                for (int a = 0; a < 4; ++a) dir[x] += ((cs >> a) & 1) ? -2 * corner[a][x] : 2 * corner[a][x];
            }
            long long u[3], v[3];
            for (int x = 0; x < 3; ++x) u[x] = m[1][x] - m[0][x], v[x] = m[2][x] - m[0][x];
            const long long s = (u[1] * v[2] - u[2] * v[1]) * dir[0] + (u[2] * v[0] - u[0] * v[2]) * dir[1] +
                                (u[0] * v[1] - u[1] * v[0]) * dir[2];
            if (s < 0) bits |= (unsigned short)(1u << cs);
        }
        w.flip[p] = bits;
    }
    return w;
}

// ---- workspace: offsets of vertices and faces (uint32 each), masks and triangle counts (bytes), the tiles' sums ---------
inline long long iso_padded(long long G) { return (G + ISO_TILE - 1) / ISO_TILE * ISO_TILE; }

struct IsoWorkspace {
    unsigned *voff, *foff;
    unsigned char *mask, *ntri;
    tpg_u64 *sums;
    int tiles;
};

inline IsoWorkspace iso_carve(void *ws, long long G) {
    const long long Gp = iso_padded(G);
    char *p = (char *)ws;
    IsoWorkspace w;
    w.voff = (unsigned *)p;
    w.foff = (unsigned *)(p + 4 * Gp);
    w.mask = (unsigned char *)(p + 8 * Gp);
    w.ntri = (unsigned char *)(p + 9 * Gp);
    w.sums = (tpg_u64 *)(p + 10 * Gp);
    w.tiles = (int)(Gp / ISO_TILE);
    return w;
}

inline bool iso_finite(float x) { return fabsf(x) < INFINITY; }                  // false for NaN

// ---- device helpers -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int iso_offset(int code, const IsoDims &dm) {
    return ((code & 1) * dm.ny + ((code >> 1) & 1)) * dm.nz + ((code >> 2) & 1);
}

// bit c: the corner with code c of node n's cube exists and is inside; `exist`: bit c set where the corner exists
__device__ __forceinline__ unsigned iso_corners(const float *__restrict__ field, int n, const IsoDims &dm, float iso,
                                                unsigned &exist) {
    const int k = n % dm.nz, ij = n / dm.nz;
    const int j = ij % dm.ny, i = ij / dm.ny;
    const unsigned ex = (i + 1 < dm.nx ? 1u : 0u) | (j + 1 < dm.ny ? 2u : 0u) | (k + 1 < dm.nz ? 4u : 0u);
    unsigned in = 0;
    exist = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if ((c & ~ex) == 0) {                               // every axis the code steps along has a next node
            exist |= 1u << c;
            if (field[n + iso_offset(c, dm)] >= iso) in |= 1u << c;           // false for NaN: outside
        }
    }
    return in;
}

__device__ __forceinline__ unsigned iso_edge_mask(unsigned in, unsigned exist) {
    const unsigned self = in & 1u;
    unsigned mask = 0;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        const int c = iso_nibble(ISO_DIR_CODE, d);
        if (((exist >> c) & 1u) && ((in >> c) & 1u) != self) mask |= 1u << d;
    }
    return mask;
}

// the 4-bit case of tetrahedron p: bit a = the corner at path position a is inside
__device__ __forceinline__ unsigned iso_case(unsigned in, int p) {
    return (in & 1u) | (((in >> iso_path_code(p, 1)) & 1u) << 1) | (((in >> iso_path_code(p, 2)) & 1u) << 2) |
           (((in >> 7) & 1u) << 3);
}

__device__ __forceinline__ int iso_case_triangles(unsigned cs) {
    const int c = __popc(cs);
    return c == 2 ? 2 : ((c == 1 || c == 3) ? 1 : 0);
}

// exclusive prefix of v over the workgroup's lanes in lane order; `total` in every lane.  lds: 4 words.
__device__ __forceinline__ tpg_u64 iso_block_scan(tpg_u64 v, tpg_u64 *lds, tpg_u64 &total) {
    const int lane = threadIdx.x & (TPG_WAVE - 1), wave = threadIdx.x >> 6;
    tpg_u64 inc = v;
#pragma unroll
    for (int s = 1; s < TPG_WAVE; s <<= 1) {
        const tpg_u64 o = __shfl_up(inc, s);
        if (lane >= s) inc += o;
    }
    __syncthreads();                                        // the previous use of lds is over
    if (lane == TPG_WAVE - 1) lds[wave] = inc;
    __syncthreads();
    tpg_u64 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < ISO_THREADS / TPG_WAVE; ++w) {
        const tpg_u64 t = lds[w];
        if (w < wave) before += t;
        all += t;
    }
    total = all;
    return before + inc - v;
}

// ---- count ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ISO_THREADS) void iso_classify_kernel(const float *__restrict__ field, IsoDims dm, float iso,
                                                                   unsigned char *__restrict__ mask,
                                                                   unsigned char *__restrict__ ntri,
                                                                   tpg_u64 *__restrict__ sums) {
    __shared__ tpg_u64 lds[ISO_THREADS / TPG_WAVE];
    const int base = blockIdx.x * ISO_TILE;
    tpg_u64 mine = 0;
#pragma unroll 1
    for (int s = 0; s < ISO_ITEMS; ++s) {
        const int n = base + s * ISO_THREADS + threadIdx.x;                   // < padded G: both arrays are padded
        unsigned m = 0, t = 0;
        if (n < dm.G) {
            unsigned exist;
            const unsigned in = iso_corners(field, n, dm, iso, exist);
            m = iso_edge_mask(in, exist);
            if (exist == 0xFFu) {
#pragma unroll
                for (int p = 0; p < 6; ++p) t += iso_case_triangles(iso_case(in, p));
            }
        }
        mask[n] = (unsigned char)m;
        ntri[n] = (unsigned char)t;
        mine += ((tpg_u64)t << 32) | (tpg_u64)__popc(m);
    }
    tpg_u64 total;
    iso_block_scan(mine, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(ISO_THREADS) void iso_scan_sums_kernel(tpg_u64 *__restrict__ sums, int tiles,
                                                                    int64_t *__restrict__ counts) {
    __shared__ tpg_u64 lds[ISO_THREADS / TPG_WAVE];
    tpg_u64 carry = 0;
    for (int at = 0; at < tiles; at += ISO_THREADS) {
        const int i = at + threadIdx.x;
        const tpg_u64 v = i < tiles ? sums[i] : 0;
        tpg_u64 total;
        const tpg_u64 before = iso_block_scan(v, lds, total);
        if (i < tiles) sums[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)(carry & 0xFFFFFFFFull);
        counts[1] = (int64_t)(carry >> 32);
    }
}

__global__ __launch_bounds__(ISO_THREADS) void iso_offsets_kernel(const unsigned char *__restrict__ mask,
                                                                  const unsigned char *__restrict__ ntri,
                                                                  const tpg_u64 *__restrict__ sums,
                                                                  unsigned *__restrict__ voff, unsigned *__restrict__ foff) {
    __shared__ tpg_u64 lds[ISO_THREADS / TPG_WAVE];
    const size_t first = (size_t)blockIdx.x * ISO_TILE + (size_t)threadIdx.x * ISO_ITEMS;   // a multiple of 8
    const tpg_u64 m8 = *(const tpg_u64 *)(mask + first), t8 = *(const tpg_u64 *)(ntri + first);
    unsigned v[ISO_ITEMS], f[ISO_ITEMS], vs = 0, fs = 0;
#pragma unroll
    for (int s = 0; s < ISO_ITEMS; ++s) {
        v[s] = vs;
        f[s] = fs;
        vs += __popc((unsigned)(m8 >> (8 * s)) & 0x7Fu);
        fs += (unsigned)(t8 >> (8 * s)) & 0xFFu;
    }
    tpg_u64 total;
    const tpg_u64 before = iso_block_scan(((tpg_u64)fs << 32) | vs, lds, total) + sums[blockIdx.x];
    const unsigned vb = (unsigned)before, fb = (unsigned)(before >> 32);
    uint4 *vo = (uint4 *)(voff + first), *fo = (uint4 *)(foff + first);
    vo[0] = make_uint4(vb + v[0], vb + v[1], vb + v[2], vb + v[3]);
    vo[1] = make_uint4(vb + v[4], vb + v[5], vb + v[6], vb + v[7]);
    fo[0] = make_uint4(fb + f[0], fb + f[1], fb + f[2], fb + f[3]);
    fo[1] = make_uint4(fb + f[4], fb + f[5], fb + f[6], fb + f[7]);
}

// ---- emit -----------------------------------------------------------------------------------------------------------------
// g_a = field[index_a + 1] - field[index_a - 1], indices clamped into the lattice
__device__ __forceinline__ void iso_gradient(const float *__restrict__ field, int i, int j, int k, const IsoDims &dm,
                                             float g[3]) {
    const int ip = min(i + 1, dm.nx - 1), im = max(i - 1, 0);
    const int jp = min(j + 1, dm.ny - 1), jm = max(j - 1, 0);
    const int kp = min(k + 1, dm.nz - 1), km = max(k - 1, 0);
    const int row = (i * dm.ny + j) * dm.nz;
    g[0] = field[(ip * dm.ny + j) * dm.nz + k] - field[(im * dm.ny + j) * dm.nz + k];
    g[1] = field[(i * dm.ny + jp) * dm.nz + k] - field[(i * dm.ny + jm) * dm.nz + k];
    g[2] = field[row + kp] - field[row + km];
}

__global__ __launch_bounds__(ISO_THREADS) void iso_vertices_kernel(
    const float *__restrict__ field, IsoDims dm, IsoOrigin org, float step, float iso,
    const unsigned char *__restrict__ mask, const unsigned *__restrict__ voff, long long V_cap,
    float *__restrict__ vertices, float *__restrict__ normals) {
    const int n = blockIdx.x * ISO_THREADS + threadIdx.x;
    if (n >= dm.G) return;
    const unsigned m = mask[n];
    if (m == 0) return;
    const int k = n % dm.nz, ij = n / dm.nz;
    const int j = ij % dm.ny, i = ij / dm.ny;
    const float fa = field[n];
    const float pa[3] = {org.o[0] + (float)i * step, org.o[1] + (float)j * step, org.o[2] + (float)k * step};
    float ga[3] = {0.0f, 0.0f, 0.0f};
    if (normals) iso_gradient(field, i, j, k, dm, ga);
    long long at = voff[n];
#pragma unroll 1
    for (int d = 0; d < 7; ++d) {
        if (!((m >> d) & 1u)) continue;
        if (at >= V_cap) return;                            // a short buffer is truncated, never overrun
        const int c = iso_nibble(ISO_DIR_CODE, d);
        const int bi = i + (c & 1), bj = j + ((c >> 1) & 1), bk = k + ((c >> 2) & 1);      // in the lattice: the edge exists
        const float fb = field[(bi * dm.ny + bj) * dm.nz + bk];
        const float t = (iso - fa) / (fb - fa);
        const float pb[3] = {org.o[0] + (float)bi * step, org.o[1] + (float)bj * step, org.o[2] + (float)bk * step};
        float *x = vertices + at * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] = pa[a] + t * (pb[a] - pa[a]);
        if (normals) {
            float gb[3], gv[3];
            iso_gradient(field, bi, bj, bk, dm, gb);
#pragma unroll
            for (int a = 0; a < 3; ++a) gv[a] = ga[a] + t * (gb[a] - ga[a]);
            const float len = sqrtf((gv[0] * gv[0] + gv[1] * gv[1]) + gv[2] * gv[2]);
            float *o = normals + at * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) o[a] = len == 0.0f ? 0.0f : -gv[a] / len;
        }
        ++at;
    }
}

// the vertex on the edge between the path positions a and b of tetrahedron p of cell n
__device__ __forceinline__ int iso_edge_vertex(int n, int p, int a, int b, const IsoDims &dm,
                                               const unsigned char *__restrict__ mask,
                                               const unsigned *__restrict__ voff) {
    const int lo = min(a, b), hi = max(a, b);
    const int cl = lo == 0 ? 0 : (lo == 1 ? iso_nibble(ISO_PATH1, p) : iso_nibble(ISO_PATH2, p));
    const int ch = hi == 3 ? 7 : (hi == 2 ? iso_nibble(ISO_PATH2, p) : iso_nibble(ISO_PATH1, p));
    const int d = iso_nibble(ISO_CODE_DIR, ch ^ cl);        // cl is a subset of ch: the owner is the earlier corner
    const int owner = n + iso_offset(cl, dm);
    return (int)(voff[owner] + (unsigned)__popc((unsigned)mask[owner] & ((1u << d) - 1u)));
}

__global__ __launch_bounds__(ISO_THREADS) void iso_faces_kernel(
    const float *__restrict__ field, IsoDims dm, float iso, IsoWinding wind, const unsigned char *__restrict__ mask,
    const unsigned char *__restrict__ ntri, const unsigned *__restrict__ voff, const unsigned *__restrict__ foff,
    long long F_cap, int32_t *__restrict__ faces) {
    const int n = blockIdx.x * ISO_THREADS + threadIdx.x;
    if (n >= dm.G || ntri[n] == 0) return;                  // ntri > 0: the cell exists, all 8 corners are nodes
    unsigned exist;
    const unsigned in = iso_corners(field, n, dm, iso, exist);
    if (exist != 0xFFu) return;                             // (a workspace left by other dimensions: nothing is read astray)
    long long at = foff[n];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const unsigned cs = iso_case(in, p);
        const int count = iso_case_triangles(cs);
        if (count == 0) continue;
        const bool flip = (wind.flip[p] >> cs) & 1u;
        // the edges e0..e3 as pairs of path positions; triangle 0 = (e0, e1, e2), triangle 1 = (e0, e2, e3)
        int a0, b0, a1, b1, a2, b2, a3 = 0, b3 = 0;
        if (count == 2) {
            const unsigned os = ~cs & 0xFu;
            const int A = __ffs(cs) - 1, B = 31 - __clz(cs), Cc = __ffs(os) - 1, Dd = 31 - __clz(os);
            a0 = A, b0 = Cc;                                // ac
            a1 = A, b1 = Dd;                                // ad
            a2 = B, b2 = Dd;                                // bd
            a3 = B, b3 = Cc;                                // bc
        } else {
            const int s = __ffs(__popc(cs) == 1 ? cs : (~cs & 0xFu)) - 1;     // the corner that is alone on its side
            a0 = a1 = a2 = s;
            b0 = s == 0 ? 1 : 0;
            b1 = s <= 1 ? 2 : 1;
            b2 = s <= 2 ? 3 : 2;
        }
        const int v0 = iso_edge_vertex(n, p, a0, b0, dm, mask, voff);
        const int v2 = iso_edge_vertex(n, p, a2, b2, dm, mask, voff);
        {
            if (at >= F_cap) return;                        // a short buffer is truncated, never overrun
            const int v1 = iso_edge_vertex(n, p, a1, b1, dm, mask, voff);
            int32_t *o = faces + at * 3;
            o[0] = v0;
            o[1] = flip ? v2 : v1;
            o[2] = flip ? v1 : v2;
            ++at;
        }
        if (count == 2) {
            if (at >= F_cap) return;
            const int v3 = iso_edge_vertex(n, p, a3, b3, dm, mask, voff);
            int32_t *o = faces + at * 3;
            o[0] = v0;
            o[1] = flip ? v3 : v2;
            o[2] = flip ? v2 : v3;
            ++at;
        }
    }
}

inline bool iso_aligned(const void *p) { return p && ((uintptr_t)p & 255) == 0; }

}  // namespace

extern "C" size_t tpg_iso_workspace_bytes(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    const long long G = (long long)nx * ny * nz;
    if (G > ISO_MAX_NODES) return 0;
    const long long Gp = iso_padded(G), tiles = Gp / ISO_TILE;
    return (size_t)(10 * Gp + 8 * ((tiles + 31) / 32 * 32));
}

extern "C" int tpg_iso_count_f32(const float *field, int nx, int ny, int nz, float iso, void *ws, int64_t *counts,
                                 void *stream) {
    if (nx < 0 || ny < 0 || nz < 0 || !counts || !iso_finite(iso)) return TPG_ERR_ARG;
    const bool cells = nx >= 2 && ny >= 2 && nz >= 2;
    if (cells && !iso_aligned(ws)) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    if (!cells) {                                           // no cells: V = F = 0
        if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st) != hipSuccess) return TPG_ERR_LAUNCH;
        return TPG_OK;
    }
    const long long G = (long long)nx * ny * nz;
    if (G > ISO_MAX_NODES) return TPG_ERR_UNSUPPORTED;
    if (!field) return TPG_ERR_ARG;
    const IsoDims dm{nx, ny, nz, (int)G};
    const IsoWorkspace w = iso_carve(ws, G);
    hipLaunchKernelGGL(iso_classify_kernel, dim3(w.tiles), dim3(ISO_THREADS), 0, st, field, dm, iso, w.mask, w.ntri, w.sums);
    TPG_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(iso_scan_sums_kernel, dim3(1), dim3(ISO_THREADS), 0, st, w.sums, w.tiles, counts);
    TPG_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(iso_offsets_kernel, dim3(w.tiles), dim3(ISO_THREADS), 0, st, w.mask, w.ntri, w.sums, w.voff, w.foff);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_iso_emit_f32(const float *field, int nx, int ny, int nz, const float *origin, float step, float iso,
                                const void *ws, long long V_cap, long long F_cap, float *vertices, float *normals,
                                int32_t *faces, void *stream) {
    if (nx < 0 || ny < 0 || nz < 0 || V_cap < 0 || F_cap < 0 || !origin) return TPG_ERR_ARG;
    if (!iso_finite(iso) || !iso_finite(step) || !(step > 0.0f)) return TPG_ERR_ARG;
    if (!iso_finite(origin[0]) || !iso_finite(origin[1]) || !iso_finite(origin[2])) return TPG_ERR_ARG;
    if ((V_cap > 0 && !vertices) || (F_cap > 0 && !faces)) return TPG_ERR_ARG;
    const bool cells = nx >= 2 && ny >= 2 && nz >= 2;
    if (cells && !iso_aligned(ws)) return TPG_ERR_ARG;
    if (!cells) return TPG_OK;
    const long long G = (long long)nx * ny * nz;
    if (G > ISO_MAX_NODES) return TPG_ERR_UNSUPPORTED;
    if (!field) return TPG_ERR_ARG;
    if (V_cap == 0 && F_cap == 0) return TPG_OK;
    hipStream_t st = tpg_stream(stream);
    const IsoDims dm{nx, ny, nz, (int)G};
    const IsoWorkspace w = iso_carve(const_cast<void *>(ws), G);
    const IsoOrigin org{{origin[0], origin[1], origin[2]}};
    const unsigned blocks = (unsigned)((G + ISO_THREADS - 1) / ISO_THREADS);
    if (V_cap > 0) {
        hipLaunchKernelGGL(iso_vertices_kernel, dim3(blocks), dim3(ISO_THREADS), 0, st, field, dm, org, step, iso, w.mask,
                           w.voff, V_cap, vertices, normals);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    if (F_cap > 0) {
        hipLaunchKernelGGL(iso_faces_kernel, dim3(blocks), dim3(ISO_THREADS), 0, st, field, dm, iso, iso_winding(), w.mask,
                           w.ntri, w.voff, w.foff, F_cap, faces);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}
