// Triangle meshes on the device: a z-buffered rasteriser of a ragged batch of indexed meshes, many frames per call, and
// a deferred shading pass.  (The project makes meshes in three places -- the isosurface of a particle frame, the solids
// of a simulated scene, .obj / .ply files -- and the reference hands all such geometry to an external renderer; nothing
// of that kind runs on a display-less GPU node.  The LOOK is this project's own.)
//
// include/tpgan_ops.h has the rule in full ("mesh pictures").  The camera table, the projection of a vertex and the
// 64-bit key are the point renderer's (render_common.hpp).  Coverage is decided in integers: the projected vertices are
// snapped to 1/256 pixel, the three edge functions of a pixel centre are exact in int64, a centre ON an edge belongs to
// the triangle iff that edge is a left or a horizontal top one.  Depth is interpolated in float64 from those integers,
// each operation rounded on its own: the library is built with -ffp-contract=off, which is what keeps the products and
// sums below apart (no __dadd_rn / __dmul_rn spelling is needed, and none is used).
//
// Two entries:
//   tpg_render_mesh_f32   fill (hipMemsetAsync) + raster + tiles + resolve
//       raster: one lane per face does the setup: three indices, three gathered vertices, projection, cull, snap, signed
//       area, the bounding box of pixel centres clipped to the picture.  The faces then fall into two classes.
//         small  at most MR_SMALL candidate pixels (an isosurface of half a million faces on a 768 x 768 picture, an
//                obstacle meshed at one particle spacing: one to a few pixels each).  The face's own lane walks its box,
//                a loop of at most MR_SMALL steps; 64 faces are in flight per wave and nothing is exchanged.
//         large  every other kept face (a hand-made box: a dozen triangles of hundreds of pixels).  They are drawn by the
//                WAVE, one face after the other, as surface_spheres_kernel draws its discs: a ballot of the lanes that
//                hold one, the face's figures broadcast with v_readlane, the 64 lanes laid over the box as lw x 64/lw
//                pixels, lw = the box's width rounded up to a power of two, at most 64, stepping through the box.
//         huge   a box of more than MR_HUGE pixels (a wall across the picture).  One wave would step through it alone
//                while the chip idles (12 triangles over 0.72 of a 768 x 768 picture: 13.5 ms), so the
//                lane only appends the face's index to the frame's list (an integer atomicAdd on its counter; the list's
//                order changes nothing, the keys' minimum is the same) and a second launch, tiles, draws the list: one
//                workgroup per 32 x 32 tile of the picture takes every listed face, sets it up again and draws the part
//                of its box inside the tile.  A frame's list holds TPG_MESH_LIST faces; one that finds it full is drawn
//                as a large face, which gives the same picture.
//       A covered pixel costs one 64-bit atomicMin -- an ordinary vector-memory atomic; a lane first READS the pixel's
//       key and skips the atomic when the key there is already smaller, as the splat does.  min is associative and
//       commutative and the keys of a frame are distinct, so neither the order in which lanes arrive nor which lane
//       draws which pixel changes the buffer's final contents.
//       resolve: one lane per pixel, key -> depth (+inf: background) and winner (-1).
//   tpg_mesh_shade_f32    one lane per pixel: the winner face is set up again exactly as above, its weights at the pixel
//       centre give the normal (interpolated vertex normals, or the face's own) and the base colour; light, specular
//       term, Fresnel rim and rounding are tpg_surface_shade_f32's.
// No LDS, no scratch, no floating-point atomics, no inline assembly; the only atomic is the 64-bit integer min.
#include "render_common.hpp"

#include <math.h>

namespace {

constexpr int MR_SMALL = TPG_MESH_SMALL;      // a clipped box of at most this many pixels is drawn by the face's own lane
constexpr int MR_HUGE = TPG_MESH_HUGE;        // a clipped box of more pixels goes on the list of the tile launch
constexpr int MR_LIST = TPG_MESH_LIST;        // faces a frame's list holds
constexpr int MR_TILE = 32;                   // the tile launch: 32 x 32 pixels per workgroup
constexpr int MR_SHADE = TPG_SURFACE_SHADE_FLOATS;
constexpr float MR_GUARD = (float)TPG_MESH_GUARD;

struct MeshShadeTable {
    float v[MR_SHADE];
};

// What a kept face is drawn from: the snapped vertices, what its depth interpolates (zv under a pinhole camera, else t),
// |A|, the sign of A and the three ownership bits of its edges.
struct MeshFace {
    int X[3], Y[3];
    float d[3];
    long long area;     // |A| > 0
    int flip;           // A < 0
    int own;            // bit i: the edge OPPOSITE vertex i owns the points on it
};

__device__ __forceinline__ int mr_length(const int64_t *__restrict__ lengths, int m, int n) {
    if (!lengths) return n;
    const long long l = lengths[m];
    return l < 0 ? 0 : (l < n ? (int)l : n);
}

// E(a, b, p) = (bx-ax)*(py-ay) - (by-ay)*(px-ax): every difference is below 2^25 in magnitude, the products below 2^50
__device__ __forceinline__ long long mr_edge(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}

// the edge a -> b, seen with the sign of A applied, owns its points: a left edge or a horizontal top edge (y is down,
// the inside is where E > 0)
__device__ __forceinline__ int mr_owns(int ax, int ay, int bx, int by, int flip) {
    const int dx = flip ? ax - bx : bx - ax, dy = flip ? ay - by : by - ay;
    return dy < 0 || (dy == 0 && dx > 0);
}

// Face j of mesh m under `cam`: false if the rule drops it.  Never addresses memory with an index outside 0..vlen-1.
// view: the three view-space vertices (xv, yv, zv), for the face normal.
__device__ __forceinline__ bool mr_setup(const float *__restrict__ verts, const int32_t *__restrict__ tri, int vlen,
                                         const float *cam, MeshFace &fc, float (*view)[3]) {
    const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
    if ((unsigned)i0 >= (unsigned)vlen || (unsigned)i1 >= (unsigned)vlen || (unsigned)i2 >= (unsigned)vlen) return false;
    const int idx[3] = {i0, i1, i2};
    bool ok = true;
    float u[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *p = verts + (size_t)idx[k] * 3;
        float zv, t;
        rd_project(p, cam, u[k], v[k], zv, t);
        // every comparison is false for a NaN operand: only a vertex for which ALL hold goes on
        ok = ok && t >= 0.0f && zv <= cam[16] && fabsf(u[k]) < MR_GUARD && fabsf(v[k]) < MR_GUARD;
        fc.d[k] = cam[17] != 0.0f ? zv : t;
        if (view) {
            const float qx = p[0] - cam[0], qy = p[1] - cam[1], qz = p[2] - cam[2];
            view[k][0] = rd_dot(qx, qy, qz, cam[3], cam[4], cam[5]);
            view[k][1] = rd_dot(qx, qy, qz, cam[6], cam[7], cam[8]);
            view[k][2] = zv;
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                   // |u| < 32768: the product and the sum are exact, the conversion safe
        fc.X[k] = (int)floorf(u[k] * 256.0f + 0.5f);
        fc.Y[k] = (int)floorf(v[k] * 256.0f + 0.5f);
    }
    const long long A = mr_edge(fc.X[0], fc.Y[0], fc.X[1], fc.Y[1], fc.X[2], fc.Y[2]);
    if (A == 0) return false;
    fc.flip = A < 0;
    fc.area = A < 0 ? -A : A;
    fc.own = mr_owns(fc.X[1], fc.Y[1], fc.X[2], fc.Y[2], fc.flip) | (mr_owns(fc.X[2], fc.Y[2], fc.X[0], fc.Y[0], fc.flip) << 1) |
             (mr_owns(fc.X[0], fc.Y[0], fc.X[1], fc.Y[1], fc.flip) << 2);
    return true;
}

// the three edge functions at the centre of pixel (x, y), in the original vertex order with the sign of A applied
__device__ __forceinline__ void mr_weights(const MeshFace &fc, int x, int y, long long w[3]) {
    const int px = 256 * x + 128, py = 256 * y + 128;
    w[0] = mr_edge(fc.X[1], fc.Y[1], fc.X[2], fc.Y[2], px, py);
    w[1] = mr_edge(fc.X[2], fc.Y[2], fc.X[0], fc.Y[0], px, py);
    w[2] = mr_edge(fc.X[0], fc.Y[0], fc.X[1], fc.Y[1], px, py);
    if (fc.flip) w[0] = -w[0], w[1] = -w[1], w[2] = -w[2];
}

__device__ __forceinline__ bool mr_covered(const MeshFace &fc, const long long w[3]) {
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) in = in && (w[k] > 0 || (w[k] == 0 && ((fc.own >> k) & 1)));
    return in;
}

// float64, every operation rounded on its own (-ffp-contract=off)
__device__ __forceinline__ float mr_depth(const MeshFace &fc, const long long w[3], const float *cam, double l[3]) {
    const double A = (double)fc.area;
    l[0] = (double)w[0] / A, l[1] = (double)w[1] / A, l[2] = (double)w[2] / A;
    float t;
    if (cam[17] != 0.0f) {
        const double Z = 1.0 / ((l[0] / (double)fc.d[0] + l[1] / (double)fc.d[1]) + l[2] / (double)fc.d[2]);
        t = (float)(Z - (double)cam[15]);
    } else {
        t = (float)((l[0] * (double)fc.d[0] + l[1] * (double)fc.d[1]) + l[2] * (double)fc.d[2]);
    }
    return t > 0.0f ? t : 0.0f;                     // clamped at the near plane; a NaN goes there too
}

__device__ __forceinline__ void mr_pixel(const MeshFace &fc, unsigned index, int x, int y, const float *cam,
                                         tpg_u64 *__restrict__ img, int W) {
    long long w[3];
    mr_weights(fc, x, y, w);
    if (!mr_covered(fc, w)) return;
    double l[3];
    const float t = mr_depth(fc, w, cam, l);
    const tpg_u64 key = ((tpg_u64)__float_as_uint(t) << 32) | index;
    tpg_u64 *k = img + (size_t)y * W + x;
    if (__hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(k, key);
}

__device__ __forceinline__ float mr_lane(float x, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

// the pixels whose centres lie in the snapped bounding box, clipped to the picture: x0..x1, y0..y1 (empty: x1 < x0)
__device__ __forceinline__ void mr_box(const MeshFace &fc, int W, int H, int &x0, int &x1, int &y0, int &y1) {
    const int xa = min(fc.X[0], min(fc.X[1], fc.X[2])), xb = max(fc.X[0], max(fc.X[1], fc.X[2]));
    const int ya = min(fc.Y[0], min(fc.Y[1], fc.Y[2])), yb = max(fc.Y[0], max(fc.Y[1], fc.Y[2]));
    x0 = max((xa + 127) >> 8, 0), x1 = min((xb - 128) >> 8, W - 1);        // >> of a negative int: floor
    y0 = max((ya + 127) >> 8, 0), y1 = min((yb - 128) >> 8, H - 1);
}

// frames f0 .. f0 + gridDim.y - 1; per_cam == 0: every frame uses camera 0 of `cams`; per_mesh == 0: mesh 0
__global__ __launch_bounds__(RD_THREADS) void mesh_raster_kernel(
    const float *__restrict__ vertices, const int64_t *__restrict__ vlengths, const int32_t *__restrict__ faces,
    const int64_t *__restrict__ flengths, RenderCams cams, int per_cam, int per_mesh, int f0, int V, int T, int W, int H,
    int nframes, tpg_u64 *__restrict__ keys, int32_t *__restrict__ list) {
    const int f = f0 + blockIdx.y;
    const int m = per_mesh ? f : 0;
    const int j = blockIdx.x * RD_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (TPG_WAVE - 1);
    const int vlen = mr_length(vlengths, m, V), tlen = mr_length(flengths, m, T);
    const float *cam = cams.c[per_cam ? blockIdx.y : 0];
    MeshFace fc = {};
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    bool keep = false;
    if (j < tlen) {                                 // no early return: the whole wave draws the large faces below
        keep = mr_setup(vertices + (size_t)m * V * 3, faces + ((size_t)m * T + j) * 3, vlen, cam, fc, nullptr);
        if (keep) {
            mr_box(fc, W, H, x0, x1, y0, y1);
            keep = x1 >= x0 && y1 >= y0;
        }
    }
    tpg_u64 *img = keys + (size_t)f * H * W;
    const int bw = x1 - x0 + 1;
    const long long count = (long long)bw * (y1 - y0 + 1);
    const bool small = keep && count <= MR_SMALL;
    if (keep && count > MR_HUGE) {                  // counts: list[0 .. nframes-1]; frame f's faces: MR_LIST ints behind
        const int slot = atomicAdd(list + f, 1);
        if (slot < MR_LIST) {
            list[nframes + (size_t)f * MR_LIST + slot] = j;
            keep = false;                           // the tile launch draws it
        }
    }
    if (small) {
        int x = x0, y = y0;
        for (int k = 0; k < MR_SMALL && y <= y1; ++k) {
            mr_pixel(fc, (unsigned)j, x, y, cam, img, W);
            if (++x > x1) x = x0, ++y;
        }
    }
    for (tpg_u64 todo = __ballot(keep && !small); todo != 0; todo &= todo - 1) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        MeshFace s;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s.X[k] = __builtin_amdgcn_readlane(fc.X[k], src);
            s.Y[k] = __builtin_amdgcn_readlane(fc.Y[k], src);
            s.d[k] = mr_lane(fc.d[k], src);
        }
        const long long A = mr_edge(s.X[0], s.Y[0], s.X[1], s.Y[1], s.X[2], s.Y[2]);       // uniform: on the scalar unit
        s.flip = A < 0;
        s.area = A < 0 ? -A : A;
        s.own = __builtin_amdgcn_readlane(fc.own, src);
        const int bx0 = __builtin_amdgcn_readlane(x0, src), bx1 = __builtin_amdgcn_readlane(x1, src);
        const int by0 = __builtin_amdgcn_readlane(y0, src), by1 = __builtin_amdgcn_readlane(y1, src);
        const int sbw = bx1 - bx0 + 1;
        const int sh = sbw <= 1 ? 0 : min(32 - __builtin_clz((unsigned)(sbw - 1)), 6);
        const int lw = 1 << sh, rows = TPG_WAVE >> sh;
        const unsigned index = (unsigned)(j - lane + src);
        for (int y = by0 + (lane >> sh); y <= by1; y += rows)
            for (int x = bx0 + (lane & (lw - 1)); x <= bx1; x += lw) mr_pixel(s, index, x, y, cam, img, W);
    }
}

// frames f0 .. f0 + gridDim.y - 1; blockIdx.x: the tile.  Every lane sets every listed face up again (uniform work).
__global__ __launch_bounds__(RD_THREADS) void mesh_tiles_kernel(
    const float *__restrict__ vertices, const int64_t *__restrict__ vlengths, const int32_t *__restrict__ faces,
    const int64_t *__restrict__ flengths, RenderCams cams, int per_cam, int per_mesh, int f0, int V, int T, int W, int H,
    int nframes, tpg_u64 *__restrict__ keys, const int32_t *__restrict__ list) {
    const int f = f0 + blockIdx.y;
    const int n = min(list[f], MR_LIST);
    if (n <= 0) return;
    const int m = per_mesh ? f : 0;
    const int tiles_x = (W + MR_TILE - 1) / MR_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int vlen = mr_length(vlengths, m, V), tlen = mr_length(flengths, m, T);
    const float *cam = cams.c[per_cam ? blockIdx.y : 0];
    tpg_u64 *img = keys + (size_t)f * H * W;
    const int lx = threadIdx.x & (MR_TILE - 1), ly = threadIdx.x / MR_TILE;          // 32 x 8 lanes, four steps down
    for (int e = 0; e < n; ++e) {
        const int j = list[nframes + (size_t)f * MR_LIST + e];
        if (j < 0 || j >= tlen) continue;           // what the raster launch wrote is always inside
        MeshFace fc = {};
        if (!mr_setup(vertices + (size_t)m * V * 3, faces + ((size_t)m * T + j) * 3, vlen, cam, fc, nullptr)) continue;
        int x0, x1, y0, y1;
        mr_box(fc, W, H, x0, x1, y0, y1);
        x0 = max(x0, tx * MR_TILE), x1 = min(x1, tx * MR_TILE + MR_TILE - 1);
        y0 = max(y0, ty * MR_TILE), y1 = min(y1, ty * MR_TILE + MR_TILE - 1);
        const int x = tx * MR_TILE + lx;
        if (x < x0 || x > x1) continue;
        for (int y = ty * MR_TILE + ly; y <= y1; y += RD_THREADS / MR_TILE)
            if (y >= y0) mr_pixel(fc, (unsigned)j, x, y, cam, img, W);
    }
}

__global__ __launch_bounds__(RD_THREADS) void mesh_resolve_kernel(const tpg_u64 *__restrict__ keys, long long pixels,
                                                                  float *__restrict__ depth, int32_t *__restrict__ winner) {
    const long long at = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (at >= pixels) return;
    const tpg_u64 key = keys[at];
    const bool hit = key != RD_EMPTY;
    depth[at] = hit ? __uint_as_float((unsigned)(key >> 32)) : INFINITY;
    winner[at] = hit ? (int)(unsigned)key : -1;
}

__device__ __forceinline__ float mr_mix(const double l[3], float a, float b, float c) {
    return (float)((l[0] * (double)a + l[1] * (double)b) + l[2] * (double)c);
}

// frames f0 .. f0 + gridDim.y - 1
__global__ __launch_bounds__(RD_THREADS) void mesh_shade_kernel(
    const float *__restrict__ depth, const int32_t *__restrict__ winner, const float *__restrict__ vertices,
    const int64_t *__restrict__ vlengths, const int32_t *__restrict__ faces, const int64_t *__restrict__ flengths,
    const float *__restrict__ normals, const float *__restrict__ scalar, const uint8_t *__restrict__ lut,
    const uint8_t *__restrict__ base, const uint8_t *__restrict__ background, RenderCams cams, int per_cam, int per_mesh,
    int f0, MeshShadeTable shade, int V, int T, int W, int H, float lo, float inv, uint8_t *__restrict__ image) {
    const int f = f0 + blockIdx.y;
    const int m = per_mesh ? f : 0;
    const int e = blockIdx.x * RD_THREADS + threadIdx.x;
    if (e >= H * W) return;
    const int y = e / W, x = e - y * W;
    const size_t at = (size_t)f * H * W + e;
    const float *cam = cams.c[per_cam ? blockIdx.y : 0];
    const int vlen = mr_length(vlengths, m, V), tlen = mr_length(flengths, m, T);
    uint8_t r = background[0], g = background[1], b = background[2];
    const int j = winner[at];
    MeshFace fc = {};
    float view[3][3];
    const int32_t *tri = faces + ((size_t)m * T + (j >= 0 && j < tlen ? j : 0)) * 3;
    if (j >= 0 && j < tlen && mr_setup(vertices + (size_t)m * V * 3, tri, vlen, cam, fc, view)) {
        long long w[3];
        double l[3];
        mr_weights(fc, x, y, w);
        (void)mr_depth(fc, w, cam, l);
        float nx, ny, nz;
        if (normals) {
            const float *n0 = normals + ((size_t)m * V + tri[0]) * 3, *n1 = normals + ((size_t)m * V + tri[1]) * 3,
                        *n2 = normals + ((size_t)m * V + tri[2]) * 3;
            const float wx = mr_mix(l, n0[0], n1[0], n2[0]), wy = mr_mix(l, n0[1], n1[1], n2[1]),
                        wz = mr_mix(l, n0[2], n1[2], n2[2]);
            nx = rd_dot(wx, wy, wz, cam[3], cam[4], cam[5]);
            ny = rd_dot(wx, wy, wz, cam[6], cam[7], cam[8]);
            nz = rd_dot(wx, wy, wz, cam[9], cam[10], cam[11]);
        } else {
            const float ax = view[1][0] - view[0][0], ay = view[1][1] - view[0][1], az = view[1][2] - view[0][2];
            const float bx = view[2][0] - view[0][0], by = view[2][1] - view[0][1], bz = view[2][2] - view[0][2];
            nx = ay * bz - az * by;
            ny = az * bx - ax * bz;
            nz = ax * by - ay * bx;
        }
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        if (len > 0.0f) {
            nx = nx / len, ny = ny / len, nz = nz / len;
        } else {
            nx = 0.0f, ny = 0.0f, nz = -1.0f;
        }
        if (nz > 0.0f) nx = -nx, ny = -ny, nz = -nz;          // both sides are lit
        const float *s = shade.v;
        const float dif = fmaxf(rd_dot(nx, ny, nz, s[0], s[1], s[2]), 0.0f);
        float sp = fmaxf(rd_dot(nx, ny, nz, s[3], s[4], s[5]), 0.0f);
        const int p = (int)s[10];
        for (int q = 0; q < p; ++q) sp = sp * sp;
        const float mm = 1.0f - fmaxf(-nz, 0.0f), m2 = mm * mm, fr = (m2 * m2) * mm;
        const float lit = s[6] + s[7] * dif, gloss = 255.0f * (s[8] * sp + s[9] * fr);
        const uint8_t *col = base;
        if (!col) {
            float value = depth[at];
            if (scalar) {
                const float *sc = scalar + (size_t)m * V;
                value = mr_mix(l, sc[tri[0]], sc[tri[1]], sc[tri[2]]);
            }
            col = lut + rd_level(value, lo, inv) * 3;
        }
        const float val[3] = {(float)col[0] * lit + gloss, (float)col[1] * lit + gloss, (float)col[2] * lit + gloss};
        uint8_t out[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[ch] = !(val[ch] > 0.0f) ? 0 : (val[ch] >= 255.0f ? 255 : (int)(val[ch] + 0.5f));
        r = out[0], g = out[1], b = out[2];
    }
    image[at * 3] = r;
    image[at * 3 + 1] = g;
    image[at * 3 + 2] = b;
}

// what both entries ask of their common arguments, after the outputs and before anything is launched
inline int mr_check(const float *vertices, const int32_t *faces, int M, int V, int T, int F, const float *cams, int ncam,
                    int W, int H) {
    if (!vertices || !faces || !cams) return TPG_ERR_ARG;
    if (M != 1 && M != F) return TPG_ERR_ARG;
    if (ncam != 1 && ncam != F) return TPG_ERR_ARG;
    if (!rd_cams_ok(cams, ncam)) return TPG_ERR_ARG;
    if (W > TPG_RENDER_MAX_EXTENT || H > TPG_RENDER_MAX_EXTENT || F > 65535) return TPG_ERR_UNSUPPORTED;
    if ((long long)F * H * W > (1ll << 31)) return TPG_ERR_UNSUPPORTED;
    if (T > TPG_MESH_MAX_ROWS || V > TPG_MESH_MAX_ROWS) return TPG_ERR_UNSUPPORTED;
    return TPG_OK;
}

}  // namespace

extern "C" int tpg_render_mesh_f32(const float *vertices, const int64_t *vlengths, const int32_t *faces,
                                   const int64_t *flengths, int M, int V, int T, int F, const float *cams, int ncam, int W,
                                   int H, void *keys, int32_t *list, float *depth, int32_t *winner, void *stream) {
    if (F < 0 || M < 0 || V < 0 || T < 0 || !depth || !winner) return TPG_ERR_ARG;
    if (W < 1 || H < 1) return TPG_ERR_ARG;
    if (F == 0 || T == 0 || V == 0) return TPG_OK;
    if (!keys || ((uintptr_t)keys & 7) != 0 || !list) return TPG_ERR_ARG;
    const int rc_args = mr_check(vertices, faces, M, V, T, F, cams, ncam, W, H);
    if (rc_args != TPG_OK) return rc_args;
    const long long pixels = (long long)F * H * W;
    hipStream_t st = tpg_stream(stream);
    if (hipMemsetAsync(keys, 0xFF, sizeof(tpg_u64) * (size_t)pixels, st) != hipSuccess) return TPG_ERR_LAUNCH;
    if (hipMemsetAsync(list, 0, sizeof(int32_t) * (size_t)F, st) != hipSuccess) return TPG_ERR_LAUNCH;     // the counters
    const int blocks = (T + RD_THREADS - 1) / RD_THREADS;
    const int tiles = ((W + MR_TILE - 1) / MR_TILE) * ((H + MR_TILE - 1) / MR_TILE);
    RenderCams rc;
    const int group = ncam == 1 ? F : RD_GROUP;
    for (int f0 = 0; f0 < F; f0 += group) {
        const int nf = F - f0 < group ? F - f0 : group;
        rd_fill_cams(rc, cams, ncam, f0, nf);
        hipLaunchKernelGGL(mesh_raster_kernel, dim3(blocks, nf), dim3(RD_THREADS), 0, st, vertices, vlengths, faces,
                           flengths, rc, ncam == 1 ? 0 : 1, M == 1 ? 0 : 1, f0, V, T, W, H, F, (tpg_u64 *)keys, list);
        TPG_RETURN_IF_LAUNCH_FAILED();
        hipLaunchKernelGGL(mesh_tiles_kernel, dim3(tiles, nf), dim3(RD_THREADS), 0, st, vertices, vlengths, faces, flengths,
                           rc, ncam == 1 ? 0 : 1, M == 1 ? 0 : 1, f0, V, T, W, H, F, (tpg_u64 *)keys, (const int32_t *)list);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)((pixels + RD_THREADS - 1) / RD_THREADS)), dim3(RD_THREADS), 0,
                       st, (const tpg_u64 *)keys, pixels, depth, winner);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_mesh_shade_f32(const float *depth, const int32_t *winner, const float *vertices,
                                  const int64_t *vlengths, const int32_t *faces, const int64_t *flengths,
                                  const float *normals, const float *scalar, int M, int V, int T, int F, const float *cams,
                                  int ncam, int W, int H, float lo, float hi, const uint8_t *lut, const uint8_t *base,
                                  const uint8_t *background, const float *shade, uint8_t *image, void *stream) {
    if (F < 0 || M < 0 || V < 0 || T < 0 || !image || !shade) return TPG_ERR_ARG;
    if (W < 1 || H < 1 || !(hi > lo)) return TPG_ERR_ARG;
    MeshShadeTable table;
    for (int j = 0; j < MR_SHADE; ++j) {            // HOST table, checked before anything is launched
        if (!rd_finite(shade[j])) return TPG_ERR_ARG;
        table.v[j] = shade[j];
    }
    if (!(shade[10] >= 0.0f && shade[10] <= 8.0f) || shade[10] != (float)(int)shade[10]) return TPG_ERR_ARG;
    if (F == 0 || T == 0 || V == 0) return TPG_OK;
    if (!depth || !winner || !background || (!base && !lut)) return TPG_ERR_ARG;
    const int rc_args = mr_check(vertices, faces, M, V, T, F, cams, ncam, W, H);
    if (rc_args != TPG_OK) return rc_args;
    const float inv = 255.0f / (hi - lo);
    if (!rd_finite(lo) || !rd_finite(inv)) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    const int blocks = (H * W + RD_THREADS - 1) / RD_THREADS;
    RenderCams rc;
    const int group = ncam == 1 ? F : RD_GROUP;
    for (int f0 = 0; f0 < F; f0 += group) {
        const int nf = F - f0 < group ? F - f0 : group;
        rd_fill_cams(rc, cams, ncam, f0, nf);
        hipLaunchKernelGGL(mesh_shade_kernel, dim3(blocks, nf), dim3(RD_THREADS), 0, st, depth, winner, vertices, vlengths,
                           faces, flengths, normals, scalar, lut, base, background, rc, ncam == 1 ? 0 : 1, M == 1 ? 0 : 1,
                           f0, table, V, T, W, H, lo, inv, image);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}
