// The fluid's surface on the device: screen-space fluid rendering of a ragged batch of clouds, many frames per call.
// (The reference writes .bgeo files at the end of its demo notebooks so that an external tool reconstructs and shades the
// surface; nothing of that kind runs on a display-less GPU node.  The LOOK is this project's own.)
//
// Every particle is a sphere of `rad` world units; per pixel the nearest sphere front is kept; that depth image is
// smoothed without crossing silhouettes; normals are taken from it and it is shaded.  include/tpgan_ops.h has the rule in
// full ("fluid surface pictures"); all of it is fp32 with every operation rounded on its own, and the camera table, the
// projection and the 64-bit key are the point renderer's (render_common.hpp).
//
// Three entries, so that the host can repeat the middle one:
//   tpg_render_spheres_f32   fill (hipMemsetAsync) + spheres + resolve
//       spheres: one lane per point projects and culls it.  The discs are then drawn by the WAVE, one kept point after
//       the other (a ballot of the kept lanes, the point's figures broadcast with v_readlane): the 64 lanes lie over
//       the disc's bounding box as lw x 64/lw pixels, lw = the box's width rounded up to a power of two, at most 64, and
//       step through the box.  A fluid's discs of 2-8 pixels radius take one to five steps; the rare 129 x 129 box of a
//       disc at the 64-pixel cap takes 3 x 129 steps of a whole wave, not 16 641 of one lane with 63 waiting.  The
//       atomics of a step go to neighbouring pixels of a few rows.  A lane first READS the pixel's key and skips the
//       atomic when the key there is already smaller, as the splat does.  Which lane draws which pixel changes nothing:
//       the buffer ends as the minimum over the same set of keys.
//       resolve: one lane per pixel, key -> depth (+inf: background) and winner (-1).
//   tpg_surface_smooth_f32   one lane per pixel, 32 x 8 tiles; the tile and its halo of k pixels are loaded into LDS
//       once, row by row (coalesced); what lies outside the picture is loaded as +inf, which the depth test leaves out
//       like background.  One instantiation per half-width: the (2k+1)^2 window is unrolled, the binomial weights are
//       immediates, the summation order is the stated one.  Rows of 32 + 2k floats: the two half-waves read two
//       different rows of 32 consecutive floats, no bank conflict.
//   tpg_surface_shade_f32    the same tiling with a halo of 1; normals from one-sided differences of the view-space
//       points, Blinn-Phong plus a Fresnel rim, the colour from the look-up table.
// The second half of the technique makes the fluid translucent ("fluid thickness and absorption" in the header):
//   tpg_render_thickness_f32 fill (zeros) + thickness + resolve
//       thickness: the spheres launch again -- the per-point setup (sf_disc) and the wave-draws-the-disc loop
//       (sf_draw_discs) are the same functions -- but a covered pixel adds the length of the ray's chord through the
//       sphere, clipped at the near plane and at the opaque scene's depth, as an integer of 2^-24 units: one 64-bit
//       atomic add per sphere per covered pixel.  Integer sums: any order, any lane layout, the same bits.
//       resolve: one lane per pixel, the sum as a float.
//   tpg_surface_absorb_u8    one lane per pixel: the shaded fluid over what lies behind it, mixed by a transmittance
//       looked up by thickness (Beer-Lambert; the HOST table travels as a kernel argument and is read from there).
// No scratch, no floating-point atomics; the only atomics are the 64-bit integer min and the 64-bit integer add.
#include "render_common.hpp"

#include <math.h>

namespace {

constexpr int SF_TX = 32, SF_TY = 8;          // the stencil kernels' tile: 256 lanes, one pixel each
constexpr int SF_SHADE = TPG_SURFACE_SHADE_FLOATS;

struct ShadeTable {
    float v[SF_SHADE];
};

__device__ __forceinline__ float sf_lane(float x, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

__device__ __forceinline__ bool sf_finite(float x) { return fabsf(x) < INFINITY; }          // false for NaN

// What one lane knows of its point after entry (a)'s per-point rule: the projection, rp with its cap, the drop test and
// the candidate box.  Both disc passes (sphere fronts, thickness) take it from here, so they cannot drift apart.
struct SfDisc {
    float u, v, t, rp;
    int x0, x1, y0, y1;
    bool keep;
};

__device__ __forceinline__ SfDisc sf_disc(const float *__restrict__ points, const int64_t *__restrict__ lengths,
                                          const float *cam, int f, int i, int N, int W, int H, float rad) {
    SfDisc d{0.0f, 0.0f, 0.0f, 1.0f, 0, -1, 0, -1, false};
    int n = N;
    if (lengths) {
        const long long l = lengths[f];
        n = l < 0 ? 0 : (l < N ? (int)l : N);
    }
    if (i < n) {                                    // no early return: the whole wave draws the discs
        float zv;
        rd_project(points + ((size_t)f * N + i) * 3, cam, d.u, d.v, zv, d.t);
        d.rp = cam[17] != 0.0f ? (rad / zv) * cam[12] : rad * cam[12];
        d.rp = fminf(d.rp, (float)TPG_SURFACE_MAX_RADIUS);
        // every comparison is false for a NaN operand: only a point for which ALL hold goes on
        d.keep = d.t >= 0.0f && zv <= cam[16] && d.rp > 0.0f && d.u >= -d.rp && d.u < (float)W + d.rp && d.v >= -d.rp &&
                 d.v < (float)H + d.rp;
        if (d.keep) {                               // u - rp >= -128, u + rp < W + 128: the conversions are safe
            d.x0 = max((int)floorf(d.u - d.rp), 0), d.x1 = min((int)floorf(d.u + d.rp), W - 1);
            d.y0 = max((int)floorf(d.v - d.rp), 0), d.y1 = min((int)floorf(d.v + d.rp), H - 1);
        }
    }
    return d;
}

// The wave draws the discs of its kept lanes one after the other; pixel(x, y, s, t, index) is called by one lane for
// every covered pixel (s < 1) of the disc of point `index`, whose depth is t.
template <class Pixel> __device__ __forceinline__ void sf_draw_discs(const SfDisc &d, int i, int lane, Pixel pixel) {
    for (tpg_u64 todo = __ballot(d.keep); todo != 0; todo &= todo - 1) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const float su = sf_lane(d.u, src), sv = sf_lane(d.v, src), st = sf_lane(d.t, src), srp = sf_lane(d.rp, src);
        const int bx0 = __builtin_amdgcn_readlane(d.x0, src), bx1 = __builtin_amdgcn_readlane(d.x1, src);
        const int by0 = __builtin_amdgcn_readlane(d.y0, src), by1 = __builtin_amdgcn_readlane(d.y1, src);
        const int bw = bx1 - bx0 + 1;
        if (bw < 1 || by1 < by0) continue;          // rounding can leave a box just outside the picture
        const int sh = bw <= 1 ? 0 : min(32 - __builtin_clz((unsigned)(bw - 1)), 6);
        const int lw = 1 << sh, rows = TPG_WAVE >> sh;
        const unsigned index = (unsigned)(i - lane + src);
        for (int y = by0 + (lane >> sh); y <= by1; y += rows) {
            const float dy = (((float)y + 0.5f) - sv) / srp;
            for (int x = bx0 + (lane & (lw - 1)); x <= bx1; x += lw) {
                const float dx = (((float)x + 0.5f) - su) / srp;
                const float s = dx * dx + dy * dy;
                if (s < 1.0f) pixel(x, y, s, st, index);
            }
        }
    }
}

// frames f0 .. f0 + gridDim.y - 1; per_frame == 0: every frame uses camera 0 of `cams`
__global__ __launch_bounds__(RD_THREADS) void surface_spheres_kernel(
    const float *__restrict__ points, const int64_t *__restrict__ lengths, RenderCams cams, int per_frame, int f0, int N,
    int W, int H, float rad, tpg_u64 *__restrict__ keys) {
    const int f = f0 + blockIdx.y;
    const int i = blockIdx.x * RD_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (TPG_WAVE - 1);
    const SfDisc d = sf_disc(points, lengths, cams.c[per_frame ? blockIdx.y : 0], f, i, N, W, H, rad);
    tpg_u64 *img = keys + (size_t)f * H * W;
    sf_draw_discs(d, i, lane, [&](int x, int y, float s, float t, unsigned index) {
        float tp = t - rad * sqrtf(1.0f - s);
        if (!(tp > 0.0f)) tp = 0.0f;                // the front is clamped at the near plane
        const tpg_u64 key = ((tpg_u64)__float_as_uint(tp) << 32) | index;
        tpg_u64 *k = img + (size_t)y * W + x;
        if (__hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(k, key);
    });
}

// The thickness pass: the same discs, but every covered pixel ADDS its chord, clipped at the near plane and at `limit`,
// in units of 2^-24 and truncated: an integer sum, so neither the order nor the lane layout can change a bit.
__global__ __launch_bounds__(RD_THREADS) void surface_thickness_kernel(
    const float *__restrict__ points, const int64_t *__restrict__ lengths, RenderCams cams, int per_frame, int f0, int N,
    int W, int H, float rad, const float *__restrict__ limit, tpg_u64 *__restrict__ acc) {
    const int f = f0 + blockIdx.y;
    const int i = blockIdx.x * RD_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (TPG_WAVE - 1);
    const SfDisc d = sf_disc(points, lengths, cams.c[per_frame ? blockIdx.y : 0], f, i, N, W, H, rad);
    const size_t frame = (size_t)f * H * W;
    sf_draw_discs(d, i, lane, [&](int x, int y, float s, float t, unsigned) {
        const size_t at = frame + (size_t)y * W + x;
        const float half = rad * sqrtf(1.0f - s);
        const float tp = t - half, tb = t + half;
        const float a = tp > 0.0f ? tp : 0.0f;      // the near-plane clamp of the fronts
        float b = tb;
        if (limit) {
            const float lim = limit[at];
            if (lim < tb) b = lim;                  // false for a NaN: the whole chord
        }
        const float term = b - a;
        if (term > 0.0f) atomicAdd(acc + at, (tpg_u64)(long long)(term * 16777216.0f));     // term <= 2 rad <= 2^11
    });
}

__global__ __launch_bounds__(RD_THREADS) void surface_thickness_resolve_kernel(const tpg_u64 *__restrict__ acc,
                                                                               long long pixels,
                                                                               float *__restrict__ thickness) {
    const long long at = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (at >= pixels) return;
    thickness[at] = (float)acc[at] * 5.9604644775390625e-8f;          // round to nearest even, then 2^-24 exactly
}

struct AbsorbTable {
    float v[256 * 3];
};

// one lane per pixel of all frames
__global__ __launch_bounds__(RD_THREADS) void surface_absorb_kernel(
    const uint8_t *__restrict__ fluid, const float *__restrict__ fdepth, const float *__restrict__ thickness,
    const uint8_t *__restrict__ behind, const float *__restrict__ bdepth, AbsorbTable table, long long pixels, float inv,
    uint8_t *__restrict__ image, float *__restrict__ depth) {
    const long long at = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (at >= pixels) return;
    const float fd = fdepth[at], bd = bdepth[at];
    uint8_t out[3] = {behind[at * 3], behind[at * 3 + 1], behind[at * 3 + 2]};
    float z = bd;
    if (sf_finite(fd) && !(bd < fd)) {              // on equality the fluid is in front
        const float *T = table.v + rd_level(thickness[at], 0.0f, inv) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float val = (float)fluid[at * 3 + ch] * (1.0f - T[ch]) + (float)out[ch] * T[ch];
            out[ch] = !(val > 0.0f) ? 0 : (val >= 255.0f ? 255 : (int)(val + 0.5f));
        }
        z = fd;
    }
    image[at * 3] = out[0];
    image[at * 3 + 1] = out[1];
    image[at * 3 + 2] = out[2];
    depth[at] = z;
}

__global__ __launch_bounds__(RD_THREADS) void surface_resolve_kernel(const tpg_u64 *__restrict__ keys, long long pixels,
                                                                     float *__restrict__ depth,
                                                                     int32_t *__restrict__ winner) {
    const long long at = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (at >= pixels) return;
    const tpg_u64 key = keys[at];
    const bool hit = key != RD_EMPTY;
    depth[at] = hit ? __uint_as_float((unsigned)(key >> 32)) : INFINITY;
    winner[at] = hit ? (int)(unsigned)key : -1;
}

// The tile of frame blockIdx.z at (blockIdx.x, blockIdx.y) with a halo of HALO pixels, +inf outside the picture.
template <int HALO> __device__ __forceinline__ void sf_load_tile(const float *__restrict__ in, int W, int H, float *tile) {
    constexpr int LW = SF_TX + 2 * HALO, LH = SF_TY + 2 * HALO;
    const int gx0 = blockIdx.x * SF_TX - HALO, gy0 = blockIdx.y * SF_TY - HALO;
    for (int e = threadIdx.x; e < LW * LH; e += RD_THREADS) {
        const int ly = e / LW, lx = e - ly * LW;
        const int gx = gx0 + lx, gy = gy0 + ly;
        tile[e] = gx >= 0 && gx < W && gy >= 0 && gy < H ? in[(size_t)gy * W + gx] : INFINITY;
    }
    __syncthreads();
}

// the binomial row of order 2K: 1 2 1, 1 4 6 4 1, ...
template <int K> struct SfBinomial {
    int w[2 * K + 1];
    constexpr SfBinomial() : w{} {
        w[0] = 1;
        for (int j = 1; j <= 2 * K; ++j) w[j] = w[j - 1] * (2 * K - j + 1) / j;
    }
};

template <int K> __global__ __launch_bounds__(RD_THREADS) void surface_smooth_kernel(
    const float *__restrict__ in, float *__restrict__ out, int W, int H, float delta) {
    constexpr int LW = SF_TX + 2 * K;
    constexpr SfBinomial<K> bw;
    __shared__ float tile[LW * (SF_TY + 2 * K)];
    const size_t frame = (size_t)blockIdx.z * H * W;
    sf_load_tile<K>(in + frame, W, H, tile);
    const int lx = threadIdx.x & (SF_TX - 1), ly = threadIdx.x / SF_TX;
    const int x = blockIdx.x * SF_TX + lx, y = blockIdx.y * SF_TY + ly;
    if (x >= W || y >= H) return;
    const float zi = tile[(ly + K) * LW + lx + K];
    float o = zi;
    if (sf_finite(zi)) {
        float acc = 0.0f, ws = 0.0f;
#pragma unroll
        for (int oy = 0; oy <= 2 * K; ++oy)
#pragma unroll
            for (int ox = 0; ox <= 2 * K; ++ox) {
                const float zj = tile[(ly + oy) * LW + lx + ox];
                const float w = (float)(bw.w[oy] * bw.w[ox]);
                if (fabsf(zj - zi) <= delta) {      // false for background, NaN and what lies outside: +-inf or NaN
                    acc = acc + w * zj;
                    ws = ws + w;
                }
            }
        o = acc / ws;                               // the centre always counts: ws >= its weight
    }
    out[frame + (size_t)y * W + x] = o;
}

struct Vec3 {
    float x, y, z;
};

// the view-space point of pixel (x, y) at depth z
__device__ __forceinline__ Vec3 sf_point(int x, int y, float z, const float *cam) {
    const float Zv = z + cam[15];
    const float a = (((float)x + 0.5f) - cam[13]) / cam[12], b = (((float)y + 0.5f) - cam[14]) / cam[12];
    return cam[17] != 0.0f ? Vec3{a * Zv, b * Zv, Zv} : Vec3{a, b, Zv};
}

// forward (P1 - P) or backward (P - P0) difference: the flatter one in z, forward on equality or alone; `none` else
__device__ __forceinline__ Vec3 sf_diff(bool has0, const Vec3 &P0, const Vec3 &P, bool has1, const Vec3 &P1, const Vec3 &none) {
    const Vec3 fw{P1.x - P.x, P1.y - P.y, P1.z - P.z}, bk{P.x - P0.x, P.y - P0.y, P.z - P0.z};
    if (has1 && has0) return fabsf(bk.z) < fabsf(fw.z) ? bk : fw;
    return has1 ? fw : (has0 ? bk : none);
}

// frames f0 .. f0 + gridDim.z - 1; per_frame == 0: every frame uses camera 0 of `cams`
__global__ __launch_bounds__(RD_THREADS) void surface_shade_kernel(
    const float *__restrict__ depth, const int32_t *__restrict__ winner, const float *__restrict__ scalar,
    const uint8_t *__restrict__ lut, const uint8_t *__restrict__ background, RenderCams cams, int per_frame, int f0,
    ShadeTable shade, int N, int W, int H, float lo, float inv, uint8_t *__restrict__ image) {
    constexpr int LW = SF_TX + 2;
    __shared__ float tile[LW * (SF_TY + 2)];
    const int f = f0 + blockIdx.z;
    const size_t frame = (size_t)f * H * W;
    sf_load_tile<1>(depth + frame, W, H, tile);
    const int lx = threadIdx.x & (SF_TX - 1), ly = threadIdx.x / SF_TX;
    const int x = blockIdx.x * SF_TX + lx, y = blockIdx.y * SF_TY + ly;
    if (x >= W || y >= H) return;
    const float *cam = cams.c[per_frame ? blockIdx.z : 0];
    const float *c = tile + (ly + 1) * LW + lx + 1;
    const float z = c[0];
    const size_t at = frame + (size_t)y * W + x;
    uint8_t r = background[0], g = background[1], b = background[2];
    if (sf_finite(z)) {                             // a pixel is surface iff its depth is finite
        const float zl = c[-1], zr = c[1], zu = c[-LW], zd = c[LW];       // +inf beyond the picture's edge
        const Vec3 P = sf_point(x, y, z, cam);
        const float step = cam[17] != 0.0f ? P.z / cam[12] : 1.0f / cam[12];
        const Vec3 ddx = sf_diff(sf_finite(zl), sf_point(x - 1, y, zl, cam), P, sf_finite(zr), sf_point(x + 1, y, zr, cam),
                                 Vec3{step, 0.0f, 0.0f});
        const Vec3 ddy = sf_diff(sf_finite(zu), sf_point(x, y - 1, zu, cam), P, sf_finite(zd), sf_point(x, y + 1, zd, cam),
                                 Vec3{0.0f, step, 0.0f});
        float nx = ddy.y * ddx.z - ddy.z * ddx.y;   // n = cross(ddy, ddx): a plane facing the camera gives (0,0,-1)
        float ny = ddy.z * ddx.x - ddy.x * ddx.z;
        float nz = ddy.x * ddx.y - ddy.y * ddx.x;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        if (len > 0.0f) {
            nx = nx / len, ny = ny / len, nz = nz / len;
        } else {
            nx = 0.0f, ny = 0.0f, nz = -1.0f;
        }
        const float *s = shade.v;
        const float dif = fmaxf(rd_dot(nx, ny, nz, s[0], s[1], s[2]), 0.0f);
        float sp = fmaxf(rd_dot(nx, ny, nz, s[3], s[4], s[5]), 0.0f);
        const int p = (int)s[10];
        for (int j = 0; j < p; ++j) sp = sp * sp;
        const float m = 1.0f - fmaxf(-nz, 0.0f), m2 = m * m, fr = (m2 * m2) * m;
        const float lit = s[6] + s[7] * dif, gloss = 255.0f * (s[8] * sp + s[9] * fr);
        const float value = scalar ? scalar[(size_t)f * N + tpg_clamp_idx(winner[at], N)] : z;
        const uint8_t *base = lut + rd_level(value, lo, inv) * 3;
        const float val[3] = {(float)base[0] * lit + gloss, (float)base[1] * lit + gloss, (float)base[2] * lit + gloss};
        uint8_t out[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[ch] = !(val[ch] > 0.0f) ? 0 : (val[ch] >= 255.0f ? 255 : (int)(val[ch] + 0.5f));
        r = out[0], g = out[1], b = out[2];
    }
    image[at * 3] = r;
    image[at * 3 + 1] = g;
    image[at * 3 + 2] = b;
}

// the picture limits of the point renderer
inline int sf_extents(int F, int W, int H) {
    if (W > TPG_RENDER_MAX_EXTENT || H > TPG_RENDER_MAX_EXTENT || F > 65535) return TPG_ERR_UNSUPPORTED;
    if ((long long)F * H * W > (1ll << 31)) return TPG_ERR_UNSUPPORTED;
    return TPG_OK;
}

inline dim3 sf_tiles(int F, int W, int H) { return dim3((W + SF_TX - 1) / SF_TX, (H + SF_TY - 1) / SF_TY, F); }

}  // namespace

extern "C" int tpg_render_spheres_f32(const float *points, const int64_t *lengths, int F, int N, const float *cams,
                                      int ncam, int W, int H, float rad, void *keys, float *depth, int32_t *winner,
                                      void *stream) {
    if (F < 0 || N < 0 || !depth || !winner) return TPG_ERR_ARG;
    if (W < 1 || H < 1 || !(rad > 0.0f) || !rd_finite(rad)) return TPG_ERR_ARG;
    if (F == 0 || N == 0) return TPG_OK;
    if (!points || !cams || !keys || ((uintptr_t)keys & 7) != 0) return TPG_ERR_ARG;
    if (ncam != 1 && ncam != F) return TPG_ERR_ARG;
    if (!rd_cams_ok(cams, ncam)) return TPG_ERR_ARG;
    if (sf_extents(F, W, H) != TPG_OK) return TPG_ERR_UNSUPPORTED;
    const long long pixels = (long long)F * H * W;
    hipStream_t st = tpg_stream(stream);
    if (hipMemsetAsync(keys, 0xFF, sizeof(tpg_u64) * (size_t)pixels, st) != hipSuccess) return TPG_ERR_LAUNCH;
    const int blocks = (N + RD_THREADS - 1) / RD_THREADS;
    RenderCams rc;
    const int group = ncam == 1 ? F : RD_GROUP;
    for (int f0 = 0; f0 < F; f0 += group) {
        const int nf = F - f0 < group ? F - f0 : group;
        rd_fill_cams(rc, cams, ncam, f0, nf);
        hipLaunchKernelGGL(surface_spheres_kernel, dim3(blocks, nf), dim3(RD_THREADS), 0, st, points, lengths, rc,
                           ncam == 1 ? 0 : 1, f0, N, W, H, rad, (tpg_u64 *)keys);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    hipLaunchKernelGGL(surface_resolve_kernel, dim3((unsigned)((pixels + RD_THREADS - 1) / RD_THREADS)), dim3(RD_THREADS),
                       0, st, (const tpg_u64 *)keys, pixels, depth, winner);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_render_thickness_f32(const float *points, const int64_t *lengths, int F, int N, const float *cams,
                                        int ncam, int W, int H, float rad, const float *limit, void *acc,
                                        float *thickness, void *stream) {
    if (F < 0 || N < 0 || !thickness) return TPG_ERR_ARG;
    if (W < 1 || H < 1 || !(rad > 0.0f) || !(rad <= (float)TPG_THICKNESS_MAX_RAD)) return TPG_ERR_ARG;
    if (F == 0 || N == 0) return TPG_OK;
    if (!points || !cams || !acc || ((uintptr_t)acc & 7) != 0) return TPG_ERR_ARG;
    if (ncam != 1 && ncam != F) return TPG_ERR_ARG;
    if (!rd_cams_ok(cams, ncam)) return TPG_ERR_ARG;
    if (sf_extents(F, W, H) != TPG_OK || N > TPG_THICKNESS_MAX_N) return TPG_ERR_UNSUPPORTED;
    const long long pixels = (long long)F * H * W;
    hipStream_t st = tpg_stream(stream);
    if (hipMemsetAsync(acc, 0, sizeof(tpg_u64) * (size_t)pixels, st) != hipSuccess) return TPG_ERR_LAUNCH;
    const int blocks = (N + RD_THREADS - 1) / RD_THREADS;
    RenderCams rc;
    const int group = ncam == 1 ? F : RD_GROUP;
    for (int f0 = 0; f0 < F; f0 += group) {
        const int nf = F - f0 < group ? F - f0 : group;
        rd_fill_cams(rc, cams, ncam, f0, nf);
        hipLaunchKernelGGL(surface_thickness_kernel, dim3(blocks, nf), dim3(RD_THREADS), 0, st, points, lengths, rc,
                           ncam == 1 ? 0 : 1, f0, N, W, H, rad, limit, (tpg_u64 *)acc);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    hipLaunchKernelGGL(surface_thickness_resolve_kernel, dim3((unsigned)((pixels + RD_THREADS - 1) / RD_THREADS)),
                       dim3(RD_THREADS), 0, st, (const tpg_u64 *)acc, pixels, thickness);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_surface_absorb_u8(const uint8_t *fluid, const float *fdepth, const float *thickness,
                                     const uint8_t *behind, const float *bdepth, int F, int W, int H, float th_max,
                                     const float *table, uint8_t *image, float *depth, void *stream) {
    if (F < 0 || !image || !depth || !table) return TPG_ERR_ARG;
    if (W < 1 || H < 1 || !(th_max > 0.0f) || !rd_finite(th_max)) return TPG_ERR_ARG;
    AbsorbTable tab;
    for (int j = 0; j < 256 * 3; ++j) {             // HOST table, checked before anything is launched
        if (!(table[j] >= 0.0f && table[j] <= 1.0f)) return TPG_ERR_ARG;
        tab.v[j] = table[j];
    }
    if (F == 0) return TPG_OK;
    if (!fluid || !fdepth || !thickness || !behind || !bdepth) return TPG_ERR_ARG;
    const float inv = 255.0f / th_max;
    if (!rd_finite(inv)) return TPG_ERR_ARG;
    if (sf_extents(F, W, H) != TPG_OK) return TPG_ERR_UNSUPPORTED;
    const long long pixels = (long long)F * H * W;
    hipLaunchKernelGGL(surface_absorb_kernel, dim3((unsigned)((pixels + RD_THREADS - 1) / RD_THREADS)), dim3(RD_THREADS), 0,
                       tpg_stream(stream), fluid, fdepth, thickness, behind, bdepth, tab, pixels, inv, image, depth);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_surface_smooth_f32(const float *in, int F, int W, int H, int k, float delta, float *out, void *stream) {
    if (F < 0 || !out || out == in) return TPG_ERR_ARG;
    if (W < 1 || H < 1 || k < 1 || k > TPG_SURFACE_MAX_HALF || !(delta > 0.0f) || !rd_finite(delta)) return TPG_ERR_ARG;
    if (F == 0) return TPG_OK;
    if (!in) return TPG_ERR_ARG;
    if (sf_extents(F, W, H) != TPG_OK) return TPG_ERR_UNSUPPORTED;
    hipStream_t st = tpg_stream(stream);
    const dim3 grid = sf_tiles(F, W, H), block(RD_THREADS);
    switch (k) {
    case 1: hipLaunchKernelGGL(surface_smooth_kernel<1>, grid, block, 0, st, in, out, W, H, delta); break;
    case 2: hipLaunchKernelGGL(surface_smooth_kernel<2>, grid, block, 0, st, in, out, W, H, delta); break;
    case 3: hipLaunchKernelGGL(surface_smooth_kernel<3>, grid, block, 0, st, in, out, W, H, delta); break;
    default: hipLaunchKernelGGL(surface_smooth_kernel<4>, grid, block, 0, st, in, out, W, H, delta); break;
    }
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}

extern "C" int tpg_surface_shade_f32(const float *depth, const int32_t *winner, const float *scalar, int F, int N,
                                     const float *cams, int ncam, int W, int H, float lo, float hi, const uint8_t *lut,
                                     const uint8_t *background, const float *shade, uint8_t *image, void *stream) {
    if (F < 0 || N < 0 || !image || !shade) return TPG_ERR_ARG;
    if (W < 1 || H < 1 || !(hi > lo)) return TPG_ERR_ARG;
    ShadeTable table;
    for (int j = 0; j < SF_SHADE; ++j) {            // HOST table, checked before anything is launched
        if (!rd_finite(shade[j])) return TPG_ERR_ARG;
        table.v[j] = shade[j];
    }
    if (!(shade[10] >= 0.0f && shade[10] <= 8.0f) || shade[10] != (float)(int)shade[10]) return TPG_ERR_ARG;
    if (F == 0 || N == 0) return TPG_OK;
    if (!depth || !winner || !cams || !lut || !background) return TPG_ERR_ARG;
    if (ncam != 1 && ncam != F) return TPG_ERR_ARG;
    if (!rd_cams_ok(cams, ncam)) return TPG_ERR_ARG;
    if (sf_extents(F, W, H) != TPG_OK) return TPG_ERR_UNSUPPORTED;
    const float inv = 255.0f / (hi - lo);
    if (!rd_finite(lo) || !rd_finite(inv)) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    RenderCams rc;
    const int group = ncam == 1 ? F : RD_GROUP;
    for (int f0 = 0; f0 < F; f0 += group) {
        const int nf = F - f0 < group ? F - f0 : group;
        rd_fill_cams(rc, cams, ncam, f0, nf);
        hipLaunchKernelGGL(surface_shade_kernel, sf_tiles(nf, W, H), dim3(RD_THREADS), 0, st, depth, winner, scalar, lut,
                           background, rc, ncam == 1 ? 0 : 1, f0, table, N, W, H, lo, inv, image);
        TPG_RETURN_IF_LAUNCH_FAILED();
    }
    return TPG_OK;
}
