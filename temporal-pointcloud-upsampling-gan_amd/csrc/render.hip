// Point-cloud pictures on the device: a z-buffered square splat of a ragged batch of clouds, many frames per call.
// (The reference looks at its results through an Open3D window, train_utils.py:224-238 dump_pointcloud_visualization,
// and hands its demo frames to an external renderer; neither exists on a display-less GPU node.  The LOOK is this
// project's own; no parity with Open3D's picture is claimed.)
//
// The contract (include/tpgan_ops.h has it in full).  Per point p of frame f, all in fp32, every operation rounded on
// its own (no FMA), every dot product in the canonical order (a.x*b.x + a.y*b.y) + a.z*b.z:
//     q = p - eye;  xv = q.r, yv = q.d, zv = q.f            (r, d, f: image-right, image-DOWN, forward)
//     ortho:   u = xv*scale + cx,        v = yv*scale + cy
//     pinhole: u = (xv/zv)*scale + cx,   v = (yv/zv)*scale + cy
//     t = zv - near;  kept iff t >= 0 && zv <= far && u >= -S && u < W+S && v >= -S && v < H+S
// written so that a NaN anywhere fails it, and decided BEFORE any conversion to an integer.  A kept point covers the
// S x S pixels from (floor(u) - S/2, floor(v) - S/2), clipped to the image.  Per pixel the smallest 64-bit key
// (bits(t) << 32) | index wins: a non-negative fp32 orders like its bit pattern, equal depths go to the lower index.
//
// Three launches per group of frames:
//   fill     the (F,H,W) key buffer with all ones (hipMemsetAsync on the stream)
//   splat    one lane per point: project, cull, then one 64-bit atomicMin per covered pixel -- an ordinary
//            vector-memory atomic.  min is associative and commutative and the keys of a frame are distinct, so the
//            buffer's final contents do not depend on the order in which the lanes arrive: the same bits every run, at
//            every batch position.  A lane first READS the pixel's key and skips the atomic when the key there is
//            already smaller: keys only ever decrease, so a value read early can only be larger than the final one
//            and the skip never changes the result; on dense clouds most of the S*S atomics of a hidden point go.
//   resolve  one lane per pixel: key -> winner index (or -1) and the colour from the look-up table
#include "render_common.hpp"

namespace {

// frames f0 .. f0 + gridDim.y - 1; per_frame == 0: every frame uses camera 0 of `cams`
__global__ __launch_bounds__(RD_THREADS) void render_splat_kernel(
    const float *__restrict__ points, const int64_t *__restrict__ lengths, RenderCams cams, int per_frame, int f0, int N,
    int W, int H, int S, tpg_u64 *__restrict__ keys) {
    const int f = f0 + blockIdx.y;
    const int i = blockIdx.x * RD_THREADS + threadIdx.x;
    int n = N;
    if (lengths) {
        const long long l = lengths[f];
        n = l < 0 ? 0 : (l < N ? (int)l : N);
    }
    if (i >= n) return;
    const float *cam = cams.c[per_frame ? blockIdx.y : 0];
    const float *p = points + ((size_t)f * N + i) * 3;
    float u, v, zv, t;
    rd_project(p, cam, u, v, zv, t);
    const float fs = (float)S, far = cam[16];
    // every comparison is false for a NaN operand: only a point for which ALL hold goes on
    if (!(t >= 0.0f && zv <= far && u >= -fs && u < (float)W + fs && v >= -fs && v < (float)H + fs)) return;
    const int px = (int)floorf(u), py = (int)floorf(v);        // in [-S, W+S) x [-S, H+S): the conversion is safe
    const int x0 = max(px - S / 2, 0), x1 = min(px - S / 2 + S, W);
    const int y0 = max(py - S / 2, 0), y1 = min(py - S / 2 + S, H);
    const tpg_u64 key = ((tpg_u64)__float_as_uint(t) << 32) | (unsigned)i;
    tpg_u64 *img = keys + (size_t)f * H * W;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            tpg_u64 *k = img + (size_t)y * W + x;
            if (__hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(k, key);
        }
}

__global__ __launch_bounds__(RD_THREADS) void render_resolve_kernel(
    const tpg_u64 *__restrict__ keys, const float *__restrict__ scalar, const uint8_t *__restrict__ lut,
    const uint8_t *__restrict__ background, long long pixels, int HW, int N, float lo, float inv,
    uint8_t *__restrict__ image, int32_t *__restrict__ winner) {
    const long long at = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (at >= pixels) return;
    const tpg_u64 key = keys[at];
    uint8_t r = background[0], g = background[1], b = background[2];
    int win = -1;
    if (key != RD_EMPTY) {
        win = (int)(unsigned)key;
        const float s = scalar ? scalar[(at / HW) * N + win] : __uint_as_float((unsigned)(key >> 32));
        const int level = rd_level(s, lo, inv);
        r = lut[level * 3];
        g = lut[level * 3 + 1];
        b = lut[level * 3 + 2];
    }
    image[at * 3] = r;
    image[at * 3 + 1] = g;
    image[at * 3 + 2] = b;
    winner[at] = win;
}

}  // namespace

extern "C" int tpg_render_points_f32(const float *points, const int64_t *lengths, const float *scalar, int F, int N,
                                     const float *cams, int ncam, int W, int H, int size, float lo, float hi,
                                     const uint8_t *lut, const uint8_t *background, void *keys, uint8_t *image,
                                     int32_t *winner, void *stream) {
    if (F < 0 || N < 0 || !image || !winner) return TPG_ERR_ARG;
    if (size < 1 || size > TPG_RENDER_MAX_SIZE || W < 1 || H < 1 || !(hi > lo)) return TPG_ERR_ARG;
    if (F == 0 || N == 0) return TPG_OK;
    if (!points || !cams || !lut || !background || !keys || ((uintptr_t)keys & 7) != 0) return TPG_ERR_ARG;
    if (ncam != 1 && ncam != F) return TPG_ERR_ARG;
    if (!rd_cams_ok(cams, ncam)) return TPG_ERR_ARG;
    if (W > TPG_RENDER_MAX_EXTENT || H > TPG_RENDER_MAX_EXTENT || F > 65535) return TPG_ERR_UNSUPPORTED;
    const long long pixels = (long long)F * H * W;
    if (pixels > (1ll << 31)) return TPG_ERR_UNSUPPORTED;       // 16 GiB of keys: the caller renders F in chunks
    const float inv = 255.0f / (hi - lo);
    if (!rd_finite(lo) || !rd_finite(inv)) return TPG_ERR_ARG;
    hipStream_t st = tpg_stream(stream);
    if (hipMemsetAsync(keys, 0xFF, sizeof(tpg_u64) * (size_t)pixels, st) != hipSuccess) return TPG_ERR_LAUNCH;
    const int blocks = (N + RD_THREADS - 1) / RD_THREADS;
    RenderCams rc;
    if (ncam == 1) {
        rd_fill_cams(rc, cams, 1, 0, F);
        hipLaunchKernelGGL(render_splat_kernel, dim3(blocks, F), dim3(RD_THREADS), 0, st, points, lengths, rc, 0, 0, N, W,
                           H, size, (tpg_u64 *)keys);
        TPG_RETURN_IF_LAUNCH_FAILED();
    } else {
        for (int f0 = 0; f0 < F; f0 += RD_GROUP) {
            const int nf = F - f0 < RD_GROUP ? F - f0 : RD_GROUP;
            rd_fill_cams(rc, cams, ncam, f0, nf);
            hipLaunchKernelGGL(render_splat_kernel, dim3(blocks, nf), dim3(RD_THREADS), 0, st, points, lengths, rc, 1, f0,
                               N, W, H, size, (tpg_u64 *)keys);
            TPG_RETURN_IF_LAUNCH_FAILED();
        }
    }
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((pixels + RD_THREADS - 1) / RD_THREADS)), dim3(RD_THREADS),
                       0, st, (const tpg_u64 *)keys, scalar, lut, background, pixels, H * W, N, lo, inv, image, winner);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
