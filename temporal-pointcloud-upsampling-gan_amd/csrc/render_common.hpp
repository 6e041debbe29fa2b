// What the picture kernels share (render.hip: the square splat; surface.hip: the fluid surface): the camera table as a
// kernel argument, the projection of a point, the colour level, and the host's camera checks.  The rule is stated in
// include/tpgan_ops.h ("point-cloud pictures"); every operation is fp32 and rounded on its own.
#pragma once
#include "tpg_common.hpp"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_GROUP = 16;          // per-frame cameras travel as kernel arguments, this many frames per launch
constexpr int RD_CAM = TPG_RENDER_CAM_FLOATS;
constexpr tpg_u64 RD_EMPTY = ~0ull;

struct RenderCams {
    float c[RD_GROUP][RD_CAM];
};

__device__ __forceinline__ float rd_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// p -> u, v (pixels), zv (view depth), t = zv - near
__device__ __forceinline__ void rd_project(const float *__restrict__ p, const float *cam, float &u, float &v, float &zv,
                                           float &t) {
    const float qx = p[0] - cam[0], qy = p[1] - cam[1], qz = p[2] - cam[2];
    const float xv = rd_dot(qx, qy, qz, cam[3], cam[4], cam[5]);
    const float yv = rd_dot(qx, qy, qz, cam[6], cam[7], cam[8]);
    zv = rd_dot(qx, qy, qz, cam[9], cam[10], cam[11]);
    const float scale = cam[12], cx = cam[13], cy = cam[14];
    if (cam[17] != 0.0f) {
        u = (xv / zv) * scale + cx;
        v = (yv / zv) * scale + cy;
    } else {
        u = xv * scale + cx;
        v = yv * scale + cy;
    }
    t = zv - cam[15];
}

// c = (s - lo)*inv -> 0..255; NaN: no comparison holds, level 0
__device__ __forceinline__ int rd_level(float s, float lo, float inv) {
    const float c = (s - lo) * inv;
    int level = 0;
    if (c > 0.0f) level = c >= 255.0f ? 255 : (int)(c + 0.5f);
    return level;
}

inline bool rd_finite(float x) { return x - x == 0.0f; }

// HOST table: every camera is checked before anything is launched
inline bool rd_cams_ok(const float *cams, int ncam) {
    for (int c = 0; c < ncam; ++c) {
        const float *cam = cams + (size_t)c * RD_CAM;
        for (int j = 0; j < RD_CAM; ++j)
            if (!rd_finite(cam[j])) return false;
        if (cam[17] != 0.0f && cam[17] != 1.0f) return false;
        if (cam[17] == 1.0f && !(cam[15] > 0.0f)) return false;       // pinhole divides by zv >= near
    }
    return true;
}

// the cameras of frames f0 .. f0 + nf - 1 (ncam == 1: camera 0 in every slot); unused slots repeat the first
inline void rd_fill_cams(RenderCams &rc, const float *cams, int ncam, int f0, int nf) {
    for (int g = 0; g < RD_GROUP; ++g)
        for (int j = 0; j < RD_CAM; ++j) rc.c[g][j] = cams[(ncam == 1 ? 0 : (size_t)(f0 + (g < nf ? g : 0)) * RD_CAM) + j];
}

}  // namespace
