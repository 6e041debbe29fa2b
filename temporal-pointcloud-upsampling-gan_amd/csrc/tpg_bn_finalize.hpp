// What the BatchNorm finalize kernels of rowbn.hip and mlp_fused.hip share: the lane-group fp64 reduction of
// per-workgroup partials and the folded per-channel constants.  (The three lines of the running-statistics chain stay
// in the two statistics kernels: as a shared function they changed those kernels' register allocation.)
//
// A finalize launch runs one WAVE per channel (FIN_CH channels per workgroup, grid = ceil(C / FIN_CH)), its lanes
// split into groups, one per segment (SP segments per sweep, a power of two; L = 64 / SP lanes each), so that the
// segments' partials travel side by side and the launch waits for memory once per sweep instead of once per
// segment.  fp64, fixed butterflies, no LDS and no barrier: bitwise reproducible.
//
// The fused tail and the separate-launch route must produce the SAME constants bit for bit; write_ci / write_cb
// are the one place their expressions are spelled out:
//   ci (nseg,4,C) = sc | sh | mu | rs       input side: y = lrelu(sc*x + sh), xhat = (x - mu)*rs
//   cb (nseg,4,C) = a | f*mu | e | f        output side: dx = a*gg - f*(x - mu) + e
#pragma once
#include "tpg_common.hpp"

namespace tpg_bn {

constexpr int FIN_CH = 4;                      // channels (= waves) per workgroup
constexpr int FIN_THREADS = 64 * FIN_CH;
constexpr int FIN_R = 8;                       // requests in flight per lane and quantity

struct Split { int SP, L; };
__device__ __forceinline__ Split split(int nseg) {
    int sp = 1;
    while (sp < nseg && sp < 64) sp <<= 1;
    return {sp, 64 / sp};
}
__device__ __forceinline__ double group_sum(double v, int L) {
    for (int m = L >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);      // fixed butterfly inside the group
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);          // every lane ends with the same bits
    return v;
}
__device__ __forceinline__ double readlane(double v, int l) {            // l wave-uniform
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// The sums of two quantities over the G partials of one segment and channel, in every lane of the segment's group:
// partial g holds them at base[g * 2C] and base[g * 2C + C].  Lane `sub` of the group's L takes partials sub,
// sub + L, ...; live == false (the group has no segment): loads clamped to partial 0, both sums zero.
__device__ __forceinline__ void pair_sums(const float *base, int C, int sub, int L, int G, bool live,
                                          double &s0, double &s1) {
    double a0 = 0.0, a1 = 0.0;
    for (int g0 = 0; g0 < G; g0 += L * FIN_R) {
        float v0[FIN_R], v1[FIN_R];
#pragma unroll
        for (int i = 0; i < FIN_R; ++i) {      // unconditional, clamped: all requests of a block in flight
            const int g = g0 + sub + i * L;
            const bool ok = live && g < G;
            const float *pg = base + (size_t)(ok ? g : 0) * 2 * C;
            const float x0 = pg[0], x1 = pg[C];
            v0[i] = ok ? x0 : 0.0f;
            v1[i] = ok ? x1 : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < FIN_R; ++i) {
            a0 += (double)v0[i];
            a1 += (double)v1[i];
        }
    }
    s0 = group_sum(a0, L);
    s1 = group_sum(a1, L);
}

// o = the constants' slot of one segment and channel (stride C between the four)
__device__ __forceinline__ void write_ci(float *o, int C, float a, float beta, float mu, float rs) {
    o[0] = a; o[C] = beta - mu * a; o[2 * C] = mu; o[3 * C] = rs;
}
// a = gamma * rs; c1 = sum gg / P, c2 = sum gg*xhat / P of the same BatchNorm's backward
__device__ __forceinline__ void write_cb(float *o, int C, float a, float mu, float rs, float c1, float c2) {
    const float f = a * rs * c2;
    o[0] = a; o[C] = f * mu; o[2 * C] = -a * c1; o[3 * C] = f;
}

}  // namespace tpg_bn
