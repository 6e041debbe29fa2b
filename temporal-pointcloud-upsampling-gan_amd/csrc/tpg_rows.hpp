// Channels-last rows in registers: the bf16 <-> fp32 conventions and the 8 / 16-byte row chunk every row kernel
// (rowbn, rowgather, rowlinear, mlp_small, mlp_fused) loads, converts and stores with.
//
// ONE definition of "a bf16 is the upper half of the fp32 word; a store rounds to nearest even through
// __float2bfloat16 (NaN stays NaN; the compiler emits v_cvt_pk_bf16_f32)": the forward / backward bit-exactness
// tests compare tensors written by different kernels, so every kernel must round the same way.
#pragma once
#include <hip/hip_bf16.h>

#include <type_traits>

#include "tpg_common.hpp"

typedef float tpg_f32x4 __attribute__((ext_vector_type(4)));          // also one 16x16 MFMA accumulator tile
typedef unsigned int tpg_u32x4 __attribute__((ext_vector_type(4)));

// ---- bf16 primitives: a 32-bit word holds two bf16, the lower-indexed element in the low half ----------------
__device__ __forceinline__ float tpg_bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float tpg_bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ float tpg_bf16_one(const __hip_bfloat16 *p) {
    return __uint_as_float((unsigned)(*reinterpret_cast<const unsigned short *>(p)) << 16);
}
__device__ __forceinline__ unsigned short tpg_bf16_bits(float v) {     // round-to-nearest-even, NaN stays NaN
    const __hip_bfloat16 h = __float2bfloat16(v);
    return *reinterpret_cast<const unsigned short *>(&h);
}
__device__ __forceinline__ unsigned tpg_pack_bf16x2(float lo, float hi) {
    const unsigned short a = tpg_bf16_bits(lo), b = tpg_bf16_bits(hi);
    return (unsigned)a | ((unsigned)b << 16);
}

// one element <-> one float
__device__ __forceinline__ float tpg_load_one(const float *p) { return *p; }
__device__ __forceinline__ float tpg_load_one(const __hip_bfloat16 *p) { return tpg_bf16_one(p); }
__device__ __forceinline__ void tpg_store_one(float *p, float v) { *p = v; }
__device__ __forceinline__ void tpg_store_one(__hip_bfloat16 *p, float v) {
    *reinterpret_cast<unsigned short *>(p) = tpg_bf16_bits(v);
}

// elements per thread and row chunk: 8 as soon as one side is bf16 (16-byte bf16 vectors), else 4
template <typename TA, typename TB = TA> struct tpg_elems {
    static constexpr int NE = (sizeof(TA) == 2 || sizeof(TB) == 2) ? 8 : 4;
};

// ---- a row chunk of NE channels of T, held as raw vector registers until it is used ---------------------------
// load(p) issues the 16-byte (8-byte: bf16, NE = 4) loads, unpack(v) converts later: a software-pipelined walk keeps
// the loads of the next rows in flight while it converts and computes the current ones.
// store / store_stream (non-temporal) and one are static: NE floats -> memory, one element -> one float.
template <typename T, int NE> struct tpg_chunk;
template <int NE> struct tpg_chunk<float, NE> {
    static_assert(NE == 4 || NE == 8, "fp32 chunks are one or two 16-byte vectors");
    float4 r[NE / 4];
    __device__ __forceinline__ void load(const float *p) {
#pragma unroll
        for (int i = 0; i < NE / 4; ++i) r[i] = reinterpret_cast<const float4 *>(p)[i];
    }
    __device__ __forceinline__ void unpack(float (&v)[NE]) const {
#pragma unroll
        for (int i = 0; i < NE / 4; ++i) {
            v[4 * i] = r[i].x; v[4 * i + 1] = r[i].y; v[4 * i + 2] = r[i].z; v[4 * i + 3] = r[i].w;
        }
    }
    static __device__ __forceinline__ void store(float *p, const float (&v)[NE]) {
#pragma unroll
        for (int i = 0; i < NE / 4; ++i)
            reinterpret_cast<float4 *>(p)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    }
    static __device__ __forceinline__ void store_stream(float *p, const float (&v)[NE]) {
#pragma unroll
        for (int i = 0; i < NE / 4; ++i) {
            const tpg_f32x4 w = {v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
            __builtin_nontemporal_store(w, reinterpret_cast<tpg_f32x4 *>(p) + i);
        }
    }
    static __device__ __forceinline__ float one(const float *p) { return tpg_load_one(p); }
};
template <int NE> struct tpg_chunk<__hip_bfloat16, NE> {
    static_assert(NE == 4 || NE == 8, "bf16 chunks are one 8- or 16-byte vector");
    using Raw = typename std::conditional<NE == 8, uint4, uint2>::type;
    Raw r;
    static __device__ __forceinline__ void words(const uint4 &x, unsigned (&w)[4]) { w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w; }
    static __device__ __forceinline__ void words(const uint2 &x, unsigned (&w)[2]) { w[0] = x.x; w[1] = x.y; }
    __device__ __forceinline__ void load(const __hip_bfloat16 *p) { r = *reinterpret_cast<const Raw *>(p); }
    __device__ __forceinline__ void unpack(float (&v)[NE]) const {
        unsigned w[NE / 2];
        words(r, w);
#pragma unroll
        for (int i = 0; i < NE / 2; ++i) {
            v[2 * i] = tpg_bf16_lo(w[i]);
            v[2 * i + 1] = tpg_bf16_hi(w[i]);
        }
    }
    static __device__ __forceinline__ void store(__hip_bfloat16 *p, const float (&v)[NE]) {
        if constexpr (NE == 8) {
            *reinterpret_cast<uint4 *>(p) = make_uint4(tpg_pack_bf16x2(v[0], v[1]), tpg_pack_bf16x2(v[2], v[3]),
                                                       tpg_pack_bf16x2(v[4], v[5]), tpg_pack_bf16x2(v[6], v[7]));
        } else {
            // all four converted before they are paired: in the small-tail kernels the compiler then still emits one
            // v_cvt_pk_bf16_f32 per word (pair by pair it converted singly and merged with shift + or)
            unsigned short b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = tpg_bf16_bits(v[i]);
            *reinterpret_cast<uint2 *>(p) = make_uint2((unsigned)b[0] | ((unsigned)b[1] << 16), (unsigned)b[2] | ((unsigned)b[3] << 16));
        }
    }
    static __device__ __forceinline__ void store_stream(__hip_bfloat16 *p, const float (&v)[NE]) {
        static_assert(NE == 8, "non-temporal stores are 16 bytes");
        const tpg_u32x4 x = {tpg_pack_bf16x2(v[0], v[1]), tpg_pack_bf16x2(v[2], v[3]), tpg_pack_bf16x2(v[4], v[5]),
                             tpg_pack_bf16x2(v[6], v[7])};
        __builtin_nontemporal_store(x, reinterpret_cast<tpg_u32x4 *>(p));
    }
    static __device__ __forceinline__ float one(const __hip_bfloat16 *p) { return tpg_load_one(p); }
};

// load and convert at once / convert and store: NE consecutive channels of T <-> NE floats
template <typename T, int NE> __device__ __forceinline__ void tpg_load_row(const T *p, float (&v)[NE]) {
    tpg_chunk<T, NE> c;
    c.load(p);
    c.unpack(v);
}
template <typename T, int NE> __device__ __forceinline__ void tpg_store_row(T *p, const float (&v)[NE]) {
    tpg_chunk<T, NE>::store(p, v);
}
