// Device pieces shared by the convolution kernels (gfx950): register vector types, the buffer descriptor, the XCD block order and
// the chunk helpers of the rolling-window kernels.  The per-element expressions are bn_expr.h (through common.h).
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(2))) short s16x2_t;
typedef __attribute__((ext_vector_type(2))) unsigned short u16x2_t;
typedef __attribute__((address_space(3))) bf16x4_t* lds_bf16x4_ptr;
typedef __attribute__((address_space(3))) unsigned char* lds_u8_ptr;

// blocks b, b+8, ... share an XCD (round-robin dispatch): give each XCD a contiguous range of
// logical tiles so neighbours (same pixels, different channel tile) hit one L2.  Bijective for any G.
__device__ __forceinline__ int xcd_remap(int b, int G) {
    const int q = G >> 3, r = G & 7, x = b & 7, j = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
}

// buffer descriptor over [base, base + bytes): raw buffer (stride 0), loads beyond `bytes` return zeros, stores beyond it are
// dropped.  RSRC_WORD3 is the descriptor's last dword (gfx950 raw-buffer data format)
constexpr int RSRC_WORD3 = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, RSRC_WORD3);
}

// 8 bf16 of a 16-byte chunk (u32x4_t or uint4) -> fp32
template <class V>
__device__ __forceinline__ void unpack8(const V& v, float (&f)[8]) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}

// 8 per-channel constants from an LDS table, re-read at every use: the index is laundered through an empty asm so that the
// loop-invariant loads are not hoisted back into (40-56) registers
__device__ __forceinline__ void lds_const8(const float* table, int idx, float (&v)[8]) {
    asm volatile("" : "+v"(idx));
    const float4 a = *reinterpret_cast<const float4*>(table + idx);
    const float4 b = *reinterpret_cast<const float4*>(table + idx + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// ReLU of two packed bf16 values: a negative bf16 is a negative int16 (v_pk_max_i16; -0 -> +0)
__device__ __forceinline__ unsigned relu_pk2bf(unsigned pk) {
    const s16x2_t z = {0, 0};
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2_t, pk), z));
}

}  // namespace
