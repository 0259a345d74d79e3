// What the weight-only linear kernels share (wo_gemm.hip for decode steps, wo_tall.hip for more than
// 64 rows): the MFMA wrapper, 16-bit <-> fp32 helpers, the level -> operand conversions of the
// storage order described at the top of wo_gemm.hip, and the epilogue.
#pragma once
#include "common.h"

namespace pra {
namespace wo {

constexpr int kThreads = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <typename T> struct V8;
template <> struct V8<bf16> { typedef __bf16 type __attribute__((ext_vector_type(8))); };
template <> struct V8<f16> { typedef _Float16 type __attribute__((ext_vector_type(8))); };

template <typename T>
__device__ __forceinline__ f32x4 mma(typename V8<T>::type a, typename V8<T>::type b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mma<bf16>(V8<bf16>::type a, V8<bf16>::type b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mma<f16>(V8<f16>::type a, V8<f16>::type b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// two fp32 -> one dword of two T (exact for the integer levels; RNE for the outputs)
template <typename T> __device__ __forceinline__ uint32_t pack2(float a, float b);
template <> __device__ __forceinline__ uint32_t pack2<bf16>(float a, float b) { return pack_bf2(a, b); }
template <> __device__ __forceinline__ uint32_t pack2<f16>(float a, float b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)a) |
         ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)b) << 16);
}
template <typename T> __device__ __forceinline__ float to_f32(uint16_t u);
template <> __device__ __forceinline__ float to_f32<bf16>(uint16_t u) { return bf2f(u); }
template <> __device__ __forceinline__ float to_f32<f16>(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }

__device__ __forceinline__ float ubyte(uint32_t d, int i) { return (float)((d >> (8 * i)) & 0xffu); }

// 8 int8 levels (two dwords, k ascending) -> MFMA operand. The sign flip makes the bytes
// level + 128, which v_cvt_f32_ubyteN converts without a sign extension.
template <typename T> __device__ __forceinline__ typename V8<T>::type cvt_i8(uint32_t d0, uint32_t d1) {
  d0 ^= 0x80808080u;
  d1 ^= 0x80808080u;
  u32x4 r;
  r[0] = pack2<T>(ubyte(d0, 0) - 128.f, ubyte(d0, 1) - 128.f);
  r[1] = pack2<T>(ubyte(d0, 2) - 128.f, ubyte(d0, 3) - 128.f);
  r[2] = pack2<T>(ubyte(d1, 0) - 128.f, ubyte(d1, 1) - 128.f);
  r[3] = pack2<T>(ubyte(d1, 2) - 128.f, ubyte(d1, 3) - 128.f);
  return __builtin_bit_cast(typename V8<T>::type, r);
}
// 8 int4 levels (one dword, nibble i = level + 8 at k + i) -> MFMA operand
template <typename T> __device__ __forceinline__ typename V8<T>::type cvt_i4(uint32_t d) {
  const uint32_t lo = d & 0x0f0f0f0fu, hi = (d >> 4) & 0x0f0f0f0fu;  // nibbles 0,2,4,6 / 1,3,5,7
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = pack2<T>(ubyte(lo, j) - 8.f, ubyte(hi, j) - 8.f);
  return __builtin_bit_cast(typename V8<T>::type, r);
}

__device__ __forceinline__ float act_f(float v, int act) {
  if (act == 1) return gelu_erf_fast(v);
  if (act == 3) return fmaxf(v, 0.f);
  return v;
}

// scale (per channel, when given), bias, activation, and 4 consecutive channels of row m stored
template <typename T>
__device__ __forceinline__ void finish(f32x4 v, const float* __restrict__ chan_scale,
                                       const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int m, int n,
                                       int N, int act) {
  float o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float t = v[r];
    if (chan_scale) t *= chan_scale[n + r];
    if (bias) t += to_f32<T>(bias[n + r]);
    o[r] = act_f(t, act);
  }
  u32x2 p;
  p[0] = pack2<T>(o[0], o[1]);
  p[1] = pack2<T>(o[2], o[3]);
  *reinterpret_cast<u32x2*>(y + (size_t)m * N + n) = p;
}

}  // namespace wo
}  // namespace pra
