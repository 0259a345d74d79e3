// How a new K/V row becomes a cached row: the rotary rule and the 8-bit quantisation that the
// decode kernels (decode_attn.hip) and the prefill kernels (prefill_attn.hip) share, so that a
// row appended by either reads back the same.
#pragma once
#include "common.h"

namespace pra {

// x[8] (dims d0.. of one head row) rotated against its partner half a chunk away; c / s are
// the lane's 8 cos / sin values, shared by every row the lane rotates
template <typename T>
__device__ __forceinline__ void rotate8(const T* row, int d0, int half, bool left, const float* c, const float* s,
                                        float* x) {
  float p[8];
  load8<T>(row + (left ? d0 + half : d0 - half), p);
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = left ? x[i] * c[i] - p[i] * s[i] : x[i] * c[i] + p[i] * s[i];
}

// 8 values -> 8 stored bytes: level = clamp(round(x * qs)), byte = level + 128. One fp32
// multiply, then the rounding; contraction is off so that the product is rounded before it
// is used, exactly as x * qs is in torch
__device__ __forceinline__ uint2 quant8(const float* x, float qs, int round_type, float qmax, float qmin) {
#pragma clang fp contract(off)
  uint32_t w[2] = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float y = x[i] * qs;
    float r;
    if (round_type == 0) {
      r = rintf(y);
    } else {  // y - trunc(y) is exact
      const float tr = truncf(y);
      r = tr + (fabsf(y - tr) >= 0.5f ? copysignf(1.f, y) : 0.f);
    }
    r = fminf(fmaxf(r, qmin), qmax);
    w[i >> 2] |= (uint32_t)((int)r + 128) << (8 * (i & 3));
  }
  return make_uint2(w[0], w[1]);
}

}  // namespace pra
