// What the routed mixture-of-experts kernels share (moe_ffn.hip for decode steps, moe_tall.hip for
// prefill sizes): limits, activation codes, 16-bit <-> fp32 helpers, the index kernel of the skinny paths
// (moe_ffn.hip, moe_wo.hip) and the combine kernel that ends every path.
#pragma once
#include "common.h"

namespace pra {
namespace moe {

constexpr int kThreads = 256;
constexpr int kMaxExperts = 256, kMaxTopK = 8;
constexpr int kMaxRows = 64;                      // tokens the skinny kernels (moe_ffn.hip, moe_wo.hip) take
constexpr int kGelu = 1, kRelu = 3, kSwiglu = 4;   // ops/fused.py _ACT and _MOE_ACT; 0 = the fp32 store
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <typename T> struct V8;
template <> struct V8<bf16> { typedef __bf16 type __attribute__((ext_vector_type(8))); };
template <> struct V8<f16> { typedef _Float16 type __attribute__((ext_vector_type(8))); };

template <typename T> __device__ __forceinline__ uint32_t pack2(float a, float b);
template <> __device__ __forceinline__ uint32_t pack2<bf16>(float a, float b) { return pack_bf2(a, b); }
template <> __device__ __forceinline__ uint32_t pack2<f16>(float a, float b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)a) |
         ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)b) << 16);
}
template <typename T> __device__ __forceinline__ float to_f32(uint16_t u);
template <> __device__ __forceinline__ float to_f32<bf16>(uint16_t u) { return bf2f(u); }
template <> __device__ __forceinline__ float to_f32<f16>(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }

// 4 consecutive 16-bit values (8-byte aligned) -> fp32
template <typename T> __device__ __forceinline__ f32x4 load4(const uint16_t* p) {
  const u32x2 u = *reinterpret_cast<const u32x2*>(p);
  return f32x4{to_f32<T>((uint16_t)(u[0] & 0xffffu)), to_f32<T>((uint16_t)(u[0] >> 16)),
               to_f32<T>((uint16_t)(u[1] & 0xffffu)), to_f32<T>((uint16_t)(u[1] >> 16))};
}
template <typename T> __device__ __forceinline__ void store4(uint16_t* p, const float* o) {
  u32x2 u;
  u[0] = pack2<T>(o[0], o[1]);
  u[1] = pack2<T>(o[2], o[3]);
  *reinterpret_cast<u32x2*>(p) = u;
}

__device__ __forceinline__ int clamp_id(int id, int E) { return min(max(id, 0), E - 1); }

// ---------------------------------------------------------------------------------------- index
// Counting sort of the P <= MAXP (token, slot) pairs by expert, one workgroup (moe_ffn.hip and moe_wo.hip;
// the steps are described at the top of moe_ffn.hip). A template so that both files can hold it.
template <int MAXP>
__global__ __launch_bounds__(kThreads) void moe_index_kernel(const int* __restrict__ ids, int* __restrict__ off,
                                                             int* __restrict__ sorted, int* __restrict__ pos, int P,
                                                             int E) {
  __shared__ int sid[MAXP];
  __shared__ int cnt[kMaxExperts + 1];
  const int tid = threadIdx.x;
  for (int p = tid; p < P; p += kThreads) sid[p] = clamp_id(ids[p], E);
  __syncthreads();
  if (tid < E) {
    int c = 0;
    for (int p = 0; p < P; ++p) c += sid[p] == tid ? 1 : 0;
    cnt[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int e = 0; e < E; ++e) {
      const int c = cnt[e];
      cnt[e] = run;
      run += c;
    }
    cnt[E] = run;
  }
  __syncthreads();
  for (int i = tid; i <= E; i += kThreads) off[i] = cnt[i];
  if (tid < E) {
    int s = cnt[tid];
    for (int p = 0; p < P; ++p) {
      if (sid[p] == tid) {
        sorted[s] = p;
        pos[p] = s;
        ++s;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- combine
template <typename T>
__global__ __launch_bounds__(kThreads) void moe_combine_kernel(const float* __restrict__ ws,
                                                               const int* __restrict__ pos,
                                                               const int* __restrict__ ids,
                                                               const float* __restrict__ tw,
                                                               const uint16_t* __restrict__ b2,
                                                               uint16_t* __restrict__ out, int D, int E, int k) {
  const int m = blockIdx.x;
  for (int d = threadIdx.x * 4; d < D; d += kThreads * 4) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const int p = m * k + j;
      const float wj = tw[p];
      f32x4 v = *reinterpret_cast<const f32x4*>(ws + (size_t)pos[p] * D + d);
      if (b2) {
        const f32x4 b = load4<T>(b2 + (size_t)clamp_id(ids[p], E) * D + d);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] += b[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = fmaf(wj, v[i], o[i]);
    }
    store4<T>(out + (size_t)m * D + d, o);
  }
}

// the limits every entry shares; the row limit is the entry's own
inline bool limits_ok(int M, int D, int E, int k) {
  return M >= 1 && E >= 1 && E <= kMaxExperts && k >= 1 && k <= kMaxTopK && k <= E && D >= 64 && D % 64 == 0;
}

}  // namespace moe
}  // namespace pra
