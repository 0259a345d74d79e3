// MFMA operand fragments over swizzled LDS tile images: what the attention kernels share
// (flash_attn.hip, prefill_attn.hip). v_mfma_f32_32x32x16_{bf16,f16}; a lane is (r = lane & 31,
// h = lane >> 5); an A / B fragment is 8 consecutive k elements of row / column r at k offset 8h,
// and accumulator register i of the lane is row acc_row(i, h) of column r.
#pragma once
#include "common.h"

namespace pra {
namespace fa {

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <typename T> struct V8;
template <> struct V8<bf16> { typedef __bf16 type __attribute__((ext_vector_type(8))); };
template <> struct V8<f16> { typedef _Float16 type __attribute__((ext_vector_type(8))); };

template <typename T>
__device__ __forceinline__ f32x16 mfma(typename V8<T>::type a, typename V8<T>::type b, f32x16 c);
template <>
__device__ __forceinline__ f32x16 mfma<bf16>(V8<bf16>::type a, V8<bf16>::type b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x16 mfma<f16>(V8<f16>::type a, V8<f16>::type b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

template <typename T> __device__ __forceinline__ uint32_t pack2(float a, float b);
template <> __device__ __forceinline__ uint32_t pack2<bf16>(float a, float b) { return pack_bf2(a, b); }
template <> __device__ __forceinline__ uint32_t pack2<f16>(float a, float b) {
  _Float16 x = (_Float16)a, y = (_Float16)b;
  return (uint32_t)__builtin_bit_cast(uint16_t, x) | ((uint32_t)__builtin_bit_cast(uint16_t, y) << 16);
}
template <typename T> __device__ __forceinline__ float lo16(uint32_t w);
template <typename T> __device__ __forceinline__ float hi16(uint32_t w);
template <> __device__ __forceinline__ float lo16<bf16>(uint32_t w) { return __uint_as_float(w << 16); }
template <> __device__ __forceinline__ float hi16<bf16>(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
template <> __device__ __forceinline__ float lo16<f16>(uint32_t w) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffff));
}
template <> __device__ __forceinline__ float hi16<f16>(uint32_t w) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
}

template <typename T>
__device__ __forceinline__ typename V8<T>::type as_v8(u32x4 u) {
  return __builtin_bit_cast(typename V8<T>::type, u);
}
// 8 accumulator registers (floats) -> one MFMA operand fragment
template <typename T>
__device__ __forceinline__ typename V8<T>::type pack_frag(const f32x16& acc, int base) {
  u32x4 u;
  u[0] = pack2<T>(acc[base + 0], acc[base + 1]);
  u[1] = pack2<T>(acc[base + 2], acc[base + 3]);
  u[2] = pack2<T>(acc[base + 4], acc[base + 5]);
  u[3] = pack2<T>(acc[base + 6], acc[base + 7]);
  return as_v8<T>(u);
}

constexpr int kTile = 64;        // rows per staged tile (keys in fwd/dQ, queries in dK/dV)

// Swizzled tile image [64][D] (no padding), element offset of 16-B chunk ch of row `row`:
// 8-row x 32-column subtiles of 512 B, chunk (ch&3) XOR-ed with (row>>2)&3. One image serves
// row fragments (ds_read_b128) and transposed fragments (ds_read_b64_tr_b16) bank-conflict
// free, and the reads of one fragment set differ by immediates from 2 base registers.
template <int D>
__device__ __forceinline__ int swz(int row, int ch) {
  return (row >> 3) * (8 * D) + (ch >> 2) * 256 + (row & 7) * 32 + 8 * ((ch & 3) ^ ((row >> 2) & 3));
}

__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;
// Per-lane element offsets into a swizzled [64][D] image, computed ONCE per kernel: every
// row / transposed fragment is then (image base + lane offset + compile-time immediate), so
// the tile loops carry no per-fragment address arithmetic (swz() with runtime lane terms
// cost ~100 VALU per tile). Derivation: for row = 32*mt + r and chunk 2s+h, swz() splits into
// mt*32D + (s>>1)*256 + [lane part depending on s&1]; for the transposed read of k-step S,
// d-tile dt it is S*16D + dt*256 + [lane part], with a second lane part for rows +8.
template <int D>
struct LaneOffs {
  int row[2];
  int tra, trb;
  __device__ __forceinline__ explicit LaneOffs(int lane) {
    const int r = lane & 31, h = lane >> 5, x = (r >> 2) & 3;
    row[0] = (r >> 3) * 8 * D + (r & 7) * 32 + 8 * (h ^ x);
    row[1] = (r >> 3) * 8 * D + (r & 7) * 32 + 8 * ((2 + h) ^ x);
    const int g = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
    const int cc = 2 * g + (p >> 1);
    tra = (4 * h + q) * 32 + 8 * (cc ^ h) + 4 * (p & 1);
    trb = 8 * D + (4 * h + q) * 32 + 8 * (cc ^ (h + 2)) + 4 * (p & 1);
  }
};

// row fragment of image rows 32*mt + (lane&31), k-step s: 16 B of row at chunk 2s+h
template <typename T, int D>
__device__ __forceinline__ typename V8<T>::type frag_rows(const T* img, const LaneOffs<D>& lo, int mt, int s) {
  return *reinterpret_cast<const typename V8<T>::type*>(img + lo.row[s & 1] + mt * 32 * D + (s >> 1) * 256);
}

// Transposed A fragment (row = column 32*dt + (lane&31) of the image) over the k-step S of
// the image's rows, in the permuted k order of an accumulator-derived B operand:
// elem j <-> image row 16S + 8(j>>2) + 4h + (j&3). Two ds_read_b64_tr_b16: lane 4q+p of each
// 16-lane group addresses row (base+q), columns 4p..4p+3 of the group's 16 columns and
// receives its own column of the 4 rows. EXEC must be full (every lane takes part).
template <typename T, int D>
__device__ __forceinline__ typename V8<T>::type frag_tr(const T* img, const LaneOffs<D>& lo, int dt, int S) {
  const T* pa = img + lo.tra + S * 16 * D + dt * 256;
  const T* pb = img + lo.trb + S * 16 * D + dt * 256;
  const v4i16 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)pa);
  const v4i16 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)pb);
  const u32x2 ua = __builtin_bit_cast(u32x2, a), ub = __builtin_bit_cast(u32x2, b);
  u32x4 u;
  u[0] = ua[0]; u[1] = ua[1]; u[2] = ub[0]; u[3] = ub[1];
  return as_v8<T>(u);
}

}  // namespace fa
}  // namespace pra
