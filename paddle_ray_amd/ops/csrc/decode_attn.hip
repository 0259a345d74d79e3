// Single-token (decode-phase) multi-head attention over a KV cache, for gfx950.
//
// Parity: the reference's masked multihead attention decoder kernel behind
// fused_multi_transformer (paddle/fluid/operators/fused/fused_multi_transformer_op.cu.h,
// mmha_launch_kernel): q·K over the cache positions [0, t], additive mask, softmax, ·V, and the
// new token's K/V written into the cache at position t.
//
// MI355X design (memory bound: every step streams the whole K/V cache once):
//  * split-K "flash decoding": grid (splits, heads, batch); each workgroup owns a contiguous
//    key range and keeps an online-softmax (max, sum, acc[D]) in registers; a second tiny
//    kernel merges the splits. Splits are sized so a decode step launches >= ~1024
//    workgroups (4 per CU) even at batch 1.
//  * G = D/8 lanes per key: each lane holds 8 of the D dims, so one key row (D*2 bytes) is
//    read by G consecutive lanes as 16-byte vectors — fully coalesced — and a 64-wide wave
//    works on 64/G keys at once. q·k is reduced over the G lanes with xor-shuffles that
//    never leave the group.
//  * two keys per lane-group per iteration are loaded before any math so >= 4 16-byte loads
//    per lane are in flight.
//  * the new token's K/V never round-trips through the cache: the workgroup that owns
//    position t uses them from the qkv buffer and writes them into the cache (vector stores).
//  * ragged batches (EXT instantiation; the plain one is compiled without any of it):
//    seq_lens[b] replaces t for sequence b, so a short sequence streams only its own
//    [0, t_b) and workgroups whose key range lies past t_b leave at once with the empty
//    partial (m = -inf, l = 0). rot [2, B, D] (cos, sin) rotates q and the new k in registers
//    (half-split rule inside each of rot_dims chunks; the partner 8 dims are one more 16-byte
//    load of the same qkv row). The rotated k is rounded to the cache dtype once and that
//    value is both stored at t_b and scored against, so later steps that read the row back
//    agree with this one.
#include "common.h"

namespace pra {
namespace {

constexpr int kWaves = 4;

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// merge (m2, l2, a2) into (m, l, a)
template <int N>
__device__ __forceinline__ void merge(float& m, float& l, float* a, float m2, float l2, const float* a2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  const float c1 = (m == -INFINITY) ? 0.f : __expf(m - M);
  const float c2 = (m2 == -INFINITY) ? 0.f : __expf(m2 - M);
  l = l * c1 + l2 * c2;
#pragma unroll
  for (int i = 0; i < N; ++i) a[i] = a[i] * c1 + a2[i] * c2;
  m = M;
}

// x[8] (dims d0..d0+7 of one head row) rotated against its partner half a chunk away
template <typename T>
__device__ __forceinline__ void rotate8(const T* row, int d0, int chunk, const float* cs, const float* sn, float* x) {
  const int half = chunk >> 1;
  const bool left = (d0 % chunk) < half;
  float p[8], c[8], s[8];
  load8<T>(row + (left ? d0 + half : d0 - half), p);
  load8<float>(cs + d0, c);
  load8<float>(sn + d0, s);
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = left ? x[i] * c[i] - p[i] * s[i] : x[i] * c[i] + p[i] * s[i];
}

template <typename T, int D, bool EXT>
__global__ void __launch_bounds__(kWaves * 64) mmha_split_k(
    const T* __restrict__ qkv,      // [B, 3, H, D] (bias already added)
    T* __restrict__ cache,          // [2, B, H, L, D]
    const float* __restrict__ mask, // [B, mask_len] additive, or null
    float* __restrict__ ws_ml,      // [B, H, S, 2]
    float* __restrict__ ws_acc,     // [B, H, S, D]
    T* __restrict__ out,            // [B, H, D] (used when splits == 1)
    int B, int H, int L, int t_host, const int* __restrict__ t_dev, int keys_per_split, int mask_len,
    float scale,
    const int* __restrict__ seq_lens,  // EXT: [B] per-sequence position, or null
    const float* __restrict__ rot,     // EXT: [2, B, D] cos then sin, or null
    int rot_dims) {
  // t_dev (HIP-graph decode loops): the position comes from device memory, so one captured
  // graph serves every step; an out-of-range position writes nothing and outputs zeros
  int t = t_dev ? t_dev[0] : t_host;
  constexpr int G = D / 8;            // lanes per key
  constexpr int KPW = 64 / G;         // keys per wave per sub-step
  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int splits = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane % G, grp = lane / G;
  bool in_bound = true;
  if constexpr (EXT) {
    if (seq_lens) {  // this sequence's own position; t_host / t_dev stay the bound that sized the grid
      t = seq_lens[b];
      in_bound = t_dev || t <= t_host;  // a device bound means the splits cover all of L
    }
  }
  const bool t_ok = in_bound && t >= 0 && t < L && !(mask && mask_len < t + 1);
  const int lo = split * keys_per_split;
  const int hi = t_ok ? min(t + 1, lo + keys_per_split) : lo;

  const size_t BH = (size_t)B * H;
  const T* qrow = qkv + ((size_t)b * 3 * H + h) * D;
  const T* knew = qkv + ((size_t)b * 3 * H + H + h) * D;
  const T* vnew = qkv + ((size_t)b * 3 * H + 2 * H + h) * D;
  T* kc = cache + ((size_t)b * H + h) * (size_t)L * D;
  T* vc = cache + (BH + (size_t)b * H + h) * (size_t)L * D;

  float q[8];
  float kt[8];  // EXT: the token's own k exactly as the cache holds it
  if constexpr (EXT) {
    if (hi <= lo) {  // a key range past t_b, or a guarded position: no loads, the empty partial
      if (wave == 0 && grp == 0) {
        if (splits == 1) {
          const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          store8<T>(out + ((size_t)b * H + h) * D + gl * 8, z);
        } else if (gl == 0) {
          *reinterpret_cast<float2*>(ws_ml + (((size_t)b * H + h) * splits + split) * 2) =
              make_float2(-INFINITY, 0.f);
        }
      }
      return;
    }
    load8<T>(qrow + gl * 8, q);
    load8<T>(knew + gl * 8, kt);
    if (rot) {
      const float* cs = rot + (size_t)b * D;
      const float* sn = rot + ((size_t)B + b) * D;
      rotate8<T>(qrow, gl * 8, D / rot_dims, cs, sn, q);
      rotate8<T>(knew, gl * 8, D / rot_dims, cs, sn, kt);
#pragma unroll
      for (int i = 0; i < 8; ++i) kt[i] = Cvt<T>::to(Cvt<T>::from(kt[i]));  // rounded once
    }
    if (t < hi && wave == 0 && grp == 0) {  // append the new token (here hi > lo, so t_ok and t >= lo)
      float v[8];
      store8<T>(kc + (size_t)t * D + gl * 8, kt);
      load8<T>(vnew + gl * 8, v);
      store8<T>(vc + (size_t)t * D + gl * 8, v);
    }
  } else {
    if (t_ok && t >= lo && t < hi && wave == 0 && grp == 0) {  // append the new token to the cache
      float kv[8];
      load8<T>(knew + gl * 8, kv);
      store8<T>(kc + (size_t)t * D + gl * 8, kv);
      load8<T>(vnew + gl * 8, kv);
      store8<T>(vc + (size_t)t * D + gl * 8, kv);
    }
    load8<T>(qrow + gl * 8, q);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] *= scale;

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;

  const float* mrow = mask ? mask + (size_t)b * mask_len : nullptr;
  constexpr int STEP = kWaves * KPW * 2;
  for (int base = lo; base < hi; base += STEP) {
    int key[2];
    float kx[2][8], vx[2][8];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      key[u] = base + (u * kWaves + wave) * KPW + grp;
      const int kk = key[u] < hi ? key[u] : lo;
      const T* kp = (kk == t) ? knew : kc + (size_t)kk * D;
      const T* vp = (kk == t) ? vnew : vc + (size_t)kk * D;
      load8<T>(kp + gl * 8, kx[u]);
      load8<T>(vp + gl * 8, vx[u]);
      if constexpr (EXT) {  // the token's own key: the (rotated, rounded) registers, not the raw row
        if (kk == t) {
#pragma unroll
          for (int i = 0; i < 8; ++i) kx[u][i] = kt[i];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s += q[i] * kx[u][i];
      s = group_sum<G>(s);
      if (key[u] >= hi) continue;
      if (mrow) s += mrow[key[u]];
      const float mn = fmaxf(m, s);
      if (mn == -INFINITY) continue;  // fully masked so far
      const float c = (m == -INFINITY) ? 0.f : __expf(m - mn);
      const float p = __expf(s - mn);
      l = l * c + p;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = acc[i] * c + p * vx[u][i];
      m = mn;
    }
  }

  // merge the KPW key groups of this wave (lanes gl, gl+G, ...)
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
    const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
    float a2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a2[i] = __shfl_xor(acc[i], o, 64);
    merge<8>(m, l, acc, m2, l2, a2);
  }
  // merge the waves through LDS
  __shared__ float s_ml[kWaves][2];
  __shared__ float s_acc[kWaves][D];
  if (grp == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s_acc[wave][gl * 8 + i] = acc[i];
    if (gl == 0) { s_ml[wave][0] = m; s_ml[wave][1] = l; }
  }
  __syncthreads();
  if (wave != 0 || grp != 0) return;
  for (int w = 1; w < kWaves; ++w) merge<8>(m, l, acc, s_ml[w][0], s_ml[w][1], &s_acc[w][gl * 8]);
  if (splits == 1) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= inv;
    store8<T>(out + ((size_t)b * H + h) * D + gl * 8, acc);
    return;
  }
  const size_t w = ((size_t)b * H + h) * splits + split;
  float* wa = ws_acc + w * D + gl * 8;
  *reinterpret_cast<float4*>(wa) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  *reinterpret_cast<float4*>(wa + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  if (gl == 0) *reinterpret_cast<float2*>(ws_ml + w * 2) = make_float2(m, l);
}

template <typename T, int D>
__global__ void __launch_bounds__(D) mmha_combine_k(const float* __restrict__ ws_ml, const float* __restrict__ ws_acc,
                                                    T* __restrict__ out, int splits) {
  const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x, d = threadIdx.x;
  const size_t w0 = ((size_t)b * H + h) * splits;
  float M = -INFINITY;
  for (int s = 0; s < splits; ++s) M = fmaxf(M, ws_ml[(w0 + s) * 2]);
  float num = 0.f, den = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < splits; ++s) {
      const float ms = ws_ml[(w0 + s) * 2];
      if (ms == -INFINITY) continue;
      const float c = __expf(ms - M);
      den += ws_ml[(w0 + s) * 2 + 1] * c;
      num += ws_acc[(w0 + s) * D + d] * c;
    }
  }
  out[((size_t)b * H + h) * D + d] = Cvt<T>::from(den > 0.f ? num / den : 0.f);
}

template <typename T, int D>
int launch(const void* qkv, void* cache, const float* mask, float* ws, void* out, int B, int H, int L, int t,
           const int* t_dev, int splits, int mask_len, float scale, const int* seq_lens, const float* rot,
           int rot_dims, hipStream_t s) {
  const int keys = t_dev ? L : t + 1;  // device position: splits cover the whole cache
  const int per = (keys + splits - 1) / splits;
  float* ws_ml = ws;
  float* ws_acc = ws + (((size_t)B * H * splits * 2 + 3) / 4) * 4;  // 16-B aligned
  if (seq_lens || rot)
    hipLaunchKernelGGL((mmha_split_k<T, D, true>), dim3(splits, H, B), dim3(kWaves * 64), 0, s, (const T*)qkv,
                       (T*)cache, mask, ws_ml, ws_acc, (T*)out, B, H, L, t, t_dev, per, mask_len, scale, seq_lens, rot,
                       rot_dims);
  else
    hipLaunchKernelGGL((mmha_split_k<T, D, false>), dim3(splits, H, B), dim3(kWaves * 64), 0, s, (const T*)qkv,
                       (T*)cache, mask, ws_ml, ws_acc, (T*)out, B, H, L, t, t_dev, per, mask_len, scale, nullptr,
                       nullptr, 0);
  if (splits > 1)
    hipLaunchKernelGGL((mmha_combine_k<T, D>), dim3(H, B), dim3(D), 0, s, ws_ml, ws_acc, (T*)out, splits);
  return 0;
}

}  // namespace
}  // namespace pra

using namespace pra;

extern "C" {
// workgroups per decode step: aim for >= 1024 (4 per CU) with >= 64 keys per split
int pra_mmha_splits(int B, int H, int t) {
  const int keys = t + 1;
  int want = (1024 + B * H - 1) / (B * H);
  int cap = (keys + 63) / 64;
  int s = want < cap ? want : cap;
  if (s < 1) s = 1;
  if (s > 256) s = 256;
  return s;
}

// ws: fp32 workspace of B*H*splits*(2 + D) + 4 floats (unused when splits == 1).
// seq_lens (device int32 [B]) and rot (device fp32 [2, B, D], rot_dims chunks) are optional: null
// runs the plain kernel. t / t_dev stay the batch-wide bound that the splits were sized for.
int pra_mmha_decode(const void* qkv, void* cache, const float* mask, float* ws, void* out, int B, int H, int L,
                    int D, int t, const int* t_dev, int splits, int mask_len, float scale, int dt,
                    const int* seq_lens, const float* rot, int rot_dims, hipStream_t s) {
  if (splits < 1) return -1;
  if (!t_dev && (t < 0 || t >= L || (mask && mask_len < t + 1))) return -1;
  if (rot && (rot_dims < 1 || D % (16 * rot_dims) != 0)) return -1;  // a half chunk is whole 8-dim lanes
#define PRA_MMHA(TT)                                                                                     \
  switch (D) {                                                                                           \
    case 64: return launch<TT, 64>(qkv, cache, mask, ws, out, B, H, L, t, t_dev, splits, mask_len, scale, \
                                   seq_lens, rot, rot_dims, s);                                          \
    case 128: return launch<TT, 128>(qkv, cache, mask, ws, out, B, H, L, t, t_dev, splits, mask_len, scale, \
                                     seq_lens, rot, rot_dims, s);                                        \
    case 256: return launch<TT, 256>(qkv, cache, mask, ws, out, B, H, L, t, t_dev, splits, mask_len, scale, \
                                     seq_lens, rot, rot_dims, s);                                        \
    default: return -1;                                                                                  \
  }
  if (dt == kBF16) { PRA_MMHA(bf16) }
  if (dt == kF16) { PRA_MMHA(f16) }
  if (dt == kF32) { PRA_MMHA(float) }
#undef PRA_MMHA
  return -1;
}

// the split merge alone, for split-K kernels in other files that fill the same workspace layout
// (decode_attn_gqa.hip): ws_ml [B, H, splits, 2], ws_acc [B, H, splits, D] -> out [B, H, D]
int pra_mmha_combine(const float* ws_ml, const float* ws_acc, void* out, int B, int H, int D, int splits, int dt,
                     hipStream_t s) {
#define PRA_COMBINE(TT)                                                                                      \
  switch (D) {                                                                                               \
    case 64: hipLaunchKernelGGL((mmha_combine_k<TT, 64>), dim3(H, B), dim3(64), 0, s, ws_ml, ws_acc, (TT*)out, \
                                splits); return 0;                                                           \
    case 128: hipLaunchKernelGGL((mmha_combine_k<TT, 128>), dim3(H, B), dim3(128), 0, s, ws_ml, ws_acc,       \
                                 (TT*)out, splits); return 0;                                                \
    case 256: hipLaunchKernelGGL((mmha_combine_k<TT, 256>), dim3(H, B), dim3(256), 0, s, ws_ml, ws_acc,       \
                                 (TT*)out, splits); return 0;                                                \
    default: return -1;                                                                                      \
  }
  if (dt == kBF16) { PRA_COMBINE(bf16) }
  if (dt == kF16) { PRA_COMBINE(f16) }
  if (dt == kF32) { PRA_COMBINE(float) }
#undef PRA_COMBINE
  return -1;
}
}
