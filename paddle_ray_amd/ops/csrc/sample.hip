// Fused temperature / top-k / top-p (nucleus) token sampling for gfx950: one launch picks one
// token id per row of x [R, V] (fp32 / f16 / bf16) with per-row device parameters and no sort.
//
// One workgroup of 1024 threads per row; the row is re-read from L2 by every pass:
//   1. max pass      row maximum with its lowest index (one u64 max of key << 32 | ~index)
//   2. radix descent over the order-preserving integer image ("key") of x, 8 bits per level
//                    (2 levels for 16-bit inputs, 4 for fp32): a 256-bin LDS histogram of count
//                    and weight over the entries that match the prefix found so far, then the
//                    bin where the first of the two limits (n_k by count, top_p * Z by weight) is
//                    crossed. Level 0 sees every entry, so its bins also sum to Z.
//   3. tie count     how many entries equal to the threshold key are kept (closed form); only when
//                    that cuts the tie group, one index-order pass finds the last kept tie
//   4. draw pass     index-order block scan of the kept weights up to the entry that crosses u * M
//
// Reproducibility: a weight is a fixed-point integer q = floor(w * 2^40), w in [0, 1], and every
// sum (bins, Z, kept weight M, the running sums of the draw) is an integer sum, so no decision
// depends on the order in which threads or LDS atomics arrive; floats only produce q (an
// elementwise function of x, the row max and the temperature) and the final prob = q_id / Z.
// With V <= 2^22 a sum stays below 2^62.
//
// Semantics (ops/fused.py sample_top_p states them once for every layer): NaN counts as -inf and
// -0 as +0; w = exp((x - max) / T), or max(x, 0) / max in probs mode, and exactly 1 at the
// maximum; order = (x descending, index ascending); n_k = top_k if 1 <= top_k < V else V; n_p =
// shortest prefix of the order whose weight >= top_p * Z (V for top_p >= 1); the first
// min(n_p, n_k) entries are kept, a cut tie group keeping its lowest indices; the id is the first
// kept index, in index order, whose running kept weight exceeds u * M. Greedy (T <= 0, top_k == 1,
// top_p <= 0) returns the lowest index of the maximum. A row with no weight (maximum -inf, or
// <= 0 in probs mode) returns its argmax with prob 0, which is id 0 for a row of -inf / NaN.
// Device parameters are untrusted: NaN T counts as 0, T is capped at FLT_MAX, NaN top_p counts as
// 1, u is truncated to 24 bits in [0, 1); nothing indexes memory with them, so every id is in
// [0, V) and nothing outside the row is read.
#include "common.h"
#include "pra_api.h"

#include <float.h>

namespace pra {
namespace smp {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kCopies = 16;                // histogram copies per bin (lane & 15): <= 4-way LDS conflicts
constexpr int kMaxV = 1 << 22;             // V * 2^40 < 2^63
constexpr float kFx = 1099511627776.f;     // 2^40
typedef unsigned long long u64;

// the 32-bit finaliser of flash_attn.hip's dropout hash (fa_mix32; ops/fused.py _mix32_t)
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
// h(seed, counter, row); for one (seed, counter) it is a bijection of the row index
// (ops/fused.py sample_hash_ref is the same arithmetic on Python integers)
__device__ __forceinline__ uint32_t sample_hash(uint64_t seed, uint64_t counter, uint32_t r) {
  const uint32_t a = mix32((uint32_t)seed ^ (uint32_t)(seed >> 32) * 0x27d4eb2fU ^
                           (uint32_t)counter * 0x165667b1U ^ (uint32_t)(counter >> 32) * 0x85ebca77U);
  return mix32(a ^ r * 0xc2b2ae3dU);
}

// Storage formats: raw element type, elements per 16-byte load, key width, canonical bits
// (NaN -> -inf, -0 -> +0), the order-preserving key of canonical bits and their value.
template <int DT> struct Fmt;
template <> struct Fmt<kF32> {
  typedef uint32_t raw_t;
  static constexpr int EPV = 4, KBITS = 32;
  static constexpr uint32_t SIGN = 0x80000000u, MASK = 0xffffffffu, INF = 0x7f800000u;
  static __device__ __forceinline__ float val(uint32_t b) { return __uint_as_float(b); }
};
template <> struct Fmt<kBF16> {
  typedef uint16_t raw_t;
  static constexpr int EPV = 8, KBITS = 16;
  static constexpr uint32_t SIGN = 0x8000u, MASK = 0xffffu, INF = 0x7f80u;
  static __device__ __forceinline__ float val(uint32_t b) { return __uint_as_float(b << 16); }
};
template <> struct Fmt<kF16> {
  typedef uint16_t raw_t;
  static constexpr int EPV = 8, KBITS = 16;
  static constexpr uint32_t SIGN = 0x8000u, MASK = 0xffffu, INF = 0x7c00u;
  static __device__ __forceinline__ float val(uint32_t b) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)b);
  }
};
template <int DT> __device__ __forceinline__ uint32_t canon(uint32_t b) {
  typedef Fmt<DT> FM;
  if ((b & (FM::MASK ^ FM::SIGN)) > FM::INF) b = FM::SIGN | FM::INF;
  return b == FM::SIGN ? 0u : b;
}
template <int DT> __device__ __forceinline__ uint32_t key_of(uint32_t cb) {
  typedef Fmt<DT> FM;
  return (cb & FM::SIGN) ? (~cb & FM::MASK) : (cb | FM::SIGN);
}
template <int DT> __device__ __forceinline__ uint32_t bits_of_key(uint32_t k) {
  typedef Fmt<DT> FM;
  return (k & FM::SIGN) ? (k ^ FM::SIGN) : (~k & FM::MASK);
}

// One row as chunks in index order: chunk 0 is the scalar head up to the first 16-byte boundary
// (row bases are only element-aligned), chunks 1..nvec are 16-byte loads, chunk nvec + 1 is the
// scalar tail. Every index a chunk touches is in [0, V).
template <int DT> struct Row {
  const typename Fmt<DT>::raw_t* p;
  int V, head, nvec, nch;
};
template <int DT> __device__ __forceinline__ Row<DT> make_row(const void* x, int64_t r, int V) {
  typedef Fmt<DT> FM;
  Row<DT> w;
  w.p = reinterpret_cast<const typename FM::raw_t*>(x) + r * (int64_t)V;
  const int to_align = (int)(((16u - (uint32_t)((uintptr_t)w.p & 15u)) & 15u) / sizeof(typename FM::raw_t));
  w.V = V;
  w.head = to_align < V ? to_align : V;
  w.nvec = (V - w.head) / FM::EPV;
  w.nch = w.nvec + 2;
  return w;
}
// f(index, canonical bits) for every element of chunk c, in index order
template <int DT, typename F> __device__ __forceinline__ void for_chunk(const Row<DT>& w, int c, F&& f) {
  typedef Fmt<DT> FM;
  if (c >= 1 && c <= w.nvec) {
    const int i0 = w.head + (c - 1) * FM::EPV;
    const uint4 u = *reinterpret_cast<const uint4*>(w.p + i0);
    const uint32_t d[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (FM::EPV == 4) {
        f(i0 + j, canon<DT>(d[j]));
      } else {
        f(i0 + 2 * j, canon<DT>(d[j] & 0xffffu));
        f(i0 + 2 * j + 1, canon<DT>(d[j] >> 16));
      }
    }
  } else if (c == 0 || c == w.nvec + 1) {
    const int i0 = c == 0 ? 0 : w.head + w.nvec * FM::EPV;
    const int i1 = c == 0 ? w.head : w.V;
    for (int i = i0; i < i1; ++i) f(i, canon<DT>((uint32_t)w.p[i]));
  }
}

// fixed-point weight of value x under row maximum mx (x <= mx, mx > -inf; probs mode: mx > 0)
__device__ __forceinline__ u64 weight_q(float x, float mx, float T, bool probs) {
  float w;
  if (x == mx) w = 1.f;
  else if (probs) w = fmaxf(x, 0.f) / mx;
  else w = __expf((x - mx) / T);
  return (u64)(fminf(w, 1.f) * kFx);
}

__device__ __forceinline__ u64 wave_incl_scan(u64 v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
// exclusive prefix of v over the block in thread order and the block total; red holds kWaves u64
__device__ __forceinline__ u64 block_excl_scan(u64 v, u64* red, u64& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const u64 incl = wave_incl_scan(v);
  if (lane == 63) red[wid] = incl;
  __syncthreads();
  u64 base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const u64 t = red[i];
    if (i < wid) base += t;
    tot += t;
  }
  __syncthreads();
  total = tot;
  return base + incl - v;
}
__device__ __forceinline__ u64 block_max_u64(u64 v, u64* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) r = red[i] > r ? red[i] : r;
  __syncthreads();
  return r;
}

struct State {           // written by one thread, read by all after a barrier
  uint32_t prefix;       // key bits found so far (right-aligned)
  uint32_t cnt_above;    // entries whose key is above the prefix
  u64 wt_above;          // their weight
  u64 Z, P;              // row weight; the top_p limit ceil(top_p * Z) (all ones: no limit)
  uint32_t c_t;          // last level: entries equal to the threshold key
  u64 wq_t;              //             and their weight
  int cut, res_id;       // index of the last kept tie; the drawn index
  u64 res_q;
};

struct Params {
  const void* x;
  const float* temperature;
  const int* top_k;
  const float* top_p;
  const float* uniform;
  int64_t* ids;
  float* probs;
  float* u_out;
  int V, probs_mode;
  uint64_t seed, offset;
  const int64_t* step;
};

template <int DT> __global__ __launch_bounds__(kThreads) void sample_top_p_kernel(const Params a) {
  typedef Fmt<DT> FM;
  __shared__ uint32_t hc[256 * kCopies];
  __shared__ u64 hw[256 * kCopies];
  __shared__ uint32_t bc[256];
  __shared__ u64 bw[256];
  __shared__ u64 red[kWaves];
  __shared__ State st;

  const int tid = threadIdx.x, lane = tid & 63;
  const int r = blockIdx.x, V = a.V;
  const Row<DT> row = make_row<DT>(a.x, r, V);
  const bool probs = a.probs_mode != 0;

  // untrusted per-row parameters, clamped
  float T = a.temperature[r];
  if (!(T > 0.f)) T = 0.f;
  T = fminf(T, FLT_MAX);
  float tp = a.top_p[r];
  if (tp != tp) tp = 1.f;
  const int tk = a.top_k[r];
  const uint32_t n_k = (tk >= 1 && tk < V) ? (uint32_t)tk : (uint32_t)V;
  uint32_t k24;
  if (a.uniform) {
    float u = a.uniform[r];
    u = u > 0.f ? fminf(u, 1.f) : 0.f;                  // NaN -> 0
    const uint32_t k = (uint32_t)(u * 16777216.f);
    k24 = k > 0xffffffu ? 0xffffffu : k;
  } else {
    const uint64_t counter = a.offset + (a.step ? (uint64_t)*a.step : 0ull);
    k24 = sample_hash(a.seed, counter, (uint32_t)r) >> 8;
  }
  if (a.u_out && tid == 0) a.u_out[r] = (float)k24 * (1.f / 16777216.f);

  // 1. row maximum, lowest index first
  u64 best = 0;
  for (int c = tid; c < row.nch; c += kThreads)
    for_chunk<DT>(row, c, [&](int i, uint32_t cb) {
      const u64 v = ((u64)key_of<DT>(cb) << 32) | (uint32_t)(0x7fffffff - i);
      best = v > best ? v : best;
    });
  best = block_max_u64(best, red);
  const uint32_t kmax = (uint32_t)(best >> 32);
  const int imax = 0x7fffffff - (int)(uint32_t)best;
  const float mx = FM::val(bits_of_key<DT>(kmax));
  auto finish = [&](int id, float prob) {
    if (tid == 0) {
      a.ids[r] = (int64_t)(id >= 0 && id < V ? id : imax);
      a.probs[r] = prob;
    }
  };
  if (mx == -INFINITY || (probs && !(mx > 0.f))) return finish(imax, 0.f);
  const bool greedy = (!probs && T == 0.f) || tk == 1 || !(tp > 0.f);
  if (greedy && !probs && T == 0.f) return finish(imax, 1.f);
  if (greedy) {  // the maximum's softmax probability: one sum pass
    u64 s = 0;
    for (int c = tid; c < row.nch; c += kThreads)
      for_chunk<DT>(row, c, [&](int, uint32_t cb) { s += weight_q(FM::val(cb), mx, T, probs); });
    u64 Z;
    block_excl_scan(s, red, Z);
    return finish(imax, (float)((double)kFx / (double)Z));
  }

  // 2. radix descent
  constexpr int kLevels = FM::KBITS / 8;
  for (int lvl = 0; lvl < kLevels; ++lvl) {
    const int shift = FM::KBITS - 8 * (lvl + 1);
    for (int i = tid; i < 256 * kCopies; i += kThreads) { hc[i] = 0; hw[i] = 0; }
    __syncthreads();
    const uint32_t prefix = lvl ? st.prefix : 0u;
    for (int c = tid; c < row.nch; c += kThreads)
      for_chunk<DT>(row, c, [&](int, uint32_t cb) {
        const uint32_t k = key_of<DT>(cb);
        if (lvl == 0 || (k >> ((shift + 8) & 31)) == prefix) {
          const int slot = (int)((k >> shift) & 255u) * kCopies + (lane & (kCopies - 1));
          atomicAdd(&hc[slot], 1u);
          const u64 q = weight_q(FM::val(cb), mx, T, probs);
          if (q) atomicAdd(&hw[slot], q);
        }
      });
    __syncthreads();
    if (tid < 256) {
      uint32_t c = 0;
      u64 w = 0;
#pragma unroll
      for (int j = 0; j < kCopies; ++j) { c += hc[tid * kCopies + j]; w += hw[tid * kCopies + j]; }
      bc[tid] = c;
      bw[tid] = w;
    }
    __syncthreads();
    if (tid < 64) {  // lane l owns bins 255 - 4l .. 252 - 4l: descending keys in lane order
      uint32_t c4 = 0;
      u64 w4 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c4 += bc[255 - 4 * lane - j]; w4 += bw[255 - 4 * lane - j]; }
      const u64 ic = wave_incl_scan((u64)c4);
      const u64 iw = wave_incl_scan(w4);
      u64 Z = 0, P = 0;
      if (lvl) {
        Z = st.Z;
        P = st.P;
      } else {
        Z = __shfl(iw, 63, 64);
        if (tp >= 1.f) {
          P = ~0ull;
        } else {
          const double want = ceil((double)tp * (double)Z);
          P = want < 1.0 ? 1ull : (u64)want;
        }
      }
      uint32_t rc = (lvl ? st.cnt_above : 0u) + (uint32_t)(ic - c4);
      u64 rw = (lvl ? st.wt_above : 0ull) + (iw - w4);
      int fb = -1;
      uint32_t fc = 0, fbc = 0;
      u64 fw = 0, fbw = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = 255 - 4 * lane - j;
        const uint32_t cb = bc[b];
        const u64 wb = bw[b];
        // bin 0 ends the scan whatever the sums say, so a digit is always chosen
        const bool cross = rc + cb >= n_k || rw + wb >= P || b == 0;
        if (cross && fb < 0) { fb = b; fc = rc; fw = rw; fbc = cb; fbw = wb; }
        rc += cb;
        rw += wb;
      }
      const u64 found = __ballot(fb >= 0);
      if (lane == __ffsll((long long)found) - 1) {
        st.prefix = (prefix << 8) | (uint32_t)fb;
        st.cnt_above = fc;
        st.wt_above = fw;
        st.c_t = fbc;
        st.wq_t = fbw;
        if (lvl == 0) { st.Z = Z; st.P = P; }
      }
    }
    __syncthreads();
  }

  // 3. ties at the threshold key that stay in the set
  const uint32_t kt = st.prefix, c_t = st.c_t;
  const u64 Z = st.Z, P = st.P, wt_above = st.wt_above;
  const u64 q_t = c_t ? st.wq_t / c_t : 0ull;
  const uint32_t m_k = n_k > st.cnt_above ? n_k - st.cnt_above : 1u;
  uint32_t m = c_t < m_k ? c_t : m_k;
  if (P != ~0ull && q_t > 0 && P > wt_above) {
    const u64 m_p = (P - wt_above + q_t - 1) / q_t;
    if (m_p < m) m = (uint32_t)m_p;
  }
  const u64 M = wt_above + (u64)m * q_t;
  __syncthreads();  // every thread has read st before it is written again
  if (tid == 0) { st.cut = 0x7fffffff; st.res_id = imax; st.res_q = (u64)kFx; }
  if (m < c_t) {  // index of the m-th tie, in index order
    uint32_t carry = 0;
    for (int c0 = 0; c0 < row.nch && carry < m; c0 += kThreads) {
      const int c = c0 + tid;
      uint32_t n = 0;
      for_chunk<DT>(row, c, [&](int, uint32_t cb) { n += key_of<DT>(cb) == kt; });
      u64 tot;
      const uint32_t ex = carry + (uint32_t)block_excl_scan((u64)n, red, tot);
      if (ex < m && m <= ex + n) {
        uint32_t seen = ex;
        for_chunk<DT>(row, c, [&](int i, uint32_t cb) {
          if (key_of<DT>(cb) == kt && ++seen == m) st.cut = i;
        });
      }
      carry += (uint32_t)tot;
    }
  }
  __syncthreads();
  const int cut = st.cut;

  // 4. the draw: first kept index whose running kept weight exceeds u * M = floor(M * k24 / 2^24)
  const u64 target = (M >> 24) * k24 + (((M & 0xffffffull) * k24) >> 24);
  u64 run = 0;
  for (int c0 = 0; c0 < row.nch && run <= target; c0 += kThreads) {
    const int c = c0 + tid;
    u64 s = 0;
    for_chunk<DT>(row, c, [&](int i, uint32_t cb) {
      const uint32_t k = key_of<DT>(cb);
      if (k > kt || (k == kt && i <= cut)) s += weight_q(FM::val(cb), mx, T, probs);
    });
    u64 tot;
    const u64 ex = run + block_excl_scan(s, red, tot);
    if (ex <= target && target < ex + s) {
      u64 acc = ex;
      bool done = false;
      for_chunk<DT>(row, c, [&](int i, uint32_t cb) {
        const uint32_t k = key_of<DT>(cb);
        if (!done && (k > kt || (k == kt && i <= cut))) {
          const u64 q = weight_q(FM::val(cb), mx, T, probs);
          acc += q;
          if (acc > target) { st.res_id = i; st.res_q = q; done = true; }
        }
      });
    }
    run += tot;
  }
  __syncthreads();
  finish(st.res_id, (float)((double)st.res_q / (double)Z));
}

}  // namespace smp
}  // namespace pra

extern "C" {

// x [R, V] contiguous (dt = kF32 / kF16 / kBF16), rows only element-aligned. temperature / top_p
// fp32 [R], top_k int32 [R], uniform fp32 [R] or null (then u comes from the counter hash of
// (seed, offset + *step, row); step is a device int64 or null). ids int64 [R], probs fp32 [R];
// u_out fp32 [R] or null receives the uniform each row used. probs_mode: x holds probabilities.
// Returns non-zero, launching nothing, for an unknown dtype, R < 0, V < 1 or V > 2^22.
int pra_sample_top_p(const void* x, const float* temperature, const int* top_k, const float* top_p,
                     const float* uniform, int64_t* ids, float* probs, float* u_out, int R, int V, int dt,
                     int probs_mode, uint64_t seed, uint64_t offset, const int64_t* step, hipStream_t s) {
  using namespace pra;
  if (R < 0 || V < 1 || V > smp::kMaxV || !(dt == kF32 || dt == kF16 || dt == kBF16)) return -1;
  if (R == 0) return 0;
  const smp::Params a{x, temperature, top_k, top_p, uniform, ids, probs, u_out, V, probs_mode, seed, offset, step};
  if (dt == kF32) hipLaunchKernelGGL(smp::sample_top_p_kernel<kF32>, dim3(R), dim3(smp::kThreads), 0, s, a);
  else if (dt == kF16) hipLaunchKernelGGL(smp::sample_top_p_kernel<kF16>, dim3(R), dim3(smp::kThreads), 0, s, a);
  else hipLaunchKernelGGL(smp::sample_top_p_kernel<kBF16>, dim3(R), dim3(smp::kThreads), 0, s, a);
  return 0;
}

}  // extern "C"
