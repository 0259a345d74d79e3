// Prefill attention over the KV cache for gfx950 (CDNA4): T new tokens per sequence appended to a
// cache that may already hold t_b positions, equal to T consecutive single-token mmha_decode
// steps, for hundreds of query rows per K/V row (the decode kernels' one-row-per-lane split-K
// stops at 8). v_mfma_f32_32x32x16_{bf16,f16} for both products.
//
// qkv [B, T, H + 2*KVH, D]; cache [2, B, KVH, L, D], or with a block table [B, MB] the pool
// [2, NB, KVH, BS, D] with L = MB*BS; out [B, T, H, D]. Sequence b has t_b = seq_lens[b] (or t)
// cached positions and n_b = new_lens[b] (or T) new tokens; token j < n_b is cached at t_b + j and
// attends to [0, t_b + j]. Rows j >= n_b are zero and write nothing. A sequence is guarded as a
// whole (zeros, no write) when t_b < 0, n_b outside [0, T], t_b + n_b > L, the mask [B, mask_len]
// is shorter than t_b + n_b, or a table entry of a block holding one of its new positions is
// outside [0, NB): seq_plan() turns all of that into "n_b = 0", evaluated alike by both kernels.
//
// Two launches on one stream:
//  * append_kernel: one thread per 8 dims of one new K or V row. K is rotated in fp32 with the
//    token's own cos / sin (rot [2, B, T, D]), then rounded to the cache dtype or quantised
//    (kv_rows.h, the decode kernels' rule); an un-rotated float row is copied bit for bit. The
//    address goes through the table; 8- or 16-byte vector stores.
//  * attend_kernel: a flash-style forward over the cache alone. Every key lives in the cache by
//    now, so there is one K/V source and equality with single steps holds by construction.
//
// attend_kernel, work split: one workgroup of 4 waves per (sequence, K/V head, query tile). A
// query tile is 128 query rows = (128 / R) tokens x the R = H / KVH heads that share the K/V
// head, head fastest, so the rows of a wave are consecutive tokens and its causal range is tight;
// all R heads reuse each K/V tile from LDS (no K/V expansion). Query tiles are scheduled last
// first: the last tile sees the most keys. A tile entirely at j >= n_b writes its zeros and exits.
// R is a run-time shift: it only maps a row to (token, head) in the prologue and epilogue.
//
// Matrix path: flash_attn.hip's swapped formulation on mfma_frag.h's fragments. S^T = K Q^T puts
// one query row on each lane, so the online softmax is lane-local (fp32 registers, one shuffle
// across the lane halves); the P^T accumulator registers, rounded to the model dtype, are the B
// operand of O^T += V^T P^T, and V^T comes from the V image by ds_read_b64_tr_b16. Q is loaded
// once per workgroup straight into B fragments, rotated in fp32 with the token's own row. The
// 1/sqrt(D) scale (and the K dequant scale) multiplies the fp32 scores, not Q: one rounding
// less on Q, and for the uint8 cache the MFMA operands stay exact.
//
// K/V tiles: 64 cache rows per iteration into double-buffered swizzled LDS images; the next
// tile's global loads are issued into registers before the current tile's MFMAs and stored to
// the idle buffer after them (one barrier per tile). Registers, not LDS-DMA: a paged row needs a
// 64-bit address of its own and a uint8 row a conversion on the way. Paged: one table entry per
// staged row, fetched one iteration ahead of the loads that use it; an entry outside [0, NB) is
// never addressed: its rows are staged as zeros and carry the key bias -inf. uint8: bytes become
// the integer levels byte - 128 in the model dtype (exact in bf16 and f16); the K dequant scale
// rides on the score scale and the V dequant scale on the output normalisation.
//
// Causal rule and ragged ends: key p is visible to token j iff p <= t_b + j. Tiles whose keys all
// lie at or below t_b + (first token of the query tile) take the unmasked path; the diagonal and
// last tiles mask per element and skip 32-key halves beyond every query of the wave. The additive
// mask row and the -inf of table-less blocks reach the scores as a per-key bias staged in LDS with
// the tile (KB instantiations: a mask or a table is given); without either no tile below the
// diagonal pays for masking.
//
// No split over keys: with many query tiles the grid is large; a single short chunk on a very
// long prefix runs B * KVH * ceil(T * R / 128) workgroups only (profiles/prefill_attn.md).
#include <type_traits>

#include "common.h"
#include "kv_rows.h"
#include "mfma_frag.h"
#include "pra_api.h"

namespace pra {
namespace {
using namespace fa;

constexpr int kWaves = 4, kRows = kWaves * 32, kThreads = kWaves * 64;
constexpr int kCacheU8 = 3;  // cache dtype code of the 8-bit cache (the float ones are DType)
constexpr float kLog2e = 1.4426950408889634f;

struct Par {
  const int* seq_lens;  // [B] or null: t
  const int* new_lens;  // [B] or null: T
  const int* tables;    // [B, MB] or null: the contiguous cache
  const float* mask;    // [B, mask_len] or null
  const float* rot;     // [2, B, T, D] or null
  const float* scales;  // [4, Bs, KVH] (uint8 cache) or null
  int B, T, H, KVH, L, t, mask_len, rot_dims, sbs, round_type, NB, MB, shift, rshift;
  float scale, qmax, qmin;
};

// The new-token count of sequence b that both kernels act on: n_b, or 0 when the sequence is
// guarded. Called by every thread of the block (one barrier when there is a table).
__device__ __forceinline__ int seq_plan(const Par& p, int b, int& tb) {
  tb = p.seq_lens ? p.seq_lens[b] : p.t;
  const int n = p.new_lens ? p.new_lens[b] : p.T;
  if (!(tb >= 0 && n > 0 && n <= p.T && tb <= p.L - n && (!p.mask || p.mask_len - n >= tb))) return 0;
  if (p.tables) {  // tb + n <= L = MB << shift: every entry read is inside the table
    int bad = 0;
    for (int e = (tb >> p.shift) + (int)threadIdx.x; e <= ((tb + n - 1) >> p.shift); e += (int)blockDim.x)
      bad |= (unsigned)p.tables[(size_t)b * p.MB + e] >= (unsigned)p.NB;
    if (__syncthreads_or(bad)) return 0;
  }
  return n;
}

// row (of D elements) of position pos of (sequence b, K/V head kvh) in the K plane; blk is the
// position's table entry, already known to be in [0, NB)
__device__ __forceinline__ size_t kv_row(const Par& p, int b, int kvh, int pos, int blk) {
  if (p.tables) return (((size_t)blk * p.KVH + kvh) << p.shift) + (pos & ((1 << p.shift) - 1));
  return ((size_t)b * p.KVH + kvh) * p.L + pos;
}
__device__ __forceinline__ size_t plane_rows(const Par& p) {
  return p.tables ? ((size_t)p.NB * p.KVH) << p.shift : (size_t)p.B * p.KVH * p.L;
}
__device__ __forceinline__ size_t scale_plane(const Par& p) { return (size_t)(p.sbs ? p.B : 1) * p.KVH; }

// ---------------------------------------------------------------------------- append
template <typename T, int D, bool Q8>
__global__ void __launch_bounds__(kThreads)
append_kernel(const T* __restrict__ qkv, void* __restrict__ cache, Par p) {
  constexpr int NCH = D / 8;
  const int b = blockIdx.y;
  int tb;
  const int n = seq_plan(p, b, tb);
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  const int ch = idx % NCH, plane = (idx / NCH) & 1, kvh = (idx / (2 * NCH)) % p.KVH, j = idx / (2 * NCH * p.KVH);
  if (j >= n) return;
  const T* row = qkv + (((size_t)b * p.T + j) * (p.H + 2 * p.KVH) + p.H + plane * p.KVH + kvh) * D;
  const int pos = tb + j;
  const int blk = p.tables ? p.tables[(size_t)b * p.MB + (pos >> p.shift)] : 0;
  const size_t dst = (plane * plane_rows(p) + kv_row(p, b, kvh, pos, blk)) * D + ch * 8;
  const bool rot = p.rot && plane == 0;
  if (!Q8 && !rot) {  // the row as it is, bit for bit
    *reinterpret_cast<uint4*>(static_cast<T*>(cache) + dst) = *reinterpret_cast<const uint4*>(row + ch * 8);
    return;
  }
  float x[8];
  load8<T>(row + ch * 8, x);
  if (rot) {
    const int chunk = D / p.rot_dims, half = chunk >> 1;
    const bool left = ((ch * 8) % chunk) < half;
    float c[8], s[8];
    load8<float>(p.rot + ((size_t)b * p.T + j) * D + ch * 8, c);
    load8<float>(p.rot + (((size_t)p.B + b) * p.T + j) * D + ch * 8, s);
    rotate8<T>(row, ch * 8, half, left, c, s, x);
  }
  if constexpr (Q8) {
    const float qs = p.scales[plane * scale_plane(p) + (size_t)b * p.sbs + kvh];
    *reinterpret_cast<uint2*>(static_cast<uint8_t*>(cache) + dst) = quant8(x, qs, p.round_type, p.qmax, p.qmin);
  } else {
    store8<T>(static_cast<T*>(cache) + dst, x);
  }
}

// ---------------------------------------------------------------------------- attend
// 8 cached bytes -> their integer levels in the model dtype
template <typename T>
__device__ __forceinline__ uint4 levels8(uint2 w) {
  float f[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[i] = (float)((w.x >> (8 * i)) & 0xffu) - 128.f;
    f[4 + i] = (float)((w.y >> (8 * i)) & 0xffu) - 128.f;
  }
  return make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
}
__device__ __forceinline__ uint4 to_img(uint4 w, bf16*) { return w; }
__device__ __forceinline__ uint4 to_img(uint4 w, f16*) { return w; }
template <typename T> __device__ __forceinline__ uint4 to_img(uint2 w, T*) { return levels8<T>(w); }

template <typename T, int D, bool Q8, bool KB>
__global__ void __launch_bounds__(kThreads, 2)
attend_kernel(const T* __restrict__ qkv, const void* __restrict__ cache, T* __restrict__ out, Par p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* img0 = reinterpret_cast<T*>(smem);                                       // [2][K, V][64 * D]
  float* kbias = reinterpret_cast<float*>(smem + 4 * kTile * D * sizeof(T));  // [2][64]
  constexpr int NS = D / 16, ND = D / 32, NCH = D / 8, NP = kTile * NCH / kThreads;
  constexpr int EB = Q8 ? 1 : (int)sizeof(T);  // bytes of a cached element
  using Raw = std::conditional_t<Q8, uint2, uint4>;

  const int qt = gridDim.y - 1 - blockIdx.y;  // long-key tiles first
  const int b = blockIdx.x / p.KVH, kvh = blockIdx.x % p.KVH;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int j0 = qt * (kRows >> p.rshift);
  const int myrow = wave * 32 + r, myj = j0 + (myrow >> p.rshift);
  const int myh = (kvh << p.rshift) + (myrow & ((1 << p.rshift) - 1));
  int tb;
  const int n = seq_plan(p, b, tb);
  const bool valid = myj < n;

  // the lane's output row: 4 dims per (dt, g) at 32 dt + 8 g + 4 h, as the O^T accumulator holds them
  auto write_row = [&](const f32x16* acc, float inv) __attribute__((always_inline)) {
    if (myj >= p.T) return;
    T* orow = out + (((size_t)b * p.T + myj) * p.H + myh) * D;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 w = make_uint2(0u, 0u);
        if (valid) {
          w.x = pack2<T>(acc[dt][4 * g + 0] * inv, acc[dt][4 * g + 1] * inv);
          w.y = pack2<T>(acc[dt][4 * g + 2] * inv, acc[dt][4 * g + 3] * inv);
        }
        *reinterpret_cast<uint2*>(orow + 32 * dt + 8 * g + 4 * h) = w;
      }
  };

  f32x16 acc_o[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) acc_o[i] = f32x16{};
  if (j0 >= n) {  // uniform: a tile of padded rows, or a guarded sequence
    write_row(acc_o, 0.f);
    return;
  }

  // Q fragments: row myj of head myh, rotated with the token's own cos / sin
  typename V8<T>::type qf[NS];
  {
    const T* qrow = qkv + (((size_t)b * p.T + (valid ? myj : 0)) * (p.H + 2 * p.KVH) + myh) * D;
    const size_t rrow = ((size_t)b * p.T + (valid ? myj : 0)) * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int d0 = 16 * s + 8 * h;
      u32x4 u = {0, 0, 0, 0};
      if (valid && !p.rot) {
        const uint4 x = *reinterpret_cast<const uint4*>(qrow + d0);
        u[0] = x.x; u[1] = x.y; u[2] = x.z; u[3] = x.w;
      } else if (valid) {
        const int chunk = D / p.rot_dims, half = chunk >> 1;
        float x[8], c[8], sn[8];
        load8<T>(qrow + d0, x);
        load8<float>(p.rot + rrow + d0, c);
        load8<float>(p.rot + (size_t)p.B * p.T * D + rrow + d0, sn);
        rotate8<T>(qrow, d0, half, (d0 % chunk) < half, c, sn, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = pack2<T>(x[2 * i], x[2 * i + 1]);
      }
      qf[s] = as_v8<T>(u);
    }
  }
  float sl2 = p.scale * kLog2e, vdq = 1.f;  // scores -> the log2 domain; the V dequant scale
  if constexpr (Q8) {
    const float* sp = p.scales + (size_t)b * p.sbs + kvh;
    sl2 *= sp[2 * scale_plane(p)];
    vdq = sp[3 * scale_plane(p)];
  }

  const int kend = tb + min(n, j0 + (kRows >> p.rshift));  // keys [0, kend) are all this tile needs
  const int ntiles = (kend + kTile - 1) / kTile;
  const int nfull = min(ntiles, (tb + j0 + 1) / kTile);    // tiles every row sees whole

  // staging of one K/V tile: chunk c = tid + 256 pass is 16-byte column chunk c % NCH of row c / NCH
  Raw kr[NP], vr[NP];
  float kbv[NP];
  int blk[NP];
  const size_t vplane = plane_rows(p) * D * EB;
  const char* cbase = static_cast<const char*>(cache);
  auto lookup = [&](int kt) __attribute__((always_inline)) {  // the table entries of tile kt's rows
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int pos = kt * kTile + (tid + kThreads * q) / NCH;
      blk[q] = (p.tables && pos < kend) ? p.tables[(size_t)b * p.MB + (pos >> p.shift)] : 0;
    }
  };
  auto fetch = [&](int kt) __attribute__((always_inline)) {  // global -> registers, with blk[] of tile kt
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int c = tid + kThreads * q, row = c / NCH, dc = c % NCH, pos = kt * kTile + row;
      const bool ok = pos < kend && (!p.tables || (unsigned)blk[q] < (unsigned)p.NB);
      if constexpr (Q8) kr[q] = vr[q] = make_uint2(0x80808080u, 0x80808080u);  // level 0
      else kr[q] = vr[q] = make_uint4(0u, 0u, 0u, 0u);
      if (ok) {
        const size_t e = (kv_row(p, b, kvh, pos, blk[q]) * D + dc * 8) * EB;
        kr[q] = *reinterpret_cast<const Raw*>(cbase + e);
        vr[q] = *reinterpret_cast<const Raw*>(cbase + vplane + e);
      }
      if constexpr (KB) {
        kbv[q] = -INFINITY;
        if (ok && dc == 0) kbv[q] = p.mask ? p.mask[(size_t)b * p.mask_len + pos] * kLog2e : 0.f;
      }
    }
  };
  auto put = [&](int kt) __attribute__((always_inline)) {  // registers -> the images of buffer kt & 1
    T* Ks = img0 + (2 * (kt & 1)) * kTile * D;
    T* Vs = Ks + kTile * D;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int c = tid + kThreads * q, row = c / NCH, dc = c % NCH;
      *reinterpret_cast<uint4*>(Ks + swz<D>(row, dc)) = to_img(kr[q], (T*)nullptr);
      *reinterpret_cast<uint4*>(Vs + swz<D>(row, dc)) = to_img(vr[q], (T*)nullptr);
      if constexpr (KB) {
        if (dc == 0) kbias[(kt & 1) * kTile + row] = kbv[q];
      }
    }
  };
  lookup(0);
  fetch(0);
  if (ntiles > 1) lookup(1);
  put(0);
  __syncthreads();

  float m_run = -INFINITY, l_run = 0.f;  // m in the scaled log2 domain
  const LaneOffs<D> lo(lane);
  auto tile = [&](int kt, auto mask_c) __attribute__((always_inline)) {
    constexpr bool MASK = decltype(mask_c)::value;
    const int k0 = kt * kTile;
    const T* Ks = img0 + (2 * (kt & 1)) * kTile * D;
    const T* Vs = Ks + kTile * D;
    const float* kb = kbias + (kt & 1) * kTile;
    const bool more = kt + 1 < ntiles;
    if (more) {  // the idle buffer's next tile; the entries of the one after it
      fetch(kt + 1);
      if (kt + 2 < ntiles) lookup(kt + 2);
    }
    // masked tiles: 32-key halves beyond every query of this wave are skipped (wave-uniform)
    int nlive = 2;
    if constexpr (MASK) {
      const int kmax = min(kend - 1, tb + j0 + ((wave * 32 + 31) >> p.rshift));
      nlive = k0 > kmax ? 0 : (k0 + 32 > kmax ? 1 : 2);
      nlive = __builtin_amdgcn_readfirstlane(nlive);
    }
    if (nlive > 0) {
      f32x16 s_acc[2];
      {
        typename V8<T>::type kfr[2][NS];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int s = 0; s < NS; ++s)
            if (mt < nlive) kfr[mt][s] = frag_rows<T, D>(Ks, lo, mt, s);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          if (mt < nlive) {
            s_acc[mt] = f32x16{};
#pragma unroll
            for (int s = 0; s < NS; ++s) s_acc[mt] = mfma<T>(kfr[mt][s], qf[s], s_acc[mt]);
          } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) s_acc[mt][i] = -INFINITY;
          }
        }
      }
      // raw q.k -> scaled log2 scores plus the key bias; element i <-> key k0 + 32 mt + 8 (i >> 2) + 4 h + (i & 3)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if constexpr (KB) b4 = *reinterpret_cast<const float4*>(kb + 32 * mt + 8 * g + 4 * h);
          s_acc[mt][4 * g + 0] = fmaf(s_acc[mt][4 * g + 0], sl2, b4.x);
          s_acc[mt][4 * g + 1] = fmaf(s_acc[mt][4 * g + 1], sl2, b4.y);
          s_acc[mt][4 * g + 2] = fmaf(s_acc[mt][4 * g + 2], sl2, b4.z);
          s_acc[mt][4 * g + 3] = fmaf(s_acc[mt][4 * g + 3], sl2, b4.w);
        }
      if constexpr (MASK) {  // the causal rule; a valid row's last key tb + myj is below kend
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            s_acc[mt][i] = (k0 + 32 * mt + acc_row(i, h) > tb + myj) ? -INFINITY : s_acc[mt][i];
      }
      float mx = -INFINITY;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, s_acc[mt][i]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      if (__any(m_new > m_run)) {  // exact: lanes whose max did not grow get alpha = 1
        const float alpha = fexp2(m_run - m_use);
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) acc_o[dt] *= alpha;
      }
      m_run = m_new;
      float ps = 0.f;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pe = fexp2(s_acc[mt][i] - m_use);
          ps += pe;
          s_acc[mt][i] = pe;
        }
      ps += __shfl_xor(ps, 32, 64);
      l_run += ps;
      // O^T += V^T P^T, P rounded to the model dtype (k-steps of a dead half contribute nothing)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < 2 * nlive) {
          const typename V8<T>::type pf = pack_frag<T>(s_acc[ks >> 1], 8 * (ks & 1));
#pragma unroll
          for (int dt = 0; dt < ND; ++dt) acc_o[dt] = mfma<T>(frag_tr<T, D>(Vs, lo, dt, ks), pf, acc_o[dt]);
        }
      }
    }
    if (more) put(kt + 1);  // last read before the previous barrier
    __syncthreads();
  };
  for (int kt = 0; kt < nfull; ++kt) tile(kt, std::false_type{});
  for (int kt = nfull; kt < ntiles; ++kt) tile(kt, std::true_type{});

  write_row(acc_o, l_run > 0.f ? vdq / l_run : 0.f);
}

struct Args {
  const void* qkv;
  void* cache;
  void* out;
  Par p;
  bool q8;
  hipStream_t s;
};

// The attend kernel's dynamic LDS (64.5 KB at head dim 128) is above the default limit: raise it
// once per instantiation and device. False when the runtime refuses, so that nothing is launched.
template <typename T, int D, bool Q8, bool KB>
bool attend_ready(size_t lds) {
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return false;
  if (dev < 64 && done[dev]) return true;
  if (hipFuncSetAttribute((const void*)attend_kernel<T, D, Q8, KB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return false;
  if (dev < 64) done[dev] = true;
  return true;
}

// append, then attend, on a.s; launch errors are left for the caller's hipGetLastError()
template <typename T, int D, bool Q8, bool KB>
int run(const Args& a) {
  const size_t lds = 4 * kTile * D * sizeof(T) + 2 * kTile * sizeof(float);
  if (!attend_ready<T, D, Q8, KB>(lds)) return -2;
  const int items = a.p.T * a.p.KVH * 2 * (D / 8);
  dim3 agrid((items + kThreads - 1) / kThreads, a.p.B);
  hipLaunchKernelGGL((append_kernel<T, D, Q8>), agrid, dim3(kThreads), 0, a.s, (const T*)a.qkv, a.cache, a.p);
  const int qt = kRows >> a.p.rshift;
  dim3 grid(a.p.B * a.p.KVH, (a.p.T + qt - 1) / qt);
  hipLaunchKernelGGL((attend_kernel<T, D, Q8, KB>), grid, dim3(kThreads), lds, a.s, (const T*)a.qkv,
                     (const void*)a.cache, (T*)a.out, a.p);
  return 0;
}

template <typename T, int D>
int launch(const Args& a) {
  const bool kb = a.p.mask || a.p.tables;
  if (a.q8) return kb ? run<T, D, true, true>(a) : run<T, D, true, false>(a);
  return kb ? run<T, D, false, true>(a) : run<T, D, false, false>(a);
}

}  // namespace
}  // namespace pra

using namespace pra;

extern "C" {
// Appends and attends as described at the top of this file. A null block_tables means the
// contiguous cache [2, B, KVH, L, D] with L = MB*BS (NB unused); otherwise BS is a power of two
// >= 16. dt kF16 or kBF16, D 64 or 128, H / KVH 1, 2, 4 or 8. cache_dt = dt with null scales for
// a float cache; cache_dt 3 with the packed fp32 scales [4, Bs, KVH] (scale_batch_stride 0 or
// KVH), round_type and the level bounds for the uint8 one, as in pra_mmha_decode. seq_lens /
// new_lens (device int32 [B]), mask (fp32 [B, mask_len]) and rot (fp32 [2, B, T, D], rot_dims
// chunks) are optional. Returns non-zero, launching nothing, for what it does not support or when the
// runtime refuses the attend kernel its LDS.
int pra_mmha_prefill(const void* qkv, void* cache, const float* mask, void* out, int B, int T, int H, int KVH, int NB,
                     int BS, int MB, int D, int t, int mask_len, float scale, int dt, const int* seq_lens,
                     const int* new_lens, const float* rot, int rot_dims, hipStream_t s, int cache_dt,
                     const float* scales, int scale_batch_stride, int round_type, float qmax, float qmin,
                     const int* block_tables) {
  if (B < 1 || T < 1 || KVH < 1 || H < KVH || H % KVH || BS < 1 || MB < 1 || (int64_t)MB * BS > INT32_MAX) return -1;
  if ((int64_t)B * KVH > INT32_MAX || (int64_t)T * KVH * (D / 4) > INT32_MAX) return -1;
  const int R = H / KVH;
  if ((R != 1 && R != 2 && R != 4 && R != 8) || (D != 64 && D != 128) || (dt != kF16 && dt != kBF16)) return -1;
  int shift = 0;
  if (block_tables) {
    if (BS < 16 || (BS & (BS - 1)) || NB < 1) return -1;
    while ((1 << shift) < BS) ++shift;
  }
  if (rot && (rot_dims < 1 || D % (16 * rot_dims) != 0)) return -1;  // a half chunk is whole 8-dim pieces
  const bool q8 = cache_dt == kCacheU8;
  if (q8) {
    if (!scales || (scale_batch_stride != 0 && scale_batch_stride != KVH) || (round_type != 0 && round_type != 1) ||
        !(qmin >= -128.f && qmin < qmax && qmax <= 127.f))
      return -1;
  } else if (cache_dt != dt) {
    return -1;
  }
  if (((uintptr_t)cache & 15) || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 7) || ((uintptr_t)rot & 15)) return -1;
  int rshift = 0;
  while ((1 << rshift) < R) ++rshift;
  Args a;
  a.qkv = qkv;
  a.cache = cache;
  a.out = out;
  a.q8 = q8;
  a.s = s;
  a.p = Par{seq_lens, new_lens, block_tables, mask, rot, q8 ? scales : nullptr, B, T, H, KVH, MB * BS, t, mask_len,
            rot_dims, scale_batch_stride, round_type, NB, MB, shift, rshift, scale, qmax, qmin};
  if (dt == kBF16) return D == 64 ? launch<bf16, 64>(a) : launch<bf16, 128>(a);
  return D == 64 ? launch<f16, 64>(a) : launch<f16, 128>(a);
}
}  // extern "C"
