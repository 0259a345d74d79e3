// Single-token (decode-phase) attention over a KV cache, for gfx950: plain multi-head, ragged
// batches with in-kernel rotary, and grouped-query (KVH < H K/V heads, each shared by
// R = H / KVH consecutive query heads; query head h reads K/V head h / R), all from one kernel
// template.
//
// Parity: the reference's masked multihead attention decoder kernel behind
// fused_multi_transformer (paddle/fluid/operators/fused/fused_multi_transformer_op.cu.h,
// mmha_launch_kernel), with gqa_group_size = KVH: q·K over the cache positions [0, t], additive
// mask, softmax, ·V, and the new token's K/V written into the cache at position t. The qkv row is
// [H + 2*KVH, D] (the query heads, then KVH k heads, then KVH v heads), which for KVH = H is the
// memory layout of [3, H, D]; the cache is [2, B, KVH, L, D].
//
// MI355X design (memory bound: every step streams the whole K/V cache once):
//  * split-K "flash decoding": grid (splits, KVH, batch); each workgroup owns a contiguous
//    key range of one K/V head and a second tiny kernel merges the splits. Splits are sized so
//    a decode step launches >= ~1024 workgroups (4 per CU) even at batch 1.
//  * G = D/8 lanes per key: each lane holds 8 of the D dims, so one key row (D*2 bytes) is
//    read by G consecutive lanes as 16-byte vectors — fully coalesced — and a 64-wide wave
//    works on 64/G keys at once.
//  * every K and V row is loaded ONCE and scored against all R query rows of its K/V head,
//    which is the point of GQA on a memory-bound step. Each lane group keeps R scaled q rows
//    and R online-softmax states (m, l, acc[8]) in registers.
//  * two keys per lane group per iteration are loaded before any math so >= 4 16-byte loads
//    per lane are in flight; the two keys share one rescale of each state. q·k is written on
//    two-wide vectors (v_pk_fma_f32) and reduced over the G lanes with DPP operands on the
//    adds, so the R reductions per key cost no LDS-pipe round trips.
//  * key groups merge by xor-shuffle, waves through LDS, and lane group r of the workgroup
//    finishes query head r. The partials are indexed by query head
//    ((b*H + h)*splits + split), so mmha_combine_k merges them on grid (H, B) whatever R is.
//  * the new token's K/V never round-trips through the cache: the workgroup that owns
//    position t uses them from the qkv buffer and appends the K/V row of its K/V head (vector
//    stores).
//  * ragged batches and rotary (EXT instantiations; a non-EXT one is compiled without any of
//    it): seq_lens[b] replaces t for sequence b, so a short sequence streams only its own
//    [0, t_b) and workgroups whose key range lies past t_b leave at once with the empty
//    partial (m = -inf, l = 0); a guarded sequence gets zeros and no write. rot [2, B, D]
//    (cos, sin) rotates the R q rows and the one new k row in registers (half-split rule inside
//    each of rot_dims chunks; the partner 8 dims are one more 16-byte load of the same qkv
//    row). The rotated k is rounded to the cache dtype once and that value is both stored at
//    t_b and scored against, so later steps that read the row back agree with this one.
//    R = 1 is built with and without EXT; R = 2, 4, 8 only with it, where null seq_lens / rot
//    are runtime checks.
//  * 8-bit cache (Q8 instantiations, always EXT; a float-cache one is compiled without any of
//    it): the cache is uint8, a byte u holding the level u - 128 =
//    clamp(round(x * quant_scale), qmin, qmax), read back as (u - 128) * dequant_scale, with
//    fp32 scales per K/V head ([4, Bs, KVH]: k quant, v quant, k dequant, v dequant; Bs = 1 or
//    B). A lane keeps its 8 dims, now one 8-byte load per row, and takes four keys per
//    iteration instead of two so as many bytes stay in flight; the rows stay raw (uint2) until
//    used and a byte becomes a float with v_cvt_f32_ubyte0..3. Scales and the offset cost
//    nothing per element: k dequant is folded into the scaled q rows and the offset into one
//    constant per query row, s = q'.u - 128 * sum(q'); V accumulates the raw bytes and the
//    epilogue applies (acc - 128 * l) * v dequant before the partial is posted, so the
//    workspace and mmha_combine_k see ordinary partials. The new token's K (rotated in fp32,
//    not rounded to T) and V are quantised in registers with one fp32 multiply and one
//    rounding, appended as one 8-byte vector store per lane, and scored as those levels.
//  * paged cache (PAGED instantiations, always EXT; a contiguous-cache one is compiled without
//    any of it): the cache is a block pool [2, NB, KVH, BS, D] (the K plane, then the V plane)
//    and block_tables [B, MB] int32 names, for sequence b, the physical block of logical
//    positions [j*BS, (j+1)*BS); BS is a power of two >= 16 given as a shift. Everything above
//    keeps working on logical positions with L = MB*BS; only the row address changes: key p of
//    K/V head kvh is row (table[b][p >> shift] * KVH + kvh) * BS + (p & (BS - 1)) of a plane.
//    Table entries are untrusted: an entry outside [0, NB) never becomes an address. A key in
//    such a block scores -inf and its loads go to the token's own row (whose block the guard
//    has checked; the loop's usual fallback row lo may itself lie in a bad block), and a
//    sequence whose own block is bad is guarded like one whose position is out of range. The
//    16-byte row loads depend on a 4-byte table load, so the entries of the next iteration's
//    keys are fetched one iteration ahead, after this iteration's row loads are issued and
//    before its math: as many row bytes stay in flight per lane as without paging.
//  * several new tokens per sequence (MULTI instantiations, always EXT; a single-token one is
//    compiled without any of it): n_tok tokens at positions [t_b, t_b + n_tok), equal to n_tok
//    consecutive single-token steps. A K/V head then has NQ = R * Tp query rows (Tp = n_tok
//    rounded up to a power of two, NQ in {2, 4, 8}; row i is token i / R, query head i % R), which
//    are the register states of the R = NQ instantiation, so the template's R counts rows and the
//    ratio is a run-time shift. The loop streams only what the cache held, [lo, min(hi, t_b)):
//    every row sees all of it, so it has no per-row test and no new-token registers. The
//    workgroup whose key range holds t_b then runs a tail before the merges: lane group j takes
//    token j's k / v from the qkv buffer, rotates k with token j's cos / sin, rounds or quantises
//    it, appends the row at t_b + j and scores it as one more key, with weight 0 for the rows of
//    earlier tokens (the causal rule among the new tokens). Rows of tokens >= n_tok are zero
//    queries that are never stored and post no partial. Partials and output are indexed as if
//    there were n_tok * H heads, so mmha_combine_k runs unchanged on grid (n_tok * H, B). The
//    guard is all or nothing per sequence; PAGED: n_tok <= 8 < BS, so the new positions lie in at
//    most two blocks and both entries are checked before anything is addressed.
#include <type_traits>

#include "common.h"
#include "pra_api.h"

namespace pra {
namespace {

constexpr int kWaves = 4;
constexpr int kCacheU8 = 3;  // cache dtype code of the 8-bit cache (the float ones are DType)

typedef float f2 __attribute__((ext_vector_type(2)));

// v + (v of the lane that the DPP control selects): the cross-lane operand rides on the add
// itself, so the R reductions per key cost VALU slots only and no LDS-pipe round trips
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// sum over the G (8, 16 or 32) consecutive lanes of a key group, the same bits in every lane:
// the two quad swaps, then the mirror inside each 8 and inside each 16 lanes
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  static_assert(G == 8 || G == 16 || G == 32, "key groups of 8, 16 or 32 lanes");
  v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  if constexpr (G >= 16) v = dpp_add<0x140>(v);  // row_mirror
  if constexpr (G == 32) v += __shfl_xor(v, 16, 64);
  return v;
}

// merge (m2, l2, a2) into (m, l, a)
__device__ __forceinline__ void merge(float& m, float& l, float* a, float m2, float l2, const float* a2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  const float c1 = (m == -INFINITY) ? 0.f : __expf(m - M);
  const float c2 = (m2 == -INFINITY) ? 0.f : __expf(m2 - M);
  l = l * c1 + l2 * c2;
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = a[i] * c1 + a2[i] * c2;
  m = M;
}

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

// what only a Q8 instantiation is given (an empty parameter otherwise)
template <bool Q8> struct QParams {};
template <> struct QParams<true> {
  const float* scales;  // [4, Bs, KVH] fp32: k quant, v quant, k dequant, v dequant
  int bstride;          // 0 (Bs = 1) or KVH (Bs = B)
  int round_type;       // 1: half away from zero, 0: half to even
  float qmax, qmin;     // level bounds, -128 <= qmin < qmax <= 127
};

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

// 8 stored bytes -> 8 floats in [0, 255] (v_cvt_f32_ubyte0..3); the offset is applied elsewhere
__device__ __forceinline__ void unpack8(uint2 w, float* o) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[i] = (float)((w.x >> (8 * i)) & 0xffu);
    o[4 + i] = (float)((w.y >> (8 * i)) & 0xffu);
  }
}

// what only a PAGED instantiation is given (an empty parameter otherwise)
template <bool PAGED> struct PParams {};
template <> struct PParams<true> {
  const int* tables;  // [B, MB] int32 physical block per logical block, untrusted
  int NB, MB, shift;  // pool blocks, table columns, log2 of the block size
};

__device__ __forceinline__ size_t pool_plane(const PParams<false>&, int) { return 0; }
__device__ __forceinline__ size_t pool_plane(const PParams<true>& pp, int KVH) {  // rows of one plane
  return ((size_t)pp.NB * KVH) << pp.shift;
}

// what only a MULTI instantiation is given (an empty parameter otherwise)
template <bool MULTI> struct MParams {};
template <> struct MParams<true> {
  int n_tok;   // new tokens per sequence, 2 <= n_tok <= NQ >> rshift
  int rshift;  // log2 of the query heads per K/V head
};

// one kernel parameter for all three: empty bases take no room, so a single-token instantiation
// is given exactly what it was given before there were pages or several tokens
template <bool Q8, bool PAGED, bool MULTI> struct XParams : QParams<Q8>, PParams<PAGED>, MParams<MULTI> {};

// MULTI: R counts the query rows per K/V head, NQ = (H / KVH) * Tp with Tp = n_tok rounded up to a
// power of two; the ratio itself is then a run-time value (xp.rshift)
template <typename T, int D, int R, bool EXT, bool Q8, bool PAGED, bool MULTI = false>
__global__ void __launch_bounds__(kWaves * 64) mmha_split_k(
    const T* __restrict__ qkv,      // [B, H + 2*KVH, D] (bias already added)
    std::conditional_t<Q8, uint8_t, T>* __restrict__ cache,  // [2, B, KVH, L, D]; PAGED: [2, NB, KVH, BS, D]
    const float* __restrict__ mask, // [B, mask_len] additive, or null
    float* __restrict__ ws_ml,      // [B, H, S, 2]
    float* __restrict__ ws_acc,     // [B, H, S, D]
    T* __restrict__ out,            // [B, H, D] (used when splits == 1)
    int B, int KVH, int L, int t_host, const int* __restrict__ t_dev, int keys_per_split, int mask_len,
    float scale,
    const int* __restrict__ seq_lens,  // EXT: [B] per-sequence position, or null
    const float* __restrict__ rot,     // EXT: [2, B, D] cos then sin, or null
    int rot_dims, XParams<Q8, PAGED, MULTI> xp) {
  static_assert(EXT || !Q8, "the Q8 instantiations are EXT ones");
  static_assert(EXT || !PAGED, "the PAGED instantiations are EXT ones");
  static_assert(EXT || !MULTI, "the MULTI instantiations are EXT ones");
  [[maybe_unused]] const QParams<Q8>& qp = xp;
  [[maybe_unused]] const PParams<PAGED>& pp = xp;
  // MULTI: NT new tokens per sequence at positions [t, t + NT); query row i of the R is token
  // i >> rsh, query head h0 + (i & rmask)
  [[maybe_unused]] int NT = 1, rsh = 0, rmask = 0;
  if constexpr (MULTI) {
    const MParams<MULTI>& mp = xp;
    NT = mp.n_tok;
    rsh = mp.rshift;
    rmask = (1 << rsh) - 1;
  }
  using C = std::conditional_t<Q8, uint8_t, T>;  // a cache element
  // t_dev (HIP-graph decode loops): the position comes from device memory, so one captured
  // graph serves every step; an out-of-range position writes nothing and outputs zeros
  int t = t_dev ? t_dev[0] : t_host;
  constexpr int G = D / 8;            // lanes per key
  constexpr int KPW = 64 / G;         // keys per wave per sub-step
  static_assert(kWaves * KPW >= R, "one lane group per query head in the epilogue");
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int splits = gridDim.x;
  const int H = MULTI ? KVH << rsh : KVH * R, h0 = MULTI ? kvh << rsh : kvh * R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane % G, grp = lane / G;
  bool in_bound = true;
  if constexpr (EXT) {
    if (seq_lens) {  // this sequence's own position; t_host / t_dev stay the bound that sized the grid
      t = seq_lens[b];
      in_bound = t_dev || t <= t_host;  // a device bound means the splits cover all of L
    }
  }
  bool t_ok = in_bound && t >= 0 && t < L && !(mask && mask_len < t + 1);
  if constexpr (MULTI) t_ok = in_bound && t >= 0 && t <= L - NT && !(mask && mask_len < t + NT);  // all NT or none
  // PAGED: this sequence's table row, the entry of the token's own block, and in-block mask
  [[maybe_unused]] const int* tab = nullptr;
  [[maybe_unused]] int et = 0, bmask = 0;
  [[maybe_unused]] int et1 = 0;  // MULTI: the entry of the last new token's block (NT <= 8 < BS: it or the next)
  if constexpr (PAGED) {
    tab = pp.tables + (size_t)b * pp.MB;
    bmask = (1 << pp.shift) - 1;
    if (t_ok) {  // t in [0, L): the column is inside the table row
      et = tab[t >> pp.shift];
      t_ok = (unsigned)et < (unsigned)pp.NB;
      if constexpr (MULTI) {  // t + NT - 1 < L as well: both entries are checked before any address
        et1 = tab[(t + NT - 1) >> pp.shift];
        t_ok = t_ok && (unsigned)et1 < (unsigned)pp.NB;
      }
    }
  }
  const int lo = split * keys_per_split;
  // MULTI: the loop streams only what the cache held, [lo, min(hi, t)); the workgroup whose key
  // range holds t then scores and appends the NT new tokens (they never come from the cache)
  const int hi = t_ok ? min(MULTI ? t : t + 1, lo + keys_per_split) : lo;
  [[maybe_unused]] bool tail = false;
  if constexpr (MULTI) tail = t_ok && t >= lo && t < lo + keys_per_split;

  const size_t rows = (size_t)H + 2 * KVH;
  const T* qrow = qkv + ((size_t)b * NT * rows + h0) * D;     // R consecutive query rows (MULTI: token 0's)
  const T* knew = qkv + ((size_t)b * NT * rows + H + kvh) * D;
  const T* vnew = knew + (size_t)KVH * D;
  // PAGED: the two planes; a row index below is then a plane row, not a position
  C* kc = PAGED ? cache : cache + ((size_t)b * KVH + kvh) * (size_t)L * D;
  C* vc = PAGED ? cache + pool_plane(pp, KVH) * D : cache + (((size_t)B + b) * KVH + kvh) * (size_t)L * D;
  const size_t w0 = ((size_t)b * H + h0) * splits + split;    // partial of query head h0; head r: + r*splits
  // MULTI: output row of query row i, as if there were NT*H heads: (b*NT + token)*H + head
  [[maybe_unused]] auto orow = [&](int i) { return ((size_t)b * NT + (i >> rsh)) * H + h0 + (i & rmask); };

  if constexpr (MULTI) {
    if (hi <= lo && !tail) {  // the same for the NT << rsh rows that exist; the padded ones post nothing
      const int nrow = NT << rsh;
      if (splits == 1) {
        if (wave == 0 && grp == 0) {
          const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          for (int i = 0; i < nrow; ++i) store8<T>(out + orow(i) * D + gl * 8, z);
        }
      } else if ((int)threadIdx.x < nrow) {
        *reinterpret_cast<float2*>(ws_ml + (orow(threadIdx.x) * splits + split) * 2) = make_float2(-INFINITY, 0.f);
      }
      return;
    }
  } else if (hi <= lo) {  // a key range past t, or a guarded position: no loads, R empty partials
    if (splits == 1) {
      if (wave == 0 && grp == 0) {
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < R; ++r) store8<T>(out + ((size_t)b * H + h0 + r) * D + gl * 8, z);
      }
    } else if (threadIdx.x < R) {
      *reinterpret_cast<float2*>(ws_ml + (w0 + (size_t)threadIdx.x * splits) * 2) = make_float2(-INFINITY, 0.f);
    }
    return;
  }

  float q[R][8];
  [[maybe_unused]] float kt[8];  // the token's own k exactly as the cache holds it
  float qscale = scale;
  [[maybe_unused]] float vdq = 1.f;
  [[maybe_unused]] uint2 ktq, vtq;  // Q8: the token's own k / v as the bytes the cache holds
  if constexpr (MULTI) {
    // the R query rows, each rotated with its own token's cos / sin (rot is [2, B, NT, D]); a
    // padded row (token >= NT) is a zero query whose result is never posted. The new k / v rows
    // are the tail's business, after the loop.
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = i >> rsh;
      if (j < NT) {
        const T* qr = qkv + (((size_t)b * NT + j) * rows + h0 + (i & rmask)) * D;
        load8<T>(qr + gl * 8, q[i]);
        if (rot) {
          const int chunk = D / rot_dims, half = chunk >> 1;
          const bool left = ((gl * 8) % chunk) < half;
          float c[8], s[8];
          load8<float>(rot + ((size_t)b * NT + j) * D + gl * 8, c);
          load8<float>(rot + (((size_t)B + b) * NT + j) * D + gl * 8, s);
          rotate8<T>(qr, gl * 8, half, left, c, s, q[i]);
        }
      } else {
#pragma unroll
        for (int d = 0; d < 8; ++d) q[i][d] = 0.f;
      }
    }
    if constexpr (Q8) {
      const int plane = (qp.bstride ? B : 1) * KVH;
      const float* sp = qp.scales + (size_t)b * qp.bstride + kvh;
      qscale *= sp[2 * plane];  // k dequant rides on the q rows
      vdq = sp[3 * plane];
    }
  } else {
    // the row of position t (hi > lo here, so t_ok: PAGED, et is a block of the pool)
    size_t trow = (size_t)t;
    if constexpr (PAGED) trow = ((((size_t)et * KVH + kvh) << pp.shift) + (t & bmask));
#pragma unroll
    for (int r = 0; r < R; ++r) load8<T>(qrow + r * D + gl * 8, q[r]);
    load8<T>(knew + gl * 8, kt);
    if constexpr (EXT) {
      if (rot) {
        const int chunk = D / rot_dims, half = chunk >> 1;
        const bool left = ((gl * 8) % chunk) < half;
        float c[8], s[8];
        load8<float>(rot + (size_t)b * D + gl * 8, c);
        load8<float>(rot + ((size_t)B + b) * D + gl * 8, s);
#pragma unroll
        for (int r = 0; r < R; ++r) rotate8<T>(qrow + r * D, gl * 8, half, left, c, s, q[r]);
        rotate8<T>(knew, gl * 8, half, left, c, s, kt);
        if constexpr (!Q8) {
#pragma unroll
          for (int i = 0; i < 8; ++i) kt[i] = Cvt<T>::to(Cvt<T>::from(kt[i]));  // rounded once
        }
      }
    }
    if constexpr (Q8) {
      const int plane = (qp.bstride ? B : 1) * KVH;
      const float* sp = qp.scales + (size_t)b * qp.bstride + kvh;
      qscale *= sp[2 * plane];  // k dequant rides on the q rows
      vdq = sp[3 * plane];
      float vt[8];
      load8<T>(vnew + gl * 8, vt);
      ktq = quant8(kt, sp[0], qp.round_type, qp.qmax, qp.qmin);
      vtq = quant8(vt, sp[plane], qp.round_type, qp.qmax, qp.qmin);
      if (t < hi && wave == 0 && grp == 0) {  // append: one 8-byte store per lane and row
        *reinterpret_cast<uint2*>(kc + trow * D + gl * 8) = ktq;
        *reinterpret_cast<uint2*>(vc + trow * D + gl * 8) = vtq;
      }
    } else if (t < hi && wave == 0 && grp == 0) {  // append the new token (hi > lo here, so t_ok and t >= lo)
      float v[8];
      store8<T>(kc + trow * D + gl * 8, kt);
      load8<T>(vnew + gl * 8, v);
      store8<T>(vc + trow * D + gl * 8, v);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int i = 0; i < 8; ++i) q[r][i] *= qscale;
  }

  float m[R], l[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
  }

  const float* mrow = mask ? mask + (size_t)b * mask_len : nullptr;
  if constexpr (Q8) {
    // s = q'.(u - 128) = q'.u - qoff, the offset term reduced over the lane group once
    float qoff[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) sum += q[r][i];
      qoff[r] = 128.f * group_sum<G>(sum);
    }
    // keys per lane group per iteration: 4 keep 64 B in flight per lane, as for bf16; the 8
    // states of R = 8 leave registers for 2 (with 4 it drops to one wave per SIMD and spills)
    constexpr int U = R >= 8 ? 2 : 4;
    constexpr int STEP = kWaves * KPW * U;
    [[maybe_unused]] int ent[U];  // PAGED: the table entries of this iteration's keys
    if constexpr (PAGED) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int key = lo + (u * kWaves + wave) * KPW + grp;
        ent[u] = tab[(key < hi ? key : lo) >> pp.shift];
      }
    }
    for (int base = lo; base < hi; base += STEP) {
      uint2 kr[U], vr[U];
      float add[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int key = base + (u * kWaves + wave) * KPW + grp;
        int kk = key < hi ? key : lo;
        size_t row = (size_t)kk;
        bool live = key < hi;
        if constexpr (PAGED) {
          int e = ent[u];
          if ((unsigned)e >= (unsigned)pp.NB) {  // no address from it: the token's own row, weight 0
            e = et;
            kk = t;
            live = false;
          }
          row = (((size_t)e * KVH + kvh) << pp.shift) + (kk & bmask);
        }
        kr[u] = *reinterpret_cast<const uint2*>(kc + row * D + gl * 8);
        vr[u] = *reinterpret_cast<const uint2*>(vc + row * D + gl * 8);
        if constexpr (!MULTI) {
          if (kk == t) {  // the token's own row: the quantised registers, not what the slot held
            kr[u] = ktq;
            vr[u] = vtq;
          }
        }  // MULTI: kk == t only for a bad entry; whatever bytes the slot holds are finite, weight 0
        add[u] = live ? (mrow ? mrow[key] : 0.f) : -INFINITY;
      }
      if constexpr (PAGED) {  // the next iteration's entries, behind this one's row loads
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int key = base + STEP + (u * kWaves + wave) * KPW + grp;
          ent[u] = tab[(key < hi ? key : lo) >> pp.shift];
        }
      }
      float pw[R][U], cr[R];
      {
        float kf[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) unpack8(kr[u], kf[u]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float mn = m[r];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            f2 d = {0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 8; i += 2) d += f2{q[r][i], q[r][i + 1]} * f2{kf[u][i], kf[u][i + 1]};
            pw[r][u] = group_sum<G>(d.x + d.y) - qoff[r] + add[u];
            mn = fmaxf(mn, pw[r][u]);
          }
          const float ms = (mn == -INFINITY) ? 0.f : mn;  // fully masked so far: every weight below is 0
          cr[r] = __expf(m[r] - ms);
          float ps = 0.f;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            pw[r][u] = __expf(pw[r][u] - ms);
            ps += pw[r][u];
          }
          l[r] = l[r] * cr[r] + ps;
          m[r] = mn;
        }
      }
      float vf[U][8];
#pragma unroll
      for (int u = 0; u < U; ++u) unpack8(vr[u], vf[u]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float a = acc[r][i] * cr[r];
#pragma unroll
          for (int u = 0; u < U; ++u) a += pw[r][u] * vf[u][i];
          acc[r][i] = a;
        }
      }
    }
  } else {
    constexpr int STEP = kWaves * KPW * 2;
    [[maybe_unused]] int ent[2];  // PAGED: the table entries of this iteration's keys
    if constexpr (PAGED) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int key = lo + (u * kWaves + wave) * KPW + grp;
        ent[u] = tab[(key < hi ? key : lo) >> pp.shift];
      }
    }
    for (int base = lo; base < hi; base += STEP) {
      float kx[2][8], vx[2][8], add[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int key = base + (u * kWaves + wave) * KPW + grp;
        int kk = key < hi ? key : lo;
        size_t row = (size_t)kk;
        bool live = key < hi;
        if constexpr (PAGED) {
          int e = ent[u];
          if ((unsigned)e >= (unsigned)pp.NB) {  // no address from it: the token's own row, weight 0
            e = et;
            kk = t;
            live = false;
          }
          row = (((size_t)e * KVH + kvh) << pp.shift) + (kk & bmask);
        }
        const T* kp = (kk == t) ? knew : kc + row * D;
        const T* vp = (kk == t) ? vnew : vc + row * D;
        load8<T>(kp + gl * 8, kx[u]);
        load8<T>(vp + gl * 8, vx[u]);
        // MULTI: kk == t only for a bad entry, and the raw qkv rows of token 0 then stand in with
        // weight 0 (finite, unlike what the slot at t may hold)
        if constexpr (EXT && !MULTI) {  // the token's own key: the (rotated, rounded) registers, not the raw row
          if (kk == t) {
#pragma unroll
            for (int i = 0; i < 8; ++i) kx[u][i] = kt[i];
          }
        }
        // a key past the range (PAGED: or in a block the table does not give) scores -inf: its
        // weight is exactly 0
        add[u] = live ? (mrow ? mrow[key] : 0.f) : -INFINITY;
      }
      if constexpr (PAGED) {  // the next iteration's entries, behind this one's row loads
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int key = base + STEP + (u * kWaves + wave) * KPW + grp;
          ent[u] = tab[(key < hi ? key : lo) >> pp.shift];
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        f2 d0 = {0.f, 0.f}, d1 = {0.f, 0.f};  // packed fp32 FMAs: even and odd dims apart
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
          const f2 qq = {q[r][i], q[r][i + 1]};
          d0 += qq * f2{kx[0][i], kx[0][i + 1]};
          d1 += qq * f2{kx[1][i], kx[1][i + 1]};
        }
        float s0 = d0.x + d0.y, s1 = d1.x + d1.y;
        s0 = group_sum<G>(s0) + add[0];
        s1 = group_sum<G>(s1) + add[1];
        const float mn = fmaxf(m[r], fmaxf(s0, s1));
        const float ms = (mn == -INFINITY) ? 0.f : mn;  // fully masked so far: every weight below is 0
        const float c = __expf(m[r] - ms);
        const float p0 = __expf(s0 - ms), p1 = __expf(s1 - ms);
        l[r] = l[r] * c + p0 + p1;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[r][i] = acc[r][i] * c + p0 * vx[0][i] + p1 * vx[1][i];
        m[r] = mn;
      }
    }
  }

  if constexpr (MULTI) {
    // the tail: lane group j of the workgroup that owns t takes new token j from the qkv buffer
    // (kWaves * KPW >= 8 >= NT groups): rotate k with token j's cos / sin, round or quantise it,
    // append the row at t + j, and score it as one more key against the R rows. A row of an
    // earlier token does not see it (weight 0): the causal rule among the new tokens.
    const int j = wave * KPW + grp;
    if (tail && j < NT) {
      const T* kn = qkv + (((size_t)b * NT + j) * rows + H + kvh) * D;
      const int pos = t + j;  // t_ok: pos < L, inside the mask, and PAGED: its block is et or et1
      float kj[8], vj[8];
      load8<T>(kn + gl * 8, kj);
      load8<T>(kn + (size_t)KVH * D + gl * 8, vj);
      if (rot) {
        const int chunk = D / rot_dims, half = chunk >> 1;
        const bool left = ((gl * 8) % chunk) < half;
        float c[8], s[8];
        load8<float>(rot + ((size_t)b * NT + j) * D + gl * 8, c);
        load8<float>(rot + (((size_t)B + b) * NT + j) * D + gl * 8, s);
        rotate8<T>(kn, gl * 8, half, left, c, s, kj);
        if constexpr (!Q8) {
#pragma unroll
          for (int i = 0; i < 8; ++i) kj[i] = Cvt<T>::to(Cvt<T>::from(kj[i]));  // rounded once
        }
      }
      size_t prow = (size_t)pos;
      if constexpr (PAGED) {
        const int e = (pos >> pp.shift) == (t >> pp.shift) ? et : et1;
        prow = (((size_t)e * KVH + kvh) << pp.shift) + (pos & bmask);
      }
      if constexpr (Q8) {
        const int plane = (qp.bstride ? B : 1) * KVH;
        const float* sp = qp.scales + (size_t)b * qp.bstride + kvh;
        const uint2 kq = quant8(kj, sp[0], qp.round_type, qp.qmax, qp.qmin);
        const uint2 vq = quant8(vj, sp[plane], qp.round_type, qp.qmax, qp.qmin);
        *reinterpret_cast<uint2*>(kc + prow * D + gl * 8) = kq;
        *reinterpret_cast<uint2*>(vc + prow * D + gl * 8) = vq;
        unpack8(kq, kj);  // scored as the stored levels
        unpack8(vq, vj);
      } else {
        store8<T>(kc + prow * D + gl * 8, kj);
        store8<T>(vc + prow * D + gl * 8, vj);
      }
      const float add = mrow ? mrow[pos] : 0.f;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        f2 d2 = {0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 8; d += 2) d2 += f2{q[i][d], q[i][d + 1]} * f2{kj[d], kj[d + 1]};
        float s = group_sum<G>(d2.x + d2.y);
        if constexpr (Q8) {  // the offset term of the row, as in the loop
          float sum = 0.f;
#pragma unroll
          for (int d = 0; d < 8; ++d) sum += q[i][d];
          s -= 128.f * group_sum<G>(sum);
        }
        s = (i >> rsh) < j ? -INFINITY : s + add;
        const float mn = fmaxf(m[i], s);
        const float ms = (mn == -INFINITY) ? 0.f : mn;
        const float c = __expf(m[i] - ms), p = __expf(s - ms);
        l[i] = l[i] * c + p;
#pragma unroll
        for (int d = 0; d < 8; ++d) acc[i][d] = acc[i][d] * c + p * vj[d];
        m[i] = mn;
      }
    }
  }

  // merge the KPW key groups of this wave (lanes gl, gl+G, ...)
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float m2 = __shfl_xor(m[r], o, 64), l2 = __shfl_xor(l[r], o, 64);
      float a2[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) a2[i] = __shfl_xor(acc[r][i], o, 64);
      merge(m[r], l[r], acc[r], m2, l2, a2);
    }
  }
  // merge the waves through LDS: every wave posts its R states, lane group r finishes head r
  __shared__ float s_ml[kWaves][R][2];
  __shared__ __attribute__((aligned(16))) float s_acc[kWaves][R][D];
  if (grp == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      *reinterpret_cast<float4*>(&s_acc[wave][r][gl * 8]) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
      *reinterpret_cast<float4*>(&s_acc[wave][r][gl * 8 + 4]) =
          make_float4(acc[r][4], acc[r][5], acc[r][6], acc[r][7]);
      if (gl == 0) { s_ml[wave][r][0] = m[r]; s_ml[wave][r][1] = l[r]; }
    }
  }
  __syncthreads();
  const int r = wave * KPW + grp;  // this lane group's query head
  if (r >= R) return;
  if constexpr (MULTI) {
    if ((r >> rsh) >= NT) return;  // a padded row: never stored, no partial posted
  }
  float fm = s_ml[0][r][0], fl = s_ml[0][r][1], fa[8];
  load8<float>(&s_acc[0][r][gl * 8], fa);
  for (int w = 1; w < kWaves; ++w) {
    float a2[8];
    load8<float>(&s_acc[w][r][gl * 8], a2);
    merge(fm, fl, fa, s_ml[w][r][0], s_ml[w][r][1], a2);
  }
  if constexpr (Q8) {  // the V offset and scale, once: the partial leaves dequantised
#pragma unroll
    for (int i = 0; i < 8; ++i) fa[i] = (fa[i] - 128.f * fl) * vdq;
  }
  if (splits == 1) {
    const float inv = fl > 0.f ? 1.f / fl : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) fa[i] *= inv;
    store8<T>(out + (MULTI ? orow(r) : (size_t)b * H + h0 + r) * D + gl * 8, fa);
    return;
  }
  const size_t w = MULTI ? orow(r) * splits + split : w0 + (size_t)r * splits;
  store8<float>(ws_acc + w * D + gl * 8, fa);
  if (gl == 0) *reinterpret_cast<float2*>(ws_ml + w * 2) = make_float2(fm, fl);
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

struct Args {
  const void* qkv;
  void* cache;
  const float* mask;
  float* ws;
  void* out;
  int B, H, KVH, L, t;
  const int* t_dev;
  int splits, mask_len;
  float scale;
  const int* seq_lens;
  const float* rot;
  int rot_dims;
  hipStream_t s;
  const float* scales;  // 8-bit cache: [4, Bs, KVH], else null
  int scale_bstride, round_type;
  float qmax, qmin;
  const int* tables;  // paged cache: [B, MB] int32, else null
  int NB, MB, shift;
  int n_tok;  // new tokens per sequence (1: the single-token kernels)
};

template <bool Q8> QParams<Q8> qparams(const Args& a);
template <> QParams<false> qparams<false>(const Args&) { return {}; }
template <> QParams<true> qparams<true>(const Args& a) {
  return {a.scales, a.scale_bstride, a.round_type, a.qmax, a.qmin};
}

template <bool PAGED> PParams<PAGED> pparams(const Args& a);
template <> PParams<false> pparams<false>(const Args&) { return {}; }
template <> PParams<true> pparams<true>(const Args& a) { return {a.tables, a.NB, a.MB, a.shift}; }

template <bool Q8, bool PAGED, bool MULTI = false>
XParams<Q8, PAGED, MULTI> xparams(const Args& a, int rshift = 0) {
  XParams<Q8, PAGED, MULTI> xp;
  static_cast<QParams<Q8>&>(xp) = qparams<Q8>(a);
  static_cast<PParams<PAGED>&>(xp) = pparams<PAGED>(a);
  if constexpr (MULTI) static_cast<MParams<true>&>(xp) = {a.n_tok, rshift};
  return xp;
}

template <typename T, int D, int R, bool EXT, bool Q8 = false, bool PAGED = false>
int launch(const Args& a) {
  const int keys = a.t_dev ? a.L : a.t + 1;  // device position: splits cover the whole cache
  const int per = (keys + a.splits - 1) / a.splits;
  float* ws_ml = a.ws;
  float* ws_acc = a.ws + (((size_t)a.B * a.H * a.splits * 2 + 3) / 4) * 4;  // 16-B aligned
  hipLaunchKernelGGL((mmha_split_k<T, D, R, EXT, Q8, PAGED>), dim3(a.splits, a.KVH, a.B), dim3(kWaves * 64), 0, a.s,
                     (const T*)a.qkv, (std::conditional_t<Q8, uint8_t, T>*)a.cache, a.mask, ws_ml, ws_acc, (T*)a.out,
                     a.B, a.KVH, a.L, a.t, a.t_dev, per, a.mask_len, a.scale, a.seq_lens, a.rot, a.rot_dims,
                     xparams<Q8, PAGED>(a));
  if (a.splits > 1)
    hipLaunchKernelGGL((mmha_combine_k<T, D>), dim3(a.H, a.B), dim3(D), 0, a.s, ws_ml, ws_acc, (T*)a.out, a.splits);
  return 0;
}

// n_tok > 1 tokens per sequence: NQ query rows per K/V head; partials and output as if there
// were n_tok*H heads, so the combine kernel runs unchanged on grid (n_tok*H, B)
template <typename T, int D, int NQ, bool Q8, bool PAGED>
int launch_multi(const Args& a, int rshift) {
  const int keys = a.t_dev ? a.L : a.t + a.n_tok;  // device position: splits cover the whole cache
  const int per = (keys + a.splits - 1) / a.splits;
  const int HT = a.H * a.n_tok;
  float* ws_ml = a.ws;
  float* ws_acc = a.ws + (((size_t)a.B * HT * a.splits * 2 + 3) / 4) * 4;  // 16-B aligned
  hipLaunchKernelGGL((mmha_split_k<T, D, NQ, true, Q8, PAGED, true>), dim3(a.splits, a.KVH, a.B), dim3(kWaves * 64),
                     0, a.s, (const T*)a.qkv, (std::conditional_t<Q8, uint8_t, T>*)a.cache, a.mask, ws_ml, ws_acc,
                     (T*)a.out, a.B, a.KVH, a.L, a.t, a.t_dev, per, a.mask_len, a.scale, a.seq_lens, a.rot,
                     a.rot_dims, xparams<Q8, PAGED, true>(a, rshift));
  if (a.splits > 1)
    hipLaunchKernelGGL((mmha_combine_k<T, D>), dim3(HT, a.B), dim3(D), 0, a.s, ws_ml, ws_acc, (T*)a.out, a.splits);
  return 0;
}

template <typename T, int D, int NQ>
int launch_multi_x(const Args& a, int rshift) {
  if (a.tables)
    return a.scales ? launch_multi<T, D, NQ, true, true>(a, rshift) : launch_multi<T, D, NQ, false, true>(a, rshift);
  return a.scales ? launch_multi<T, D, NQ, true, false>(a, rshift) : launch_multi<T, D, NQ, false, false>(a, rshift);
}

// the ratio R = H / KVH and Tp = n_tok rounded up to a power of two give NQ = R * Tp in {2, 4, 8}
template <typename T, int D>
int launch_multi_r(const Args& a) {
  const int ratio = a.H / a.KVH;
  if (ratio > 8 || (ratio & (ratio - 1)) != 0 || a.n_tok > 8) return -1;
  int tp = 2;
  while (tp < a.n_tok) tp <<= 1;
  const int rshift = __builtin_ctz((unsigned)ratio);
  switch (ratio * tp) {
    case 2: return launch_multi_x<T, D, 2>(a, rshift);
    case 4: return launch_multi_x<T, D, 4>(a, rshift);
    case 8: return launch_multi_x<T, D, 8>(a, rshift);
    default: return -1;  // more than 8 query rows per K/V row
  }
}

template <typename T, int D>
int launch_r(const Args& a) {
  if (a.tables) {  // paged cache: EXT instantiations only, float and 8-bit pools
    switch (a.H / a.KVH) {
      case 1: return a.scales ? launch<T, D, 1, true, true, true>(a) : launch<T, D, 1, true, false, true>(a);
      case 2: return a.scales ? launch<T, D, 2, true, true, true>(a) : launch<T, D, 2, true, false, true>(a);
      case 4: return a.scales ? launch<T, D, 4, true, true, true>(a) : launch<T, D, 4, true, false, true>(a);
      case 8: return a.scales ? launch<T, D, 8, true, true, true>(a) : launch<T, D, 8, true, false, true>(a);
      default: return -1;
    }
  }
  if (a.scales) {  // 8-bit cache: EXT instantiations only
    switch (a.H / a.KVH) {
      case 1: return launch<T, D, 1, true, true>(a);
      case 2: return launch<T, D, 2, true, true>(a);
      case 4: return launch<T, D, 4, true, true>(a);
      case 8: return launch<T, D, 8, true, true>(a);
      default: return -1;
    }
  }
  switch (a.H / a.KVH) {
    case 1: return (a.seq_lens || a.rot) ? launch<T, D, 1, true>(a) : launch<T, D, 1, false>(a);
    case 2: return launch<T, D, 2, true>(a);
    case 4: return launch<T, D, 4, true>(a);
    case 8: return launch<T, D, 8, true>(a);
    default: return -1;
  }
}

template <typename T>
int launch_d(int D, const Args& a) {
  if (a.n_tok > 1) {
    switch (D) {
      case 64: return launch_multi_r<T, 64>(a);
      case 128: return launch_multi_r<T, 128>(a);
      case 256: return launch_multi_r<T, 256>(a);
      default: return -1;
    }
  }
  switch (D) {
    case 64: return launch_r<T, 64>(a);
    case 128: return launch_r<T, 128>(a);
    case 256: return launch_r<T, 256>(a);
    default: return -1;
  }
}

// the checks and the dispatch that the contiguous and the paged entry share (a.L is the
// logical capacity either way)
int decode(const Args& a, int D, int dt, int cache_dt) {
  if (a.splits < 1 || a.B < 1 || a.B > 65535 || a.KVH < 1 || a.KVH > 65535 || a.H < a.KVH || a.H % a.KVH != 0 ||
      a.L < 1 || a.n_tok < 1)
    return -1;
  if (!a.t_dev && (a.t < 0 || a.t > a.L - a.n_tok || (a.mask && a.mask_len < a.t + a.n_tok))) return -1;
  if (a.rot && (a.rot_dims < 1 || D % (16 * a.rot_dims) != 0)) return -1;  // a half chunk is whole 8-dim lanes
  if (cache_dt == kCacheU8) {  // a row piece is one aligned 8-byte access
    if (!a.scales || (a.scale_bstride != 0 && a.scale_bstride != a.KVH) || (a.round_type != 0 && a.round_type != 1) ||
        !(a.qmin >= -128.f && a.qmin < a.qmax && a.qmax <= 127.f) || ((uintptr_t)a.cache & 7) != 0)
      return -1;
  } else if (cache_dt != dt || a.scales) {
    return -1;
  }
  if (dt == kBF16) return launch_d<bf16>(D, a);
  if (dt == kF16) return launch_d<f16>(D, a);
  if (dt == kF32) return launch_d<float>(D, a);
  return -1;
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

// qkv [B, H + 2*KVH, D] (= [B, 3, H, D] when KVH = H), cache [2, B, KVH, L, D], R = H / KVH in
// {1, 2, 4, 8}. splits come from pra_mmha_splits(B, KVH, t) (the workgroup count is
// B*KVH*splits); ws: fp32 workspace of B*H*splits*(2 + D) + 4 floats (unused when splits == 1).
// seq_lens (device int32 [B]) and rot (device fp32 [2, B, D], rot_dims chunks) are optional.
// t / t_dev stay the batch-wide bound that the splits were sized for.
// cache_dt is dt for a float cache (scales null) or kCacheU8 for the 8-bit one: then scales is
// the packed device fp32 [4, Bs, KVH] (k quant, v quant, k dequant, v dequant) with
// scale_batch_stride 0 (Bs = 1) or KVH (Bs = B), round_type 1 (half away from zero) or 0 (half
// to even), and -128 <= qmin < qmax <= 127 the level bounds. Returns non-zero for a
// (dtype, cache dtype, head dim, ratio) without an instantiation.
int pra_mmha_decode(const void* qkv, void* cache, const float* mask, float* ws, void* out, int B, int H, int KVH,
                    int L, int D, int t, const int* t_dev, int splits, int mask_len, float scale, int dt,
                    const int* seq_lens, const float* rot, int rot_dims, hipStream_t s, int cache_dt,
                    const float* scales, int scale_batch_stride, int round_type, float qmax, float qmin) {
  const Args a{qkv, cache, mask, ws, out, B, H, KVH, L, t, t_dev, splits, mask_len, scale, seq_lens, rot,
               rot_dims, s, scales, scale_batch_stride, round_type, qmax, qmin, nullptr, 0, 0, 0, 1};
  return decode(a, D, dt, cache_dt);
}

// The same step over a paged cache: cache is the block pool [2, NB, KVH, BS, D] (the K plane,
// then the V plane; float or uint8 as above) and block_tables the device int32 [B, MB] table:
// entry j of row b is the physical block of logical positions [j*BS, (j+1)*BS) of sequence b.
// The logical capacity L = MB*BS takes the place of pra_mmha_decode's L in everything else
// (t, t_dev, seq_lens, mask_len, splits from pra_mmha_splits). Entries are not trusted: one
// outside [0, NB) is never made into an address; its keys carry weight 0, and a sequence whose
// own position lies in such a block gets zeros and no write. Returns non-zero when BS is not a
// power of two >= 16, block_tables is null, NB or MB < 1, MB*BS overflows, or for anything
// pra_mmha_decode refuses with L = MB*BS.
int pra_mmha_decode_paged(const void* qkv, void* cache, const float* mask, float* ws, void* out, int B, int H,
                          int KVH, int NB, int BS, int MB, int D, int t, const int* t_dev, int splits,
                          int mask_len, float scale, int dt, const int* seq_lens, const float* rot, int rot_dims,
                          hipStream_t s, int cache_dt, const float* scales, int scale_batch_stride, int round_type,
                          float qmax, float qmin, const int* block_tables) {
  if (!block_tables || BS < 16 || (BS & (BS - 1)) != 0 || NB < 1 || MB < 1 || (long long)MB * BS > 0x7fffffffLL)
    return -1;
  const int shift = __builtin_ctz((unsigned)BS);
  const Args a{qkv, cache, mask, ws, out, B, H, KVH, MB * BS, t, t_dev, splits, mask_len, scale, seq_lens, rot,
               rot_dims, s, scales, scale_batch_stride, round_type, qmax, qmin, block_tables, NB, MB, shift, 1};
  return decode(a, D, dt, cache_dt);
}

// n_tok new tokens per sequence in one pass over the cache, equal to n_tok consecutive
// single-token steps: qkv [B, n_tok, H + 2*KVH, D], out [B, n_tok, H, D]; token j of sequence b
// sits at position t_b + j, is appended there and attends to [0, t_b + j]. rot is
// [2, B, n_tok, D] (row j: the cos / sin of position t_b + j); the mask row is shared by the
// tokens. The arguments are pra_mmha_decode_paged's; a null block_tables means the contiguous
// cache [2, B, KVH, L, D] with L = MB*BS (NB unused, no condition on BS). splits come from
// pra_mmha_splits(B, KVH, t + n_tok - 1) (device position: L - 1) and ws holds
// B*n_tok*H*splits*(2 + D) + 4 floats. A sequence is guarded as a whole (n_tok zero rows, no
// write) when t_b < 0, t_b + n_tok > L, t_b exceeds the host bound t, the mask is shorter than
// t_b + n_tok, or (paged) the table entry of a block holding one of its new positions is outside
// [0, NB). Returns non-zero for n_tok < 1, for more than 8 query rows per K/V row
// ((H / KVH) * n_tok rounded up to a power of two > 8), and for everything the single-token
// entries refuse; n_tok = 1 is the single-token step.
int pra_mmha_decode_multi(const void* qkv, void* cache, const float* mask, float* ws, void* out, int B, int H,
                          int KVH, int NB, int BS, int MB, int D, int t, const int* t_dev, int splits,
                          int mask_len, float scale, int dt, const int* seq_lens, const float* rot, int rot_dims,
                          hipStream_t s, int cache_dt, const float* scales, int scale_batch_stride, int round_type,
                          float qmax, float qmin, const int* block_tables, int n_tok) {
  if (n_tok < 1 || BS < 1 || MB < 1 || (long long)MB * BS > 0x7fffffffLL) return -1;
  if (block_tables && (BS < 16 || (BS & (BS - 1)) != 0 || NB < 1)) return -1;
  const int shift = block_tables ? __builtin_ctz((unsigned)BS) : 0;
  const Args a{qkv, cache, mask, ws, out, B, H, KVH, MB * BS, t, t_dev, splits, mask_len, scale, seq_lens, rot,
               rot_dims, s, scales, scale_batch_stride, round_type, qmax, qmin, block_tables,
               block_tables ? NB : 0, MB, shift, n_tok};
  return decode(a, D, dt, cache_dt);
}
}
