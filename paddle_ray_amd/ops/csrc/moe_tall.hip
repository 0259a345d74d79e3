// Top-k routed mixture-of-experts FFN for prefill sizes on gfx950: the operation of moe_ffn.hip
//   out[m] = sum_j w[m, j] * (act(x[m] . W1[e_j] + b1[e_j]) . W2[e_j] + b2[e_j]),  e_j = ids[m, j]
// for any number of tokens up to kMaxPairs = 16384 (token, slot) pairs per call, with the same
// operands: E <= 256, k <= 8, D % 64 == 0, F % 64 == 0; x / W / b / out bf16 or f16; W1 [E, D, N1]
// and W2 [E, F, D] k-major, n contiguous; N1 = 2F for SwiGLU, F for GELU / ReLU.
//
// moe_ffn.hip is built for an expert that sees a handful of rows: weights are the MFMA "A" operand,
// every workgroup walks all rows of its expert (at most 64) and the call is bound by the weight
// stream. Here an expert sees tens to thousands of rows and the products are compute-bound, so the
// work is cut into row tiles of TM = 128 sorted rows of one expert, the grid is
// (row tiles, channel slabs), and a workgroup is a 128 x 128 GEMM tile over all of K with both
// operands double-buffered in LDS. Six kernels; as in moe_ffn.hip there is no host sync, no atomic,
// no grid that depends on the routing and every sum has a fixed order, so a call is bitwise
// reproducible and can be captured into a graph. A token's result does not depend on the tile or the
// row it lands in: an MFMA column is one row of x, and rows meet only in the token's own combine.
//
// Index, a stable counting sort of the P = M * k pairs by expert in three steps:
//   moe_tall_hist   one workgroup per block of 1024 pairs: the ids go to LDS, thread e counts its
//                   pairs, hist[block][e];
//   moe_tall_scan   one workgroup: thread e turns its column of hist into running starts, one thread
//                   scans the E totals (off[E + 1] and the first row tile of every expert), thread e
//                   adds its offset to its column and writes its entries of the row-tile table:
//                   ceil(cnt_e / TM) triples (expert, first sorted row, rows), the tile count behind
//                   the last possible triple. sum ceil(cnt_e / TM) <= P / TM + E bounds the table
//                   and is the grid's x extent; a workgroup past the count returns at once;
//   moe_tall_place  the blocks again: thread e walks the block's ids in ascending pair index from
//                   hist[block][e], so the order inside an expert is the stable one: sorted[P] and
//                   its inverse pos[P].
//
// moe_tall_gemm (both products), 4 waves as 2 x 2, a wave owns 64 rows x 64 channels = 2 x 2
// accumulators of v_mfma_f32_32x32x16 (weights are "A", so a lane ends with groups of 4 consecutive
// channels of one row). For SwiGLU the 128 image columns are 64 channels n and the 64 channels
// n + F, a wave takes 32 of each, and gate and up meet in registers. Per stage of 64 k:
//   rows     128 rows x 64 k, 16 bytes per lane and load, gathered by row (sorted[s] / k for the first
//            product, h[s] for the second; rows past the tile's count are zeros), written to the
//            swizzled image of mfma_frag.h (swz<64>) and read back as row fragments (frag_rows);
//   weights  [64 k x 128 n], 16 lanes covering the 256 (SwiGLU: 2 x 128) contiguous bytes of one k
//            row, written to swz<128> and read back k-contiguous per channel with ds_read_b64_tr_b16
//            (frag_tr). frag_tr hands out k in the order 0..3, 8..11 | 4..7, 12..15 of a 16-k step;
//            the image rows are free to choose when a k row is written, so k row kr goes to image
//            row kr with bits 2 and 3 swapped and both operands see k in natural order;
//   both images twice: the next stage's global loads are issued into registers before the stage's
//   MFMAs and stored to the other buffer after them, one barrier per stage. LDS is exactly 64 KB.
// A wave skips its 32-row blocks past the tile's count (wave-uniform). Epilogues as in moe_ffn.hip:
// bias, activation, h in the model dtype at sorted position s; the second product stores fp32 to
// ws[s, D]. moe_combine (moe_common.h) ends the call.
//
// Where this differs from the plan it was written to: the row tile is blockIdx.x and the channel
// slab blockIdx.y, so workgroups that are dispatched next to each other are the row tiles of one
// expert over the same weight slab, which they then share in L2 / MALL. There is one TM; a tile of
// a lightly loaded expert pays for its empty 32-row blocks in LDS traffic only. The epilogue stores
// straight from the accumulators (16 / 8 bytes per lane, 32-byte runs per row and instruction); a
// transpose through LDS for full-line stores was not tried.
#include "mfma_frag.h"
#include "moe_common.h"
#include "pra_api.h"

namespace pra {
namespace moe {

constexpr int kMaxPairs = 16384, kSortBlock = 1024;
constexpr int kTM = 128, kStage = 64;

// ---------------------------------------------------------------------------------------- index
__global__ __launch_bounds__(kThreads) void moe_tall_hist_kernel(const int* __restrict__ ids, int* __restrict__ hist,
                                                                 int P, int E) {
  __shared__ __attribute__((aligned(16))) int sid[kSortBlock];
  const int tid = threadIdx.x, p0 = blockIdx.x * kSortBlock, n = min(kSortBlock, P - p0);
  for (int p = tid; p < kSortBlock; p += kThreads) sid[p] = p < n ? clamp_id(ids[p0 + p], E) : -1;
  __syncthreads();
  if (tid < E) {
    int c = 0;
    for (int p = 0; p < n; p += 4) {                   // 4 ids per LDS read; the tail holds -1
      const int4 v = *reinterpret_cast<const int4*>(sid + p);
      c += (v.x == tid ? 1 : 0) + (v.y == tid ? 1 : 0) + (v.z == tid ? 1 : 0) + (v.w == tid ? 1 : 0);
    }
    hist[blockIdx.x * E + tid] = c;
  }
}

__global__ __launch_bounds__(kThreads) void moe_tall_scan_kernel(int* __restrict__ hist, int* __restrict__ off,
                                                                 int* __restrict__ tiles, int NB, int E, int maxT) {
  __shared__ int cnt[kMaxExperts], base[kMaxExperts], tile0[kMaxExperts];
  const int tid = threadIdx.x;
  if (tid < E) {
    int run = 0;
    for (int b = 0; b < NB; ++b) {
      const int c = hist[b * E + tid];
      hist[b * E + tid] = run;
      run += c;
    }
    cnt[tid] = run;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0, t = 0;
    for (int e = 0; e < E; ++e) {
      base[e] = run;
      tile0[e] = t;
      run += cnt[e];
      t += (cnt[e] + kTM - 1) / kTM;
    }
    off[E] = run;
    tiles[3 * maxT] = min(t, maxT);
  }
  __syncthreads();
  if (tid < E) {
    const int o = base[tid], c = cnt[tid];
    off[tid] = o;
    for (int b = 0; b < NB; ++b) hist[b * E + tid] += o;
    for (int i = 0, t = tile0[tid]; i * kTM < c && t < maxT; ++i, ++t) {
      tiles[3 * t] = tid;
      tiles[3 * t + 1] = o + i * kTM;
      tiles[3 * t + 2] = min(kTM, c - i * kTM);
    }
  }
}

__global__ __launch_bounds__(kThreads) void moe_tall_place_kernel(const int* __restrict__ ids,
                                                                  const int* __restrict__ hist,
                                                                  int* __restrict__ sorted, int* __restrict__ pos,
                                                                  int P, int E) {
  __shared__ __attribute__((aligned(16))) int sid[kSortBlock];
  const int tid = threadIdx.x, p0 = blockIdx.x * kSortBlock, n = min(kSortBlock, P - p0);
  for (int p = tid; p < kSortBlock; p += kThreads) sid[p] = p < n ? clamp_id(ids[p0 + p], E) : -1;
  __syncthreads();
  if (tid < E) {
    int s = hist[blockIdx.x * E + tid];
    for (int p = 0; p < n; p += 4) {                   // 4 ids per LDS read; the tail holds -1
      const int4 v = *reinterpret_cast<const int4*>(sid + p);
      const int id[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (id[j] == tid && s < P) {
          sorted[s] = p0 + p + j;
          pos[p0 + p + j] = s;
          ++s;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- products
// a: x [M, K] (topk > 0: the row of sorted position s is sorted[s] / topk) or h [P, K] (topk == 0: row
// s). w [E, K, NT], bias [E, NT] or null. EPI 0: ws[s, N] fp32 (NT == N); kGelu / kRelu: h[s, N]
// (NT == N); kSwiglu: h[s, N] from channels n and n + N of NT == 2N. K % 64 == 0, N % 64 == 0.
template <typename T, int EPI>
__global__ __launch_bounds__(kThreads) void moe_tall_gemm_kernel(const uint16_t* __restrict__ a,
                                                                 const uint16_t* __restrict__ w,
                                                                 const uint16_t* __restrict__ bias,
                                                                 const int* __restrict__ tiles,
                                                                 const int* __restrict__ sorted, int topk,
                                                                 uint16_t* __restrict__ h, float* __restrict__ ws,
                                                                 int K, int N, int NT, int maxT) {
  constexpr bool GLU = EPI == kSwiglu;
  constexpr int IMG = kStage * kTM;                    // elements of one image, rows or weights
  __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][IMG];   // [buffer][rows | weights]

  const int ti = blockIdx.x;
  if (ti >= tiles[3 * maxT]) return;                   // workgroup-uniform: past the tile count
  const int e = tiles[3 * ti], first = tiles[3 * ti + 1], cnt = tiles[3 * ti + 2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int n0 = blockIdx.y * (GLU ? 64 : 128);

  // staging roles. rows: lane chunk ac of rows (tid >> 3) + 32 i; weights: chunk wc of k rows
  // (tid >> 4) + 16 i, image row = k row with bits 2 and 3 swapped
  const int ac = tid & 7, ar = tid >> 3, wc = tid & 15, wk = tid >> 4;
  const int xoff = fa::swz<kStage>(ar, ac);
  const int woff = fa::swz<kTM>((wk & 3) | ((wk & 4) << 1) | ((wk & 8) >> 1), wc);
  const int wcol = GLU ? (wc < 8 ? n0 + wc * 8 : N + n0 + (wc - 8) * 8) : n0 + wc * 8;
  const bool wok = GLU || wcol < N;
  const uint16_t* ap[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ar + 32 * i;
    ap[i] = nullptr;
    if (r < cnt) ap[i] = a + (size_t)(topk > 0 ? sorted[first + r] / topk : first + r) * K + ac * 8;
  }
  const uint16_t* wp = w + (size_t)e * K * NT + (size_t)wk * NT + wcol;

  const fa::LaneOffs<kStage> lx(lane);
  const fa::LaneOffs<kTM> lw(lane);
  const bool on[2] = {wm * 64 < cnt, wm * 64 + 32 < cnt};

  fa::f32x16 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][mb][i] = 0.f;

  u32x4 ra[4], rw[4];
#define PRA_MOE_FETCH(ks)                                                                             \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                     \
    ra[i] = u32x4{0u, 0u, 0u, 0u};                                                                    \
    rw[i] = u32x4{0u, 0u, 0u, 0u};                                                                    \
    if (ap[i]) ra[i] = *reinterpret_cast<const u32x4*>(ap[i] + (ks));                                 \
    if (wok) rw[i] = *reinterpret_cast<const u32x4*>(wp + (size_t)((ks) + 16 * i) * NT);              \
  }
#define PRA_MOE_STASH(b)                                                                              \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                     \
    *reinterpret_cast<u32x4*>(&lds[b][0][xoff + i * 32 * kStage]) = ra[i];                            \
    *reinterpret_cast<u32x4*>(&lds[b][1][woff + i * 16 * kTM]) = rw[i];                               \
  }

  PRA_MOE_FETCH(0)
  PRA_MOE_STASH(0)
  __syncthreads();
  for (int ks = 0, b = 0; ks < K; ks += kStage, b ^= 1) {
    const bool more = ks + kStage < K;
    if (more) { PRA_MOE_FETCH(ks + kStage) }
    const T* ximg = reinterpret_cast<const T*>(lds[b][0]);
    const T* wimg = reinterpret_cast<const T*>(lds[b][1]);
#pragma unroll
    for (int S = 0; S < kStage / 16; ++S) {
      const typename fa::V8<T>::type w0 = fa::frag_tr<T, kTM>(wimg, lw, wn, S);
      const typename fa::V8<T>::type w1 = fa::frag_tr<T, kTM>(wimg, lw, wn + 2, S);
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        if (on[mb]) {
          const typename fa::V8<T>::type xb = fa::frag_rows<T, kStage>(ximg, lx, wm * 2 + mb, S);
          acc[0][mb] = fa::mfma<T>(w0, xb, acc[0][mb]);
          acc[1][mb] = fa::mfma<T>(w1, xb, acc[1][mb]);
        }
      }
    }
    if (more) { PRA_MOE_STASH(b ^ 1) }
    __syncthreads();
  }
#undef PRA_MOE_FETCH
#undef PRA_MOE_STASH

  // accumulator register 4g + j of lane (r, hh): row r of the block, channel 8g + 4hh + j of the 32
  const int r = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int row = wm * 64 + mb * 32 + r;
    if (row >= cnt) continue;
    const size_t s = (size_t)(first + row);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 8 * g + 4 * hh;
      if (GLU) {
        const int n = n0 + 32 * wn + c;
        f32x4 bg = f32x4{0.f, 0.f, 0.f, 0.f}, bu = bg;
        if (bias) {
          bg = load4<T>(bias + (size_t)e * NT + n);
          bu = load4<T>(bias + (size_t)e * NT + N + n);
        }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = acc[0][mb][4 * g + j] + bg[j];
          o[j] = v / (1.f + __expf(-v)) * (acc[1][mb][4 * g + j] + bu[j]);
        }
        store4<T>(h + s * N + n, o);
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int n = n0 + 32 * (wn + 2 * t) + c;
          if (n >= N) continue;
          if (EPI == 0) {
            *reinterpret_cast<f32x4*>(ws + s * N + n) = f32x4{acc[t][mb][4 * g], acc[t][mb][4 * g + 1],
                                                              acc[t][mb][4 * g + 2], acc[t][mb][4 * g + 3]};
          } else {
            f32x4 bs = f32x4{0.f, 0.f, 0.f, 0.f};
            if (bias) bs = load4<T>(bias + (size_t)e * NT + n);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float v = acc[t][mb][4 * g + j] + bs[j];
              o[j] = EPI == kGelu ? gelu_erf_fast(v) : fmaxf(v, 0.f);
            }
            store4<T>(h + s * N + n, o);
          }
        }
      }
    }
  }
}

template <typename T, int EPI>
void launch_tall_gemm(int maxT, hipStream_t s, const uint16_t* a, const uint16_t* w, const uint16_t* bias,
                      const int* tiles, const int* sorted, int topk, uint16_t* h, float* ws, int K, int N, int NT) {
  const dim3 grid(maxT, EPI == kSwiglu ? N / 64 : (N + 127) / 128);
  hipLaunchKernelGGL((moe_tall_gemm_kernel<T, EPI>), grid, dim3(kThreads), 0, s, a, w, bias, tiles, sorted, topk, h,
                     ws, K, N, NT, maxT);
}

template <typename T>
void launch_tall(const void* x, const int* ids, const float* tw, const void* w1, const void* b1, const void* w2,
                 const void* b2, void* out, void* h, float* ws, int* idx, int M, int D, int F, int E, int k, int act,
                 hipStream_t s) {
  const int P = M * k, NB = (P + kSortBlock - 1) / kSortBlock, maxT = P / kTM + E;
  int* off = idx;
  int* hist = off + E + 1;
  int* sorted = hist + NB * E;
  int* pos = sorted + P;
  int* tiles = pos + P;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* w1p = static_cast<const uint16_t*>(w1);
  const uint16_t* b1p = static_cast<const uint16_t*>(b1);
  uint16_t* hp = static_cast<uint16_t*>(h);
  hipLaunchKernelGGL(moe_tall_hist_kernel, dim3(NB), dim3(kThreads), 0, s, ids, hist, P, E);
  hipLaunchKernelGGL(moe_tall_scan_kernel, dim3(1), dim3(kThreads), 0, s, hist, off, tiles, NB, E, maxT);
  hipLaunchKernelGGL(moe_tall_place_kernel, dim3(NB), dim3(kThreads), 0, s, ids, hist, sorted, pos, P, E);
  if (act == kSwiglu) launch_tall_gemm<T, kSwiglu>(maxT, s, xp, w1p, b1p, tiles, sorted, k, hp, nullptr, D, F, 2 * F);
  else if (act == kGelu) launch_tall_gemm<T, kGelu>(maxT, s, xp, w1p, b1p, tiles, sorted, k, hp, nullptr, D, F, F);
  else launch_tall_gemm<T, kRelu>(maxT, s, xp, w1p, b1p, tiles, sorted, k, hp, nullptr, D, F, F);
  launch_tall_gemm<T, 0>(maxT, s, hp, static_cast<const uint16_t*>(w2), nullptr, tiles, sorted, 0, nullptr, ws, F, D,
                         D);
  hipLaunchKernelGGL((moe_combine_kernel<T>), dim3(M), dim3(kThreads), 0, s, ws, pos, ids, tw,
                     static_cast<const uint16_t*>(b2), static_cast<uint16_t*>(out), D, E, k);
}

}  // namespace moe
}  // namespace pra

extern "C" {

// pra_moe_ffn (moe_ffn.hip) for any number of tokens: out[M, D] of the routed FFN with the same
// operands, layouts, alignment, activations and clamping of ids, for M >= 1 with P = M*k <= 16384
// pairs per call (the caller cuts taller inputs into row chunks: tokens are independent). Workspaces,
// all written before they are read: h holds P*F values of dt, ws P*D floats, idx
//   (E + 1) + ceil(P / 1024)*E + 2*P + 3*(P / 128 + E) + 1 ints
// (off, the per-block histogram, sorted, pos, the row-tile table and its count; P / 128 rounds
// down). Returns non-zero without launching for P > 16384, E outside [1, 256], k outside
// [1, min(8, E)], D % 64, F % 64, another act / dt or a missing pointer.
int pra_moe_ffn_tall(const void* x, const int* ids, const float* tw, const void* w1, const void* b1, const void* w2,
                     const void* b2, void* out, void* h, float* ws, int* idx, int M, int D, int F, int E, int k,
                     int act, int dt, hipStream_t s) {
  if (!pra::moe::limits_ok(M, D, E, k) || M > pra::moe::kMaxPairs / k || F < 64 || F % 64) return 1;
  if (act != pra::moe::kGelu && act != pra::moe::kRelu && act != pra::moe::kSwiglu) return 1;
  if (!x || !ids || !tw || !w1 || !w2 || !out || !h || !ws || !idx) return 1;
  if (dt == pra::kBF16)
    pra::moe::launch_tall<pra::bf16>(x, ids, tw, w1, b1, w2, b2, out, h, ws, idx, M, D, F, E, k, act, s);
  else if (dt == pra::kF16)
    pra::moe::launch_tall<pra::f16>(x, ids, tw, w1, b1, w2, b2, out, h, ws, idx, M, D, F, E, k, act, s);
  else return 1;
  return 0;
}

}  // extern "C"
