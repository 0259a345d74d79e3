// Top-k routed mixture-of-experts FFN for decode steps on gfx950:
//   l[m, :]  = x[m, :] . gate_weight                      (fp32 [D, E])
//   ids, w   = the k largest logits of a token (ties to the lower expert) and softmax(l) there
//   out[m]   = sum_j w[m, j] * (act(x[m] . W1[e_j] + b1[e_j]) . W2[e_j] + b2[e_j]),  e_j = ids[m, j]
//   1 <= M <= 64 tokens, E <= 256 experts, k <= 8, D % 64 == 0, F % 64 == 0; x / W / b / out bf16 or
//   f16; W1 [E, D, N1] and W2 [E, F, D] in the reference layout (k-major, n contiguous), N1 = 2F for
//   SwiGLU (first half through silu) and F for GELU / ReLU.
//
// With 8..64 tokens and top-2..8 of 8..64 experts an active expert sees one to a handful of rows, so
// the step is bound by the HBM read of the chosen experts' weights, exactly the regime of
// wo_gemm.hip, and the two products reuse its arrangement: weights as the MFMA "A" operand, the few
// rows of x as "B" (v_mfma_f32_16x16x32: lane l gives 8 k at 8*(l/16) of row / column l%16 and gets
// rows 4*(l/16) .. +3 of column l%16, i.e. 4 consecutive channels of one token row).
//
// Five kernels, no host sync, no atomics, every step in a fixed order (a call is bitwise
// reproducible and can be captured into a graph; the grids never depend on the routing):
//
// moe_route, one workgroup per token. Thread (g, e) adds x[m, d] * gate[d, e] over d = g, g + G, ..
// (G = 256 / pow2 >= E groups), thread e adds the G partial sums in index order. The rank of expert e
// is the number of experts that beat it (larger logit, or equal logit and lower index): ranks are a
// permutation, rank < k is selected and rank is its slot, which is the order of a stable descending
// sort. Weights are exp2((l - max) * log2 e) with the rounding of the product carried as a first-order
// correction, over their sum (a fixed tree), then over the sum of the k selected in slot order. A NaN
// logit makes the sum and so every weight of the row NaN; ids are clamped into [0, E).
//
// moe_index, one workgroup: counting sort of the P = M*k (token, slot) pairs by expert. Thread e
// counts its pairs in LDS, one thread scans the E counts, thread e writes its pairs in ascending
// index: off[E + 1], sorted_pair[P] and its inverse pos[P].
//
// moe_gemm (both products), grid = (N / 64, E). A workgroup whose expert has no rows returns at
// once, so the weight bytes of an unselected expert are never read and those of a selected one are
// read exactly once. Otherwise 4 waves = 4 tiles of 16 channels over all of K, per stage of 256 k
// (128 above 32 rows; halved for SwiGLU, which carries two channel sets n and n + F):
//   1. the stage's weights [stage k x 64 n] go from HBM to registers, 16 bytes per lane and load, 8
//      lanes covering the 128 contiguous bytes of one k row, all loads issued before the barrier;
//   2. after the barrier the expert's rows of x (gathered by sorted_pair[s] / k for the first product,
//      h[off[e] + r] for the second; rows past the count zeroed) go to LDS at pitch stage + 8 as in
//      wo_gemm, and the weight registers to an LDS image [k][64 n] whose 32-byte channel-tile
//      segments are XOR-ed with k & 3;
//   3. a wave reads its tile back k-contiguous per channel with two ds_read_b64_tr_b16 per MFMA step
//      (lane 4i + p of a 16-lane group addresses k row i, channels 4p .. 4p + 3, and receives its own
//      channel at the 4 rows; the XOR puts the 4 rows of a group in different banks) and runs the
//      MFMAs of up to ceil(M / 16) row blocks (template bound), skipping blocks past the expert's
//      count by a wave-uniform test.
// Epilogue of the first product: bias, then erf GELU / ReLU / silu(gate) * up, h stored in the model
// dtype at the sorted position s ([P, F], so the second product reads contiguous rows). The second
// stores fp32 to the workspace [P, D] at s, without bias or routing weight.
//
// moe_combine, one workgroup per token: out[m] = sum_j w[m, j] * (ws[pos[m*k + j]] + b2[ids[m, j]]) in
// slot order, in fp32, rounded once.
//
// Where this differs from the per-wave plan of loading [64 k x 16 n] pieces: the four waves load the
// workgroup's [k x 64 n] piece together, so a load instruction covers whole 128-byte lines instead of
// 32-byte quarters of 32 different lines, and the image is written in the staging phase the x rows
// need anyway (no extra barrier). The transpose is the LDS one (ds_read_b64_tr_b16), a register
// transpose was not tried. There is no split over K: at decode sizes the grid is already
// slabs x active experts; a split (with a slice reduction in moe_combine) is future work for small
// F with few active experts. ids handed to moe_ffn must name an expert at most once per token (what
// moe_route returns); rows of an expert past 64 would be left uncomputed, never out of bounds.
#include "moe_common.h"
#include "pra_api.h"

namespace pra {
namespace moe {

typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;

template <typename T>
__device__ __forceinline__ f32x4 mma(typename V8<T>::type a, typename V8<T>::type b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mma<bf16>(V8<bf16>::type a, V8<bf16>::type b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mma<f16>(V8<f16>::type a, V8<f16>::type b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------- route
template <typename T>
__global__ __launch_bounds__(kThreads) void moe_route_kernel(const uint16_t* __restrict__ x,
                                                             const float* __restrict__ gw, int* __restrict__ ids,
                                                             float* __restrict__ tw, int D, int E, int k,
                                                             int norm) {
  __shared__ float part[kThreads], lg[kThreads], pr[kThreads];
  __shared__ int sel[kMaxTopK];
  __shared__ float sw[kMaxTopK];
  const int m = blockIdx.x, tid = threadIdx.x;
  int Ep = 1;
  while (Ep < E) Ep <<= 1;
  const int G = kThreads / Ep, g = tid / Ep, e = tid % Ep;
  float a = 0.f;
  if (e < E) {
    for (int d = g; d < D; d += G) a = fmaf(to_f32<T>(x[(size_t)m * D + d]), gw[(size_t)d * E + e], a);
  }
  part[tid] = a;
  if (tid < kMaxTopK) {
    sel[tid] = 0;
    sw[tid] = __builtin_nanf("");               // a slot no rank reaches (NaN logits) stays NaN
  }
  __syncthreads();
  if (tid < E) {
    float s = part[tid];
    for (int i = 1; i < G; ++i) s += part[i * Ep + tid];
    lg[tid] = s;
  }
  __syncthreads();
  const float mine = tid < E ? lg[tid] : 0.f;
  int rank = kMaxTopK;
  if (tid < E) {
    rank = 0;
    for (int j = 0; j < E; ++j) {
      const float o = lg[j];
      rank += (o > mine || (o == mine && j < tid)) ? 1 : 0;
    }
    if (rank < k) sel[rank] = tid;
  }
  __syncthreads();
  // exp(t) = exp2(y + r), y = fl(t * hi), r = the product's rounding error plus t * lo, hi + lo = log2 e
  float p = 0.f;
  if (tid < E) {
    const float t = mine - lg[sel[0]], hi = 1.44269502162933349609375f, lo = 1.925963033500e-8f;
    const float y = t * hi, r = fmaf(t, lo, fmaf(t, hi, -y));
    p = __builtin_amdgcn_exp2f(y) * fmaf(r, 0.693147180559945f, 1.f);
  }
  pr[tid] = p;
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if (tid < st) pr[tid] += pr[tid + st];
    __syncthreads();
  }
  if (rank < k) sw[rank] = p / pr[0];
  __syncthreads();
  if (tid < k) {
    float v = sw[tid];
    if (norm) {
      float s = sw[0];
      for (int j = 1; j < k; ++j) s += sw[j];
      v = v / s;
    }
    ids[m * k + tid] = clamp_id(sel[tid], E);
    tw[m * k + tid] = v;
  }
}

// ---------------------------------------------------------------------------------------- products
// a: x [M, K] (topk > 0: the row of sorted position s is sorted[s] / topk) or h [P, K] (topk == 0: row
// s). w [E, K, NT], bias [E, NT] or null. EPI 0: ws[s, N] fp32 (NT == N); kGelu / kRelu: h[s, N]
// (NT == N); kSwiglu: h[s, N] from channels n and n + N of NT == 2N. MB = row blocks of 16.
template <typename T, int MB, int EPI>
__global__ __launch_bounds__(kThreads) void moe_gemm_kernel(const uint16_t* __restrict__ a,
                                                            const uint16_t* __restrict__ w,
                                                            const uint16_t* __restrict__ bias,
                                                            const int* __restrict__ off,
                                                            const int* __restrict__ sorted, int topk,
                                                            uint16_t* __restrict__ h, float* __restrict__ ws, int K,
                                                            int N, int NT) {
  constexpr int NS = EPI == kSwiglu ? 2 : 1;          // channel sets
  constexpr int SK = (MB <= 2 ? 256 : 128) / NS;      // k per stage
  constexpr int SC = SK / 64, LDX = SK + 8, ROWS = MB * 16;
  constexpr int PER = SK / 32, NW = PER * NS;         // 16-byte weight registers per set / per stage
  typedef typename V8<T>::type v8;
  __shared__ __attribute__((aligned(16))) uint16_t xs[ROWS * LDX];
  __shared__ __attribute__((aligned(16))) uint16_t wimg[NS * SK * 64];
  __shared__ int rows[ROWS];

  const int e = blockIdx.y, base = off[e], cnt = min(off[e + 1] - base, ROWS);
  if (cnt <= 0) return;                               // workgroup-uniform: an expert nobody chose
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cm = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 64, nrows = ((cnt + 15) >> 4) << 4;
  if (tid < ROWS) rows[tid] = tid < cnt ? (topk > 0 ? sorted[base + tid] / topk : base + tid) : -1;
  // transposed read: lane 4i + p of group q addresses k row 8q + i, channels 16 wv + 4p .. + 3
  const int ti = (lane >> 2) & 3, toff = (8 * q + ti) * 64 + ((wv ^ ti) << 4) + 4 * (lane & 3);
  const uint16_t* wp = w + (size_t)e * K * NT + n0;

  f32x4 acc[NS][MB];
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[t][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int ks = 0; ks < K; ks += SK) {
    // 1. every weight byte of the stage, in flight before the staging barrier
    u32x4 wr[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int i = (j % PER) * kThreads + tid, kr = i >> 3, c = i & 7;
      wr[j] = u32x4{0u, 0u, 0u, 0u};
      if (ks + kr < K)
        wr[j] = *reinterpret_cast<const u32x4*>(wp + (size_t)(ks + kr) * NT + (j / PER) * N + c * 8);
    }
    // 2. the expert's rows of the stage (zeros past the count and past K) and the weight image -> LDS
    __syncthreads();
    for (int u = tid; u < nrows * SC * 8; u += kThreads) {
      const int row = u / (SC * 8), cc = u % (SC * 8), k = ks + cc * 8, r = rows[row];
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (r >= 0 && k < K) v = *reinterpret_cast<const uint4*>(a + (size_t)r * K + k);
      *reinterpret_cast<uint4*>(xs + row * LDX + cc * 8) = v;
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int i = (j % PER) * kThreads + tid, kr = i >> 3, c = i & 7;
      *reinterpret_cast<u32x4*>(wimg + (j / PER) * SK * 64 + kr * 64 + ((((c >> 1) ^ (kr & 3)) << 1) + (c & 1)) * 8) =
          wr[j];
    }
    __syncthreads();
    // 3. transposed weight fragments -> MFMA over the expert's row blocks
#pragma unroll
    for (int j = 0; j < SC; ++j) {
      if (ks + j * 64 < K) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int kk = j * 64 + s * 32;
          v8 wa[NS];
#pragma unroll
          for (int t = 0; t < NS; ++t) {
            const uint16_t* pa = wimg + t * SK * 64 + kk * 64 + toff;
            const u32x2 lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)pa));
            const u32x2 hi =
                __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(pa + 4 * 64)));
            wa[t] = __builtin_bit_cast(v8, u32x4{lo[0], lo[1], hi[0], hi[1]});
          }
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) {
            if (mb * 16 < cnt) {
              const v8 b = *reinterpret_cast<const v8*>(xs + (mb * 16 + cm) * LDX + kk + q * 8);
#pragma unroll
              for (int t = 0; t < NS; ++t) acc[t][mb] = mma<T>(wa[t], b, acc[t][mb]);
            }
          }
        }
      }
    }
  }

  const int n = n0 + wv * 16 + q * 4;
  f32x4 bs[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) {
    bs[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (EPI != 0 && bias) bs[t] = load4<T>(bias + (size_t)e * NT + t * N + n);
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int r = mb * 16 + cm;
    if (r >= cnt) continue;
    const size_t s = (size_t)(base + r);
    if (EPI == 0) {
      *reinterpret_cast<f32x4*>(ws + s * N + n) = acc[0][mb];
    } else {
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = acc[0][mb][i] + bs[0][i];
        if (EPI == kGelu) o[i] = gelu_erf_fast(v);
        else if (EPI == kRelu) o[i] = fmaxf(v, 0.f);
        else o[i] = v / (1.f + __expf(-v)) * (acc[NS - 1][mb][i] + bs[NS - 1][i]);
      }
      store4<T>(h + s * N + n, o);
    }
  }
}

template <typename T, int EPI>
void launch_gemm(int mb, dim3 grid, hipStream_t s, const uint16_t* a, const uint16_t* w, const uint16_t* bias,
                 const int* off, const int* sorted, int topk, uint16_t* h, float* ws, int K, int N, int NT) {
#define PRA_MOE_MB(MB)                                                                                          \
  case MB:                                                                                                      \
    hipLaunchKernelGGL((moe_gemm_kernel<T, MB, EPI>), grid, dim3(kThreads), 0, s, a, w, bias, off, sorted, topk, \
                       h, ws, K, N, NT);                                                                        \
    break;
  switch (mb) {
    PRA_MOE_MB(1)
    PRA_MOE_MB(2)
    PRA_MOE_MB(3)
    PRA_MOE_MB(4)
  }
#undef PRA_MOE_MB
}

template <typename T>
void launch_ffn(const void* x, const int* ids, const float* tw, const void* w1, const void* b1, const void* w2,
                const void* b2, void* out, void* h, float* ws, int* idx, int M, int D, int F, int E, int k, int act,
                hipStream_t s) {
  const int P = M * k, mb = (M + 15) / 16;
  int* off = idx;
  int* sorted = idx + E + 1;
  int* pos = sorted + P;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* w1p = static_cast<const uint16_t*>(w1);
  const uint16_t* b1p = static_cast<const uint16_t*>(b1);
  uint16_t* hp = static_cast<uint16_t*>(h);
  hipLaunchKernelGGL(moe_index_kernel<kMaxRows * kMaxTopK>, dim3(1), dim3(kThreads), 0, s, ids, off, sorted, pos, P, E);
  const dim3 g1(F / 64, E), g2(D / 64, E);
  if (act == kSwiglu) launch_gemm<T, kSwiglu>(mb, g1, s, xp, w1p, b1p, off, sorted, k, hp, nullptr, D, F, 2 * F);
  else if (act == kGelu) launch_gemm<T, kGelu>(mb, g1, s, xp, w1p, b1p, off, sorted, k, hp, nullptr, D, F, F);
  else launch_gemm<T, kRelu>(mb, g1, s, xp, w1p, b1p, off, sorted, k, hp, nullptr, D, F, F);
  launch_gemm<T, 0>(mb, g2, s, hp, static_cast<const uint16_t*>(w2), nullptr, off, sorted, 0, nullptr, ws, F, D, D);
  hipLaunchKernelGGL((moe_combine_kernel<T>), dim3(M), dim3(kThreads), 0, s, ws, pos, ids, tw,
                     static_cast<const uint16_t*>(b2), static_cast<uint16_t*>(out), D, E, k);
}

}  // namespace moe
}  // namespace pra

extern "C" {

// ids[M, k] (int32) and tw[M, k] (fp32) of x[M, D] (`dt`, f16 / bf16) under gate_weight[D, E] (fp32):
// the k largest logits in the order of a stable descending sort, softmax over all E at those, divided
// by their own sum when norm != 0. One workgroup per token, so any M whose M * k indexes as an int:
// returns non-zero without launching for M outside [1, 2^27], E outside [1, 256], k outside
// [1, min(8, E)], D % 64, another dt or a missing pointer.
int pra_moe_route(const void* x, const float* gate_weight, int* ids, float* tw, int M, int D, int E, int k, int norm,
                  int dt, hipStream_t s) {
  if (!pra::moe::limits_ok(M, D, E, k) || M > (1 << 27) || !x || !gate_weight || !ids || !tw) return 1;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  if (dt == pra::kBF16)
    hipLaunchKernelGGL((pra::moe::moe_route_kernel<pra::bf16>), dim3(M), dim3(pra::moe::kThreads), 0, s, xp,
                       gate_weight, ids, tw, D, E, k, norm);
  else if (dt == pra::kF16)
    hipLaunchKernelGGL((pra::moe::moe_route_kernel<pra::f16>), dim3(M), dim3(pra::moe::kThreads), 0, s, xp,
                       gate_weight, ids, tw, D, E, k, norm);
  else return 1;
  return 0;
}

// out[M, D] of the routed FFN described at the top of this file. x, w1 [E, D, N1], b1 [E, N1]
// (optional), w2 [E, F, D], b2 [E, D] (optional) and out are `dt` (f16 / bf16), contiguous and 16-byte
// aligned; ids / tw [M, k] as pra_moe_route returns them (an id outside [0, E) is clamped); act 1 erf
// GELU, 3 ReLU (N1 = F), 4 SwiGLU (N1 = 2F). Workspaces, all written before they are read: h holds
// M*k*F values of dt, ws M*k*D floats, idx E + 1 + 2*M*k ints. Returns non-zero without launching
// for M > 64, the other limits of pra_moe_route, F % 64, another act / dt or a missing pointer.
int pra_moe_ffn(const void* x, const int* ids, const float* tw, const void* w1, const void* b1, const void* w2,
                const void* b2, void* out, void* h, float* ws, int* idx, int M, int D, int F, int E, int k, int act,
                int dt, hipStream_t s) {
  if (!pra::moe::limits_ok(M, D, E, k) || M > pra::moe::kMaxRows || F < 64 || F % 64) return 1;
  if (act != pra::moe::kGelu && act != pra::moe::kRelu && act != pra::moe::kSwiglu) return 1;
  if (!x || !ids || !tw || !w1 || !w2 || !out || !h || !ws || !idx) return 1;
  if (dt == pra::kBF16)
    pra::moe::launch_ffn<pra::bf16>(x, ids, tw, w1, b1, w2, b2, out, h, ws, idx, M, D, F, E, k, act, s);
  else if (dt == pra::kF16)
    pra::moe::launch_ffn<pra::f16>(x, ids, tw, w1, b1, w2, b2, out, h, ws, idx, M, D, F, E, k, act, s);
  else return 1;
  return 0;
}

}  // extern "C"
