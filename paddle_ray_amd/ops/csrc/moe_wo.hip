// Top-k routed mixture-of-experts FFN over weight-only int8 / int4 expert weights, decode steps on gfx950:
//   out[m] = sum_j w[m, j] * (act(x[m] . W1[e_j] + b1[e_j]) . W2[e_j] + b2[e_j]),  e_j = ids[m, j],
//   W = level * scale with integer levels (int8: [-127, 127]; int4: [-7, 7], two per byte) and fp32
//   scales, one per output channel or one per `group` (64 / 128) consecutive k of a channel.
//   1 <= M <= 64 tokens, E <= 256, k <= 8, D % 64 == 0, F % 64 == 0; x / b / out bf16 or f16.
//
// Weights: expert e of a product with K inputs and NT output channels is the byte image that
// ops/fused.py weight_quantize writes for a [K, NT] matrix (the storage order at the top of
// wo_gemm.hip: 16-channel tiles, 64-k chunks, a lane's 16 bytes being the MFMA operands of its
// channel; int4 in superchunks of 128 k with a 64-k tail when K % 128 == 64). The images are stacked:
// w1 [E, N1, D] / [E, N1, D/2] bytes, w2 [E, D, F] / [E, D, F/2], scales [E, NT] or [E, K/group, NT].
// There is no second layout and nothing is repacked.
//
// The step is bound by the HBM read of the chosen experts' weights, so the path is moe_ffn.hip's with
// 1-byte or half-byte weights: moe_index (moe_common.h) sorts the (token, slot) pairs by expert, the
// two products run as moe_wo_kernel below, moe_combine (moe_common.h) adds a token's slots. No
// atomics, no split over K, no host sync; the grids never depend on the routing, so a call is bitwise
// reproducible and can be captured into a graph.
//
// moe_wo_kernel, grid = (N / 64, E). A workgroup whose expert has no rows returns at once: the bytes
// of an unselected expert are never read, those of a selected one exactly once. Otherwise 4 waves =
// 4 tiles of 16 channels over all of K, in stages of 512 k (256 above 32 rows; halved for SwiGLU,
// where a wave owns tile nt of the gate half and tile nt + F/16 of the up half, so a lane ends with
// both values of its 4 channels):
//   1. the stage's weights go from HBM to registers, 16 bytes per lane and load (one 64-k chunk of
//      int8, one 128-k superchunk of int4), all loads issued before the staging barrier;
//   2. after the barrier the expert's rows of x (gathered by sorted_pair[s] / k for the first product,
//      h[off[e] + r] for the second; rows past the count zeroed, row blocks past it not touched) go to
//      LDS at the conflict-free pitch stage + 8, and with them the stage's group scales for the 64
//      (SwiGLU: 2 x 64) channels;
//   3. a wave turns its registers into exact 16-bit integer operands (wo_common.h cvt_i8 / cvt_i4) and
//      runs v_mfma_f32_16x16x32 with the weights as "A" and the rows as "B" over up to ceil(M / 16)
//      row blocks (template bound), skipping blocks past the expert's count by a wave-uniform test.
// Unlike moe_gemm_kernel there is no weight image in LDS and no transposed read: the byte image is
// already k-contiguous per channel, so no weight byte touches LDS.
// Scales never touch the 16-bit operand. Per channel: the fp32 sum times the scale in the epilogue.
// Per group: a second accumulator set takes the group's partial sum, which is multiplied by the
// group's scale and added to the first when the group ends (every chunk, or every second one).
// Epilogue of the first product: scale, bias, erf GELU / ReLU / silu(gate) * up, h in the model dtype
// at the sorted position; of the second: scale, fp32 to the workspace at the sorted position.
//
// Registers of the widest instantiations (grouped, SwiGLU, 4 row blocks; -O3 without packed fp32, as
// ops/build.py compiles this file), bf16 and f16 alike: int8 96 VGPRs + 32 AGPRs (4 waves per SIMD),
// int4 100 VGPRs + 32 AGPRs (3 waves per SIMD), 18688 bytes of LDS. None of the 128 instantiations
// uses scratch.
#include "moe_common.h"
#include "pra_api.h"
#include "wo_common.h"

namespace pra {
namespace moe {

// a: x [M, K] (topk > 0: the row of sorted position s is sorted[s] / topk) or h [P, K] (topk == 0: row
// s). qw: E stacked byte images of [K, NT]; scale [E, NT] or (GROUPED) [E, K / (64 gch), NT]; bias
// [E, NT] or null. EPI 0: ws[s, N] fp32 (NT == N); kGelu / kRelu: h[s, N] (NT == N); kSwiglu: h[s, N]
// from channels n and n + N of NT == 2N. MB = row blocks of 16; gch = chunks per scale group (1 or 2).
template <typename T, bool W4, bool GROUPED, int MB, int EPI>
__global__ __launch_bounds__(kThreads) void moe_wo_kernel(const uint16_t* __restrict__ a,
                                                          const uint8_t* __restrict__ qw,
                                                          const float* __restrict__ scale,
                                                          const uint16_t* __restrict__ bias,
                                                          const int* __restrict__ off,
                                                          const int* __restrict__ sorted, int topk,
                                                          uint16_t* __restrict__ h, float* __restrict__ ws, int K,
                                                          int N, int NT, int gch) {
  constexpr int NS = EPI == kSwiglu ? 2 : 1;          // channel sets
  constexpr int SC = (MB <= 2 ? 8 : 4) / NS;          // chunks of 64 k per stage (even: int4 superchunks)
  constexpr int SK = SC * 64, LDX = SK + 8, ROWS = MB * 16;
  constexpr int NW = W4 ? SC / 2 : SC;                // 16-byte weight registers per set and stage
  typedef typename V8<T>::type v8;
  __shared__ __attribute__((aligned(16))) uint16_t xs[ROWS * LDX];
  __shared__ __attribute__((aligned(16))) float ss[GROUPED ? NS * SC * 64 : 4];
  __shared__ int rows[ROWS];

  const int e = blockIdx.y, base = off[e], cnt = min(off[e + 1] - base, ROWS);
  if (cnt <= 0) return;                               // workgroup-uniform: an expert nobody chose
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cm = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 64, nrows = ((cnt + 15) >> 4) << 4, nchunks = K >> 6;
  if (tid < ROWS) rows[tid] = tid < cnt ? (topk > 0 ? sorted[base + tid] / topk : base + tid) : -1;
  // tile nt (+ N / 16 for the up half) of expert e: 16 K bytes of int8, 8 K of int4
  const uint8_t* wp[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t)
    wp[t] = qw + ((size_t)e * NT + (size_t)(t * N + n0 + wv * 16)) * (size_t)(W4 ? K / 2 : K);
  const float* sp = scale + (size_t)e * (GROUPED ? nchunks / gch : 1) * NT;

  f32x4 acc[NS][MB], accg[NS][MB];
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[t][mb] = accg[t][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int cs = 0; cs < nchunks; cs += SC) {
    // 1. every weight byte of the stage, in flight before the staging barrier
    u32x4 wr[NS][NW];
#pragma unroll
    for (int t = 0; t < NS; ++t) {
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        wr[t][j] = u32x4{0u, 0u, 0u, 0u};
        if (!W4) {
          if (cs + j < nchunks) wr[t][j] = *reinterpret_cast<const u32x4*>(wp[t] + (size_t)(cs + j) * 1024 + lane * 16);
        } else {
          const int c = cs + 2 * j;
          if (c + 1 < nchunks) {
            wr[t][j] = *reinterpret_cast<const u32x4*>(wp[t] + (size_t)(c >> 1) * 1024 + lane * 16);
          } else if (c < nchunks) {                   // the 64-k tail of an odd chunk count
            const u32x2 hw = *reinterpret_cast<const u32x2*>(wp[t] + (size_t)(nchunks >> 1) * 1024 + lane * 8);
            wr[t][j][0] = hw[0];
            wr[t][j][1] = hw[1];
          }
        }
      }
    }
    // 2. the expert's rows of the stage (zeros past the count and past K) and its group scales -> LDS
    __syncthreads();
    for (int u = tid; u < nrows * SC * 8; u += kThreads) {
      const int row = u / (SC * 8), cc = u % (SC * 8), k = cs * 64 + cc * 8, r = rows[row];
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (r >= 0 && k < K) v = *reinterpret_cast<const uint4*>(a + (size_t)r * K + k);
      *reinterpret_cast<uint4*>(xs + row * LDX + cc * 8) = v;
    }
    if (GROUPED) {
      for (int u = tid; u < NS * SC * 64; u += kThreads) {
        const int t = u / (SC * 64), g = cs / gch + ((u >> 6) % SC);
        ss[u] = g < nchunks / gch ? sp[(size_t)g * NT + t * N + n0 + (u & 63)] : 0.f;
      }
    }
    __syncthreads();
    // 3. levels -> 16-bit operands -> MFMA over the expert's row blocks
#pragma unroll
    for (int j = 0; j < SC; ++j) {
      if (cs + j < nchunks) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          v8 wa[NS];
#pragma unroll
          for (int t = 0; t < NS; ++t)
            wa[t] = W4 ? wo::cvt_i4<T>(wr[t][j / 2][(j % 2) * 2 + s])
                       : wo::cvt_i8<T>(wr[t][j % NW][2 * s], wr[t][j % NW][2 * s + 1]);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) {
            if (mb * 16 < cnt) {
              const v8 b = *reinterpret_cast<const v8*>(xs + (mb * 16 + cm) * LDX + j * 64 + s * 32 + q * 8);
#pragma unroll
              for (int t = 0; t < NS; ++t) {
                if (GROUPED) accg[t][mb] = wo::mma<T>(wa[t], b, accg[t][mb]);
                else acc[t][mb] = wo::mma<T>(wa[t], b, acc[t][mb]);
              }
            }
          }
        }
      }
      if (GROUPED && ((j + 1) & (gch - 1)) == 0) {    // a group ends: its scale on its partial sum
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          const f32x4 sc =
              *reinterpret_cast<const f32x4*>(ss + t * SC * 64 + (j >> (gch - 1)) * 64 + wv * 16 + q * 4);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][mb][r] = fmaf(sc[r], accg[t][mb][r], acc[t][mb][r]);
            accg[t][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
      }
    }
  }

  const int n = n0 + wv * 16 + q * 4;
  f32x4 cs4[NS], bs[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) {
    cs4[t] = f32x4{1.f, 1.f, 1.f, 1.f};
    bs[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!GROUPED) cs4[t] = *reinterpret_cast<const f32x4*>(sp + t * N + n);
    if (EPI != 0 && bias) bs[t] = load4<T>(bias + (size_t)e * NT + t * N + n);
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int r = mb * 16 + cm;
    if (r >= cnt) continue;
    const size_t s = (size_t)(base + r);
    if (EPI == 0) {
      f32x4 o = acc[0][mb];
      if (!GROUPED) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] *= cs4[0][i];
      }
      *reinterpret_cast<f32x4*>(ws + s * N + n) = o;
    } else {
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = (GROUPED ? acc[0][mb][i] : acc[0][mb][i] * cs4[0][i]) + bs[0][i];
        if (EPI == kGelu) o[i] = gelu_erf_fast(v);
        else if (EPI == kRelu) o[i] = fmaxf(v, 0.f);
        else
          o[i] = v / (1.f + __expf(-v)) *
                 ((GROUPED ? acc[NS - 1][mb][i] : acc[NS - 1][mb][i] * cs4[NS - 1][i]) + bs[NS - 1][i]);
      }
      store4<T>(h + s * N + n, o);
    }
  }
}

template <typename T, bool W4, bool GROUPED, int EPI>
void launch_wo_mb(int mb, dim3 grid, hipStream_t s, const uint16_t* a, const uint8_t* qw, const float* scale,
                  const uint16_t* bias, const int* off, const int* sorted, int topk, uint16_t* h, float* ws, int K,
                  int N, int NT, int gch) {
#define PRA_MOE_WO_MB(MB)                                                                                      \
  case MB:                                                                                                     \
    hipLaunchKernelGGL((moe_wo_kernel<T, W4, GROUPED, MB, EPI>), grid, dim3(kThreads), 0, s, a, qw, scale, bias, \
                       off, sorted, topk, h, ws, K, N, NT, gch);                                               \
    break;
  switch (mb) {
    PRA_MOE_WO_MB(1)
    PRA_MOE_WO_MB(2)
    PRA_MOE_WO_MB(3)
    PRA_MOE_WO_MB(4)
  }
#undef PRA_MOE_WO_MB
}

template <typename T, int EPI>
void launch_wo(int w4, int group, int mb, dim3 grid, hipStream_t s, const uint16_t* a, const void* qw,
               const float* scale, const uint16_t* bias, const int* off, const int* sorted, int topk, uint16_t* h,
               float* ws, int K, int N, int NT) {
  const uint8_t* wp = static_cast<const uint8_t*>(qw);
  const int gch = group > 0 ? group / 64 : 1;
  if (w4) {
    if (group > 0) launch_wo_mb<T, true, true, EPI>(mb, grid, s, a, wp, scale, bias, off, sorted, topk, h, ws, K, N, NT, gch);
    else launch_wo_mb<T, true, false, EPI>(mb, grid, s, a, wp, scale, bias, off, sorted, topk, h, ws, K, N, NT, gch);
  } else {
    if (group > 0) launch_wo_mb<T, false, true, EPI>(mb, grid, s, a, wp, scale, bias, off, sorted, topk, h, ws, K, N, NT, gch);
    else launch_wo_mb<T, false, false, EPI>(mb, grid, s, a, wp, scale, bias, off, sorted, topk, h, ws, K, N, NT, gch);
  }
}

template <typename T>
void launch_ffn_wo(const void* x, const int* ids, const float* tw, const void* w1, const float* s1, const void* b1,
                   const void* w2, const float* s2, const void* b2, void* out, void* h, float* ws, int* idx, int M,
                   int D, int F, int E, int k, int act, int w4, int group, hipStream_t s) {
  const int P = M * k, mb = (M + 15) / 16;
  int* off = idx;
  int* sorted = idx + E + 1;
  int* pos = sorted + P;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* b1p = static_cast<const uint16_t*>(b1);
  uint16_t* hp = static_cast<uint16_t*>(h);
  hipLaunchKernelGGL(moe_index_kernel<kMaxRows * kMaxTopK>, dim3(1), dim3(kThreads), 0, s, ids, off, sorted, pos, P,
                     E);
  const dim3 g1(F / 64, E), g2(D / 64, E);
  if (act == kSwiglu)
    launch_wo<T, kSwiglu>(w4, group, mb, g1, s, xp, w1, s1, b1p, off, sorted, k, hp, nullptr, D, F, 2 * F);
  else if (act == kGelu) launch_wo<T, kGelu>(w4, group, mb, g1, s, xp, w1, s1, b1p, off, sorted, k, hp, nullptr, D, F, F);
  else launch_wo<T, kRelu>(w4, group, mb, g1, s, xp, w1, s1, b1p, off, sorted, k, hp, nullptr, D, F, F);
  launch_wo<T, 0>(w4, group, mb, g2, s, hp, w2, s2, nullptr, off, sorted, 0, nullptr, ws, F, D, D);
  hipLaunchKernelGGL((moe_combine_kernel<T>), dim3(M), dim3(kThreads), 0, s, ws, pos, ids, tw,
                     static_cast<const uint16_t*>(b2), static_cast<uint16_t*>(out), D, E, k);
}

}  // namespace moe
}  // namespace pra

extern "C" {

// out[M, D] of the routed FFN described at the top of this file: pra_moe_ffn (moe_ffn.hip) with w1 / w2
// the stacked int8 (w4 == 0: [E, N1, D] / [E, D, F] bytes) or int4 (w4 != 0: half of that) byte
// images and fp32 scales s1 / s2, [E, N1] / [E, D] for group == -1 and [E, D / group, N1] /
// [E, F / group, D] for group 64 / 128. x, b1 [E, N1] (optional), b2 [E, D] (optional) and out are `dt`
// (f16 / bf16); x, w1, w2, s1, s2, b1, b2 and the workspaces are contiguous and 16-byte aligned; ids /
// tw [M, k] as pra_moe_route returns them (an id outside [0, E) is clamped); act 1 erf GELU, 3 ReLU
// (N1 = F), 4 SwiGLU (N1 = 2F). Workspaces, all written before they are read: h holds M*k*F values
// of dt, ws M*k*D floats, idx E + 1 + 2*M*k ints. Returns non-zero without launching for M > 64, the
// other limits of pra_moe_ffn, D % group or F % group, another group / act / dt or a missing pointer.
int pra_moe_ffn_wo(const void* x, const int* ids, const float* tw, const void* w1, const float* s1, const void* b1,
                   const void* w2, const float* s2, const void* b2, void* out, void* h, float* ws, int* idx, int M,
                   int D, int F, int E, int k, int act, int w4, int group, int dt, hipStream_t s) {
  if (!pra::moe::limits_ok(M, D, E, k) || M > pra::moe::kMaxRows || F < 64 || F % 64) return 1;
  if (act != pra::moe::kGelu && act != pra::moe::kRelu && act != pra::moe::kSwiglu) return 1;
  if (group != -1 && group != 64 && group != 128) return 1;
  if (group > 0 && (D % group || F % group)) return 1;
  if (!x || !ids || !tw || !w1 || !s1 || !w2 || !s2 || !out || !h || !ws || !idx) return 1;
  if (dt == pra::kBF16)
    pra::moe::launch_ffn_wo<pra::bf16>(x, ids, tw, w1, s1, b1, w2, s2, b2, out, h, ws, idx, M, D, F, E, k, act, w4,
                                       group, s);
  else if (dt == pra::kF16)
    pra::moe::launch_ffn_wo<pra::f16>(x, ids, tw, w1, s1, b1, w2, s2, b2, out, h, ws, idx, M, D, F, E, k, act, w4,
                                      group, s);
  else return 1;
  return 0;
}

}  // extern "C"
