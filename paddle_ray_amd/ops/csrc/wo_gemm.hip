// Weight-only int8 / int4 linear for decode steps on gfx950:
//   y[M, N] = act(x[M, K] . W[K, N] + bias),  1 <= M <= 64,  x / bias / y bf16 or f16,
//   W = level * scale with integer levels (int8: [-127, 127]; int4: [-7, 7], two per byte) and
//   fp32 scales, one per output channel ([N]) or one per `group` consecutive k of a channel
//   ([K / group, N], group 64 or 128).
//
// The product is bound by the HBM read of W (M is tiny), so the kernel is built around streaming
// W once and doing as little as possible to it on the way into the matrix unit.
//
// Weights as the MFMA "A" operand, x as "B". v_mfma_f32_16x16x32 takes from lane l the 8 values
// k = 8*(l/16) .. +7 of row (A) / column (B) l%16 and returns to it rows 4*(l/16) .. +3 of column
// l%16. With 16 output channels as the rows and 16 rows of x as the columns a lane ends up with 4
// consecutive channels of one row of y: one 8-byte store, one float4 of scales, no transpose.
// 16x16x32 and not 32x32x16: both do the same FLOPs per cycle, but M is 1..64 and usually 8..32, so
// a 16-row block wastes at most 15 padded rows where a 32-row block wastes up to 31; the
// accumulator of a block is 4 VGPRs instead of 16, which is what lets a wave keep a second set for
// the per-group partial sums; and a lane's operand is 8 consecutive k of ONE channel, i.e. 8 bytes
// of int8 or 4 bytes of int4, so a 16-byte global load is two (int8) or four (int4) ready operands.
//
// Storage order (ops/fused.py weight_quantize writes it; this file and wo_tall.hip, which takes the
// products of more than 64 rows, read it and nothing else does). Channels are cut
// into tiles of 16, k into chunks of 64 (two MFMA steps). int8: tile nt is 16*K bytes, chunk c of it
// 1024 bytes, lane l = q*16 + ch owns bytes [16*l, 16*l + 16) = the levels of channel nt*16 + ch at
// k = c*64 + s*32 + q*8 + i, s = 0..1, i = 0..7. int4: a tile is 8*K bytes in superchunks of 128 k,
// 1024 bytes each, lane l owns 16 bytes = dwords s = 0..3 whose nibble i (bits 4i..4i+3) is
// level + 8 at k = sc*128 + s*32 + q*8 + i; if K % 128 == 64 the last 64 k follow as 512 bytes, 8 per
// lane (s = 0..1). Levels become exact bf16 / f16 integers in registers (byte or nibble -> fp32 ->
// packed 16-bit); scales never touch the 16-bit operand: a per-channel scale multiplies the fp32
// sum in the epilogue, a per-group scale multiplies the group's own fp32 partial sum.
//
// Work split: a workgroup is 4 waves = 4 channel tiles (64 channels) over one K slice; grid =
// (ceil(N / 64), splits). The 4 waves share x: per stage of 512 k (256 k above 32 rows) the
// workgroup copies x[0:M, stage] into LDS as rows of pitch stage + 8 elements, which puts the 16
// rows a ds_read_b128 phase touches 16 bytes apart modulo 256 (no bank conflict), rows >= M
// zeroed; a stage's group scales for the 64 channels go to LDS with it. A wave issues all the
// weight loads of a stage (up to 8 x 16 bytes per lane) before the staging barrier, so the HBM
// latency of W overlaps the L2 latency of x, and other workgroups on the CU cover the rest.
// Every byte of W is read once whatever M is: all row blocks reuse the converted operand.
//
// Split-K: slices are cut in superchunks of 128 k (uneven when splits does not divide their
// number). Slice s writes its fp32 partial [M, N] to ws[s]; wo_reduce_kernel adds the slices in
// index order and applies scale, bias and activation. No atomics: a call is bitwise reproducible.
// With splits == 1 the same epilogue runs in the main kernel. Nothing syncs with the host, and the
// workspace is written before it is read, so launches can be captured into a graph.
#include "pra_api.h"
#include "wo_common.h"

namespace pra {
namespace wo {

constexpr int kMaxRows = 64;

// The slice [c0, c1) of split sp, in chunks of 64 k: whole superchunks of 128 k, the last one cut
// at K. Used by the kernel only; the host clamps splits to the number of superchunks.
__device__ __forceinline__ void slice_of(int K, int sp, int splits, int& c0, int& c1) {
  const int nchunks = K >> 6, nsc = (nchunks + 1) >> 1;
  c0 = 2 * (int)((long long)nsc * sp / splits);
  c1 = min(2 * (int)((long long)nsc * (sp + 1) / splits), nchunks);
}

// MB = row blocks of 16 (M <= 16 * MB); gch = chunks per scale group (1 or 2) when GROUPED
template <typename T, bool W4, bool GROUPED, int MB>
__global__ __launch_bounds__(kThreads) void wo_gemm_kernel(const uint16_t* __restrict__ x,
                                                           const uint8_t* __restrict__ qw,
                                                           const float* __restrict__ scale,
                                                           const uint16_t* __restrict__ bias,
                                                           uint16_t* __restrict__ y, float* __restrict__ ws, int M,
                                                           int N, int K, int gch, int splits, int act) {
  constexpr int SC = MB <= 2 ? 8 : 4;          // chunks per stage
  constexpr int SK = SC * 64, LDX = SK + 8, ROWS = MB * 16;
  constexpr int NW = W4 ? SC / 2 : SC;         // 16-byte weight registers per stage
  typedef typename V8<T>::type v8;
  __shared__ __attribute__((aligned(16))) uint16_t xs[ROWS * LDX];
  __shared__ __attribute__((aligned(16))) float ss[GROUPED ? SC * 64 : 4];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cm = lane & 15, q = lane >> 4;
  const int nt = blockIdx.x * 4 + wv;
  const bool live = nt < (N >> 4);             // wave-uniform; a dead wave still stages and syncs
  const int nchunks = K >> 6, sp = blockIdx.y;
  int c0, c1;
  slice_of(K, sp, splits, c0, c1);
  const uint8_t* wp = qw + (size_t)nt * (W4 ? 8 : 16) * K;   // only dereferenced by live waves

  f32x4 acc[MB], accg[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = accg[mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int cs = c0; cs < c1; cs += SC) {
    // 1. every weight byte of the stage, in flight before the staging barrier
    u32x4 wr[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      wr[j] = u32x4{0u, 0u, 0u, 0u};
      if (!W4) {
        if (live && cs + j < c1) wr[j] = *reinterpret_cast<const u32x4*>(wp + (size_t)(cs + j) * 1024 + lane * 16);
      } else {
        const int c = cs + 2 * j;
        if (live && c + 1 < c1) {
          wr[j] = *reinterpret_cast<const u32x4*>(wp + (size_t)(c >> 1) * 1024 + lane * 16);
        } else if (live && c < c1) {           // the 64-k tail of an odd chunk count
          const u32x2 h = *reinterpret_cast<const u32x2*>(wp + (size_t)(nchunks >> 1) * 1024 + lane * 8);
          wr[j][0] = h[0];
          wr[j][1] = h[1];
        }
      }
    }
    // 2. x[0:M, stage] (zeros past M and past the slice) and the stage's group scales -> LDS
    __syncthreads();
    for (int u = tid; u < ROWS * SC * 8; u += kThreads) {
      const int row = u / (SC * 8), cc = u % (SC * 8), k = cs * 64 + cc * 8;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row < M && k < c1 * 64) v = *reinterpret_cast<const uint4*>(x + (size_t)row * K + k);
      *reinterpret_cast<uint4*>(xs + row * LDX + cc * 8) = v;
    }
    if (GROUPED) {
      for (int u = tid; u < SC * 64; u += kThreads) {
        const int gi = u >> 6, n = blockIdx.x * 64 + (u & 63), g = cs / gch + gi;
        ss[u] = (n < N && g < nchunks / gch) ? scale[(size_t)g * N + n] : 0.f;
      }
    }
    __syncthreads();
    // 3. levels -> 16-bit operands -> MFMA over every row block
    if (live) {
#pragma unroll
      for (int j = 0; j < SC; ++j) {
        if (cs + j < c1) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const v8 a = W4 ? cvt_i4<T>(wr[j / 2][(j % 2) * 2 + s]) : cvt_i8<T>(wr[j % NW][2 * s], wr[j % NW][2 * s + 1]);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              const v8 b = *reinterpret_cast<const v8*>(xs + (mb * 16 + cm) * LDX + j * 64 + s * 32 + q * 8);
              if (GROUPED) accg[mb] = mma<T>(a, b, accg[mb]);
              else acc[mb] = mma<T>(a, b, acc[mb]);
            }
          }
        }
        if (GROUPED && ((j + 1) & (gch - 1)) == 0) {   // a group ends: its scale on its partial sum
          const f32x4 sc = *reinterpret_cast<const f32x4*>(ss + (j >> (gch - 1)) * 64 + wv * 16 + q * 4);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mb][r] = fmaf(sc[r], accg[mb][r], acc[mb][r]);
            accg[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
      }
    }
  }
  if (!live) return;
  const int n = nt * 16 + q * 4;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + cm;
    if (m >= M) continue;
    if (splits > 1) *reinterpret_cast<f32x4*>(ws + ((size_t)sp * M + m) * N + n) = acc[mb];
    else finish<T>(acc[mb], GROUPED ? nullptr : scale, bias, y, m, n, N, act);
  }
}

// y = act(scale * sum_s ws[s] + bias), the slices added in index order; one thread per 4 channels
template <typename T>
__global__ __launch_bounds__(kThreads) void wo_reduce_kernel(const float* __restrict__ ws,
                                                             const float* __restrict__ chan_scale,
                                                             const uint16_t* __restrict__ bias,
                                                             uint16_t* __restrict__ y, int M, int N, int splits,
                                                             int act) {
  const int idx = blockIdx.x * kThreads + threadIdx.x, nq = N >> 2;
  if (idx >= M * nq) return;
  const int m = idx / nq, n = (idx % nq) * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(ws + (size_t)m * N + n);
  for (int s = 1; s < splits; ++s) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(ws + ((size_t)s * M + m) * N + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += p[r];
  }
  finish<T>(v, chan_scale, bias, y, m, n, N, act);
}

template <typename T, bool W4, bool GROUPED>
void launch_mb(int mb, dim3 grid, hipStream_t s, const uint16_t* x, const uint8_t* qw, const float* scale,
               const uint16_t* bias, uint16_t* y, float* ws, int M, int N, int K, int gch, int splits, int act) {
#define PRA_WO_MB(MB)                                                                                          \
  case MB:                                                                                                     \
    hipLaunchKernelGGL((wo_gemm_kernel<T, W4, GROUPED, MB>), grid, dim3(kThreads), 0, s, x, qw, scale, bias, y, \
                       ws, M, N, K, gch, splits, act);                                                         \
    break;
  switch (mb) {
    PRA_WO_MB(1)
    PRA_WO_MB(2)
    PRA_WO_MB(3)
    PRA_WO_MB(4)
  }
#undef PRA_WO_MB
}

template <typename T>
void launch(const void* x, const void* qw, const float* scale, const void* bias, void* y, float* ws, int M, int N,
            int K, int w4, int group, int splits, int act, hipStream_t s) {
  const dim3 grid((N + 63) / 64, splits);
  const int mb = (M + 15) / 16, gch = group > 0 ? group / 64 : 1;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint8_t* wp = static_cast<const uint8_t*>(qw);
  const uint16_t* bp = static_cast<const uint16_t*>(bias);
  uint16_t* yp = static_cast<uint16_t*>(y);
  if (w4) {
    if (group > 0) launch_mb<T, true, true>(mb, grid, s, xp, wp, scale, bp, yp, ws, M, N, K, gch, splits, act);
    else launch_mb<T, true, false>(mb, grid, s, xp, wp, scale, bp, yp, ws, M, N, K, gch, splits, act);
  } else {
    if (group > 0) launch_mb<T, false, true>(mb, grid, s, xp, wp, scale, bp, yp, ws, M, N, K, gch, splits, act);
    else launch_mb<T, false, false>(mb, grid, s, xp, wp, scale, bp, yp, ws, M, N, K, gch, splits, act);
  }
  if (splits > 1) {
    const int nthr = M * (N / 4);
    hipLaunchKernelGGL((wo_reduce_kernel<T>), dim3((nthr + kThreads - 1) / kThreads), dim3(kThreads), 0, s, ws,
                       group > 0 ? nullptr : scale, bp, yp, M, N, splits, act);
  }
}

}  // namespace wo
}  // namespace pra

extern "C" {

// Default split count: enough K slices that about two workgroups per CU stream W (512 over the
// ceil(N / 64) channel slabs), each slice at least 256 k, never more slices than superchunks.
int pra_wo_gemm_splits(int M, int N, int K) {
  (void)M;
  if (N < 1 || K < 1) return 1;
  const int slabs = (N + 63) / 64, nsc = (K / 64 + 1) / 2;
  const int want = (512 + slabs - 1) / slabs, most = nsc / 2 > 1 ? nsc / 2 : 1;
  return want < 1 ? 1 : (want > most ? most : want);
}

// y[M, N] = act(x[M, K] . (levels * scale) + bias). x, bias (optional) and y are `dt` (f16 / bf16),
// contiguous and 16-byte aligned; qw is the tile-ordered byte image described at the top of this
// file (w4: int4, else int8); scale is fp32 [N] for group == -1 and [K / group, N] for group 64 /
// 128; act 0 none, 1 erf GELU, 3 ReLU; ws holds splits * M * N floats when splits > 1 (unused
// otherwise). Returns non-zero without launching for M outside [1, 64], N % 16, K % 64, K % group,
// another group / act / dt, splits outside [1, ceil(K / 128)] or a missing pointer.
int pra_wo_gemm(const void* x, const void* qw, const float* scale, const void* bias, void* y, float* ws, int M, int N,
                int K, int w4, int group, int splits, int act, int dt, hipStream_t s) {
  if (M < 1 || M > pra::wo::kMaxRows || N < 16 || N % 16 || K < 64 || K % 64) return 1;
  if (group != -1 && group != 64 && group != 128) return 1;
  if (group > 0 && K % group) return 1;
  if (act != 0 && act != 1 && act != 3) return 1;
  if (splits < 1 || splits > (K / 64 + 1) / 2 || (splits > 1 && !ws)) return 1;
  if (!x || !qw || !scale || !y) return 1;
  if (dt == pra::kBF16) pra::wo::launch<pra::bf16>(x, qw, scale, bias, y, ws, M, N, K, w4, group, splits, act, s);
  else if (dt == pra::kF16) pra::wo::launch<pra::f16>(x, qw, scale, bias, y, ws, M, N, K, w4, group, splits, act, s);
  else return 1;
  return 0;
}

}  // extern "C"
