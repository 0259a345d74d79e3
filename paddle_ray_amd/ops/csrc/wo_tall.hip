// Weight-only int8 / int4 linear above the decode sizes on gfx950: the operation of wo_gemm.hip,
//   y[M, N] = act(x[M, K] . W[K, N] + bias),  x / bias / y bf16 or f16,  W = level * scale,
// for any M >= 1 (ops/fused.py sends M > 64 here), reading the byte image weight_quantize writes for
// wo_gemm.hip (the storage order at the top of that file) as it is: no repacking, no second layout.
// Same shape rule (K % 64 == 0, N % 16 == 0, K % group == 0) and same numerical contract: a level
// enters the matrix unit as an exact 16-bit integer, a per-channel scale multiplies the fp32 sum in
// the epilogue, a per-group scale multiplies the group's own fp32 partial sum. No split-K, no
// atomics, no host sync, the grid comes from the shapes: a call is bitwise reproducible and can be
// captured into a graph.
//
// wo_gemm.hip is bound by the one pass over W; here x is tall and W is reused by every row tile, so
// the kernel is a tiled GEMM: a workgroup of 256 threads owns 128 rows x 128 channels of y over all
// of K, grid = (ceil(N / 128), ceil(M / 128)). v_mfma_f32_16x16x32 with the weights as "A" and x as
// "B", as in wo_gemm.hip: lane l = q*16 + cm ends with channels 4q .. 4q+3 of a 16-channel tile for
// row cm of a 16-row block, i.e. one 8-byte store, one float4 of group scales.
//
// Waves split the channels, not the rows: wave w owns the 16-channel tiles 2w and 2w + 1 of the 128
// channels over all 8 row blocks, 16 f32x4 accumulators (and 16 more for the running group when the
// scales are per group). A tile belongs to one wave only, so every byte of W is loaded and converted
// once per workgroup and a converted operand feeds 8 MFMAs. W does not pass through LDS: the 16
// bytes the storage order gives a lane are its own operands (int8: the two of one chunk of 64 k;
// int4: the four of a superchunk of 128 k) through cvt_i8 / cvt_i4. A tile past N costs its wave no
// loads and no MFMAs; the wave still stages x and meets the barriers.
//
// x goes through LDS, shared by the four waves, in stages of 128 rows x 64 k, two buffers: the next
// stage's global loads (4 x 16 bytes per thread, 8 threads covering the 128-byte line of a row;
// rows >= M are zeros) are issued before the stage's MFMAs and stored to the other buffer after
// them, one barrier per stage. The row pitch is 64 + 8 elements = 144 bytes = 9 x 16: the 16 rows a
// ds_read_b128 phase touches then start at 16 distinct multiples of 16 bytes modulo 256 (9 is odd),
// the rule behind wo_gemm.hip's pitch of stage + 8. A lane's B operand is one ds_read_b128: 8 k of
// row cm at k = 8q of a 32-k step. LDS is 2 x 128 x 144 = 36864 bytes.
//
// Group scales: the float4 of a (group, tile) is loaded with the weights of its k range and applied
// when the group's last chunk is done: acc = fma(scale, partial, acc), partial = 0.
//
// Where this differs from the plan it was written to: weights and group scales are fetched per
// superchunk of 128 k (two stages of x), one superchunk ahead, not per chunk. The superchunk is the
// unit of the int4 storage order (a lane's 16 bytes span both chunks), and with the same loop for
// int8 every register index is a compile-time constant (chunk j = 0 / 1 of the pair reads LDS buffer
// j). An odd chunk count ends with a pair of one chunk: int8 loads its 16 bytes, int4 the 8 bytes
// per lane of the 512-byte tail (K = 64 is that tail alone). Row offsets are 64-bit; the row count is
// limited by the grid's y extent alone (65535 tiles), and ops/fused.py walks row chunks past that.
#include "pra_api.h"
#include "wo_common.h"

namespace pra {
namespace wo {

constexpr int kTM = 128, kTN = 128, kStage = 64, kPitch = kStage + 8;
constexpr int kMaxRowsTall = 65535 * kTM;

// Two waves per SIMD asked for: the per-group instantiations otherwise take 292 registers and leave
// a CU with one workgroup, whose barrier waits nothing would cover; with the bound they fit 256
// without scratch (the per-channel ones use 136 to 154 and run three).
template <typename T, bool W4, bool GROUPED>
__global__ __launch_bounds__(kThreads, 2) void wo_tall_kernel(const uint16_t* __restrict__ x,
                                                           const uint8_t* __restrict__ qw,
                                                           const float* __restrict__ scale,
                                                           const uint16_t* __restrict__ bias,
                                                           uint16_t* __restrict__ y, int M, int N, int K, int gch,
                                                           int act) {
  constexpr int NWR = W4 ? 1 : 2;              // 16-byte weight registers per tile and superchunk
  typedef typename V8<T>::type v8;
  __shared__ __attribute__((aligned(16))) uint16_t xs[2][kTM * kPitch];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cm = lane & 15, q = lane >> 4;
  const int nchunks = K >> 6, npairs = (nchunks + 1) >> 1;
  const int m0 = blockIdx.y * kTM, xrow = tid >> 3, xk = (tid & 7) * 8;

  bool live[2];                                // wave-uniform
  const uint8_t* wp[2];                        // only dereferenced for live tiles
  int n4[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int nt = blockIdx.x * (kTN / 16) + wv * 2 + t;
    live[t] = nt < (N >> 4);
    wp[t] = qw + (size_t)nt * (W4 ? 8 : 16) * K;
    n4[t] = nt * 16 + q * 4;
  }

  f32x4 acc[2][8], accg[2][8];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc[t][mb] = accg[t][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // stage c of x: global -> registers, registers -> LDS buffer
  auto load_x = [&](int c, uint4* xr) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + i * 32 + xrow;
      xr[i] = make_uint4(0u, 0u, 0u, 0u);
      if (m < M) xr[i] = *reinterpret_cast<const uint4*>(x + (size_t)m * K + c * kStage + xk);
    }
  };
  auto store_x = [&](int buf, const uint4* xr) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(xs[buf] + (i * 32 + xrow) * kPitch + xk) = xr[i];
  };
  // superchunk p (chunks 2p, 2p + 1) of both tiles: the weight bytes and the scales of the groups
  // that end in it
  auto load_w = [&](int p, u32x4 (*w)[NWR], f32x4 (*sc)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int j = 0; j < NWR; ++j) w[t][j] = u32x4{0u, 0u, 0u, 0u};
      sc[t][0] = sc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (!live[t]) continue;
      if (!W4) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (2 * p + j < nchunks)
            w[t][j] = *reinterpret_cast<const u32x4*>(wp[t] + (size_t)(2 * p + j) * 1024 + lane * 16);
      } else if (2 * p + 1 < nchunks) {
        w[t][0] = *reinterpret_cast<const u32x4*>(wp[t] + (size_t)p * 1024 + lane * 16);
      } else {                                 // the 64-k tail of an odd chunk count
        const u32x2 h = *reinterpret_cast<const u32x2*>(wp[t] + (size_t)(nchunks >> 1) * 1024 + lane * 8);
        w[t][0][0] = h[0];
        w[t][0][1] = h[1];
      }
      if (GROUPED) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (2 * p + j < nchunks && ((j + 1) & (gch - 1)) == 0)
            sc[t][j] = *reinterpret_cast<const f32x4*>(scale + (size_t)((2 * p + j) / gch) * N + n4[t]);
      }
    }
  };

  u32x4 wc[2][NWR];
  f32x4 sc[2][2];
  uint4 xr[4];
  load_w(0, wc, sc);
  load_x(0, xr);
  store_x(0, xr);
  __syncthreads();

  for (int p = 0; p < npairs; ++p) {
    u32x4 wn[2][NWR];
    f32x4 sn[2][2];
    if (p + 1 < npairs) load_w(p + 1, wn, sn);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = 2 * p + j;                 // chunk c sits in LDS buffer j
      if (c < nchunks) {
        const bool more = c + 1 < nchunks;
        if (more) load_x(c + 1, xr);
        if (live[0]) {                         // tile 2w + 1 is never live without tile 2w
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            v8 a[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
              a[t] = W4 ? cvt_i4<T>(wc[t][0][j * 2 + s]) : cvt_i8<T>(wc[t][j % NWR][2 * s], wc[t][j % NWR][2 * s + 1]);
#pragma unroll
            for (int mb = 0; mb < 8; ++mb) {
              const v8 b = *reinterpret_cast<const v8*>(xs[j] + (mb * 16 + cm) * kPitch + s * 32 + q * 8);
              if (GROUPED) {
                accg[0][mb] = mma<T>(a[0], b, accg[0][mb]);
                if (live[1]) accg[1][mb] = mma<T>(a[1], b, accg[1][mb]);
              } else {
                acc[0][mb] = mma<T>(a[0], b, acc[0][mb]);
                if (live[1]) acc[1][mb] = mma<T>(a[1], b, acc[1][mb]);
              }
            }
          }
          if (GROUPED && ((j + 1) & (gch - 1)) == 0) {   // a group ends: its scale on its partial sum
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int mb = 0; mb < 8; ++mb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][mb][r] = fmaf(sc[t][j][r], accg[t][mb][r], acc[t][mb][r]);
                accg[t][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
              }
          }
        }
        if (more) store_x(j ^ 1, xr);
        __syncthreads();
      }
    }
    if (p + 1 < npairs) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int j = 0; j < NWR; ++j) wc[t][j] = wn[t][j];
        sc[t][0] = sn[t][0];
        sc[t][1] = sn[t][1];
      }
    }
  }

#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (!live[t]) continue;
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) {
      const int m = m0 + mb * 16 + cm;
      if (m < M) finish<T>(acc[t][mb], GROUPED ? nullptr : scale, bias, y, m, n4[t], N, act);
    }
  }
}

template <typename T>
void launch_tall(const void* x, const void* qw, const float* scale, const void* bias, void* y, int M, int N, int K,
                 int w4, int group, int act, hipStream_t s) {
  const dim3 grid((N + kTN - 1) / kTN, (M + kTM - 1) / kTM), block(kThreads);
  const int gch = group > 0 ? group / 64 : 1;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint8_t* wp = static_cast<const uint8_t*>(qw);
  const uint16_t* bp = static_cast<const uint16_t*>(bias);
  uint16_t* yp = static_cast<uint16_t*>(y);
#define PRA_WO_TALL(W4, G) \
  hipLaunchKernelGGL((wo_tall_kernel<T, W4, G>), grid, block, 0, s, xp, wp, scale, bp, yp, M, N, K, gch, act)
  if (w4) {
    if (group > 0) PRA_WO_TALL(true, true);
    else PRA_WO_TALL(true, false);
  } else {
    if (group > 0) PRA_WO_TALL(false, true);
    else PRA_WO_TALL(false, false);
  }
#undef PRA_WO_TALL
}

}  // namespace wo
}  // namespace pra

extern "C" {

// y[M, N] = act(x[M, K] . (levels * scale) + bias) for any 1 <= M <= 65535 * 128. Operands as for
// pra_wo_gemm (wo_gemm.hip): x, bias (optional) and y are `dt` (f16 / bf16), contiguous and 16-byte
// aligned; qw is the tile-ordered byte image (w4: int4, else int8); scale is fp32 [N] for
// group == -1 and [K / group, N] for group 64 / 128; act 0 none, 1 erf GELU, 3 ReLU. Returns
// non-zero without launching for M outside that range, N % 16, K % 64, K % group, another group /
// act / dt or a missing pointer.
int pra_wo_gemm_tall(const void* x, const void* qw, const float* scale, const void* bias, void* y, int M, int N,
                     int K, int w4, int group, int act, int dt, hipStream_t s) {
  if (M < 1 || M > pra::wo::kMaxRowsTall || N < 16 || N % 16 || K < 64 || K % 64) return 1;
  if (group != -1 && group != 64 && group != 128) return 1;
  if (group > 0 && K % group) return 1;
  if (act != 0 && act != 1 && act != 3) return 1;
  if (!x || !qw || !scale || !y) return 1;
  if (dt == pra::kBF16) pra::wo::launch_tall<pra::bf16>(x, qw, scale, bias, y, M, N, K, w4, group, act, s);
  else if (dt == pra::kF16) pra::wo::launch_tall<pra::f16>(x, qw, scale, bias, y, M, N, K, w4, group, act, s);
  else return 1;
  return 0;
}

}  // extern "C"
