// pybind11 entry points of the _pra_hip kernel library. Arguments are raw device
// pointers (ints from torch.Tensor.data_ptr()) and the current HIP stream, so the
// Python side pays one pybind11 call per launch and no tensor marshalling.
//
// The C entries are declared once, in pra_api.h, and a binding takes its Python signature from
// that prototype: Launch<&pra_x>::def(m, "x", text) binds x with the C parameter list in the C
// order, every pointer parameter (hipStream_t included) accepted as an integer and cast back to
// its declared type, everything else passed through as its own type. A non-zero return of an int
// entry raises ValueError("x: " + text); after the call hipGetLastError() is checked. Pure host
// queries are bound directly (m.def("x", &pra_x)): they return their value and launch nothing.
//
// Hand-written, because the Python form differs from the C form:
//   flash_fwd                    nine scalar strides instead of a stride array
//   flash_fwd_ext, flash_bwd_ext, flash_bwd
//                                a stride list whose length is checked
//   colsum_multi                 lists of pointers / flags, 1-3 jobs
//   colsum16, colsum16_acc       one C entry, the accumulate flag fixed per name
//   colsum_rows                  the cols % 8 check (the entry launches nothing otherwise)
//   gemm_probe                   returns the entry's code (the workgroup count) instead of raising
//   spin_hog                     no launch check (it runs beside the kernel being probed)
//   capture_id, build_info       no C launch entry behind them / a string conversion
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <vector>
#include <stdexcept>
#include <string>
#include <type_traits>
#include "pra_api.h"

namespace py = pybind11;
typedef uintptr_t P;

#define V(x) reinterpret_cast<void*>(x)
#define CV(x) reinterpret_cast<const void*>(x)
#define F(x) reinterpret_cast<float*>(x)
#define CF(x) reinterpret_cast<const float*>(x)
#define S(x) reinterpret_cast<hipStream_t>(x)

static void check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

template <typename A> struct PyArg     { using type = A; static A to(A a) { return a; } };
template <typename A> struct PyArg<A*> { using type = P; static A* to(P p) { return reinterpret_cast<A*>(p); } };

template <auto Fn> struct Launch;
template <typename R, typename... A, R (*Fn)(A...)> struct Launch<Fn> {
  static void def(py::module_& m, const char* name, const char* unsupported = nullptr) {
    m.def(name, [name, unsupported](typename PyArg<A>::type... a) {
      if constexpr (std::is_void_v<R>) Fn(PyArg<A>::to(a)...);
      else if (Fn(PyArg<A>::to(a)...) != 0) throw std::invalid_argument(std::string(name) + ": " + unsupported);
      check_launch(name);
    });
  }
};

PYBIND11_MODULE(_pra_hip, m) {
  m.doc() = "paddle_ray_amd gfx950 HIP kernels";
  // host queries
  m.def("conv_lds_splits", &pra_conv_lds_splits);
  m.def("conv_wgrad_rows", &pra_conv_wgrad_rows);
  m.def("conv_lds_stat_rows", &pra_conv_lds_stat_rows);
  m.def("gemm_lds_splits", &pra_gemm_lds_splits);
  m.def("gemm_set_w4", &pra_gemm_set_w4);
  m.def("gemm_set_pts", &pra_gemm_set_pts);
  m.def("gemm_get_pts", &pra_gemm_get_pts);
  m.def("gemm_get_w4", &pra_gemm_get_w4);
  m.def("mmha_splits", &pra_mmha_splits);
  m.def("adl_supported", &pra_adl_supported);
  m.def("bn_nrb", &pra_bn_nrb);
  m.def("build_info", []() { return std::string(pra_build_info()); });
  // id of the stream capture in progress on s (0 when s is not capturing): the graph-safe dropout
  // RNG advances its device step counter once per capture (ops/fused.py _graph_seq)
  m.def("capture_id", [](P s) -> unsigned long long {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    if (hipStreamGetCaptureInfo(S(s), &st, &id) != hipSuccess || st != hipStreamCaptureStatusActive) return 0ull;
    return id;
  });

  // launches with the C signature
  Launch<&pra_gemm_bias_act>::def(m, "gemm_bias_act", "unsupported shape/stride/dtype");
  Launch<&pra_gemm_lds>::def(m, "gemm_lds", "unsupported shape/stride/dtype");
  Launch<&pra_gemm_tn_grouped2>::def(m, "gemm_tn_grouped2", "unsupported shape");
  Launch<&pra_colsum_partials>::def(m, "colsum_partials", "unsupported dtype");
  Launch<&pra_conv_lds>::def(m, "conv_lds", "unsupported shape/dtype");
  Launch<&pra_conv_dgrad_phase>::def(m, "conv_dgrad_phase", "unsupported shape/dtype");
  Launch<&pra_conv_wgrad_lds>::def(m, "conv_wgrad_lds", "unsupported shape/dtype");
  Launch<&pra_space_to_depth2>::def(m, "space_to_depth2", "unsupported geometry");
  Launch<&pra_layernorm_fwd>::def(m, "layernorm_fwd", "unsupported dtype pair");
  Launch<&pra_layernorm_bwd>::def(m, "layernorm_bwd", "unsupported dtype pair");
  Launch<&pra_rmsnorm_fwd>::def(m, "rmsnorm_fwd", "unsupported dtype pair");
  Launch<&pra_rmsnorm_bwd>::def(m, "rmsnorm_bwd", "unsupported dtype pair");
  Launch<&pra_colsum>::def(m, "colsum");
  Launch<&pra_softmax_fwd>::def(m, "softmax_fwd");
  Launch<&pra_softmax_bwd>::def(m, "softmax_bwd");
  Launch<&pra_softmax_ce_fwd>::def(m, "softmax_ce_fwd");
  Launch<&pra_softmax_ce_bwd>::def(m, "softmax_ce_bwd");
  Launch<&pra_vp_ce_part_fwd>::def(m, "vp_ce_part_fwd");
  Launch<&pra_vp_ce_final>::def(m, "vp_ce_final");
  Launch<&pra_vp_ce_bwd>::def(m, "vp_ce_bwd");
  // cache_dt = dt and null scales for a float cache; cache_dt 3 and the packed fp32 scales
  // [4, Bs, KVH] for the uint8 one (contract above the definition in decode_attn.hip)
  Launch<&pra_mmha_decode>::def(m, "mmha_decode",
                                "unsupported head_dim/group ratio/dtype/rotary_dims/quantisation arguments for a "
                                "uint8 cache, or time_step out of range");
  // the same step over a block pool [2, NB, KVH, BS, D] and an int32 block table [B, MB]
  Launch<&pra_mmha_decode_paged>::def(m, "mmha_decode_paged",
                                      "block size not a power of two >= 16, null block table, or anything "
                                      "mmha_decode refuses at L = MB*BS");
  // n_tok tokens per sequence in one cache pass; a null block table means the contiguous cache
  Launch<&pra_mmha_decode_multi>::def(m, "mmha_decode_multi",
                                      "n_tok < 1, more than 8 query rows per K/V row, or anything mmha_decode / "
                                      "mmha_decode_paged refuses");
  // temperature / top-k / top-p sampling, one id per row (contract above the definition in sample.hip)
  Launch<&pra_sample_top_p>::def(m, "sample_top_p", "unsupported dtype, R < 0, V < 1 or V > 2^22");
  Launch<&pra_bias_gelu_fwd>::def(m, "bias_gelu_fwd");
  Launch<&pra_bias_gelu_bwd>::def(m, "bias_gelu_bwd");
  Launch<&pra_bias_gelu_bwd_db>::def(m, "bias_gelu_bwd_db");
  Launch<&pra_zero_mt>::def(m, "zero_mt");
  Launch<&pra_adamw_mt>::def(m, "adamw_mt");
  Launch<&pra_momentum_mt>::def(m, "momentum_mt");
  Launch<&pra_lamb_shard_stage1>::def(m, "lamb_shard_stage1");
  Launch<&pra_lamb_shard_stage2>::def(m, "lamb_shard_stage2");
  Launch<&pra_sumsq_accum>::def(m, "sumsq_accum");
  Launch<&pra_adl_fwd>::def(m, "adl_fwd", "unsupported dtype pair");
  Launch<&pra_adl_bwd>::def(m, "adl_bwd", "unsupported dtype pair");
  Launch<&pra_flash_bwd_pre>::def(m, "flash_bwd_pre");
  Launch<&pra_bn_fwd_train>::def(m, "bn_fwd_train");
  Launch<&pra_bn_fwd_parts>::def(m, "bn_fwd_parts");
  Launch<&pra_bn_fwd_infer>::def(m, "bn_fwd_infer");
  Launch<&pra_bn_bwd>::def(m, "bn_bwd");
  Launch<&pra_bn_premerge>::def(m, "bn_premerge");
  Launch<&pra_bn_bwd_parts>::def(m, "bn_bwd_parts");
  Launch<&pra_gap_bwd>::def(m, "gap_bwd", "unsupported shape");
  Launch<&pra_max_pool_fwd>::def(m, "max_pool_fwd", "unsupported geometry");
  Launch<&pra_max_pool_bwd>::def(m, "max_pool_bwd", "unsupported geometry");
  Launch<&pra_wflip_t>::def(m, "wflip_t", "unsupported shape");
  Launch<&pra_embedding_fwd>::def(m, "embedding_fwd", "unsupported D/dtype");
  Launch<&pra_embedding_bwd>::def(m, "embedding_bwd", "unsupported D/dtype");

  // hand-written (see the header comment)
  m.def("spin_hog", [](int nwg, long long cycles, P sink, P s) { pra_spin_hog(nwg, cycles, F(sink), S(s)); });
  m.def("gemm_probe", [](int cfg, int layout, P a, P b, P c, int M, int N, int K, int lda, int ldb, int ldc, P st,
                         P s) {
    return pra_gemm_probe(cfg, layout, CV(a), CV(b), V(c), M, N, K, lda, ldb, ldc,
                          reinterpret_cast<unsigned long long*>(st), S(s));
  });
  m.def("colsum16", [](P part, P out, int nblk, int cols, int dt, P s) {
    pra_colsum16(CF(part), V(out), nblk, cols, dt, 0, S(s));
    check_launch("colsum16");
  });
  m.def("colsum16_acc", [](P part, P out, int nblk, int cols, int dt, P s) {
    pra_colsum16(CF(part), V(out), nblk, cols, dt, 1, S(s));
    check_launch("colsum16_acc");
  });
  m.def("colsum_rows", [](P x, P part, int rows, int cols, int nrb, int dt, P s) {
    if (cols % 8) throw std::invalid_argument("colsum_rows: cols % 8 != 0");
    pra_colsum_rows(CV(x), F(part), rows, cols, nrb, dt, S(s));
    check_launch("colsum_rows");
  });
  m.def("colsum_multi", [](std::vector<P> parts, std::vector<P> outs, std::vector<int> accs, int nblk, int cols,
                           int dt, P s) {
    const int n = (int)parts.size();
    if (n != (int)outs.size() || n != (int)accs.size() || n < 1 || n > 3)
      throw std::invalid_argument("colsum_multi: 1-3 jobs with matching lists");
    const float* pp[3];
    void* po[3];
    for (int j = 0; j < n; ++j) { pp[j] = CF(parts[j]); po[j] = V(outs[j]); }
    if (pra_colsum_multi(pp, po, accs.data(), n, nblk, cols, dt, S(s)) != 0)
      throw std::invalid_argument("colsum_multi: unsupported shape/alignment");
    check_launch("colsum_multi");
  });
  m.def("flash_fwd", [](P q, P k, P v, P o, P lse, int B, int H, int Sq, int Sk, int D, int64_t qsb, int64_t qss,
                        int64_t qsh, int64_t ksb, int64_t kss, int64_t ksh, int64_t vsb, int64_t vss, int64_t vsh,
                        float scale, int causal, int dt, P s) {
    int64_t st[9] = {qsb, qss, qsh, ksb, kss, ksh, vsb, vss, vsh};
    if (pra_flash_fwd(CV(q), CV(k), CV(v), V(o), F(lse), B, H, Sq, Sk, D, st, scale, causal, dt, S(s)) != 0)
      throw std::invalid_argument("flash_fwd: unsupported head_dim/dtype");
    check_launch("flash_fwd");
  });
  m.def("flash_fwd_ext", [](P q, P k, P v, P o, P lse, int B, int H, int Sq, int Sk, int D, std::vector<int64_t> st,
                            float scale, int causal, int dt, P cu_q, P cu_k, P mask, int64_t msb, int64_t msh,
                            int64_t msq, int mask_f32, float p_drop, uint64_t seed, uint64_t offset, P dbits, P dseq,
                            P s) {
    if (st.size() != 9) throw std::invalid_argument("flash_fwd_ext: need 9 strides");
    if (pra_flash_fwd_ext(CV(q), CV(k), CV(v), V(o), F(lse), B, H, Sq, Sk, D, st.data(), scale, causal, dt,
                          reinterpret_cast<const int*>(cu_q), reinterpret_cast<const int*>(cu_k), CV(mask), msb, msh,
                          msq, mask_f32, p_drop, seed, offset, reinterpret_cast<uint32_t*>(dbits),
                          reinterpret_cast<const uint64_t*>(dseq), S(s)) != 0)
      throw std::invalid_argument("flash_fwd_ext: unsupported arguments");
    check_launch("flash_fwd_ext");
  });
  m.def("flash_bwd_ext", [](P q, P k, P v, P dO, P lse, P delta, P dq, P dk, P dv, P dsT, int B, int H, int Sq, int Sk,
                            int D, std::vector<int64_t> st, float scale, int causal, int dt, P cu_q, P cu_k, P mask,
                            int64_t msb, int64_t msh, int64_t msq, int mask_f32, float p_drop, uint64_t seed,
                            uint64_t offset, P dbits, P dseq, P bsum, P s) {
    if (st.size() != 18) throw std::invalid_argument("flash_bwd_ext: need 18 strides");
    if (pra_flash_bwd_ext(CV(q), CV(k), CV(v), CV(dO), CF(lse), CF(delta), V(dq), V(dk), V(dv), V(dsT), B, H, Sq, Sk,
                          D, st.data(), scale, causal, dt, reinterpret_cast<const int*>(cu_q),
                          reinterpret_cast<const int*>(cu_k), CV(mask), msb, msh, msq, mask_f32, p_drop, seed,
                          offset, reinterpret_cast<uint32_t*>(dbits), reinterpret_cast<const uint64_t*>(dseq),
                          F(bsum), S(s)) != 0)
      throw std::invalid_argument("flash_bwd_ext: unsupported arguments");
    check_launch("flash_bwd_ext");
  });
  m.def("flash_bwd", [](P q, P k, P v, P dO, P o, P lse, P delta, P dq, P dk, P dv, P dsT, int B, int H, int Sq,
                        int Sk, int D, std::vector<int64_t> st, float scale, int causal, int dt, P bsum, P s) {
    if (st.size() != 18) throw std::invalid_argument("flash_bwd: need 18 strides");
    if (pra_flash_bwd(CV(q), CV(k), CV(v), CV(dO), CV(o), CF(lse), F(delta), V(dq), V(dk), V(dv), V(dsT), B, H, Sq, Sk,
                      D, st.data(), scale, causal, dt, F(bsum), S(s)) != 0)
      throw std::invalid_argument("flash_bwd: unsupported head_dim/dtype");
    check_launch("flash_bwd");
  });
}
