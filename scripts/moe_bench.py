"""Top-k routed MoE FFN at decode sizes on the GPU: the moe_ffn.hip kernels against the 'ref'
composition and a byte floor.

    python scripts/moe_bench.py [--quick] [--samples 5] [--tall | --wo]

``--wo`` runs the decode cells over weight-only int8 / int4 expert weights (the moe_wo.hip kernel against
the bf16 kernels, the fp32 'ref' and the quantised byte floor; see wo_cell).
``--tall`` runs the prefill cells instead (M = 512 and 4096, the moe_tall.hip kernels; see tall_cell).
Decode cells: M = 8 and 32 tokens; E = 8 top-2 and E = 64 top-8; D = 2048; F = 1024 and 8192; SwiGLU; bf16.
Three figures per cell:
  hip    ``moe_route`` + ``moe_ffn`` on the 'hip' kernels, replayed from a HIP graph that walks over
         enough copies of the expert weights to exceed the 256 MB last-level cache, so every replay
         streams the selected experts from HBM as a decode step over a whole model does;
  ref    the 'ref' composition (fp32 products, a Python loop over the selected experts) on the same
         GPU and the same copies. It reads the routing on the host, so it cannot be captured and is
         timed eagerly between two events;
  floor  the bytes of the experts actually selected (W1 and W2 of every expert some token chose) over
         the 5.4 TB/s the decode-attention kernel reaches, the HBM rate this project has measured.
The two variants alternate inside each sample. One JSON line per cell; no GPU is an error, not a
fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_weight_only import ATTN_TBS, CACHE_BYTES, _graph, _stats, _time  # noqa: E402


def cell(M, E, k, D, F, quick, samples):
    from paddle_ray_amd.ops import fused as K
    from paddle_ray_amd.ops import registry as R
    dt, dev = torch.bfloat16, 'cuda'
    torch.manual_seed(M + E + F)
    x = torch.randn(M, D, device=dev).to(dt)
    gw = torch.randn(D, E, device=dev) * D ** -0.5
    per_expert = 3 * D * F * 2                                   # W1 [D, 2F] + W2 [F, D], bf16
    copies = 2 if quick else max(1, -(-CACHE_BYTES // (E * per_expert)))
    ws = [(torch.empty(E, D, 2 * F, device=dev, dtype=dt).normal_(0, D ** -0.5),
           torch.empty(E, F, D, device=dev, dtype=dt).normal_(0, F ** -0.5)) for _ in range(copies)]

    def hip():
        for w1, w2 in ws:
            ids, w = K.moe_route(x, gw, k)
            y = K.moe_ffn(x, ids, w, w1, w2)
        return y

    def ref():
        for w1, w2 in ws:
            ids, w = K._moe_route_ref(x, gw, k, True)
            y = K._moe_ffn_ref(x, ids, w, w1, w2, None, None, 4)
        return y

    R.reset_stats()
    with torch.no_grad():
        graph = _graph(hip)
        assert R.stats() == {('moe_route', 'hip'): 2 * copies, ('moe_ffn', 'hip'): 2 * copies}, R.stats()
        err = float((hip().float() - ref().float()).abs().max())
        active = int(K.moe_route(x, gw, k)[0].unique().numel())
        times = {'hip': [], 'ref': []}
        for _ in range(samples):
            times['hip'].append(_time(graph.replay, 2 if quick else 10) / copies)
            times['ref'].append(_time(ref, 1 if quick else 3) / copies)
    hip_us, ref_us = _stats(times['hip'], 1e6), _stats(times['ref'], 1e6)
    floor_us = active * per_expert / (ATTN_TBS * 1e12) * 1e6
    print(json.dumps(dict(M=M, E=E, top_k=k, D=D, F=F, active_experts=active, weight_copies=copies,
                          selected_bytes=active * per_expert, hip_us=hip_us, ref_us=ref_us,
                          floor_us=round(floor_us, 2), hip_over_floor=round(hip_us['median'] / floor_us, 2),
                          ref_over_hip=round(ref_us['median'] / hip_us['median'], 2),
                          max_abs_diff_hip_ref=round(err, 5))), flush=True)


WO_VARIANTS = (('int8', 'int8', -1), ('int4', 'int4', -1), ('int4 g128', 'int4', 128))


def wo_cell(M, E, k, D, F, quick, samples):
    """A decode cell over weight-only int8 / int4 experts (moe_wo.hip). Per variant, in the same run:
    hip = route + moe_ffn(weight_dtype=...) from a graph over enough copies of the byte images to
    exceed the last-level cache; bf16 = the moe_ffn.hip kernels from a graph over bf16 weights of the
    same shapes; ref = the fp32 'ref' of the quantised op (dequantise each used expert), eager, one
    copy; floor = the selected experts' quantised bytes and scales at ATTN_TBS. The byte images are
    random bytes (every byte is a level, or two), since the time does not depend on the levels."""
    from paddle_ray_amd.ops import fused as K
    from paddle_ray_amd.ops import registry as R
    dt, dev = torch.bfloat16, 'cuda'
    torch.manual_seed(M + E + F)
    x = torch.randn(M, D, device=dev).to(dt)
    gw = torch.randn(D, E, device=dev) * D ** -0.5
    active = int(K.moe_route(x, gw, k)[0].unique().numel())

    def copies_of(per_expert):
        return 2 if quick else max(1, -(-CACHE_BYTES // (E * per_expert)))

    def timed(fn, copies):
        R.reset_stats()
        graph = _graph(fn)
        assert all(b == 'hip' for _, b in R.stats()), R.stats()
        return lambda: _time(graph.replay, 2 if quick else 10) / copies

    with torch.no_grad():
        nb = copies_of(3 * D * F * 2)
        wb = [(torch.empty(E, D, 2 * F, device=dev, dtype=dt).normal_(0, D ** -0.5),
               torch.empty(E, F, D, device=dev, dtype=dt).normal_(0, F ** -0.5)) for _ in range(nb)]

        def bf16():
            for w1, w2 in wb:
                ids, w = K.moe_route(x, gw, k)
                y = K.moe_ffn(x, ids, w, w1, w2)
            return y
        t_bf16 = timed(bf16, nb)
        for name, wdt, g in WO_VARIANTS:
            pk, qmax = (2, 7.0) if wdt == 'int4' else (1, 127.0)
            s1 = torch.rand((E, D // g, 2 * F) if g > 0 else (E, 2 * F), device=dev) * (3 * D ** -0.5 / qmax)
            s2 = torch.rand((E, F // g, D) if g > 0 else (E, D), device=dev) * (3 * F ** -0.5 / qmax)
            per_expert = 3 * D * F // pk + 4 * (s1.numel() + s2.numel()) // E
            nq = copies_of(per_expert)
            wq = [(torch.randint(-128, 128, (E, 2 * F, D // pk), device=dev, dtype=torch.int8),
                   torch.randint(-128, 128, (E, D, F // pk), device=dev, dtype=torch.int8)) for _ in range(nq)]
            kw = dict(w1_scale=s1, w2_scale=s2, weight_dtype=wdt, group_size=g)

            def hip():
                for w1, w2 in wq:
                    ids, w = K.moe_route(x, gw, k)
                    y = K.moe_ffn(x, ids, w, w1, w2, **kw)
                return y

            def ref():
                ids, w = K._moe_route_ref(x, gw, k, True)
                return K._moe_ffn_wo_ref(x, ids, w, wq[-1][0], wq[-1][1], s1, s2, None, None, 4, wdt, g)
            t_hip = timed(hip, nq)
            err = float((hip().float() - ref().float()).abs().max())
            times = {'hip': [], 'bf16': [], 'ref': []}
            for _ in range(samples):
                times['hip'].append(t_hip())
                times['bf16'].append(t_bf16())
                times['ref'].append(_time(ref, 1))
            hip_us, bf16_us, ref_us = (_stats(times[n], 1e6) for n in ('hip', 'bf16', 'ref'))
            floor_us = active * per_expert / (ATTN_TBS * 1e12) * 1e6
            print(json.dumps(dict(wo=name, M=M, E=E, top_k=k, D=D, F=F, active_experts=active, weight_copies=nq,
                                  bf16_copies=nb, selected_bytes=active * per_expert, hip_us=hip_us,
                                  bf16_us=bf16_us, ref_us=ref_us, floor_us=round(floor_us, 2),
                                  hip_over_floor=round(hip_us['median'] / floor_us, 2),
                                  hip_over_bf16=round(hip_us['median'] / bf16_us['median'], 2),
                                  ref_over_hip=round(ref_us['median'] / hip_us['median'], 2),
                                  max_abs_diff_hip_ref=round(err, 5))), flush=True)
            del wq


GEMM_PFS = 1.51          # best bf16 rate of the project's training GEMM (README, MFMA GEMM row), PFLOP/s


def tall_cell(M, E, k, D, F, quick, samples):
    """Prefill sizes (moe_tall.hip): compute-bound, so one copy of the weights and a flop floor.
    hip = route + moe_ffn from a graph; ref = the 'ref' composition, eager (what ran before the tiled
    kernels); lib = a host-routed loop of bf16 library products per expert, eager, for information."""
    from paddle_ray_amd.ops import fused as K
    from paddle_ray_amd.ops import registry as R
    dt, dev = torch.bfloat16, 'cuda'
    torch.manual_seed(M + E + F)
    x = torch.randn(M, D, device=dev).to(dt)
    gw = torch.randn(D, E, device=dev) * D ** -0.5
    w1 = torch.empty(E, D, 2 * F, device=dev, dtype=dt).normal_(0, D ** -0.5)
    w2 = torch.empty(E, F, D, device=dev, dtype=dt).normal_(0, F ** -0.5)

    def hip():
        ids, w = K.moe_route(x, gw, k)
        return K.moe_ffn(x, ids, w, w1, w2)

    def ref():
        ids, w = K._moe_route_ref(x, gw, k, True)
        return K._moe_ffn_ref(x, ids, w, w1, w2, None, None, 4)

    def lib():
        ids, w = K.moe_route(x, gw, k)
        flat = ids.reshape(-1).long()
        slots = torch.empty(M * k, D, dtype=dt, device=dev)
        for e in flat.unique().tolist():
            sel = (flat == e).nonzero().squeeze(1)
            z = x[sel // k] @ w1[e]
            slots[sel] = (torch.nn.functional.silu(z[:, :F]) * z[:, F:]) @ w2[e]
        return (slots.view(M, k, D).float() * w[..., None]).sum(1).to(dt)

    R.reset_stats()
    with torch.no_grad():
        graph = _graph(hip)
        assert R.stats() == {('moe_route', 'hip'): 2, ('moe_ffn', 'hip'): 2}, R.stats()
        err = float((hip().float() - ref().float()).abs().max())
        times = {'hip': [], 'ref': [], 'lib': []}
        for _ in range(samples):
            times['hip'].append(_time(graph.replay, 2 if quick else 10))
            times['ref'].append(_time(ref, 1 if quick else 2))
            times['lib'].append(_time(lib, 1 if quick else 3))
    hip_us, ref_us, lib_us = (_stats(times[n], 1e6) for n in ('hip', 'ref', 'lib'))
    floor_us = 2.0 * M * k * 3 * D * F / (GEMM_PFS * 1e15) * 1e6
    print(json.dumps(dict(tall=True, M=M, E=E, top_k=k, D=D, F=F, pairs=M * k, hip_us=hip_us, ref_us=ref_us,
                          lib_us=lib_us, floor_us=round(floor_us, 2),
                          hip_over_floor=round(hip_us['median'] / floor_us, 2),
                          hip_over_lib=round(hip_us['median'] / lib_us['median'], 2),
                          ref_over_hip=round(ref_us['median'] / hip_us['median'], 2),
                          faster_beyond_spreads=ref_us['median'] - hip_us['median'] >
                          ref_us['spread'] + hip_us['spread'],
                          max_abs_diff_hip_ref=round(err, 5))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true', help='small cells, two copies: a rehearsal, not a measurement')
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--tall', action='store_true', help='the prefill cells (M 512 and 4096) instead of the decode ones')
    ap.add_argument('--wo', action='store_true', help='the decode cells over weight-only int8 / int4 experts')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench: no GPU (the measurement does not fall back to the CPU)")
    from paddle_ray_amd.ops import _native
    _native.require()
    for E, k in ((8, 2), (64, 8)):
        for F in (1024, 8192):
            for M in (512, 4096) if a.tall else ():
                if a.quick:
                    tall_cell(M, E, k, 256, F // 8, True, 1)
                else:
                    tall_cell(M, E, k, 2048, F, False, a.samples)
                torch.cuda.empty_cache()
            for M in () if a.tall else (8, 32):
                run = wo_cell if a.wo else cell
                if a.quick:
                    run(M, E, k, 256, F // 8, True, 1)
                else:
                    run(M, E, k, 2048, F, False, a.samples)
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
