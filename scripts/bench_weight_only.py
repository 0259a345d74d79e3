"""Weight-only int8 / int4 linear on the GPU against the bf16 library product it replaces.

    python scripts/bench_weight_only.py [--quick] [--sections products,decoder,tall,prefill] [--samples 5]

Part 1 times the four products of a 2048-wide, 8192-FFN transformer layer at M = 8 and 32 rows:
int8 per channel, int4 per channel and int4 with group 128 on ``ops.fused.weight_only_linear``, and
the parent's path for the same product (``torch.mm``, or ``torch.addmm`` + GELU for FFN1) on bf16
weights. Every variant is replayed from a HIP graph that walks over enough copies of the weight to
exceed the 256 MB last-level cache, so each launch streams its weight from HBM as a decode step
over a whole model does. Variants alternate inside each of five samples. Bytes are computed from
the shapes: the weight image, its scales, x, y and the bias.
Part 2 times ``step`` and ``step_multi(T = 4)`` of the 24-layer 2048-wide graph decoder of
``profiles/decode_multi.md`` with ``weight_only`` None / int8 / int4.
Section ``tall`` times the same four products at M = 128, 512 and 2048 rows, where the tiled kernel
of ``wo_tall.hip`` runs, for int8 and int4 with per-channel and group-128 scales, against what the
call did before that kernel (``ref``: dequantise to fp32 + the fp32 library product), what the
decoder's prefill did (``dequant+mm``: ``weight_dequantize`` to bf16 + the bf16 library product) and
the bf16 library product alone on a weight dequantised beforehand (``mm``), the floor for a kernel
that does the same flops. The weights (at most 32 MB) stay in the last-level cache, as they do
between the row tiles of a prompt. Section ``prefill`` times ``prefill`` of the 24-layer decoder and
reads its peak allocated memory with the products on the kernels and with the per-layer dequantised
copies (``ops.fused.WO_DECODER_MAX_ROWS`` set to ``WO_MAX_ROWS``, the behaviour before wo_tall.hip).
One JSON line per measurement; no GPU is an error, not a fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ATTN_TBS = 5.4           # what the decode-attention kernel reaches at ctx 4096, TB/s
CACHE_BYTES = 512 << 20  # walk over at least this much weight per graph replay


def _stats(xs, scale):
    xs = [x * scale for x in xs]
    return dict(samples=[round(x, 2) for x in xs], median=round(statistics.median(xs), 2),
                spread=round(max(xs) - min(xs), 2))


def _graph(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def _time(replay, iters):
    """Seconds per replay over ``iters`` replays between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    replay()
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def products(quick, samples):
    from paddle_ray_amd.ops import fused as K
    from paddle_ray_amd.ops import registry as R
    shapes = [('qkv', 2048, 6144, False), ('out', 2048, 2048, False), ('ffn1', 2048, 8192, True),
              ('ffn2', 8192, 2048, False)]
    variants = [('bf16 library', None, -1), ('int8', 'int8', -1), ('int4', 'int4', -1), ('int4 g128', 'int4', 128)]
    gen = torch.Generator().manual_seed(0)
    for name, Kd, N, epi in shapes[:1] if quick else shapes:
        w = torch.randn(Kd, N, generator=gen) * 0.05
        bias = torch.randn(N, generator=gen).bfloat16().cuda() if epi else None
        for M in (8, 32):
            x = torch.randn(M, Kd, generator=gen).bfloat16().cuda()
            runs = {}
            for label, wdt, g in variants:
                if wdt is None:
                    one, wbytes = [w.bfloat16().cuda()], Kd * N * 2
                else:
                    q, s = K.weight_quantize(w, wdt, g)
                    one, wbytes = [q.cuda(), s.cuda()], q.numel() + s.numel() * 4
                copies = 2 if quick else -(-CACHE_BYTES // wbytes)
                ws = [[t.clone() for t in one] for _ in range(copies)]

                def fn(ws=ws, wdt=wdt, g=g):
                    for c in ws:
                        if wdt is not None:
                            y = K.weight_only_linear(x, c[0], c[1], bias, 'gelu' if epi else None, wdt, g)
                        elif epi:
                            y = torch.nn.functional.gelu(torch.addmm(bias, x, c[0]))
                        else:
                            y = torch.mm(x, c[0])
                    return y
                R.reset_stats()
                with torch.no_grad():
                    graph = _graph(fn)
                if wdt is not None:
                    assert R.stats().get(('weight_only_linear', 'hip'), 0) == 2 * copies, R.stats()
                total = wbytes + (M * Kd + M * N + (N if epi else 0)) * 2
                runs[label] = (graph, copies, total, ws)
            times = {label: [] for label in runs}
            for _ in range(samples):                       # the variants alternate inside a sample
                for label, (graph, copies, _, _) in runs.items():
                    times[label].append(_time(graph.replay, 2 if quick else 10) / copies)
            base = statistics.median(times['bf16 library'])
            for label, (_, copies, total, _) in runs.items():
                st = _stats(times[label], 1e6)
                tbs = total / (st['median'] * 1e-6) / 1e12
                print(json.dumps(dict(product=name, K=Kd, N=N, M=M, variant=label, us=st, bytes=total,
                                      tb_per_s=round(tbs, 2), share_of_attn=round(tbs / ATTN_TBS, 2),
                                      over_bf16=round(st['median'] / (base * 1e6), 3), weight_copies=copies)),
                      flush=True)
            del runs


def decoder(quick, samples):
    import paddle_ray_amd as paddle
    from paddle_ray_amd.incubate.nn import FusedMultiTransformer, FusedMultiTransformerDecoder
    paddle.set_device('gpu')
    E, H, layers, B, ctx, T = 2048, 16, (2 if quick else 24), 8, 1024, 4
    m = FusedMultiTransformer(E, H, 4 * E, num_layers=layers)
    m.eval()
    m.to(dtype='bfloat16')
    x = torch.randn(B, T, E, device='cuda', dtype=torch.bfloat16)
    decs = {}
    for wo in (None, 'int8', 'int4'):
        d = FusedMultiTransformerDecoder(m, B, ctx + 256, weight_only=wo)
        d.t.fill_(ctx)

        def step(d=d):
            d.step(x[:, :1])
            d.t.fill_(ctx)   # keep the context length fixed for the measurement

        def multi(d=d):
            d.step_multi(x)  # nothing advances without commit
        step(), multi()
        decs[wo] = (step, multi)
    times = {(wo, k): [] for wo in decs for k in (0, 1)}
    for _ in range(samples):
        for wo, fns in decs.items():
            for k, fn in enumerate(fns):
                times[(wo, k)].append(_time(fn, 5 if quick else 20))
    for (wo, k), ts in times.items():
        st = _stats(ts, 1e3)
        base = statistics.median(times[(None, k)]) * 1e3
        print(json.dumps(dict(model=f'{layers}x{E} FusedMultiTransformerDecoder (HIP graph)', batch=B, ctx=ctx,
                              call='step' if k == 0 else f'step_multi(T={T})', weight_only=wo, ms=st,
                              over_bf16=round(st['median'] / base, 3))), flush=True)


def tall(quick, samples):
    from paddle_ray_amd.ops import fused as K
    from paddle_ray_amd.ops import registry as R
    shapes = [('qkv', 2048, 6144, False), ('out', 2048, 2048, False), ('ffn1', 2048, 8192, True),
              ('ffn2', 8192, 2048, False)]
    variants = [('int8', 'int8', -1), ('int8 g128', 'int8', 128), ('int4', 'int4', -1), ('int4 g128', 'int4', 128)]
    gen = torch.Generator().manual_seed(0)
    for name, Kd, N, epi in shapes[:1] if quick else shapes:
        w = torch.randn(Kd, N, generator=gen) * 0.05
        bias = torch.randn(N, generator=gen).bfloat16().cuda() if epi else None
        act = 'gelu' if epi else None
        for label, wdt, g in variants[:1] if quick else variants:
            q, s = (t.cuda() for t in K.weight_quantize(w, wdt, g))
            wd = K.weight_dequantize(q, s, wdt, g, torch.bfloat16)
            for M in (128,) if quick else (128, 512, 2048):
                x = torch.randn(M, Kd, generator=gen).bfloat16().cuda()

                def mm(wd=wd):
                    return torch.nn.functional.gelu(torch.addmm(bias, x, wd)) if epi else torch.mm(x, wd)
                paths = {'kernel': lambda: K.weight_only_linear(x, q, s, bias, act, wdt, g),
                         'ref': lambda: K._wo_ref(x, q, s, bias, K._ACT[act], wdt, g),
                         'dequant+mm': lambda: mm(K.weight_dequantize(q, s, wdt, g, torch.bfloat16)),
                         'mm': mm}
                R.reset_stats()
                with torch.no_grad():
                    y, yr = paths['kernel'](), paths['mm']()
                assert R.stats() == {('weight_only_linear', 'hip'): 1}, R.stats()
                err = float((y.float() - yr.float()).abs().max() / yr.float().abs().max())
                times = {k: [] for k in paths}
                with torch.no_grad():
                    for _ in range(samples):               # the paths alternate inside a sample
                        for k, fn in paths.items():
                            times[k].append(_time(fn, (2 if quick else 5) if k in ('ref', 'dequant+mm') else
                                                  (5 if quick else 100)))
                med = {k: statistics.median(v) for k, v in times.items()}
                for k in paths:
                    print(json.dumps(dict(section='tall', product=name, K=Kd, N=N, M=M, variant=label, path=k,
                                          us=_stats(times[k], 1e6),
                                          tflops=round(2.0 * M * N * Kd / med[k] / 1e12, 1),
                                          over_mm=round(med[k] / med['mm'], 2),
                                          kernel_vs_mm_max_rel_diff=round(err, 5))), flush=True)


def prefill(quick, samples):
    import paddle_ray_amd as paddle
    from paddle_ray_amd.incubate.nn import FusedMultiTransformer, FusedMultiTransformerDecoder
    from paddle_ray_amd.device import cuda as mem
    from paddle_ray_amd.ops import fused as K
    paddle.set_device('gpu')
    E, H, layers, B = 2048, 16, (2 if quick else 24), 8
    m = FusedMultiTransformer(E, H, 4 * E, num_layers=layers)
    m.eval()
    m.to(dtype='bfloat16')
    for wo in ('int8', 'int4'):
        d = FusedMultiTransformerDecoder(m, B, 256 + 8, weight_only=wo, use_graph=False)
        for S in (64,) if quick else (16, 64, 256):        # 128, 512 and 2048 rows
            x = paddle.Tensor(torch.randn(B, S, E, device='cuda', dtype=torch.bfloat16))
            limits = {'kernels': None, 'dequantised copies': K.WO_MAX_ROWS}
            times, peak = {k: [] for k in limits}, {}
            try:
                for _ in range(samples + 1):               # the first round warms up and reads the peaks
                    for k, lim in limits.items():
                        K.WO_DECODER_MAX_ROWS = lim
                        torch.cuda.synchronize()
                        base = mem.memory_allocated()
                        mem.reset_max_memory_allocated()
                        t = _time(lambda: d.prefill(x), 1 if quick else 3)
                        if k in peak:
                            times[k].append(t)
                        peak[k] = mem.max_memory_allocated() - base
            finally:
                K.WO_DECODER_MAX_ROWS = None
            base = statistics.median(times['dequantised copies'])
            for k in limits:
                st = _stats(times[k], 1e3)
                print(json.dumps(dict(section='prefill', model=f'{layers}x{E}', batch=B, S=S, rows=B * S,
                                      weight_only=wo, products=k, ms=st, peak_mb_above_resident=round(peak[k] / 2**20, 1),
                                      over_dequantised=round(st['median'] / (base * 1e3), 3))), flush=True)
        del d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true', help='one product, two layers: a rehearsal, not a measurement')
    ap.add_argument('--sections', default='products,decoder')
    ap.add_argument('--samples', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_only: no GPU (the measurement does not fall back to the CPU)")
    from paddle_ray_amd.ops import _native
    _native.require()
    if 'products' in a.sections:
        products(a.quick, a.samples)
    if 'decoder' in a.sections:
        decoder(a.quick, a.samples)
    if 'tall' in a.sections:
        tall(a.quick, a.samples)
    if 'prefill' in a.sections:
        prefill(a.quick, a.samples)


if __name__ == '__main__':
    main()
