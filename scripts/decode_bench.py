"""Decode-attention bandwidth: the HIP split-K kernel (K.mmha_decode) vs torch SDPA over
the same KV cache, a ragged batch (per-sequence seq_lens) next to its padded-and-masked twin,
grouped-query attention next to the expanded multi-head cache and the byte floor, end-to-end
FusedMultiTransformer decode steps/s, and the 8-bit KV cache next to the bf16 one (kernel rows
and the graph decoder), and the paged cache (a block pool behind shuffled block tables) next to
the contiguous cache of the same logical contents, and the multi-token step (T new tokens per
sequence in one cache pass) next to T single-token steps on the same cache.

usage: python scripts/decode_bench.py [--quick] [--sections plain,ragged,gqa,e2e,q8,paged,multi]"""
import argparse
import json
import math
import time

import torch


def bench(fn, iters=50, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_graph(fn, calls=20, reps=10):
    """Per-call time of ``fn`` replayed from one captured HIP graph of ``calls`` calls: the
    kernels back to back, without the host's launch path between them."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--sections', default='plain,ragged,gqa,e2e,q8,paged,multi',
                    help='comma-separated: plain, ragged, gqa, e2e, q8, paged, multi')
    a = ap.parse_args()
    sections = set(a.sections.split(','))
    from paddle_ray_amd.ops import fused as K
    if 'plain' in sections:
        plain_rows(a, K)
    if 'ragged' in sections:
        ragged_rows(K)
    if 'gqa' in sections:
        gqa_rows(K)
    if 'e2e' in sections:
        end_to_end(a)
    if 'q8' in sections:
        q8_rows(K)
    if 'paged' in sections:
        paged_rows(K)
    if 'multi' in sections:
        multi_rows(a, K)


def plain_rows(a, K):
    rows = []
    shapes = [(1, 32, 128, 4095), (8, 32, 128, 4095), (32, 16, 128, 2047), (64, 32, 128, 1023),
              (8, 16, 64, 8191)]
    if a.quick:
        shapes = shapes[:2]
    for B, H, D, t in shapes:
        L = t + 1
        qkv = torch.randn(B, 3, H, D, device='cuda', dtype=torch.bfloat16)
        cache = torch.randn(2, B, H, L, D, device='cuda', dtype=torch.bfloat16)
        hip = bench(lambda: K.mmha_decode(qkv, cache, t))
        q = qkv[:, 0].unsqueeze(2)                                 # [B, H, 1, D]

        def sdpa():
            cache[0, :, :, t] = qkv[:, 1]
            cache[1, :, :, t] = qkv[:, 2]
            return torch.nn.functional.scaled_dot_product_attention(q, cache[0], cache[1])
        ref = bench(sdpa)
        gb = 2 * B * H * (t + 1) * D * 2 / 1e9
        rows.append(dict(B=B, H=H, D=D, ctx=t + 1, hip_us=round(hip * 1e6, 1),
                         sdpa_us=round(ref * 1e6, 1), hip_TBps=round(gb / hip / 1e3, 2),
                         sdpa_TBps=round(gb / ref / 1e3, 2), splits=K._native.lib().mmha_splits(B, H, t)))
        print(json.dumps(rows[-1]), flush=True)


def ragged_rows(K):
    # ragged batch: every sequence at its own length (seq_lens), next to the same batch run
    # the only way possible without it — all sequences at 4095 behind an additive mask.
    # TB/s counts the bytes actually valid, sum(len_b + 1) K and V rows, for both.
    B, H, D, t = 8, 32, 128, 4095
    lens = [int(round(512 + i * (4095 - 512) / (B - 1))) for i in range(B)]
    qkv = torch.randn(B, 3, H, D, device='cuda', dtype=torch.bfloat16)
    cache = torch.randn(2, B, H, t + 1, D, device='cuda', dtype=torch.bfloat16)
    sl = torch.tensor(lens, dtype=torch.int32, device='cuda')
    mask = torch.zeros(B, t + 1, device='cuda')
    for b, n in enumerate(lens):
        mask[b, n:t] = float('-inf')
    ragged = bench(lambda: K.mmha_decode(qkv, cache, t, seq_lens=sl))
    masked = bench(lambda: K.mmha_decode(qkv, cache, t, mask))
    gb = 2 * H * sum(n + 1 for n in lens) * D * 2 / 1e9
    print(json.dumps(dict(B=B, H=H, D=D, lens=lens, ragged_us=round(ragged * 1e6, 1),
                          masked_us=round(masked * 1e6, 1), valid_GB=round(gb, 4),
                          ragged_TBps=round(gb / ragged / 1e3, 2),
                          masked_TBps=round(gb / masked / 1e3, 2))), flush=True)


def gqa_rows(K):
    # grouped-query attention (KVH K/V heads shared by H query heads): the GQA kernel on the
    # KVH-head cache, next to the plain kernel on the cache expanded to H heads (the only way
    # to run such a model without it) and the plain kernel at H = KVH (the same cache bytes with
    # 1/R of the scoring work: the byte floor). TB/s counts the KVH-head cache bytes.
    for H, KVH in ((32, 8), (64, 8)):
        B, D, t, r = 8, 128, 4095, H // KVH
        row = torch.randn(B, H + 2 * KVH, D, device='cuda', dtype=torch.bfloat16)
        cache = torch.randn(2, B, KVH, t + 1, D, device='cuda', dtype=torch.bfloat16)
        gqa = bench(lambda: K.mmha_decode(row, cache, t))
        qkv_x = torch.stack([row[:, :H], row[:, H:H + KVH].repeat_interleave(r, 1),
                             row[:, H + KVH:].repeat_interleave(r, 1)], 1).contiguous()
        cache_x = cache.repeat_interleave(r, 2).contiguous()
        expanded = bench(lambda: K.mmha_decode(qkv_x, cache_x, t))
        del cache_x
        qkv_s = torch.randn(B, 3, KVH, D, device='cuda', dtype=torch.bfloat16)
        same = bench(lambda: K.mmha_decode(qkv_s, cache, t))
        gb = 2 * B * KVH * (t + 1) * D * 2 / 1e9
        print(json.dumps(dict(B=B, H=H, KVH=KVH, D=D, ctx=t + 1, gqa_us=round(gqa * 1e6, 1),
                              expanded_us=round(expanded * 1e6, 1),
                              same_bytes_us=round(same * 1e6, 1), kv_GB=round(gb, 4),
                              gqa_TBps=round(gb / gqa / 1e3, 2),
                              splits=K._native.lib().mmha_splits(B, KVH, t))), flush=True)


def end_to_end(a):
    # end-to-end decode: 24-layer 2048-wide model (GPT-3 1.3B shape), batch 8
    import paddle_ray_amd as paddle
    from paddle_ray_amd.incubate.nn import FusedMultiTransformer
    paddle.set_device('gpu')
    E, H, L, B, ctx = 2048, 16, (4 if a.quick else 24), 8, 1024
    m = FusedMultiTransformer(E, H, 4 * E, num_layers=L)
    m.eval()
    m.to(dtype='bfloat16')
    caches = [paddle.Tensor(torch.zeros(2, B, H, ctx + 64, E // H, device='cuda',
                                        dtype=torch.bfloat16)) for _ in range(L)]
    x = paddle.Tensor(torch.randn(B, 1, E, device='cuda', dtype=torch.bfloat16))
    step = [ctx]

    def one():
        with paddle.no_grad():
            m(x, caches=caches, time_step=step[0])
    dt = bench(one, iters=20, warmup=3)
    print(json.dumps(dict(model=f'{L}x{E} FusedMultiTransformer decode', batch=B, ctx=ctx,
                          ms_per_token_step=round(dt * 1e3, 3),
                          tokens_per_s=round(B / dt, 1))), flush=True)
    # the same step replayed from one captured HIP graph (device-side position counter)
    from paddle_ray_amd.incubate.nn import FusedMultiTransformerDecoder
    dec = FusedMultiTransformerDecoder(m, B, ctx + 256)
    dec.t.fill_(ctx)
    xt = torch.randn(B, 1, E, device='cuda', dtype=torch.bfloat16)

    def gstep():
        dec.step(xt)
        dec.t.fill_(ctx)  # keep the context length fixed for the measurement
    dg = bench(gstep, iters=50, warmup=3)
    print(json.dumps(dict(model=f'{L}x{E} FusedMultiTransformerDecoder (HIP graph)', batch=B,
                          ctx=ctx, ms_per_token_step=round(dg * 1e3, 3),
                          tokens_per_s=round(B / dg, 1))), flush=True)
    # the graph decoder again, its caches 8-bit
    mib16 = sum(c[:, 0].numel() * c.element_size() for c in dec.caches) / 2 ** 20
    dec8 = FusedMultiTransformerDecoder(m, B, ctx + 256, kv_cache_dtype='int8')
    dec8.t.fill_(ctx)

    def gstep8():
        dec8.step(xt)
        dec8.t.fill_(ctx)
    d8 = bench(gstep8, iters=50, warmup=3)
    mib8 = sum(c[:, 0].numel() * c.element_size() for c in dec8.caches) / 2 ** 20
    print(json.dumps(dict(model=f'{L}x{E} FusedMultiTransformerDecoder (HIP graph, int8 KV cache)',
                          batch=B, ctx=ctx, ms_per_token_step=round(d8 * 1e3, 3),
                          bf16_cache_ms_per_token_step=round(dg * 1e3, 3),
                          tokens_per_s=round(B / d8, 1), cache_MiB_per_sequence_bf16=round(mib16, 1),
                          cache_MiB_per_sequence_int8=round(mib8, 1))), flush=True)


def q8_rows(K):
    # 8-bit KV cache (uint8 + per-head scales) next to the bf16 cache on the same problem: the
    # plain shapes at batch 1 and 8, then the two grouped-query shapes. TB/s counts the cache
    # bytes each kernel streams: 1 byte per element for int8, 2 for bf16. The *_graph_us columns
    # replay the same calls from a captured HIP graph, as the decoder runner does: at these
    # sizes the eager columns of the smaller rows are the host's launch path, not the kernel.
    for Bq, H, KVH in ((1, 32, 32), (8, 32, 32), (8, 32, 8), (8, 64, 8)):
        D, t = 128, 4095
        row = torch.randn(Bq, H + 2 * KVH, D, device='cuda', dtype=torch.bfloat16)
        if H == KVH:
            row = row.reshape(Bq, 3, H, D)
        cache16 = torch.randn(2, Bq, KVH, t + 1, D, device='cuda', dtype=torch.bfloat16)
        packed = torch.empty(4, 1, KVH, device='cuda')          # k quant, v quant, k dequant, v dequant
        packed[:2] = 127.0 / 4.5
        packed[2:] = 4.5 / 127.0
        cache8 = torch.stack([K.kv_quantize(cache16[i], packed[i, 0]) for i in range(2)])
        kw = dict(cache_k_quant_scales=packed[0, 0], cache_v_quant_scales=packed[1, 0],
                  cache_k_dequant_scales=packed[2, 0], cache_v_dequant_scales=packed[3, 0])
        bf = bench(lambda: K.mmha_decode(row, cache16, t))
        q8 = bench(lambda: K.mmha_decode(row, cache8, t, **kw))
        with torch.no_grad():
            bfg = bench_graph(lambda: K.mmha_decode(row, cache16, t))
            q8g = bench_graph(lambda: K.mmha_decode(row, cache8, t, **kw))
        elems = 2 * Bq * KVH * (t + 1) * D
        print(json.dumps(dict(B=Bq, H=H, KVH=KVH, D=D, ctx=t + 1, int8_us=round(q8 * 1e6, 1),
                              bf16_us=round(bf * 1e6, 1), int8_over_bf16=round(q8 / bf, 3),
                              int8_graph_us=round(q8g * 1e6, 1), bf16_graph_us=round(bfg * 1e6, 1),
                              int8_graph_TBps=round(elems / q8g / 1e12, 2),
                              bf16_graph_TBps=round(2 * elems / bfg / 1e12, 2),
                              int8_over_bf16_graph=round(q8g / bfg, 3))), flush=True)
        del cache16, cache8


def paged_rows(K):
    # paged cache: the same logical contents cut into blocks of a pool in shuffled physical
    # order (sequences interleaved) behind a device block table, next to the contiguous cache,
    # both replayed from a captured HIP graph as the decoder runner does. paged_over_contig is
    # the price of the table lookup; TB/s counts the cache bytes either kernel streams.
    D, t, Bq = 128, 4095, 8
    L = t + 1
    for H, KVH, BS, u8 in ((32, 32, 16, False), (32, 32, 64, False), (32, 32, 128, False),
                           (32, 8, 64, False), (32, 32, 64, True), (32, 8, 64, True)):
        row = torch.randn(Bq, H + 2 * KVH, D, device='cuda', dtype=torch.bfloat16)
        if H == KVH:
            row = row.reshape(Bq, 3, H, D)
        cache = torch.randn(2, Bq, KVH, L, D, device='cuda', dtype=torch.bfloat16)
        kw = {}
        if u8:
            packed = torch.empty(4, 1, KVH, device='cuda')
            packed[:2] = 127.0 / 4.5
            packed[2:] = 4.5 / 127.0
            cache = torch.stack([K.kv_quantize(cache[i], packed[i, 0]) for i in range(2)])
            kw = dict(cache_k_quant_scales=packed[0, 0], cache_v_quant_scales=packed[1, 0],
                      cache_k_dequant_scales=packed[2, 0], cache_v_dequant_scales=packed[3, 0])
        MB = L // BS
        perm = torch.randperm(Bq * MB, generator=torch.Generator().manual_seed(BS))
        table = perm.reshape(MB, Bq).t().contiguous().to(device='cuda', dtype=torch.int32)
        pool = torch.empty(2, Bq * MB, KVH, BS, D, device='cuda', dtype=cache.dtype)
        pool[:, table.long()] = cache.reshape(2, Bq, KVH, MB, BS, D).permute(0, 1, 3, 2, 4, 5)
        with torch.no_grad():
            same = bool(torch.equal(K.mmha_decode(row, cache, t, **kw),
                                    K.mmha_decode(row, pool, t, block_tables=table, **kw)))
            cg = bench_graph(lambda: K.mmha_decode(row, cache, t, **kw))
            pg = bench_graph(lambda: K.mmha_decode(row, pool, t, block_tables=table, **kw))
        ce = bench(lambda: K.mmha_decode(row, cache, t, **kw))
        pe = bench(lambda: K.mmha_decode(row, pool, t, block_tables=table, **kw))
        nbytes = 2 * Bq * KVH * L * D * cache.element_size()
        print(json.dumps(dict(paged=True, B=Bq, H=H, KVH=KVH, D=D, ctx=L, block_size=BS,
                              cache='uint8' if u8 else 'bf16', contig_graph_us=round(cg * 1e6, 1),
                              paged_graph_us=round(pg * 1e6, 1), paged_over_contig=round(pg / cg, 3),
                              contig_us=round(ce * 1e6, 1), paged_us=round(pe * 1e6, 1),
                              contig_graph_TBps=round(nbytes / cg / 1e12, 2),
                              paged_graph_TBps=round(nbytes / pg / 1e12, 2), bit_equal=same)), flush=True)
        del cache, pool


def _stats(samples, scale):
    v = sorted(x * scale for x in samples)
    return dict(samples=[round(x, 2) for x in (s * scale for s in samples)], median=round(v[len(v) // 2], 2),
                spread=round(v[-1] - v[0], 2))


def multi_rows(a, K, samples=5):
    # the multi-token step (T new tokens per sequence scored against the cache in one pass) next
    # to the single-token kernel on the same cache, both replayed from a captured HIP graph,
    # `samples` samples each. over_single is what T tokens cost in single steps' time;
    # over_T_single below 1 is the point of the feature: T tokens for less than T steps.
    D, Bq, BS = 128, 8, 64
    t, L = 4095, 4096 + BS                      # room for the new tokens, a whole number of blocks
    for H, KVH, T, kind in ((32, 32, 2, 'bf16'), (32, 32, 4, 'bf16'), (32, 32, 8, 'bf16'), (32, 8, 2, 'bf16'),
                            (32, 32, 4, 'uint8'), (32, 32, 4, 'paged')):
        rows = torch.randn(Bq, T, H + 2 * KVH, D, device='cuda', dtype=torch.bfloat16)
        one = rows[:, 0].contiguous()
        if H == KVH:
            one = one.reshape(Bq, 3, H, D)
        cache = torch.randn(2, Bq, KVH, L, D, device='cuda', dtype=torch.bfloat16)
        kw = {}
        if kind == 'uint8':
            packed = torch.empty(4, 1, KVH, device='cuda')
            packed[:2] = 127.0 / 4.5
            packed[2:] = 4.5 / 127.0
            cache = torch.stack([K.kv_quantize(cache[i], packed[i, 0]) for i in range(2)])
            kw = dict(cache_k_quant_scales=packed[0, 0], cache_v_quant_scales=packed[1, 0],
                      cache_k_dequant_scales=packed[2, 0], cache_v_dequant_scales=packed[3, 0])
        if kind == 'paged':
            MB = L // BS
            perm = torch.randperm(Bq * MB, generator=torch.Generator().manual_seed(BS))
            table = perm.reshape(MB, Bq).t().contiguous().to(device='cuda', dtype=torch.int32)
            pool = torch.empty(2, Bq * MB, KVH, BS, D, device='cuda', dtype=cache.dtype)
            pool[:, table.long()] = cache.reshape(2, Bq, KVH, MB, BS, D).permute(0, 1, 3, 2, 4, 5)
            cache, kw = pool, dict(block_tables=table)
        with torch.no_grad():
            single = [bench_graph(lambda: K.mmha_decode(one, cache, t, **kw)) for _ in range(samples)]
            multi = [bench_graph(lambda: K.mmha_decode_multi(rows, cache, t, **kw)) for _ in range(samples)]
        s1, sm = _stats(single, 1e6), _stats(multi, 1e6)
        print(json.dumps(dict(multi=True, B=Bq, H=H, KVH=KVH, D=D, ctx=t + 1, T=T, cache=kind,
                              single_graph_us=s1, multi_graph_us=sm,
                              over_single=round(sm['median'] / s1['median'], 3),
                              over_T_single=round(sm['median'] / (T * s1['median']), 3))), flush=True)
        del cache
    # end to end: the 24-layer graph decoder, step_multi(T = 4) next to four step calls
    import paddle_ray_amd as paddle
    from paddle_ray_amd.incubate.nn import FusedMultiTransformer, FusedMultiTransformerDecoder
    paddle.set_device('gpu')
    E, H, layers, B, ctx, T = 2048, 16, (4 if a.quick else 24), 8, 1024, 4
    m = FusedMultiTransformer(E, H, 4 * E, num_layers=layers)
    m.eval()
    m.to(dtype='bfloat16')
    d1 = FusedMultiTransformerDecoder(m, B, ctx + 256)
    dm = FusedMultiTransformerDecoder(m, B, ctx + 256)
    x = torch.randn(B, T, E, device='cuda', dtype=torch.bfloat16)
    d1.t.fill_(ctx)
    dm.t.fill_(ctx)

    def four():
        for j in range(T):
            d1.step(x[:, j:j + 1])
        d1.t.fill_(ctx)  # keep the context length fixed for the measurement

    def multi4():
        dm.step_multi(x)  # nothing advances without commit
    s4 = _stats([bench(four, iters=20, warmup=3) for _ in range(samples)], 1e3)
    sm = _stats([bench(multi4, iters=20, warmup=3) for _ in range(samples)], 1e3)
    print(json.dumps(dict(model=f'{layers}x{E} FusedMultiTransformerDecoder (HIP graph)', batch=B, ctx=ctx, T=T,
                          four_steps_ms=s4, step_multi_ms=sm,
                          step_multi_over_four_steps=round(sm['median'] / s4['median'], 3))), flush=True)


if __name__ == '__main__':
    main()
