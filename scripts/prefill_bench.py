"""Prefill attention over the KV cache (K.mmha_prefill, FusedMultiTransformerDecoder.extend) next to
what the tree could do for the same job before it: (a) a fresh prompt against the context-phase
composition (rotary, repeat_interleave, causally masked SDPA, cache write), (b) a chunk appended to
a long prefix against gather / dequantise / concatenate / masked SDPA / write back, (c) extend of a
24-layer decoder against prefill of the same tokens from empty. Each pair is timed in the same run,
alternating, the median of the rounds reported, with the achieved TF/s (4 D flops per visible
query-key pair and head) and TB/s (cache rows streamed by the query tiles, plus qkv in and out).

usage: PYTHONPATH=. python scripts/prefill_bench.py [--quick] [--sections fresh,chunk,extend]"""
import argparse
import json
import statistics
import time

import torch


def bench(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def pair(new, old, window, rounds=5):
    """Median seconds per call of ``new`` and ``old``, alternated round by round; every round times
    as many calls as fill ``window`` seconds (sized from a short first measurement), so that a round
    is not a few milliseconds of clock and scheduler."""
    na, nb = (max(10, int(window / bench(f, 10))) for f in (new, old))
    a, b = [], []
    for _ in range(rounds):
        a.append(bench(new, na))
        b.append(bench(old, nb))
    return statistics.median(a), statistics.median(b), (na, nb)


def work(B, T, t0, H, KVH, D, cache_bytes, el=2):
    """(flops, bytes) of one prefill step: every sequence at prefix t0 with T new tokens."""
    pairs = T * t0 + T * (T + 1) // 2
    flops = 4 * D * pairs * H * B
    qt = 128 // (H // KVH)                                    # tokens per query tile
    keys = sum(t0 + min(T, j0 + qt) for j0 in range(0, T, qt))
    byts = B * KVH * keys * 2 * D * cache_bytes + B * T * (2 * H + 2 * KVH) * D * el + B * T * 2 * KVH * D * cache_bytes
    return flops, byts


def row(name, tn, to, flops, byts, **extra):
    print(json.dumps(dict(case=name, new_ms=round(tn * 1e3, 3), parent_ms=round(to * 1e3, 3),
                          speedup=round(to / tn, 2), new_tflops=round(flops / tn / 1e12, 1),
                          new_tbps=round(byts / tn / 1e12, 2), **extra)), flush=True)


def rot_tables(B, T, D, t0, dev):
    inv = 1.0 / (10000 ** (torch.arange(0, D // 2, dtype=torch.float32) / (D // 2)))
    ang = torch.arange(t0, t0 + T, dtype=torch.float32)[:, None] * torch.cat([inv, inv])[None, :]
    return torch.stack([ang.cos(), ang.sin()])[:, None].expand(2, B, T, D).contiguous().to(dev)


def rotate(x, rot):
    """Half-split rotation of x [B, T, h, D] in fp32 (rotary_dims 1), as the context phase does it."""
    c, s = rot[0][:, :, None].float(), rot[1][:, :, None].float()
    xf = x.float()
    half = x.shape[-1] // 2
    return (xf * c + torch.cat([-xf[..., half:], xf[..., :half]], -1) * s).to(x.dtype)


def sdpa_chunk(q, k, v, t0):
    """Masked SDPA of T queries [B, T, H, D] over t0 + T keys [B, t0 + T, H, D] with the materialised mask."""
    B, T = q.shape[:2]
    S = k.shape[1]
    m = torch.zeros(T, S, device=q.device, dtype=q.dtype).masked_fill(
        torch.arange(S, device=q.device)[None, :] > (t0 + torch.arange(T, device=q.device))[:, None], float('-inf'))
    return torch.nn.functional.scaled_dot_product_attention(
        q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), m.expand(B, 1, T, S)).transpose(1, 2)


def attention_rows(K, quick, fresh):
    B, H, KVH, D, dev, dt = 8, 32, 8, 128, 'cuda', torch.bfloat16
    T, t0 = (2048, 0) if fresh else (512, 4096)
    if quick:
        T, t0 = T // 4, t0 // 4
    L, rep = t0 + T, H // KVH
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, T, H + 2 * KVH, D, generator=g).to(dev, dt)
    rot = rot_tables(B, T, D, t0, dev)
    lens = torch.full((B,), t0, dtype=torch.int32, device=dev)
    base = torch.randn(2, B, KVH, L, D, generator=g).to(dev, dt)
    for kind in (['bf16'] if fresh else ['bf16', 'bf16 paged BS 64', 'uint8']):
        kw, cache, cb = dict(seq_lens=lens, rotary=rot, rotary_dims=1), base.clone(), 2
        if 'paged' in kind:
            BS = 64
            MB = L // BS
            table = torch.randperm(B * MB, generator=g).reshape(B, MB).to(dev)
            cache = torch.empty(2, B * MB, KVH, BS, D, device=dev, dtype=dt)
            cache[:, table] = base.view(2, B, KVH, MB, BS, D).permute(0, 1, 3, 2, 4, 5)
            kw['block_tables'] = table.int()
        if kind == 'uint8':
            kq = torch.full((KVH,), 127.0 / 5.0, device=dev)
            cache, cb = K.kv_quantize(base.view(2 * B, KVH, L, D), kq).view(2, B, KVH, L, D), 1
            kw.update(cache_k_quant_scales=kq, cache_v_quant_scales=kq)

        def new():
            return K.mmha_prefill(qkv, cache, t0, **kw)

        def old():
            q = rotate(qkv[:, :, :H], rot)
            k = rotate(qkv[:, :, H:H + KVH], rot)
            v = qkv[:, :, H + KVH:]
            if 'paged' in kind:                               # gather the prefix through the table
                pre = cache[:, table].permute(0, 1, 3, 2, 4, 5).reshape(2, B, KVH, L, D)[:, :, :, :t0]
            else:
                pre = cache[:, :, :, :t0]
            if kind == 'uint8':
                pre = K.kv_dequantize(pre.reshape(2 * B, KVH, t0, D), 1.0 / kq, dt).view(2, B, KVH, t0, D)
            kk = torch.cat([pre[0].transpose(1, 2), k], 1).repeat_interleave(rep, 2)
            vv = torch.cat([pre[1].transpose(1, 2), v], 1).repeat_interleave(rep, 2)
            o = sdpa_chunk(q, kk, vv, t0)
            kn, vn = k.transpose(1, 2), v.transpose(1, 2)     # write back
            if kind == 'uint8':
                kn, vn = K.kv_quantize(kn, kq), K.kv_quantize(vn, kq)
            if 'paged' in kind:
                pos = torch.arange(t0, L, device=dev)
                cache[0, table[:, pos // BS], :, pos % BS] = kn.transpose(1, 2)
                cache[1, table[:, pos // BS], :, pos % BS] = vn.transpose(1, 2)
            else:
                cache[0, :, :, t0:] = kn
                cache[1, :, :, t0:] = vn
            return o

        err = float((new().float() - old().float()).abs().max())
        tn, to, calls = pair(new, old, 0.05 if quick else 0.4)
        row(('fresh prompt ' if fresh else 'chunk on prefix ') + kind, tn, to, *work(B, T, t0, H, KVH, D, cb),
            B=B, T=T, prefix=t0, max_abs_diff=round(err, 4), calls_per_round=calls)


def extend_rows(quick):
    import paddle_ray_amd as paddle
    from paddle_ray_amd.incubate.nn import FusedMultiTransformer, FusedMultiTransformerDecoder
    paddle.set_device('gpu')
    E, Hh, KVH, layers, B, T = 2048, 16, 4, (4 if quick else 24), 8, 512
    paddle.seed(0)
    m = FusedMultiTransformer(E, Hh, 4 * E, num_layers=layers, gqa_group_size=KVH)
    m.to(dtype='bfloat16')
    m.eval()
    x = paddle.Tensor((torch.randn(B, T, E, generator=torch.Generator().manual_seed(1)) * 0.1).cuda().bfloat16())
    d1 = FusedMultiTransformerDecoder(m, B, T, use_graph=False)
    d2 = FusedMultiTransformerDecoder(m, B, T, use_graph=False)

    def new():
        d1.lens.zero_()
        d1.t.zero_()
        return d1.extend(x)

    def old():
        return d2.prefill(x)

    err = float((new()._t.float() - old()._t.float()).abs().max())
    scale = float(old()._t.float().abs().max())
    tn, to, calls = pair(new, old, 0.05 if quick else 0.5)
    print(json.dumps(dict(case=f'decoder {layers} layers, {T}-token chunk from empty', extend_ms=round(tn * 1e3, 2),
                          prefill_ms=round(to * 1e3, 2), speedup=round(to / tn, 2), max_abs_diff=round(err, 4),
                          max_abs_output=round(scale, 2), calls_per_round=calls)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--sections', default='fresh,chunk,extend')
    a = ap.parse_args()
    from paddle_ray_amd.ops import fused as K
    sections = set(a.sections.split(','))
    if 'fresh' in sections:
        attention_rows(K, a.quick, True)
    if 'chunk' in sections:
        attention_rows(K, a.quick, False)
    if 'extend' in sections:
        extend_rows(a.quick)


if __name__ == '__main__':
    main()
