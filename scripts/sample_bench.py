"""Token sampling: the fused top-k / top-p kernel (ops.fused.sample_top_p, sample.hip) next to the
PyTorch composition a caller would write without it (softmax, sort, cumsum, mask, multinomial) and
to the floor of any sampler (one softmax + argmax pass), on the same GPU tensors.

The kernel and the floor are timed as the per-call time of a captured HIP graph of CALLS calls,
replayed REPS times (the kernels back to back, as in a captured decode step). The composition is
timed with eager launches between two device synchronisations, CALLS * REPS calls per sample, and
is never captured: replaying a graph that holds ``torch.sort`` of a [64, 50304] tensor ends in an
illegal address inside rocprim's onesweep radix-sort kernel.
Eager timing includes the host's launch path of the composition's ~10 kernels; ``hip_eager_us`` is
the kernel timed the same way, for a like-for-like ratio. Five samples per cell; the median and
the spread are printed. GB/s counts the bytes of x once per call. ``passes`` is how often the
kernel reads a row: the max pass, one per 8 key bits (2 for 16-bit inputs, 4 for fp32) and the
draw, plus one more for rows whose limit cuts a group of equal values.

usage: python -m scripts.sample_bench [--rows 8,64,256] [--vocab 50304,131072]
           [--dtypes bfloat16,float32] [--no-composition]"""
import argparse
import json
import time

import torch

CALLS, REPS, SAMPLES = 10, 5, 5


def bench_graph(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (REPS * CALLS)


def bench_eager(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS * CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (REPS * CALLS)


def _stats(fn, how):
    v = sorted(how(fn) * 1e6 for _ in range(SAMPLES))
    return dict(median=round(v[len(v) // 2], 1), spread=round(v[-1] - v[0], 1))


def composition(x, temperature, top_k, top_p):
    p = torch.softmax(x.float() / temperature, -1)
    sp, idx = torch.sort(p, -1, descending=True)
    drop = (sp.cumsum(-1) - sp) >= top_p
    if top_k:
        drop[:, top_k:] = True
    sp = sp.masked_fill(drop, 0.0)
    return idx.gather(1, torch.multinomial(sp, 1))


def floor(x):
    return torch.softmax(x.float(), -1).argmax(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', default='8,64,256')
    ap.add_argument('--vocab', default='50304,131072')
    ap.add_argument('--dtypes', default='bfloat16,float32')
    ap.add_argument('--no-composition', action='store_true')
    a = ap.parse_args()
    from paddle_ray_amd.ops import fused as K
    from paddle_ray_amd.ops import registry
    assert torch.cuda.is_available(), "sample_bench needs the GPU"
    for dtype in (getattr(torch, d) for d in a.dtypes.split(',')):
        for V in (int(v) for v in a.vocab.split(',')):
            for Rn in (int(r) for r in a.rows.split(',')):
                x = (torch.randn(Rn, V, device='cuda', generator=torch.Generator('cuda').manual_seed(V + Rn)) * 4
                     ).to(dtype)
                step = torch.zeros(1, dtype=torch.int64, device='cuda')
                nbytes = x.numel() * x.element_size()
                for top_k, top_p in ((50, 0.9), (0, 0.9)):
                    t = torch.ones(Rn, device='cuda')
                    k = torch.full((Rn,), top_k, dtype=torch.int32, device='cuda')
                    p = torch.full((Rn,), top_p, device='cuda')
                    cell = dict(R=Rn, V=V, dtype=str(dtype)[6:], top_k=top_k, top_p=top_p)

                    def hip_call():
                        return K.sample_top_p(x, t, k, p, seed=1, step=step)
                    registry.reset_stats()
                    with torch.no_grad():
                        hip = _stats(hip_call, bench_graph)
                        assert registry.stats().get(('sample_top_p', 'hip'), 0) > 0
                        fl = _stats(lambda: floor(x), bench_graph)
                    print(json.dumps(dict(cell, hip_graph_us=hip, floor_graph_us=fl,
                                          hip_GBps=round(nbytes / hip['median'] / 1e3, 1),
                                          hip_over_floor=round(hip['median'] / fl['median'], 2),
                                          passes='4-5' if dtype != torch.float32 else '6-7')), flush=True)
                    if a.no_composition:
                        continue
                    with torch.no_grad():
                        comp = _stats(lambda: composition(x, 1.0, top_k, top_p), bench_eager)
                        hip_e = _stats(hip_call, bench_eager)
                    print(json.dumps(dict(cell, composition_eager_us=comp, hip_eager_us=hip_e,
                                          composition_over_hip_graph=round(comp['median'] / hip['median'], 2),
                                          composition_over_hip_eager=round(comp['median'] / hip_e['median'], 2))),
                          flush=True)
                del x


if __name__ == '__main__':
    main()
