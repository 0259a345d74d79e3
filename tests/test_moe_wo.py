"""Weight-only int8 / int4 expert weights in the routed MoE FFN: ``ops.fused.moe_ffn(weight_dtype=...)`` and
``incubate.nn.functional.fused_moe(quant_method=...)`` ('ref' on the CPU, the moe_wo.hip kernel on the GPU)
against a float64 per-token loop over the dequantised weights.

Inputs as in test_fused_moe.py: tokens are multiples of 1/4 in [-1, 1] and gate weights multiples of 1/8, so
every logit is exact in fp32 (|logit| < 2^9 in units of 1/32) and the ids equal those of a float64 stable sort."""
import functools

import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import functional as FF
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

_U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
#          M    E   k   D    F
_SHAPES = [(1, 4, 1, 64, 64),        # one row, empty experts, the int4 64-k tail alone in both products
           (5, 8, 2, 128, 64),       # one int4 superchunk, then the tail in the second product
           (17, 8, 2, 192, 128),     # expert 3 takes all 17 rows (two row blocks); superchunk + tail, 3 groups of 64
           (64, 16, 8, 256, 128),    # the row limit, and group 128 spanning two chunks
           (130, 4, 2, 64, 64)]      # the 64-token chunk loop: 64 + 64 + 2
_ALL = pytest.mark.parametrize(
    'shape,wdt,g,act,dtype',
    [(s, w, g, a, d) for s in _SHAPES for w in ('int8', 'int4') for g in (-1, 64, 128) if g < 0 or s[3] % g + s[4] % g == 0
     for a in ('swiglu', 'gelu') for d in (torch.bfloat16, torch.float16)],
    ids=lambda v: str(v).replace('torch.', '').replace(' ', ''))


@functools.lru_cache(None)
def _case(shape, wdt, g, act, dtype):
    """Inputs (CPU; bias with SwiGLU) and the float64 oracle: (x, gw, q1, q2, s1, s2, b1, b2, ids, w64, ref, S)."""
    M, E, k, D, F = shape
    gen = torch.Generator().manual_seed(11 + M + E)
    x = torch.randint(-4, 5, (M, D), generator=gen).to(dtype) / 4
    gw = torch.randint(-4, 5, (D, E), generator=gen).float() / 8
    if M == 17:                       # logit 3 >= 256 - 191/2 > 96 >= any other; still exact in fp32
        x[:, 0], gw[0, 3] = 1, 256
    N1, bias = (2 * F if act == 'swiglu' else F), act == 'swiglu'
    q1, s1 = K.weight_quantize(torch.randn(E, D, N1, generator=gen) / D ** 0.5, wdt, g)
    q2, s2 = K.weight_quantize(torch.randn(E, F, D, generator=gen) / F ** 0.5, wdt, g)
    b1 = (0.1 * torch.randn(E, 1, N1, generator=gen)).to(dtype) if bias else None
    b2 = (0.1 * torch.randn(E, 1, D, generator=gen)).to(dtype) if bias else None
    logits = x.double() @ gw.double()
    assert torch.equal(logits, (x.float() @ gw).double())
    ids = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]
    assert M != 17 or int((ids == 3).sum()) == 17
    w = torch.softmax(logits, -1).gather(1, ids)
    w = w / w.sum(1, keepdim=True)
    W1 = K.weight_dequantize(q1, s1, wdt, g, torch.float32).double()
    W2 = K.weight_dequantize(q2, s2, wdt, g, torch.float32).double()
    ref, S = torch.zeros(M, D, dtype=torch.float64), torch.zeros(M, D, dtype=torch.float64)
    for m in range(M):
        for j in range(k):
            e = int(ids[m, j])
            z = x[m].double() @ W1[e] + (b1[e, 0].double() if bias else 0)
            h = torch.nn.functional.silu(z[:F]) * z[F:] if act == 'swiglu' else torch.nn.functional.gelu(z)
            o, a = h @ W2[e], h.abs() @ W2[e].abs()
            if bias:
                o, a = o + b2[e, 0].double(), a + b2[e, 0].double().abs()
            ref[m] += w[m, j] * o
            S[m] += w[m, j] * a
    return x, gw, q1, q2, s1, s2, b1, b2, ids.to(torch.int32), w, ref, S


def _bound(y, ref, S):
    """test_fused_moe.py's bound, |y - ref| <= 2u (|ref| + S); scaling the sum instead of each weight
    (2^-24 relative) is inside the factor 2."""
    assert y.dtype in _U and y.shape == ref.shape
    worst = float(((y.double().cpu() - ref).abs() / (2 * _U[y.dtype] * (ref.abs() + S))).max())
    print(f"worst |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


def _run_both(dev, shape, wdt, g, act, dtype):
    x, gw, q1, q2, s1, s2, b1, b2, ids, w, ref, S = (None if t is None else t.to(dev)
                                                     for t in _case(shape, wdt, g, act, dtype))
    kw = dict(w1_scale=s1, w2_scale=s2, weight_dtype=wdt, group_size=g)
    _bound(K.moe_ffn(x, ids, w.float(), q1, q2, b1, b2, act, **kw), ref.cpu(), S.cpu())
    P = paddle.Tensor
    y = FF.fused_moe(P(x[None]), P(gw), P(q1), P(q2), b1 if b1 is None else P(b1), P(s1), b2 if b2 is None else P(b2),
                     P(s2), quant_method='weight_only_' + wdt, moe_topk=shape[2])
    assert tuple(y._t.shape) == (1,) + tuple(x.shape)
    _bound(y._t[0], ref.cpu(), S.cpu())
    return lambda: K.moe_ffn(x, ids, w.float(), q1, q2, b1, b2, act, **kw)


# ----------------------------------------------------------------------------- CPU
@_ALL
def test_ref_against_float64(shape, wdt, g, act, dtype):
    R.reset_stats()
    _run_both('cpu', shape, wdt, g, act, dtype)
    assert ('moe_ffn_wo', 'hip') not in R.stats() and R.stats()[('moe_ffn_wo', 'ref')] == 2


@pytest.mark.parametrize('wdt', ['int8', 'int4'])
@pytest.mark.parametrize('g', [-1, 64])
def test_stacked_quantize_is_the_2d_call_per_expert(wdt, g):
    w = torch.randn(3, 192, 32, generator=torch.Generator().manual_seed(5)).bfloat16()
    q, s = K.weight_quantize(w, wdt, g)
    assert tuple(q.shape) == (3, 32, 192 // (2 if wdt == 'int4' else 1)) and s.shape == ((3, 3, 32) if g > 0 else (3, 32))
    back = K.weight_dequantize(q, s, wdt, g, torch.float32)
    for e in range(3):
        qe, se = K.weight_quantize(w[e], wdt, g)
        assert torch.equal(q[e], qe) and torch.equal(s[e], se)
        assert torch.equal(back[e], K.weight_dequantize(qe, se, wdt, g, torch.float32))


def test_errors():
    x, gw, q1, q2, s1, s2, b1, b2, ids, w, _, _ = _case(_SHAPES[1], 'int4', 64, 'swiglu', torch.bfloat16)
    kw = dict(x=x, ids=ids, weights=w.float(), w1=q1, w2=q2, act='swiglu', w1_scale=s1, w2_scale=s2,
              weight_dtype='int4', group_size=64)
    for bad in (dict(w1_scale=s1[:, 0]), dict(w2_scale=None), dict(group_size=128), dict(w1=q1[:, :64]),
                dict(weight_dtype='int8')):                                 # group 128 does not divide F = 64
        with pytest.raises(ValueError, match=r'\(\d+, |group_size = 128'):
            K.moe_ffn(**{**kw, **bad})
    P = paddle.Tensor
    with pytest.raises(ValueError, match=r'\(8, 128\)\)'):
        FF.fused_moe(P(x[None]), P(gw), P(q1), P(q2), None, P(s1), None, P(s2[:, 0]), 'weight_only_int4')
    with pytest.raises(NotImplementedError, match='weight_quantize'):
        FF.fused_moe(P(x[None]), P(gw), P(q1.float()), P(q2.float()), None, P(s1), None, P(s2), 'weight_only_int4')
    with pytest.raises(NotImplementedError, match='fp8'):
        FF.fused_moe(P(x[None]), P(gw), P(q1), P(q2), None, P(s1), None, P(s2), 'fp8')


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@_ALL
def test_hip_against_float64_and_reproducible(shape, wdt, g, act, dtype):
    R.reset_stats()
    again = _run_both('cuda', shape, wdt, g, act, dtype)
    assert R.stats() == {('moe_ffn_wo', 'hip'): 2, ('moe_route', 'hip'): 1}
    assert torch.equal(again(), again())


@pytest.mark.gpu
@pytest.mark.parametrize('wdt,g', [('int8', -1), ('int4', 64)])
def test_graph_replay_follows_the_routing(wdt, g):
    c = _case(_SHAPES[1], wdt, g, 'swiglu', torch.bfloat16)
    x, gw, q1, q2, s1, s2, b1, b2 = (paddle.Tensor(t.cuda()) for t in c[:8])
    x = paddle.Tensor(x._t[None].clone())

    def call():
        return FF.fused_moe(x, gw, q1, q2, b1, s1, b2, s2, 'weight_only_' + wdt)._t
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                       # warm up outside the capture
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    ids0 = K.moe_route(x._t, gw._t, 2)[0]
    for seed in (1, 2, 3):
        x._t.copy_(torch.randint(-4, 5, (1, 5, 128), generator=torch.Generator().manual_seed(seed)).bfloat16() / 4)
        assert not torch.equal(K.moe_route(x._t, gw._t, 2)[0], ids0)
        graph.replay()
        assert torch.equal(out, call())
