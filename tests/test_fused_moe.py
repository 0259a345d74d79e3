"""Top-k routed MoE FFN: ``ops.fused.moe_route`` / ``moe_ffn`` and ``incubate.nn.functional.fused_moe``
('ref' on the CPU, the moe_ffn.hip kernels on the GPU) against a float64 per-token loop.

Tokens are multiples of 1/4 in [-1, 1] and gate weights multiples of 1/8 in [-1/2, 1/2] with D <= 128,
so every logit is exact in fp32 in any summation order, ties are frequent, and the ids of every
implementation must equal those of a float64 stable sort."""
import functools

import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import functional as FF
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

_U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
#          M   E   k   D    F
_SHAPES = [(1, 4, 1, 64, 64),        # one row, three empty experts, one 64-k chunk
           (5, 8, 2, 128, 64),
           (17, 8, 2, 64, 128),      # expert 3 takes all 17 rows: two row blocks, the second partial
           (64, 16, 8, 128, 64),     # the row limit, every expert crowded
           (3, 256, 8, 64, 64)]      # the expert and k limits, almost all experts empty
_ACTS = ('swiglu', 'gelu', 'relu')
_DTYPES = [torch.bfloat16, torch.float16]
_ALL = pytest.mark.parametrize('shape,act,bias,dtype', [(s, a, b, d) for s in _SHAPES for a in _ACTS
                                                        for b in (False, True) for d in _DTYPES],
                               ids=lambda v: str(v).replace('torch.', '').replace(' ', ''))


def _route64(x, gw, k, norm=True):
    """float64 stable descending sort and softmax -> (ids int32, weights float64)."""
    logits = x.double() @ gw.double()
    assert torch.equal(logits, (x.float() @ gw).double())           # exact in fp32: the premise of the file
    ids = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]
    w = torch.softmax(logits, -1).gather(1, ids)
    return ids.to(torch.int32), (w / w.sum(1, keepdim=True) if norm else w)


@functools.lru_cache(None)
def _case(shape, act, bias, dtype):
    """Inputs (CPU) and the float64 oracle of one case: (x, gw, w1, w2, b1, b2, ids, w64, ref, S)."""
    M, E, k, D, F = shape
    gen = torch.Generator().manual_seed(7 + M + E)
    x = torch.randint(-4, 5, (M, D), generator=gen).to(dtype) / 4
    gw = torch.randint(-4, 5, (D, E), generator=gen).float() / 8
    if M == 17:                       # logit 3 >= 64 - 63/2 > 32 >= any other; still exact in fp32
        x[:, 0], gw[0, 3] = 1, 64
    N1 = 2 * F if act == 'swiglu' else F
    w1 = (torch.randn(E, D, N1, generator=gen) / D ** 0.5).to(dtype)
    w2 = (torch.randn(E, F, D, generator=gen) / F ** 0.5).to(dtype)
    b1 = (0.1 * torch.randn(E, 1, N1, generator=gen)).to(dtype) if bias else None
    b2 = (0.1 * torch.randn(E, 1, D, generator=gen)).to(dtype) if bias else None
    ids, w = _route64(x, gw, k)
    ref, S = torch.zeros(M, D, dtype=torch.float64), torch.zeros(M, D, dtype=torch.float64)
    for m in range(M):
        for j in range(k):
            e = int(ids[m, j])
            z = x[m].double() @ w1[e].double() + (b1[e, 0].double() if bias else 0)
            h = {'swiglu': lambda: torch.nn.functional.silu(z[:F]) * z[F:], 'relu': lambda: torch.relu(z),
                 'gelu': lambda: torch.nn.functional.gelu(z)}[act]()
            o, a = h @ w2[e].double(), h.abs() @ w2[e].double().abs()
            if bias:
                o, a = o + b2[e, 0].double(), a + b2[e, 0].double().abs()
            ref[m] += w[m, j] * o
            S[m] += w[m, j] * a
    return x, gw, w1, w2, b1, b2, ids, w, ref, S


def _bound(y, ref, S):
    """|y - ref| <= 2u (|ref| + S): h rounded to 16 bits (u S), the output rounding (u |ref|), the
    fp32 sums at K <= 128 and the fast erf (< 2^-14 S) inside the factor 2."""
    assert y.dtype in _U and y.shape == ref.shape
    worst = float(((y.double().cpu() - ref).abs() / (2 * _U[y.dtype] * (ref.abs() + S))).max())
    print(f"worst |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


def _run_both(dev, shape, act, bias, dtype):
    """moe_ffn on the routed ids, and fused_moe (reference shapes) where the weights imply the act."""
    x, gw, w1, w2, b1, b2, ids, w, ref, S = (None if t is None else t.to(dev) for t in _case(shape, act, bias, dtype))
    _bound(K.moe_ffn(x, ids, w.float(), w1, w2, b1, b2, act), ref.cpu(), S.cpu())
    if act != 'relu':
        P = paddle.Tensor
        y = FF.fused_moe(P(x[None]), P(gw), P(w1), P(w2), b1 if b1 is None else P(b1), None,
                         b2 if b2 is None else P(b2), moe_topk=shape[2])
        assert tuple(y._t.shape) == (1,) + tuple(x.shape)
        _bound(y._t[0], ref.cpu(), S.cpu())
    return x, ids, w, w1, w2, b1, b2


# ----------------------------------------------------------------------------- CPU
@_ALL
def test_ref_against_float64(shape, act, bias, dtype):
    R.reset_stats()
    _run_both('cpu', shape, act, bias, dtype)
    assert ('moe_ffn', 'hip') not in R.stats() and R.stats()[('moe_ffn', 'ref')] == 1 + (act != 'relu')


@pytest.mark.parametrize('norm', [True, False])
@pytest.mark.parametrize('k', [1, 2, 6])
def test_routing_exact(k, norm):
    x = torch.zeros(3, 64)
    x[0, 0] = x[1, 1] = x[2, 2] = 1
    gw = torch.zeros(64, 6)
    gw[0] = torch.tensor([0.25, 0.5, 0.5, 0.25, 0.5, -0.5])          # ties: 1, 2, 4 then 0, 3 then 5
    gw[1] = 0.125                                                    # all equal: index order
    gw[2] = torch.tensor([-0.5, -0.25, 0, 0.125, 0.25, 0.5])         # strictly rising: reversed
    ids, w = K.moe_route(x.bfloat16(), gw, k, norm)
    want = torch.tensor([[1, 2, 4, 0, 3, 5], [0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]], dtype=torch.int32)[:, :k]
    ids64, w64 = _route64(x, gw, k, norm)
    assert ids.dtype == torch.int32 and torch.equal(ids, want) and torch.equal(ids64, want)
    assert w.dtype == torch.float32 and float((w.double() / w64 - 1).abs().max()) <= 2.0 ** -21
    assert float((w.sum(1) - 1).abs().max()) <= 2.0 ** -22 or not (norm or k == 6)


def test_errors():
    x, gw, w1, w2, b1, b2, ids, w, _, _ = _case(_SHAPES[1], 'swiglu', True, torch.bfloat16)
    w = w.float()
    for bad in (dict(w1=w1[:7]), dict(w1=w1[:, :, :64]), dict(w2=w2[:, :, :64]), dict(b1=b1[:, :, :64]),
                dict(b2=b2[:4]), dict(ids=ids[:4]),
                dict(ids=ids.repeat(1, 5), weights=w.repeat(1, 5))):                  # k = 10 > E = 8
        kw = dict(x=x, ids=ids, weights=w, w1=w1, w2=w2, b1=b1, b2=b2, act='swiglu')
        kw.update(bad)
        with pytest.raises(ValueError, match=r'\(\d+, '):
            K.moe_ffn(**kw)
    with pytest.raises(ValueError, match=r'top_k = 9'):
        K.moe_route(x, gw, 9)
    with pytest.raises(ValueError, match=r'float64 \(128, 8\)'):
        K.moe_route(x, gw.double(), 2)
    P = paddle.Tensor
    for kw in (dict(ffn1_scale=P(torch.ones(8))), dict(ffn2_scale=P(torch.ones(8))),
               dict(quant_method='weight_only_int8')):
        with pytest.raises(NotImplementedError):
            FF.fused_moe(P(x[None]), P(gw), P(w1), P(w2), **kw)
    R.reset_stats()                                                  # taller than the kernel takes: 'ref'
    K.moe_ffn(x.repeat(13, 1), ids.repeat(13, 1), w.repeat(13, 1), w1, w2)
    assert R.stats() == {('moe_ffn', 'ref'): 1}


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize('norm', [True, False])
@pytest.mark.parametrize('dtype', _DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('shape', _SHAPES, ids=str)
def test_route_hip(shape, dtype, norm):
    x, gw = _case(shape, 'swiglu', False, dtype)[:2]
    ids64, w64 = _route64(x, gw, shape[2], norm)
    R.reset_stats()
    ids, w = K.moe_route(x.cuda(), gw.cuda(), shape[2], norm)
    assert R.stats() == {('moe_route', 'hip'): 1}
    ref_ids, _ = K._moe_route_ref(x.cuda(), gw.cuda(), shape[2], norm)
    assert torch.equal(ids, ref_ids) and torch.equal(ids.cpu(), ids64)
    worst = float((w.double().cpu() / w64 - 1).abs().max()) / 2.0 ** -19
    print(f"worst relative weight error / 2^-19 = {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.gpu
@_ALL
def test_ffn_hip_against_float64_and_reproducible(shape, act, bias, dtype):
    R.reset_stats()
    x, ids, w, w1, w2, b1, b2 = _run_both('cuda', shape, act, bias, dtype)
    assert R.stats() == ({('moe_ffn', 'hip'): 1} if act == 'relu' else
                         {('moe_ffn', 'hip'): 2, ('moe_route', 'hip'): 1})
    y = K.moe_ffn(x, ids, w.float(), w1, w2, b1, b2, act)
    assert torch.equal(y, K.moe_ffn(x, ids, w.float(), w1, w2, b1, b2, act))


@pytest.mark.gpu
def test_graph_replay_follows_the_routing():
    x, gw, w1, w2, b1, b2 = (paddle.Tensor(t.cuda()) for t in _case(_SHAPES[1], 'swiglu', True, torch.bfloat16)[:6])
    x = paddle.Tensor(x._t[None].clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                       # warm up outside the capture
        FF.fused_moe(x, gw, w1, w2, b1, None, b2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = FF.fused_moe(x, gw, w1, w2, b1, None, b2)._t
    ids0 = K.moe_route(x._t, gw._t, 2)[0]
    for seed in (1, 2, 3):
        x._t.copy_(torch.randint(-4, 5, (1, 5, 128), generator=torch.Generator().manual_seed(seed)).bfloat16() / 4)
        assert not torch.equal(K.moe_route(x._t, gw._t, 2)[0], ids0)
        g.replay()
        assert torch.equal(out, FF.fused_moe(x, gw, w1, w2, b1, None, b2)._t)
