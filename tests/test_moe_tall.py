"""Routed MoE FFN above the decode kernels' 64 tokens: ``ops.fused.moe_route`` / ``moe_ffn`` and
``incubate.nn.functional.fused_moe`` on the tiled kernels of moe_tall.hip against a float64 oracle
computed per expert over its rows.

Inputs as in test_fused_moe.py: tokens are multiples of 1/4 in [-1, 1], gate weights multiples of 1/8
in [-1/2, 1/2] (one entry of +-64 where a case forces an expert), D <= 128, so every logit is exact in
fp32 and the ids must equal a float64 stable sort. Bound: |y - ref| <= 2u (|ref| + S), u = 2^-9 (bf16)
or 2^-11 (f16): h rounded to 16 bits (u S), the output rounding (u |ref|), the fp32 sums at K <= 128
and the fast erf inside the factor 2."""
import functools

import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import functional as FF
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

_U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
#         M   E  k   D    F
_OVER = (65, 4, 1, 64, 128)           # first shape past the skinny limit; expert 3 gets no row
_ONE = (129, 4, 2, 128, 64)           # expert 3 takes every row: a full row tile and a one-row tile
_BLOCKS = (600, 8, 2, 64, 128)        # 1200 pairs: two blocks of the counting sort
_LIMITS = (200, 256, 8, 64, 64)       # the expert and k limits, most experts empty, a long tile table
_SEAM = (K.MOE_MAX_PAIRS // 2 + 1, 8, 2, 64, 64)   # one token past the pairs of a call: two row chunks
_GRAPH = (96, 8, 2, 128, 64)
_ID = lambda v: str(v).replace('torch.', '').replace(' ', '')       # noqa: E731
_CASES = [(s, a, b, d) for s in (_OVER, _ONE) for a in ('swiglu', 'gelu', 'relu') for b in (False, True)
          for d in (torch.bfloat16, torch.float16)] + \
         [(s, 'swiglu', True, torch.bfloat16) for s in (_BLOCKS, _LIMITS, _SEAM)]


def _route64(x, gw, k):
    logits = x.double() @ gw.double()
    assert torch.equal(logits, (x.float() @ gw).double())           # exact in fp32: the premise of the file
    ids = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]
    w = torch.softmax(logits, -1).gather(1, ids)
    return ids.to(torch.int32), w / w.sum(1, keepdim=True)


@functools.lru_cache(None)
def _case(shape, act, bias, dtype):
    """Inputs (CPU) and the float64 oracle of one case: (x, gw, w1, w2, b1, b2, ids, w64, ref, S)."""
    M, E, k, D, F = shape
    gen = torch.Generator().manual_seed(11 + M + E)
    x = torch.randint(-4, 5, (M, D), generator=gen).to(dtype) / 4
    gw = torch.randint(-4, 5, (D, E), generator=gen).float() / 8
    if shape in (_OVER, _ONE):        # |any other logit| <= 32 < 64 - 63/2: expert 3 always last / first
        x[:, 0], gw[0, 3] = 1, (-64 if shape == _OVER else 64)
    N1 = 2 * F if act == 'swiglu' else F
    w1 = (torch.randn(E, D, N1, generator=gen) / D ** 0.5).to(dtype)
    w2 = (torch.randn(E, F, D, generator=gen) / F ** 0.5).to(dtype)
    b1 = (0.1 * torch.randn(E, 1, N1, generator=gen)).to(dtype) if bias else None
    b2 = (0.1 * torch.randn(E, 1, D, generator=gen)).to(dtype) if bias else None
    ids, w = _route64(x, gw, k)
    ref, S = torch.zeros(M, D, dtype=torch.float64), torch.zeros(M, D, dtype=torch.float64)
    for e in ids.unique().tolist():
        rows, slots = (ids == e).nonzero(as_tuple=True)
        z = x[rows].double() @ w1[e].double() + (b1[e, 0].double() if bias else 0)
        h = {'swiglu': lambda: torch.nn.functional.silu(z[:, :F]) * z[:, F:], 'relu': lambda: torch.relu(z),
             'gelu': lambda: torch.nn.functional.gelu(z)}[act]()
        o, a = h @ w2[e].double(), h.abs() @ w2[e].double().abs()
        if bias:
            o, a = o + b2[e, 0].double(), a + b2[e, 0].double().abs()
        ref.index_put_((rows,), w[rows, slots, None] * o, accumulate=True)      # an expert once per token
        S.index_put_((rows,), w[rows, slots, None] * a, accumulate=True)
    return x, gw, w1, w2, b1, b2, ids, w, ref, S


def _bound(y, ref, S):
    assert y.dtype in _U and y.shape == ref.shape
    worst = float(((y.double().cpu() - ref.cpu()).abs() / (2 * _U[y.dtype] * (ref.abs() + S).cpu())).max())
    print(f"worst |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


def _fused_moe(x, gw, w1, w2, b1, b2, k):
    P = paddle.Tensor
    return FF.fused_moe(P(x[None]), P(gw), P(w1), P(w2), b1 if b1 is None else P(b1), None,
                        b2 if b2 is None else P(b2), moe_topk=k)._t[0]


def _run(dev, shape, act, bias, dtype):
    """Route, moe_ffn twice (bit-equal) and, where the weights imply the act, fused_moe: every result
    inside the bound. Returns the number of fused_moe calls."""
    x, gw, w1, w2, b1, b2, ids, w, ref, S = (None if t is None else t.to(dev) for t in _case(shape, act, bias, dtype))
    got = K.moe_route(x, gw, shape[2])[0]
    assert torch.equal(got, ids) and torch.equal(got, K._moe_route_ref(x, gw, shape[2], True)[0])
    y = K.moe_ffn(x, ids, w.float(), w1, w2, b1, b2, act)
    _bound(y, ref, S)
    assert torch.equal(y, K.moe_ffn(x, ids, w.float(), w1, w2, b1, b2, act))
    if act != 'relu':
        _bound(_fused_moe(x, gw, w1, w2, b1, b2, shape[2]), ref, S)
    return int(act != 'relu')


def test_cpu_stays_on_ref():
    R.reset_stats()
    n = _run('cpu', _OVER, 'swiglu', True, torch.bfloat16)
    assert R.stats() == {('moe_route', 'ref'): 1 + n, ('moe_ffn', 'ref'): 2 + n}


@pytest.mark.gpu
@pytest.mark.parametrize('shape,act,bias,dtype', _CASES, ids=_ID)
def test_tall_hip_against_float64_and_reproducible(shape, act, bias, dtype):
    R.reset_stats()
    n = _run('cuda', shape, act, bias, dtype)
    assert R.stats() == {('moe_route', 'hip'): 1 + n, ('moe_ffn', 'hip'): 2 + n}


@pytest.mark.gpu
def test_a_token_does_not_depend_on_its_row():
    x, _, w1, w2, b1, b2, ids, w = (t.cuda() for t in _case(_BLOCKS, 'swiglu', True, torch.bfloat16)[:8])
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(5)).cuda()
    R.reset_stats()
    y = K.moe_ffn(x, ids, w.float(), w1, w2, b1, b2)
    assert torch.equal(K.moe_ffn(x[perm], ids[perm], w.float()[perm], w1, w2, b1, b2), y[perm])
    assert R.stats() == {('moe_ffn', 'hip'): 2}


@pytest.mark.gpu
def test_graph_replay_follows_the_routing():
    M, E, k, D, F = _GRAPH
    x, gw, w1, w2, b1, b2 = (t.cuda() for t in _case(_GRAPH, 'swiglu', True, torch.bfloat16)[:6])
    x = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                       # warm up outside the capture
        _fused_moe(x, gw, w1, w2, b1, b2, k)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    R.reset_stats()
    with torch.cuda.graph(g):
        out = _fused_moe(x, gw, w1, w2, b1, b2, k)
    assert R.stats() == {('moe_route', 'hip'): 1, ('moe_ffn', 'hip'): 1}
    ids0 = K.moe_route(x, gw, k)[0]
    for seed in (1, 2, 3):
        x.copy_(torch.randint(-4, 5, (M, D), generator=torch.Generator().manual_seed(seed)).bfloat16() / 4)
        assert not torch.equal(K.moe_route(x, gw, k)[0], ids0)
        g.replay()
        assert torch.equal(out, _fused_moe(x, gw, w1, w2, b1, b2, k))
