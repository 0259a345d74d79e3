"""Weight-only int8 / int4 linear: quantise / dequantise, ``ops.fused.weight_only_linear`` ('ref' on
the CPU, the wo_gemm.hip kernel on the GPU) against a float64 product, and the decoder runner with
``weight_only=`` against a twin over the dequantised weights."""
import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import FusedMultiTransformerDecoder
from paddle_ray_amd.nn import quant as Q
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

from test_fused_multi_transformer import _close, _model

_QMAX = {'int8': 127, 'int4': 7}
# one output rounding, doubled
_U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -23}
_WG = [('int8', -1), ('int8', 64), ('int4', -1), ('int4', 64)]


def _lossless(Kd, N, wdt, g, seed=0):
    """A weight that quantisation reproduces exactly: integer levels with a level of magnitude qmax
    in every channel / group, times scales of 7 significant bits, so that level * scale and
    absmax / qmax are exact in fp32. Returns (w [K, N] fp32, scale)."""
    gen = torch.Generator().manual_seed(seed + Kd + N)
    qmax, G = _QMAX[wdt], (Kd // g if g > 0 else 1)
    lv = torch.randint(-qmax, qmax + 1, (G, Kd // G, N), generator=gen)
    lv[:, 0] = qmax * (1 - 2 * torch.randint(0, 2, (G, N), generator=gen))
    scale = (64 + torch.randint(0, 64, (G, N), generator=gen)).float() / 4096
    return (lv.float() * scale[:, None]).reshape(Kd, N), (scale if g > 0 else scale[0])


def _bound(y, x, w, bias=None, act=None):
    """|y - ref| <= u_out |ref| + 2 K 2^-24 A with A = sum_k |x_k w_kn| in float64: one output
    rounding (doubled) and the worst-case fp32 accumulation in any order. With an activation the
    pre-activation bound is scaled by GELU's Lipschitz constant 1.13, plus the output rounding and
    1e-6 for the fp32 erf."""
    xd, wd = x.double().cpu(), w.double().cpu()
    ref, A = xd @ wd, xd.abs() @ wd.abs()
    if bias is not None:
        ref = ref + bias.double().cpu()
    u = _U[y.dtype]
    tol = u * ref.abs() + 2 * x.shape[-1] * 2.0 ** -24 * A
    if act is not None:
        ref = torch.nn.functional.gelu(ref) if act == 'gelu' else torch.relu(ref)
        tol = 1.13 * tol + u * ref.abs() + 1e-6
    err = (y.double().cpu() - ref).abs()
    worst = float((err / tol).max())
    print(f"worst |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('wdt,g,Kd,N', [(wdt, g, Kd, N) for wdt in ('int8', 'int4') for g in (-1, 64, 128)
                                        for Kd, N in ((384, 32), (192, 80)) if g < 0 or Kd % g == 0])
def test_quantize_dequantize(wdt, g, Kd, N):
    algo, qmax = 'weight_only_' + wdt, _QMAX[wdt]
    w = torch.randn(Kd, N, generator=torch.Generator().manual_seed(1))
    w[:, 3] = 0.0                                                   # an all-zero channel: scale 1
    q, s = K.weight_quantize(w, algo, g)
    assert q.dtype == torch.int8 and tuple(q.shape) == (N, Kd if wdt == 'int8' else Kd // 2)
    assert s.dtype == torch.float32 and tuple(s.shape) == ((Kd // g, N) if g > 0 else (N,))
    assert bool((s.reshape(-1, N)[:, 3] == 1).all())
    d = K.weight_dequantize(q, s, algo, g, torch.float32)
    srow = s.repeat_interleave(g, 0) if g > 0 else s.expand(Kd, N)
    lv = (d / srow).round()                                         # d is level * scale in fp32
    assert torch.equal(lv * srow, d) and float(lv.abs().max()) == qmax
    assert bool(((d - w).abs() <= srow / 2).all())
    wl, sl = _lossless(Kd, N, wdt, g)
    ql, s2 = K.weight_quantize(wl, algo, g)
    assert torch.equal(s2, sl) and torch.equal(K.weight_dequantize(ql, s2, algo, g, torch.float32), wl)
    q3, s3 = K.weight_quantize(K.weight_dequantize(ql, s2, algo, g, torch.float32), algo, g)
    assert torch.equal(q3, ql) and torch.equal(s3, s2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('wdt,g', _WG)
def test_ref_linear_against_float64(wdt, g, dtype):
    Kd, N = 192, 80
    w, _ = _lossless(Kd, N, wdt, g)
    q, s = K.weight_quantize(w, wdt, g)
    gen = torch.Generator().manual_seed(2)
    x, bias = torch.randn(2, 5, Kd, generator=gen).to(dtype), torch.randn(N, generator=gen).to(dtype)
    R.reset_stats()
    y = K.weight_only_linear(x, q, s, weight_dtype=wdt, group_size=g)
    assert y.dtype == dtype and tuple(y.shape) == (2, 5, N)
    assert R.stats() == {('weight_only_linear', 'ref'): 1}
    _bound(y, x, w)
    for act in ('gelu', 'relu'):
        _bound(K.weight_only_linear(x, q, s, bias, act, wdt, g), x, w, bias, act)


def _twin_model(E, H, F, wo=None, bf16=False):
    """The test model with every parameter rounded to bf16 values (so an fp32 and a bf16 copy hold
    the same numbers) and, with ``wo`` (a decoder's ``wo_weights``), the four weights of each layer
    replaced by the dequantised ones."""
    m = _model(True, E=E, H=H, F=F, L=2)
    with torch.no_grad():
        for p in m.parameters():
            p._t.copy_(p._t.bfloat16().float())
        for name in ('qkv', 'linear', 'ffn1', 'ffn2') if wo else ():
            for p, q, s in zip(getattr(m, name + '_weights'), wo[name + '_weights'], wo[name + '_weight_scales']):
                w = K.weight_dequantize(q, s, wo['weight_dtype'], wo['weight_group_size'], torch.float32)
                p._t.copy_(w.t().reshape(p._t.shape) if name == 'qkv' else w)
    if bf16:
        m.to(dtype='bfloat16')
    return m


def _generate(dec, x, lens, T=2):
    """prefill (ragged), three steps, one step_multi(T) + commit: every output, flattened."""
    S0, outs = max(lens), []
    outs.append(dec.prefill(paddle.Tensor(x[:, :S0]), seq_lens=list(lens))._t)
    for i in range(3):
        outs.append(dec.step(paddle.Tensor(x[:, S0 + i:S0 + i + 1]))._t)
    outs.append(dec.step_multi(paddle.Tensor(x[:, S0 + 3:S0 + 3 + T]))._t)
    dec.commit([T] * len(lens))
    assert dec.lens.tolist() == [n + 3 + T for n in lens]
    valid = torch.arange(S0)[None, :] < torch.tensor(lens)[:, None]             # padding rows: unspecified
    outs[0] = outs[0] * valid[:, :, None].to(outs[0])
    return torch.cat([o.float().reshape(-1).cpu() for o in outs])


@pytest.mark.parametrize('wdt,g', [('int8', -1), ('int4', 64)])
def test_decoder_matches_the_dequantised_twin_cpu(wdt, g):
    E, H, F, lens = 64, 4, 128, (3, 5)
    x = torch.randn(2, max(lens) + 5, E, generator=torch.Generator().manual_seed(3))
    dq = FusedMultiTransformerDecoder(_twin_model(E, H, F), 2, 16, weight_only=wdt, weight_group_size=g)
    assert dq.wo_weights['qkv_weights'][0].dtype == torch.int8
    twin = FusedMultiTransformerDecoder(_twin_model(E, H, F, dq.wo_weights), 2, 16)
    R.reset_stats()
    a = _generate(dq, x, lens)
    assert R.stats()[('weight_only_linear', 'ref')] == 4 * 2 * 4     # 4 products, 2 layers, 3 steps + 1 multi
    _close(a, _generate(twin, x, lens), 2e-5)                        # two fp32 orderings of the same sums


def test_validation():
    w = torch.randn(128, 32)
    q, s = Q.weight_quantize(paddle.Tensor(w), 'weight_only_int4', group_size=64)
    x = paddle.Tensor(torch.randn(3, 128))
    Q.weight_only_linear(x, q, weight_scale=s, weight_dtype='int4', arch=950, group_size=64)
    assert Q.weight_dequantize(q, s, 'weight_only_int4', 'float32', 64)._t.dtype == torch.float32
    bad = [dict(weight_scale=s, weight_dtype='int4', group_size=-1),              # scale vs group
           dict(weight_scale=s, weight_dtype='int4', group_size=128),
           dict(weight_scale=paddle.Tensor(s._t[:, :16]), weight_dtype='int4', group_size=64),   # vs N
           dict(weight_scale=paddle.Tensor(s._t[:1]), weight_dtype='int4', group_size=64),       # vs K
           dict(weight_scale=s, weight_dtype='int8', group_size=64),              # K from the bytes
           dict(weight_scale=s, weight_dtype='int2', group_size=64),
           dict(weight_scale=s, weight_dtype='int4', group_size=64, arch=90)]
    for kw in bad:
        with pytest.raises(ValueError):
            Q.weight_only_linear(x, q, **kw)
    with pytest.raises(ValueError, match=r'\(128, 32\)'):                         # a float weight
        Q.weight_only_linear(x, paddle.Tensor(w), weight_scale=s, weight_dtype='int4', group_size=64)
    with pytest.raises(ValueError, match='odd'):
        Q.weight_quantize(paddle.Tensor(torch.randn(7, 16)), 'weight_only_int4')
    with pytest.raises(ValueError):
        Q.weight_quantize(paddle.Tensor(w), 'weight_only_int8', arch=942)
    with pytest.raises(ValueError):
        Q.weight_quantize(paddle.Tensor(w), 'llm.int8')
    with pytest.raises(ValueError):
        FusedMultiTransformerDecoder(_model(True), 2, 8, weight_only='fp8')


# ----------------------------------------------------------------------------- GPU
_MS = (1, 5, 16, 17, 33, 64)
#          K     N   group  splits
_SHAPES = [(64, 16, -1, None), (64, 16, 64, None), (192, 80, -1, None), (192, 80, 64, None),
           (2112, 48, -1, None), (2112, 48, 64, None), (2112, 48, -1, 3), (2112, 48, 64, 3),
           (1152, 48, 128, None)]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('wdt', ['int8', 'int4'])
@pytest.mark.parametrize('Kd,N,g,splits', _SHAPES)
def test_kernel_against_float64(Kd, N, g, splits, wdt, dtype):
    w, _ = _lossless(Kd, N, wdt, g)
    q, s = (t.cuda() for t in K.weight_quantize(w, wdt, g))
    xs = torch.randn(max(_MS), Kd, generator=torch.Generator().manual_seed(4)).to(dtype).cuda()
    R.reset_stats()
    for M in _MS:
        x = xs[:M]
        y = K.weight_only_linear(x, q, s, weight_dtype=wdt, group_size=g, splits=splits)
        _bound(y, x, w)
        assert torch.equal(y, K.weight_only_linear(x, q, s, weight_dtype=wdt, group_size=g, splits=splits))
    assert R.stats() == {('weight_only_linear', 'hip'): 2 * len(_MS)}


@pytest.mark.gpu
@pytest.mark.parametrize('act', ['gelu', 'relu'])
@pytest.mark.parametrize('wdt,g', [('int8', -1), ('int4', 64)])
@pytest.mark.parametrize('Kd,N,splits', [(192, 80, None), (2112, 48, 3)])
def test_kernel_epilogue(Kd, N, splits, wdt, g, act):
    w, _ = _lossless(Kd, N, wdt, g)
    q, s = (t.cuda() for t in K.weight_quantize(w, wdt, g))
    gen = torch.Generator().manual_seed(5)
    for dtype in (torch.bfloat16, torch.float16):
        x, bias = torch.randn(17, Kd, generator=gen).to(dtype).cuda(), torch.randn(N, generator=gen).to(dtype).cuda()
        _bound(K.weight_only_linear(x, q, s, bias, act, wdt, g, splits), x, w, bias, act)


@pytest.mark.gpu
@pytest.mark.parametrize('wdt,g,cache', [('int8', -1, {}), ('int4', 64, {}),
                                         ('int8', -1, dict(kv_cache_dtype='int8', block_size=16))],
                         ids=['int8', 'int4_g64', 'int8_q8_paged'])
def test_decoder_graph_gpu(wdt, g, cache):
    """The weight-only decoder may be at most twice as far from the fp32 twin (fp32 model over the
    dequantised weights) as the bf16 twin (the same weights in bf16 on the library products) is."""
    paddle.set_device('gpu')
    E, H, F, lens, B, L = 256, 4, 512, (5, 9, 12), 3, 32
    x = torch.randn(B, max(lens) + 5, E, generator=torch.Generator().manual_seed(6)).bfloat16()
    dq = FusedMultiTransformerDecoder(_twin_model(E, H, F, bf16=True), B, L, weight_only=wdt,
                                      weight_group_size=g, **cache)
    R.reset_stats()
    a = _generate(dq, x.cuda(), lens)
    assert dq._graph is not None and R.stats()[('weight_only_linear', 'hip')] >= 4 * 2 * 4
    assert ('weight_only_linear', 'ref') not in R.stats()
    t16 = FusedMultiTransformerDecoder(_twin_model(E, H, F, dq.wo_weights, bf16=True), B, L, **cache)
    t32 = FusedMultiTransformerDecoder(_twin_model(E, H, F, dq.wo_weights), B, L, **cache)
    ref = _generate(t32, x.float().cuda(), lens)
    d_wo = float((a - ref).abs().max() / ref.abs().max())
    d_16 = float((_generate(t16, x.cuda(), lens) - ref).abs().max() / ref.abs().max())
    print(f"distance to the fp32 twin: weight-only {wdt} g{g} {d_wo:.3e}, bf16 twin {d_16:.3e}")
    assert d_wo <= 2 * d_16, (d_wo, d_16)
