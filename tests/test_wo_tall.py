"""Weight-only int8 / int4 linear above ``WO_MAX_ROWS`` rows: the tiled kernel of wo_tall.hip through
``ops.fused.weight_only_linear`` against a float64 product, and the decoder's ``prefill`` /
``extend`` on it against the twins over the dequantised weights."""
import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import FusedMultiTransformerDecoder
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

from test_weight_only_linear import _bound, _lossless, _twin_model

pytestmark = pytest.mark.gpu
_MS = (65, 128, 129, 300)
#          K     N   group
_SHAPES = [(64, 16, -1),       # one chunk (the int4 tail alone), a single channel tile
           (192, 80, 64),      # int4 superchunk + tail, both LDS buffers reused, idle waves, groups
           (320, 144, -1),     # a second workgroup along N that holds one 16-channel tile
           (1152, 272, 128)]   # 18 chunks, group 128, three workgroups along N


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('wdt', ['int8', 'int4'])
@pytest.mark.parametrize('Kd,N,g', _SHAPES)
def test_tall_kernel_against_float64(Kd, N, g, wdt, dtype):
    w, _ = _lossless(Kd, N, wdt, g)
    q, s = (t.cuda() for t in K.weight_quantize(w, wdt, g))
    xs = torch.randn(max(_MS), Kd, generator=torch.Generator().manual_seed(7)).to(dtype).cuda()
    R.reset_stats()
    for M in _MS:
        x = xs[:M]
        y = K.weight_only_linear(x, q, s, weight_dtype=wdt, group_size=g)
        _bound(y, x, w)
        assert torch.equal(y, K.weight_only_linear(x, q, s, weight_dtype=wdt, group_size=g))
    assert R.stats() == {('weight_only_linear', 'hip'): 2 * len(_MS)}


@pytest.mark.parametrize('act', [None, 'gelu', 'relu'])
@pytest.mark.parametrize('wdt,g', [('int8', -1), ('int4', 64)])
def test_tall_kernel_epilogue(wdt, g, act):
    Kd, N, M = 192, 80, 129
    w, _ = _lossless(Kd, N, wdt, g)
    q, s = (t.cuda() for t in K.weight_quantize(w, wdt, g))
    gen = torch.Generator().manual_seed(8)
    for dtype in (torch.bfloat16, torch.float16):
        x, bias = torch.randn(M, Kd, generator=gen).to(dtype).cuda(), torch.randn(N, generator=gen).to(dtype).cuda()
        _bound(K.weight_only_linear(x, q, s, bias, act, wdt, g), x, w, bias, act)


def _run(dec, x, lens, T):
    """Ragged prefill, one extend of T tokens per slot, one step: every output, flattened."""
    S0 = max(lens)
    outs = [dec.prefill(paddle.Tensor(x[:, :S0]), seq_lens=list(lens))._t]
    stats = dict(R.stats())
    outs.append(dec.extend(paddle.Tensor(x[:, S0:S0 + T]))._t)
    outs.append(dec.step(paddle.Tensor(x[:, S0 + T:S0 + T + 1]))._t)
    valid = torch.arange(S0)[None, :] < torch.tensor(lens)[:, None]             # padding rows: unspecified
    outs[0] = outs[0] * valid[:, :, None].to(outs[0])
    return torch.cat([o.float().reshape(-1).cpu() for o in outs]), stats


@pytest.mark.parametrize('wdt,g', [('int8', -1), ('int4', 64)])
def test_decoder_prefill_and_extend(wdt, g):
    """The model of test_decoder_graph_gpu (head dim 64, which ``extend`` needs) with an 80-row prefill
    and a 66-row extend, under that test's rule: at most twice as far from the fp32 twin as the
    bf16 twin is."""
    paddle.set_device('gpu')
    E, H, F, lens, B, L, T = 256, 4, 512, (40, 37), 2, 128, 33
    x = torch.randn(B, max(lens) + T + 1, E, generator=torch.Generator().manual_seed(9)).bfloat16()
    dq = FusedMultiTransformerDecoder(_twin_model(E, H, F, bf16=True), B, L, weight_only=wdt, weight_group_size=g)
    R.reset_stats()
    a, after_prefill = _run(dq, x.cuda(), lens, T)
    assert after_prefill[('weight_only_linear', 'hip')] == 4 * 2
    assert ('weight_only_linear', 'ref') not in R.stats()
    t16 = FusedMultiTransformerDecoder(_twin_model(E, H, F, dq.wo_weights, bf16=True), B, L)
    t32 = FusedMultiTransformerDecoder(_twin_model(E, H, F, dq.wo_weights), B, L)
    ref = _run(t32, x.float().cuda(), lens, T)[0]
    d_wo = float((a - ref).abs().max() / ref.abs().max())
    d_16 = float((_run(t16, x.cuda(), lens, T)[0] - ref).abs().max() / ref.abs().max())
    print(f"distance to the fp32 twin: weight-only {wdt} g{g} {d_wo:.3e}, bf16 twin {d_16:.3e}")
    assert d_wo <= 2 * d_16, (d_wo, d_16)
