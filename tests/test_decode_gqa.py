"""Grouped-query attention on the decode path: ``KVH < H`` K/V heads, each shared by
``R = H / KVH`` query heads (``gqa_group_size`` = KVH).

CPU: the fp32 ``'ref'`` kernel on a grouped-query row against itself on the problem expanded
to ``H`` K/V heads; a grouped-query ``FusedMultiTransformer`` against a multi-head twin whose
k/v head blocks are the grouped ones repeated ``R`` times, through the context phase and decode
steps of a ragged batch with rotary; the ``FusedMultiTransformerDecoder`` runner against each
sequence generated alone. GPU: the HIP grouped-query kernel against ``'ref'`` on a cloned
cache — one split and split-K, host and device ``time_step``, masks, every (R, D, dtype),
in-kernel rotary, the per-sequence guard — and the whole path in bf16 from one captured graph."""
import functools

import numpy as np
import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import FusedMultiTransformer, FusedMultiTransformerDecoder
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

from test_decode_ragged import LENS, MAXLEN, STEPS, _i32, _rot, _tables, _tok
from test_fused_multi_transformer import _causal, _close, _model


# ----------------------------------------------------------------------------- CPU: the ref kernel
def _problem(B, H, KVH, L, D, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, H + 2 * KVH, D, generator=g).to(dtype)
    cache = torch.randn(2, B, KVH, L, D, generator=g).to(dtype)
    return qkv, cache


def _expanded(qkv, cache, H, KVH):
    """The multi-head problem that computes the same thing: k/v heads repeated R times."""
    r = H // KVH
    q, k, v = qkv[:, :H], qkv[:, H:H + KVH], qkv[:, H + KVH:]
    return (torch.stack([q, k.repeat_interleave(r, 1), v.repeat_interleave(r, 1)], 1).contiguous(),
            cache.repeat_interleave(r, 2).contiguous())


@pytest.mark.parametrize('r', [2, 3, 4])
@pytest.mark.parametrize('variant', ['plain', 'ragged_mask_rotary', 'guarded'])
def test_ref_gqa_is_ref_mha_on_the_expanded_problem(r, variant):
    B, KVH, L, D = 3, 2, 12, 16
    H = KVH * r
    qkv, cache = _problem(B, H, KVH, L, D, seed=r)
    qkv4, cache4 = _expanded(qkv, cache, H, KVH)
    t, kw, mask = 6, {}, None
    if variant == 'ragged_mask_rotary':
        g = torch.Generator().manual_seed(11)
        ang = torch.rand(B, D, generator=g) * (2 * np.pi)
        kw = dict(seq_lens=torch.tensor([0, 6, 3]), rotary=torch.stack([ang.cos(), ang.sin()]),
                  rotary_dims=1)
        mask = torch.zeros(B, t + 2)
        mask[:, 1::3] = float('-inf')
        for b, n in enumerate((0, 6, 3)):
            mask[b, n] = 0.0
    elif variant == 'guarded':     # device-style positions: the middle sequence is out of range
        t = torch.tensor([L - 1], dtype=torch.int32)
        kw = dict(seq_lens=torch.tensor([6, L, 2]))
    ref = R.get_kernel('mmha_decode', 'ref')
    c3, c4 = cache.clone(), cache4.clone()
    out3 = ref(qkv, c3, t, mask, **kw)
    out4 = ref(qkv4, c4, t, mask, **kw)
    assert out3.shape == (B, H, D)
    torch.testing.assert_close(out3, out4, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(c3, c4[:, :, ::r], rtol=0, atol=0)
    assert not torch.equal(c3, cache)                # something was appended
    if variant == 'guarded':
        assert float(out3[1].abs().sum()) == 0.0
        assert torch.equal(c3[:, 1], cache[:, 1])    # nothing written for the bad sequence


def test_3d_qkv_with_as_many_kv_heads_is_the_4d_form():
    g = torch.Generator().manual_seed(2)
    B, H, L, D = 2, 3, 10, 8
    qkv4, cache = torch.randn(B, 3, H, D, generator=g), torch.randn(2, B, H, L, D, generator=g)
    for kw in ({}, dict(seq_lens=[2, 5])):
        c3, c4 = cache.clone(), cache.clone()
        out3 = K.mmha_decode(qkv4.reshape(B, 3 * H, D), c3, 5, **kw)
        out4 = K.mmha_decode(qkv4, c4, 5, **kw)
        assert torch.equal(out3, out4) and torch.equal(c3, c4)
        assert not torch.equal(c3, cache)


# ----------------------------------------------------------------------------- CPU: the layers
def _gqa_model(E=32, H=4, KVH=2, L=2, seed=0):
    """As ``_model``: non-trivial LayerNorm parameters and biases, eval mode."""
    paddle.seed(seed)
    m = FusedMultiTransformer(E, H, 2 * E, num_layers=L, gqa_group_size=KVH)
    rs = np.random.RandomState(seed)
    for p in m.parameters():
        p.set_value((rs.randn(*p.shape) * (0.3 if len(p.shape) > 1 else 0.2)).astype('float32')
                    + (1.0 if 'scale' in p.name else 0.0))
    m.eval()
    return m


def _mha_twin(m):
    """The multi-head model that computes the same function: k/v head blocks repeated R times."""
    E, H, KVH = m.embed_dim, m.num_heads, m.kv_num_heads
    r = H // KVH
    twin = _model(True, E=E, H=H, F=2 * E, L=len(m.qkv_weights))
    for a, b in zip(twin.parameters(), m.parameters()):
        v = b._t.detach().float()
        if tuple(a.shape) != tuple(b.shape):         # qkv weight [N, D, E] / bias [N, D]
            v = torch.stack([v[:H], v[H:H + KVH].repeat_interleave(r, 0),
                             v[H + KVH:].repeat_interleave(r, 0)])
        a.set_value(v.numpy())
    return twin


def test_gqa_parameter_shapes():
    m = _gqa_model()
    assert m.kv_num_heads == 2 and m.num_heads == 4
    assert tuple(m.qkv_weights[0].shape) == (8, 8, 32) and tuple(m.qkv_biases[0].shape) == (8, 8)
    m2 = FusedMultiTransformer(32, 4, 64, num_layers=1, gqa_group_size=2, trans_qkvw=False)
    assert tuple(m2.qkv_weights[0].shape) == (32, 8, 8)
    plain = FusedMultiTransformer(32, 4, 64, num_layers=1)
    assert plain.kv_num_heads == 4 and tuple(plain.qkv_weights[0].shape) == (3, 4, 8, 32)


def test_gqa_generation_matches_the_expanded_multi_head_twin():
    m = _gqa_model()
    twin = _mha_twin(m)
    H, KVH, D, r = m.num_heads, m.kv_num_heads, m.head_dim, m.num_heads // m.kv_num_heads
    B, S0 = len(LENS), max(LENS)
    cos, sin = _tables(D)
    x = torch.randn(B, S0 + STEPS, 32, generator=torch.Generator().manual_seed(5))
    caches = {id(mm): [paddle.Tensor(torch.zeros(2, B, heads, S0 + STEPS + 3, D)) for _ in range(2)]
              for mm, heads in ((m, KVH), (twin, H))}

    def both(xs, mask, lens, pos, **kw):
        outs = []
        for mm in (m, twin):
            with torch.no_grad():
                o, _ = mm(paddle.Tensor(xs), attn_mask=paddle.Tensor(mask), caches=caches[id(mm)],
                          seq_lens=_i32(lens, 'cpu'), rotary_embs=_rot(cos, sin, pos, 'cpu'),
                          rotary_emb_dims=1, **kw)
            outs.append(o._t)
        _close(outs[0], outs[1], 2e-5)
        for cg, ct in zip(caches[id(m)], caches[id(twin)]):
            assert tuple(cg._t.shape) == (2, B, KVH, S0 + STEPS + 3, D)
            torch.testing.assert_close(cg._t, ct._t[:, :, ::r], rtol=2e-5, atol=2e-5)
            assert float(cg._t.abs().sum()) > 0
    both(x[:, :S0], _causal(S0, B), LENS, torch.arange(S0).expand(B, S0))
    for i in range(STEPS):
        lens = [n + i for n in LENS]
        both(x[:, S0 + i:S0 + i + 1], torch.zeros(B, 1, 1, S0 + i + 1), lens,
             torch.tensor(lens)[:, None], time_step=S0 + i)


@functools.lru_cache(None)
def _case(device='cpu', dtype=torch.float32, E=32, H=4, KVH=2):
    """The grouped-query model, each sequence's own tokens, and its reference: the sequence
    alone (B=1) through the causal context phase with rotary. Computed once."""
    m = _gqa_model(E, H, KVH)
    if dtype != torch.float32:
        m.to(dtype='bfloat16')
    g = torch.Generator().manual_seed(7)
    cos, sin = _tables(E // H)
    seqs, refs = [], []
    for n in LENS:
        S = n + STEPS
        x = torch.randn(1, S, E, generator=g).to(device=device, dtype=dtype)
        with torch.no_grad():
            full = m(paddle.Tensor(x), attn_mask=paddle.Tensor(_causal(S, 1).to(device, dtype)),
                     rotary_embs=_rot(cos, sin, torch.arange(S)[None], device), rotary_emb_dims=1)._t
        seqs.append(x[0])
        refs.append(full[0])
    S0 = max(LENS)
    xp = torch.randn(len(LENS), S0, E, generator=g).to(device=device, dtype=dtype)   # padding
    for b, n in enumerate(LENS):
        xp[b, :n] = seqs[b][:n]
    return m, seqs, refs, xp, cos, sin


def _functional(device='cpu', dtype=torch.float32, tol=2e-5, **size):
    m, seqs, refs, xp, cos, sin = _case(device, dtype, **size)
    B, S0 = len(LENS), max(LENS)
    caches = [paddle.Tensor(torch.zeros(2, B, m.kv_num_heads, S0 + STEPS + 3, m.head_dim,
                                        device=device, dtype=dtype)) for _ in range(2)]
    with torch.no_grad():
        out, caches = m(paddle.Tensor(xp), attn_mask=paddle.Tensor(_causal(S0, B).to(device, dtype)),
                        caches=caches, seq_lens=_i32(LENS, device),
                        rotary_embs=_rot(cos, sin, torch.arange(S0).expand(B, S0), device),
                        rotary_emb_dims=1)
    for b, n in enumerate(LENS):
        _close(out._t[b, :n], refs[b][:n], tol)
    for i in range(STEPS):
        t = S0 + i
        lens = [n + i for n in LENS]
        with torch.no_grad():
            out, caches = m(paddle.Tensor(_tok(seqs, i)),
                            attn_mask=paddle.Tensor(torch.zeros(B, 1, 1, t + 1, device=device)),
                            caches=caches, seq_lens=_i32(lens, device), time_step=t,
                            rotary_embs=_rot(cos, sin, torch.tensor(lens)[:, None], device),
                            rotary_emb_dims=1)
        for b, n in enumerate(LENS):
            _close(out._t[b, 0], refs[b][n + i], tol)


def _runner(device='cpu', dtype=torch.float32, tol=2e-5, **size):
    m, seqs, refs, xp, cos, sin = _case(device, dtype, **size)
    dec = FusedMultiTransformerDecoder(m, len(LENS), MAXLEN)
    assert all(tuple(c.shape) == (2, len(LENS), m.kv_num_heads, MAXLEN, m.head_dim)
               for c in dec.caches)
    dec.set_rotary(cos, sin, 1)
    out = dec.prefill(paddle.Tensor(xp), seq_lens=list(LENS))
    for b, n in enumerate(LENS):
        _close(out._t[b, :n], refs[b][:n], tol)
    for i in range(STEPS):
        o = dec.step(paddle.Tensor(_tok(seqs, i)))
        for b, n in enumerate(LENS):
            _close(o._t[b, 0], refs[b][n + i], tol)
    assert dec.lens.tolist() == [n + STEPS for n in LENS]
    return dec


def test_gqa_ragged_generation_matches_each_sequence_alone():
    _functional()


def test_gqa_decoder_runner_ragged_rotary_cpu():
    dec = _runner()
    assert dec._graph is None


def test_gqa_validation():
    with pytest.raises(ValueError):
        FusedMultiTransformer(32, 4, 64, num_layers=1, gqa_group_size=3)     # 4 % 3
    with pytest.raises(ValueError):                  # 7 - 2*2 = 3 query heads over 2 K/V heads
        K.mmha_decode(torch.randn(2, 7, 8), torch.zeros(2, 2, 2, 12, 8), 5)
    with pytest.raises(ValueError):                  # no query head left
        K.mmha_decode(torch.randn(2, 4, 8), torch.zeros(2, 2, 2, 12, 8), 5)
    with pytest.raises(ValueError):                  # another batch / head dim
        K.mmha_decode(torch.randn(2, 8, 8), torch.zeros(2, 3, 2, 12, 8), 5)
    m = _gqa_model()
    x = paddle.Tensor(torch.randn(2, 1, 32))
    for heads in (4, 1):                             # the cache must hold KVH = 2 heads
        caches = [paddle.Tensor(torch.zeros(2, 2, heads, 12, 8)) for _ in range(2)]
        with pytest.raises(ValueError):
            m(x, caches=caches, time_step=3)
        with pytest.raises(ValueError):
            m(paddle.Tensor(torch.randn(2, 3, 32)), caches=caches)


# ----------------------------------------------------------------------------- GPU: the kernel
_TOL = {torch.bfloat16: 2e-2, torch.float32: 2e-5}

#        B  H  KVH L    lens         time_step  mask   D
_A = (3, 4, 2, 40, (0, 17, 39), 39, False, 64)      # one split; t_b = 0; the last cache slot
_B = (2, 8, 2, 700, (5, 650), 650, False, 128)      # split-K; sequence 0: all but one split empty
_C = (2, 16, 2, 700, (5, 650), 'dev', False, 64)    # device time_step: splits cover L; R = 8
_D = (2, 4, 2, 700, (5, 650), 650, True, 256)       # with a mask; t_b always visible; R = 2


def _kernel_vs_ref(case, dtype, rot_dims=0):
    B, H, KVH, L, lens, t, use_mask, D = case
    g = torch.Generator().manual_seed(D + L + H)
    qkv = torch.randn(B, H + 2 * KVH, D, generator=g).to(dtype).cuda()
    cache = torch.randn(2, B, KVH, L, D, generator=g).to(dtype).cuda()
    orig = cache.clone()
    if t == 'dev':
        t = torch.tensor([max(lens)], dtype=torch.int32).cuda()
    mask = None
    if use_mask:
        mask = torch.zeros(B, max(lens) + 1 + 3)
        mask[:, ::7] = float('-inf')
        for b, n in enumerate(lens):
            mask[b, n] = 0.0
        mask = mask.cuda()
    rotary = None
    if rot_dims:
        ang = torch.rand(B, D, generator=g) * (2 * np.pi)        # per-sequence angles
        rotary = (ang.cos().cuda(), ang.sin().cuda())
    sl = torch.tensor(lens, dtype=torch.int32).cuda()
    c_ref = cache.clone()
    ref = R.get_kernel('mmha_decode', 'ref')(
        qkv, c_ref, t, mask, seq_lens=sl,
        rotary=None if rotary is None else torch.stack(rotary), rotary_dims=rot_dims)
    before = R.stats().get(('mmha_decode_gqa', 'hip'), 0)
    out = K.mmha_decode(qkv, cache, t, mask, seq_lens=sl, rotary=rotary, rotary_dims=rot_dims)
    assert R.stats().get(('mmha_decode_gqa', 'hip'), 0) == before + 1
    assert out.shape == (B, H, D)
    return out, ref, cache, c_ref, orig


@pytest.mark.gpu
@pytest.mark.parametrize('case', [_A, _B, _C, _D], ids=['a', 'b', 'c', 'd'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_gqa_hip_kernel_gpu(case, dtype):
    out, ref, cache, c_ref, orig = _kernel_vs_ref(case, dtype)
    tol = _TOL[dtype]
    torch.testing.assert_close(out.float(), ref.float(), rtol=tol, atol=tol)
    torch.testing.assert_close(cache, c_ref)       # K/V appended at each t_b, nothing else
    assert not torch.equal(cache, orig)


@pytest.mark.gpu
@pytest.mark.parametrize('D,rot_dims', [(64, 1), (128, 1), (128, 2), (256, 1)])
@pytest.mark.parametrize('r', [2, 4, 8])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_gqa_sweep_with_rotary_in_kernel_gpu(D, rot_dims, r, dtype):
    tol = _TOL[dtype]
    case = (2, 2 * r, 2, 700, (5, 650), 650, False, D)
    before = R.stats().get(('mmha_decode_rotary', 'hip'), 0)
    out, ref, cache, c_ref, _ = _kernel_vs_ref(case, dtype, rot_dims=rot_dims)
    assert R.stats().get(('mmha_decode_rotary', 'hip'), 0) == before + 1
    torch.testing.assert_close(out.float(), ref.float(), rtol=tol, atol=tol)
    torch.testing.assert_close(cache, c_ref)       # a rotated row may differ by one rounding
    for b, n in enumerate(case[4]):                # the appended k row is the rotated one
        torch.testing.assert_close(cache[0, b, :, n], c_ref[0, b, :, n])


@pytest.mark.gpu
@pytest.mark.parametrize('r', [2, 4, 8])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_gqa_sweep_plain_host_step_gpu(r, dtype):
    # no seq_lens, rotary or mask: every runtime null check of the one instantiation is off
    B, KVH, L, D, t = 2, 3, 300, 128, 257
    g = torch.Generator().manual_seed(r)
    qkv = torch.randn(B, (r + 2) * KVH, D, generator=g).to(dtype).cuda()
    cache = torch.randn(2, B, KVH, L, D, generator=g).to(dtype).cuda()
    c_ref = cache.clone()
    ref = R.get_kernel('mmha_decode', 'ref')(qkv, c_ref, t, None)
    out = K.mmha_decode(qkv, cache, t)
    tol = _TOL[dtype]
    torch.testing.assert_close(out.float(), ref.float(), rtol=tol, atol=tol)
    torch.testing.assert_close(cache, c_ref)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_gqa_out_of_range_sequence_is_guarded_gpu(dtype):
    # the bad sequence is the middle one: an unguarded kernel's stray accesses stay inside the
    # cache tensor and show up in the cache comparison
    case = (3, 4, 2, 40, (3, 40, 7), 'dev', False, 64)
    out, ref, cache, c_ref, orig = _kernel_vs_ref(case, dtype)
    assert float(out[1].float().abs().sum()) == 0.0
    assert torch.equal(cache[:, 1], orig[:, 1])    # nothing written for b = 1
    tol = _TOL[dtype]
    torch.testing.assert_close(out[[0, 2]].float(), ref[[0, 2]].float(), rtol=tol, atol=tol)
    torch.testing.assert_close(cache, c_ref)
    assert not torch.equal(cache[:, 0], orig[:, 0]) and not torch.equal(cache[:, 2], orig[:, 2])


@pytest.mark.gpu
def test_gqa_dispatch_counts_gpu():
    qkv = torch.randn(2, 4 + 2 * 2, 64).cuda()
    cache = torch.zeros(2, 2, 2, 16, 64).cuda()
    R.reset_stats()
    for n in (1, 2):
        K.mmha_decode(qkv, cache, 3 + n)
        st = R.stats()
        assert st.get(('mmha_decode_gqa', 'hip'), 0) == n == st.get(('mmha_decode', 'hip'), 0), st
    assert ('mmha_decode', 'ref') not in st and ('mmha_decode_gqa', 'ref') not in st, st
    K.mmha_decode(torch.randn(2, 3, 2, 64).cuda(), cache, 7)     # the 4-D form: the plain kernel
    st = R.stats()
    assert st[('mmha_decode_gqa', 'hip')] == 2 and st[('mmha_decode', 'hip')] == 3, st


@pytest.mark.gpu
def test_gqa_unsupported_ratio_raises_gpu():
    qkv = torch.randn(2, 6 + 2 * 2, 64).cuda()                   # 6 query heads over 2: R = 3
    cache = torch.zeros(2, 2, 2, 16, 64).cuda()
    with pytest.raises(ValueError, match='2, 4, 8'):
        K.mmha_decode(qkv, cache, 3)
    assert float(cache.abs().sum()) == 0.0


# ----------------------------------------------------------------------------- one kernel, R = 1 too
# f16 against 'ref'. 'ref' computes in fp32 and rounds its result to f16 once, half an ulp or
# 2^-11 = 4.9e-4 relative; test_ref_in_f16_is_inside_the_f16_tolerance_of_float64 holds it to
# this bound against float64 on the CPU, so no wider power of ten was needed.
_TOL_F16 = 2e-3

#                     H  KVH lens      mask and rotary
_STEP = {'r1_plain': (4, 4, None, False),
         'r1_ragged': (4, 4, (5, 257), True),
         'r4_ragged': (8, 2, (5, 257), True)}


def _step(name, D, dtype, device='cpu'):
    """One decode step at B = 2, L = 300, time_step = 257: five splits of 52 keys, which is no
    multiple of the keys a workgroup takes per iteration (64 at D = 64, 32 at D = 128).
    Returns qkv (4-D when KVH = H), cache, time_step, mask and the keyword arguments."""
    H, KVH, lens, ext = _STEP[name]
    B, L, t = 2, 300, 257
    g = torch.Generator().manual_seed(D + H)
    qkv = torch.randn(B, H + 2 * KVH, D, generator=g).to(dtype).to(device)
    cache = torch.randn(2, B, KVH, L, D, generator=g).to(dtype).to(device)
    mask, kw = None, {}
    if ext:
        mask = torch.zeros(B, t + 1 + 3)
        mask[:, ::7] = float('-inf')
        for b, n in enumerate(lens):
            mask[b, n] = 0.0
        mask = mask.to(device)
        ang = torch.rand(B, D, generator=g) * (2 * np.pi)
        kw = dict(seq_lens=torch.tensor(lens, dtype=torch.int32).to(device),
                  rotary=torch.stack([ang.cos(), ang.sin()]).to(device), rotary_dims=1)
    if H == KVH:
        qkv = qkv.reshape(B, 3, H, D)
    return qkv, cache, t, mask, kw


def _f64(qkv, cache, t, mask, seq_lens=None, rotary=None, rotary_dims=0):
    """The step in float64; only the rotated new k is rounded to the cache dtype, as cached."""
    B, KVH, D = qkv.shape[0], cache.shape[2], qkv.shape[-1]
    row = qkv.reshape(B, -1, D).double()
    H = row.shape[1] - 2 * KVH
    q, k, v = row[:, :H], row[:, H:H + KVH], row[:, H + KVH:]
    if rotary is not None:
        cos, sin = rotary.double()
        q, k = K._rotate_rows(q, cos, sin, rotary_dims), K._rotate_rows(k, cos, sin, rotary_dims)
    k = k.to(qkv.dtype).double()
    out = torch.zeros(B, H, D, dtype=torch.float64)
    for b in range(B):
        n = t if seq_lens is None else int(seq_lens[b])
        K_ = torch.cat([cache[0, b, :, :n].double(), k[b][:, None]], 1).repeat_interleave(H // KVH, 0)
        V_ = torch.cat([cache[1, b, :, :n].double(), v[b][:, None]], 1).repeat_interleave(H // KVH, 0)
        s = torch.einsum('hd,hld->hl', q[b], K_) / np.sqrt(D)
        if mask is not None:
            s = s + mask[b, None, :n + 1].double()
        out[b] = torch.einsum('hl,hld->hd', torch.softmax(s, -1), V_)
    return out


@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('name', list(_STEP))
def test_ref_in_f16_is_inside_the_f16_tolerance_of_float64(name, D):
    qkv, cache, t, mask, kw = _step(name, D, torch.float16)
    ref = R.get_kernel('mmha_decode', 'ref')(qkv, cache.clone(), t, mask, **kw)
    torch.testing.assert_close(ref.double(), _f64(qkv, cache, t, mask, **kw), rtol=_TOL_F16, atol=_TOL_F16)


@pytest.mark.gpu
@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('name', list(_STEP))
def test_f16_hip_kernel_gpu(name, D):
    qkv, cache, t, mask, kw = _step(name, D, torch.float16, 'cuda')
    orig, c_ref = cache.clone(), cache.clone()
    ref = R.get_kernel('mmha_decode', 'ref')(qkv, c_ref, t, mask, **kw)
    out = K.mmha_decode(qkv, cache, t, mask, **kw)
    torch.testing.assert_close(out.float(), ref.float(), rtol=_TOL_F16, atol=_TOL_F16)
    torch.testing.assert_close(cache, c_ref)       # a rotated row may differ by one rounding
    assert not torch.equal(cache, orig)


@pytest.mark.gpu
@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('name', ['r1_plain', 'r1_ragged'])
def test_3d_and_4d_forms_agree_gpu(name, D):
    qkv4, cache, t, mask, kw = _step(name, D, torch.bfloat16, 'cuda')
    B, _, H, _ = qkv4.shape
    c3, c4 = cache.clone(), cache.clone()
    before = R.stats().get(('mmha_decode_gqa', 'hip'), 0)
    out3 = K.mmha_decode(qkv4.reshape(B, 3 * H, D), c3, t, mask, **kw)
    out4 = K.mmha_decode(qkv4, c4, t, mask, **kw)
    assert torch.equal(out3, out4) and torch.equal(c3, c4)
    assert not torch.equal(c3, cache)
    assert R.stats().get(('mmha_decode_gqa', 'hip'), 0) == before    # KVH = H is not grouped


@pytest.mark.gpu
@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_r1_split_boundaries_with_device_step_gpu(D, dtype):
    # a device time_step: five splits of 60 keys cover L = 300. Sequence 0 is at t = 0 (one key
    # of weight exactly 1 in split 0, four empty partials), sequence 1 in the last cache slot.
    B, H, L, lens = 2, 4, 300, (0, 299)
    g = torch.Generator().manual_seed(D)
    qkv = torch.randn(B, 3, H, D, generator=g).to(dtype).cuda()
    cache = torch.randn(2, B, H, L, D, generator=g).to(dtype).cuda()
    orig, c_ref = cache.clone(), cache.clone()
    t = torch.tensor([L - 1], dtype=torch.int32).cuda()
    sl = torch.tensor(lens, dtype=torch.int32).cuda()
    ref = R.get_kernel('mmha_decode', 'ref')(qkv, c_ref, t, None, seq_lens=sl)
    out = K.mmha_decode(qkv, cache, t, seq_lens=sl)
    assert torch.equal(out[0], ref[0]) and torch.equal(out[0], qkv[0, 2])
    tol = _TOL[dtype]
    torch.testing.assert_close(out[1].float(), ref[1].float(), rtol=tol, atol=tol)
    assert torch.equal(cache, c_ref)
    for b, n in enumerate(lens):                   # the appended rows, and no other row changed
        assert torch.equal(cache[0, b, :, n], qkv[b, 1]) and torch.equal(cache[1, b, :, n], qkv[b, 2])
        cache[:, b, :, n] = orig[:, b, :, n]
    assert torch.equal(cache, orig)


# ----------------------------------------------------------------------------- GPU: end to end
_BIG = dict(E=512, H=4, KVH=2)                       # head dim 128


def _only_the_gqa_hip_kernel(st):
    n = st.get(('mmha_decode_gqa', 'hip'), 0)
    assert n > 0 and st.get(('mmha_decode', 'hip'), 0) == n, st
    assert ('mmha_decode', 'ref') not in st and ('mmha_decode_gqa', 'ref') not in st, st
    # rotary went into the kernel on every decode call: no _rotary element-wise launches
    assert st.get(('mmha_decode_rotary', 'hip'), 0) == n, st
    return n


@pytest.mark.gpu
def test_gqa_ragged_generation_on_gpu_bf16():
    paddle.set_device('gpu')
    _case('cuda', torch.bfloat16, **_BIG)            # the references: context phase only
    R.reset_stats()
    _functional('cuda', torch.bfloat16, 2e-2, **_BIG)
    assert _only_the_gqa_hip_kernel(R.stats()) == 2 * STEPS


@pytest.mark.gpu
def test_gqa_decoder_runner_hip_graph_gpu():
    paddle.set_device('gpu')
    _case('cuda', torch.bfloat16, **_BIG)
    R.reset_stats()
    dec = _runner('cuda', torch.bfloat16, 2e-2, **_BIG)
    assert dec._graph is not None                    # one graph replayed for the ragged batch
    _only_the_gqa_hip_kernel(R.stats())
