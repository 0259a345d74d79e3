"""Multi-token decode step: T new tokens per sequence in one pass over the KV cache.

One definition for every layer: a multi-token step equals T consecutive single-token steps.
``'ref'`` is checked against that loop of the existing ``mmha_decode`` on the CPU, the HIP kernel
against ``'ref'`` on the GPU, ``fused_multi_transformer`` and the decoder runner against
single-token steps of themselves.

Tolerances are the project's: ``_TOL`` / ``_TOL_F16`` of ``test_decode_gqa`` (bf16 2e-2, fp32
2e-5, f16 2e-3) for kernel against ``'ref'``, for uint8 caches too (as ``test_decode_q8``), where
the appended bytes are compared bit for bit. Without rotary the appended float rows are bit-equal
as well; a rotated k is rounded from an fp32 rotation whose operation order differs between the
kernel and torch, so it is compared within the dtype's tolerance (as ``test_decode_paged`` does).
"""
import functools

import numpy as np
import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import FusedMultiTransformerDecoder
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

from test_decode_ragged import LENS, MAXLEN, _rot, _tables
from test_fused_multi_transformer import _causal, _close, _model
from test_decode_gqa import _BIG, _TOL, _TOL_F16, _case, _gqa_model
from test_decode_q8 import _scales
from test_decode_paged import _gathered, _paged, _same_bits, _spares_untouched

_TOLS = dict(_TOL)
_TOLS[torch.float16] = _TOL_F16


def _problem(B, T, H, KVH, L, D, seed, dtype=torch.float32, u8=False):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, H + 2 * KVH, D, generator=g).to(dtype)
    if u8:
        cache = torch.randint(1, 256, (2, B, KVH, L, D), generator=g, dtype=torch.uint8)
    else:
        cache = torch.randn(2, B, KVH, L, D, generator=g).to(dtype)
    return qkv, cache


def _rot_rows(B, T, D, seed):
    """[2, B, T, D]: an angle of its own for every token, so no row can stand in for another."""
    ang = torch.rand(B, T, D, generator=torch.Generator().manual_seed(seed)) * (2 * np.pi)
    return torch.stack([ang.cos(), ang.sin()])


def _mask_for(B, n, lens, T):
    """-inf in every 7th column, the new tokens' own columns open."""
    m = torch.zeros(B, n)
    m[:, ::7] = float('-inf')
    for b, t in enumerate(lens):
        m[b, max(t, 0):max(min(t + T, n), 0)] = 0.0
    return m


def _loop(qkv, cache, lens, mask=None, rotary=None, rot_dims=0, **kw):
    """T explicit single-token steps of the public ``mmha_decode`` at ``lens + j``."""
    B, T = qkv.shape[:2]
    outs = []
    for j in range(T):
        rkw = dict(rotary=rotary[:, :, j], rotary_dims=rot_dims) if rotary is not None else {}
        outs.append(K.mmha_decode(qkv[:, j].contiguous(), cache, max(lens) + j, mask,
                                  seq_lens=[n + j for n in lens], **rkw, **kw))
    return torch.stack(outs, 1)


# ----------------------------------------------------------------------------- CPU: 'ref' is the loop
_VARIANTS = ['plain', 'ragged_mask_rotary', 'gqa2', 'gqa3', 'q8_per_head', 'q8_per_seq', 'paged', 'paged_q8']


@pytest.mark.parametrize('variant', _VARIANTS)
def test_ref_is_the_loop_of_single_steps(variant):
    B, T, KVH, D, L = 3, 3, 2, 16, 16
    r = {'gqa2': 2, 'gqa3': 3}.get(variant, 1)
    H = KVH * r
    u8 = 'q8' in variant
    qkv, cache = _problem(B, T, H, KVH, L, D, seed=len(variant), u8=u8)
    lens, mask, kw, lkw = (6, 6, 6), None, {}, {}
    if variant != 'plain':
        lens = (2, 7, 10)                         # with BS 4: every sequence's tokens straddle a block
        kw['seq_lens'] = torch.tensor(lens)
    if variant == 'ragged_mask_rotary':
        mask = _mask_for(B, 14, lens, T)
        lkw = dict(rotary=_rot_rows(B, T, D, 5), rot_dims=1)
        kw.update(rotary=lkw['rotary'], rotary_dims=1)
    if u8:
        kq, vq = _scales(B, KVH, variant == 'q8_per_seq')
        kw.update(cache_k_quant_scales=kq, cache_v_quant_scales=vq)
        lkw.update(cache_k_quant_scales=kq, cache_v_quant_scales=vq)
    table = None
    if variant.startswith('paged'):
        cache, table = _paged(cache, 4, spare=3, seed=1)
        kw['block_tables'] = lkw['block_tables'] = table
    before, c_loop = cache.clone(), cache.clone()
    want = _loop(qkv, c_loop, lens, mask, **lkw)
    st = R.stats().get(('mmha_decode_multi', 'ref'), 0)
    got = K.mmha_decode_multi(qkv, cache, max(lens), mask, **kw)
    assert R.stats()[('mmha_decode_multi', 'ref')] == st + 1
    assert got.shape == (B, T, H, D) and torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert _same_bits(cache, c_loop) and not _same_bits(cache, before)
    if table is not None:
        assert _spares_untouched(cache, before, table)
        rows = _gathered(cache, table)
    else:
        rows = cache
    for b, n in enumerate(lens):                  # T rows appended per sequence
        assert not _same_bits(rows[0, b, :, n + T - 1], (_gathered(before, table) if table is not None
                                                        else before)[0, b, :, n + T - 1])


def test_ref_guard_is_all_or_nothing():
    B, T, KVH, D, L = 3, 3, 2, 16, 16
    ref = R.get_kernel('mmha_decode_multi', 'ref')
    qkv, cache = _problem(B, T, KVH, KVH, L, D, seed=3)
    dev_t = torch.tensor([L - 1], dtype=torch.int32)          # device-style position: nothing validated
    lens = (L - T, L - T + 1, 4)                  # the last position that fits; one past it
    c, before = cache.clone(), cache.clone()
    out = ref(qkv, c, dev_t, None, seq_lens=torch.tensor(lens, dtype=torch.int32))
    c_loop = cache.clone()
    want = _loop(qkv[[0, 2]], c_loop[:, [0, 2]].contiguous(), (lens[0], lens[2]))
    assert torch.equal(out[[0, 2]], want) and float(out[1].abs().sum()) == 0.0
    assert _same_bits(c[:, 1], before[:, 1]) and not _same_bits(c[:, 0], before[:, 0])
    # t_b < 0, t_b past a host bound, a mask shorter than t_b + T: guarded as a whole
    for lens, t, mlen, bad in (((-1, 4, 5), dev_t, None, 0), ((6, 5, 2), 5, None, 0), ((3, 9, 5), dev_t, 11, 1)):
        c = cache.clone()
        mask = None if mlen is None else torch.zeros(B, mlen)
        out = ref(qkv, c, t, mask, seq_lens=torch.tensor(lens, dtype=torch.int32))
        assert float(out[bad].abs().sum()) == 0.0 and _same_bits(c[:, bad], before[:, bad])
        for b in set(range(B)) - {bad}:
            assert float(out[b].abs().sum()) > 0.0 and not _same_bits(c[:, b], before[:, b])
    # paged: the second own block of sequence 1 has no entry
    pool, table = _paged(cache, 4, spare=2, seed=2)
    lens = (2, 7, 9)
    tab = table.clone()
    tab[1, 2] = -1                                # positions 8..11; sequence 1 writes 7, 8, 9
    p, pb = pool.clone(), pool.clone()
    out = ref(qkv, p, dev_t, None, seq_lens=torch.tensor(lens, dtype=torch.int32), tables=tab.int())
    assert float(out[1].abs().sum()) == 0.0 and float(out[0].abs().sum()) > 0.0
    assert _same_bits(p[:, table[1]], pb[:, table[1]]) and not _same_bits(p[:, table[0]], pb[:, table[0]])
    assert _spares_untouched(p, pb, table)


def test_host_validation():
    B, T, KVH, D, L = 3, 3, 2, 16, 16
    qkv, cache = _problem(B, T, KVH, KVH, L, D, seed=4)
    with pytest.raises(ValueError, match='T >= 1'):
        K.mmha_decode_multi(qkv[:, :0], cache, 3)
    with pytest.raises(ValueError, match='T >= 1'):
        K.mmha_decode_multi(qkv[:, 0], cache, 3)                  # a single-token row is mmha_decode's
    before = cache.clone()
    with pytest.raises(ValueError, match='time_step'):
        K.mmha_decode_multi(qkv, cache, L - T + 1)
    with pytest.raises(ValueError, match='seq_lens'):
        K.mmha_decode_multi(qkv, cache, 5, seq_lens=[2, 6, 1])    # past the bound
    with pytest.raises(ValueError, match='seq_lens'):
        K.mmha_decode_multi(qkv, cache, L - 2, seq_lens=[2, L - 2, 1])   # seq_lens + T > L
    assert _same_bits(cache, before)
    K.mmha_decode_multi(qkv, cache, L - T, seq_lens=[2, L - T, 1])       # the last position that fits
    pool, table = _paged(before, 4, spare=2, seed=2)
    tab = table.clone()
    tab[2, 1] = tab[0, 0]                         # sequence 2 (positions 3..5) appends to sequence 0's block
    with pytest.raises(ValueError, match='same block'):
        K.mmha_decode_multi(qkv, pool, 9, seq_lens=[1, 9, 3], block_tables=tab)
    tab = table.clone()
    tab[1, 3] = pool.shape[1]
    with pytest.raises(ValueError, match='outside the pool'):
        K.mmha_decode_multi(qkv, pool, 11, seq_lens=[1, 11, 3], block_tables=tab)
    K.mmha_decode_multi(qkv, pool, 9, seq_lens=[1, 9, 3], block_tables=table)


# ----------------------------------------------------------------------------- CPU: functional
@pytest.mark.parametrize('rotary', [False, True], ids=['plain', 'rotary'])
@pytest.mark.parametrize('model', ['mha', 'gqa', 'gqa_d64'])
def test_functional_three_tokens_are_three_steps(model, rotary):
    m = {'mha': lambda: _model(True), 'gqa': _gqa_model, 'gqa_d64': lambda: _gqa_model(E=128, H=2, KVH=1)}[model]()
    B, S0, S, Lc = 2, 5, 3, 12
    E, D = m.embed_dim, m.head_dim
    KVH = getattr(m, 'kv_num_heads', m.num_heads)
    x = torch.randn(B, S0 + S, E, generator=torch.Generator().manual_seed(1))
    cos, sin = _tables(D, Lc)

    def rot(lo, hi):
        return dict(rotary_embs=_rot(cos, sin, torch.arange(lo, hi).expand(B, -1), 'cpu'),
                    rotary_emb_dims=1) if rotary else {}

    caches = [paddle.Tensor(torch.zeros(2, B, KVH, Lc, D)) for _ in m.qkv_weights]
    with torch.no_grad():
        m(paddle.Tensor(x[:, :S0]), attn_mask=paddle.Tensor(_causal(S0, B)), caches=caches, **rot(0, S0))
        one = [paddle.Tensor(c._t.clone()) for c in caches]
        st = R.stats().get(('mmha_decode_multi', 'ref'), 0)
        got, _ = m(paddle.Tensor(x[:, S0:]), caches=caches, time_step=S0, **rot(S0, S0 + S))
        assert R.stats()[('mmha_decode_multi', 'ref')] == st + len(m.qkv_weights)
        want = [m(paddle.Tensor(x[:, S0 + j:S0 + j + 1]), caches=one, time_step=S0 + j,
                  **rot(S0 + j, S0 + j + 1))[0]._t for j in range(S)]
    assert tuple(got.shape) == (B, S, E)
    _close(got._t, torch.cat(want, 1), 2e-5)
    for a, b in zip(caches, one):
        _close(a._t, b._t, 2e-5)


# ----------------------------------------------------------------------------- the runner
def _runner_kw(kind, m, device, B):
    if kind == 'float':
        return {}
    if kind == 'int8_dynamic':
        return dict(kv_cache_dtype='int8', cache_scales=None)
    return dict(kv_cache_dtype='int8', cache_scales=[
        tuple(s.to(device) for s in _scales(B, m.kv_num_heads, False, base=(5.0 + i, 4.0 + i)))
        for i in range(len(m.qkv_weights))])


def _alone_steps(m, cos, sin, maxlen, prompt, toks, kw):
    """One sequence alone in a batch-1 runner: prefill, then one ``step`` per token."""
    d = FusedMultiTransformerDecoder(m, 1, maxlen, use_graph=False, **kw)
    d.set_rotary(cos, sin, 1)
    d.prefill(paddle.Tensor(prompt[None]))
    return [d.step(paddle.Tensor(t[None, None]))._t[0, 0] for t in toks]


def _speculative(m, cos, sin, lens, maxlen, plan, device='cpu', dtype=torch.float32, tol=2e-5, kind='float',
                 BS=None, num_blocks=None, use_graph=True):
    """prefill, then per entry of ``plan``: ``('multi', T, accepted)`` is step_multi + commit,
    ``('step',)`` a single step. Every output row against that sequence alone with single steps
    over the tokens it kept, so a rejected row that leaked into a later step would show."""
    B, E = len(lens), m.embed_dim
    g = torch.Generator().manual_seed(23)
    xp = torch.randn(B, max(lens), E, generator=g).to(device, dtype)
    kw = _runner_kw(kind, m, device, B)
    d = FusedMultiTransformerDecoder(m, B, maxlen, use_graph=use_graph, **kw,
                                     **({} if BS is None else dict(block_size=BS, num_blocks=num_blocks)))
    d.set_rotary(cos, sin, 1)
    d.prefill(paddle.Tensor(xp), seq_lens=list(lens))
    kept = [[] for _ in lens]                     # the tokens each sequence has kept so far
    pos = list(lens)
    for step in plan:
        if step[0] == 'step':
            tok = torch.randn(B, 1, E, generator=g).to(device, dtype)
            out = d.step(paddle.Tensor(tok))._t
            for b in range(B):
                kept[b].append(tok[b, 0])
                _close(out[b, 0], _alone_steps(m, cos, sin, maxlen, xp[b, :lens[b]], kept[b], kw)[-1], tol)
            pos = [p + 1 for p in pos]
            continue
        _, T, acc = step
        tok = torch.randn(B, T, E, generator=g).to(device, dtype)
        out = d.step_multi(paddle.Tensor(tok))._t
        assert tuple(out.shape) == (B, T, E) and d.lens.tolist() == pos          # nothing advanced
        for b in range(B):
            ref = _alone_steps(m, cos, sin, maxlen, xp[b, :lens[b]], kept[b] + list(tok[b]), kw)
            _close(out[b], torch.stack(ref[len(kept[b]):]), tol)
            kept[b] += list(tok[b, :acc[b]])
        d.commit(acc if step is not plan[0] else torch.tensor(acc))             # a tensor and a list
        pos = [p + a for p, a in zip(pos, acc)]
        assert d.lens.tolist() == pos and int(d.t) == max(pos)
        if BS is not None:
            assert d._pos == pos
    return d


def test_runner_cpu_contiguous():
    m, _, _, _, cos, sin = _case()
    d = _speculative(m, cos, sin, LENS, MAXLEN, [('multi', 4, [4, 2, 0]), ('step',), ('multi', 2, [1, 2, 0])])
    with pytest.raises(RuntimeError, match='step_multi'):
        d.commit([0, 0, 0])                       # nothing to commit
    d.step_multi(paddle.Tensor(torch.zeros(3, 2, m.embed_dim)))
    with pytest.raises(ValueError, match='counts'):
        d.commit([3, 0, 0])


def test_runner_cpu_uniform_prefill_switches_to_per_sequence_positions():
    m, _, _, _, cos, sin = _case()
    B, S0, E = 2, 5, m.embed_dim
    x = torch.randn(B, S0 + 4, E, generator=torch.Generator().manual_seed(3))
    d = FusedMultiTransformerDecoder(m, B, MAXLEN)
    d.set_rotary(cos, sin, 1)
    d.prefill(paddle.Tensor(x[:, :S0]))
    a = d.step(paddle.Tensor(x[:, S0:S0 + 1]))._t
    assert not d.ragged
    out = d.step_multi(paddle.Tensor(x[:, S0 + 1:S0 + 3]))._t
    assert d.ragged and d.lens.tolist() == [S0 + 1] * B
    d.commit([2, 1])
    last = d.step(paddle.Tensor(x[:, S0 + 3:S0 + 4]))._t
    for b, keep in enumerate(([0, 1, 2, 3], [0, 1, 3])):          # the tokens each sequence kept
        ref = _alone_steps(m, cos, sin, MAXLEN, x[b, :S0], list(x[b, S0:S0 + 3]), {})
        _close(a[b, 0], ref[0], 2e-5)
        _close(out[b], torch.stack(ref[1:3]), 2e-5)
        ref = _alone_steps(m, cos, sin, MAXLEN, x[b, :S0], [x[b, S0 + i] for i in keep], {})
        _close(last[b, 0], ref[-1], 2e-5)


@pytest.mark.parametrize('kind', ['float', 'int8_static'])
def test_runner_cpu_paged(kind):
    m, _, _, _, cos, sin = _case()
    # prompts 2, 5, 7 hold 1 + 2 + 2 blocks of 4; [2, 6), [5, 9) and [7, 11) need one more each,
    # and after commit and step sequence 0 is at 7, where [7, 9) starts its third block
    d = _speculative(m, cos, sin, LENS, MAXLEN, [('multi', 4, [4, 2, 0]), ('step',), ('multi', 2, [1, 2, 0])],
                     kind=kind, BS=4, num_blocks=9)
    assert d.free_blocks == 0 and [len(b) for b in d._blocks] == [3, 3, 3]


def test_runner_cpu_pool_too_small_changes_nothing():
    m, _, _, _, cos, sin = _case()
    d = FusedMultiTransformerDecoder(m, len(LENS), MAXLEN, block_size=4, num_blocks=7)
    d.set_rotary(cos, sin, 1)
    xp = torch.randn(len(LENS), max(LENS), m.embed_dim, generator=torch.Generator().manual_seed(2))
    d.prefill(paddle.Tensor(xp), seq_lens=list(LENS))
    state = (d.lens.clone(), d.tables.clone(), list(d._pos), [list(b) for b in d._blocks],
             [c.clone() for c in d.caches])
    assert d.free_blocks == 2
    with pytest.raises(RuntimeError, match='free'):
        d.step_multi(paddle.Tensor(torch.zeros(len(LENS), 4, m.embed_dim)))
    assert d.free_blocks == 2 and torch.equal(d.tables, state[1]) and torch.equal(d.lens, state[0])
    assert d._pos == state[2] and d._blocks == state[3]
    assert all(torch.equal(a, b) for a, b in zip(d.caches, state[4]))
    d.step_multi(paddle.Tensor(torch.zeros(len(LENS), 2, m.embed_dim)))   # [2, 4), [5, 7), [7, 9): one block
    assert d.free_blocks == 1


# ----------------------------------------------------------------------------- GPU: the HIP kernel
_B, _KVH, _L = 3, 2, 256                          # device time_step: 4 splits of 64 keys


def _straddle(T):
    return 64 - T // 2                            # 62 for T = 4: the new tokens straddle the split at 64


def _len_sets(T):
    return [(0, 1, _straddle(T)),                 # only new tokens; one cached key; across the split boundary
            (64, _L - T, _L - T + 1),             # the split's first key; the last position that fits; guarded
            (_L, 5, 130)]                         # guarded


def _kernel_vs_ref(r, T, D, dtype, lens, t='dev', use_mask=False, rot_dims=0, dyn=None, round_type=1,
                   BS=None, table_edit=None, mask_len=None, L=_L, seed=0):
    """One multi-token step of the HIP kernel and of ``'ref'`` on clones of the same cache."""
    B, KVH = _B, _KVH
    H, u8 = KVH * r, dyn is not None
    qkv, cache = _problem(B, T, H, KVH, L, D, seed=D + T + H + seed, dtype=dtype, u8=u8)
    table = None
    if BS is not None:
        cache, table = _paged(cache, BS, spare=3, seed=D + BS)
        if table_edit is not None:
            table = table_edit(table.clone(), cache.shape[1])
    qkv, cache = qkv.cuda(), cache.cuda()
    kw, pub = {}, {}
    if lens is not None:
        kw['seq_lens'] = torch.tensor(lens, dtype=torch.int32).cuda()
    tt = torch.tensor([max(lens)], dtype=torch.int32).cuda() if t == 'dev' else t
    pos = lens if lens is not None else (t,) * B
    mask = None
    if use_mask:
        mask = _mask_for(B, mask_len or L, pos, T).cuda()
    if rot_dims:
        kw.update(rotary=_rot_rows(B, T, D, D + T).cuda(), rotary_dims=rot_dims)
    rkw = dict(kw)
    if u8:
        kq, vq = (s.cuda() for s in _scales(B, KVH, dyn, base=(3.6, 3.9)))
        pub = dict(cache_k_quant_scales=kq, cache_v_quant_scales=vq, quant_round_type=round_type)
        rkw['quant'] = K._kv_quant_args(B, cache, kq, vq, round_type=round_type, device=qkv.device)
    if table is not None:
        pub['block_tables'] = table.int().cuda()                 # a device table: never validated
        rkw['tables'] = table.int().cuda()
    before, c_ref = cache.clone(), cache.clone()
    ref = R.get_kernel('mmha_decode_multi', 'ref')(qkv, c_ref, tt, mask, **rkw)
    R.reset_stats()
    out = K.mmha_decode_multi(qkv, cache, tt, mask, **kw, **pub)
    st = R.stats()
    assert st.get(('mmha_decode_multi', 'hip'), 0) == 1 and not [k for k in st if k[1] == 'ref'], st
    assert out.shape == (B, T, H, D) and bool(torch.isfinite(out.float()).all())
    tol = _TOLS[dtype]
    torch.testing.assert_close(out.float(), ref.float(), rtol=tol, atol=tol)
    for b in range(B):
        if float(ref[b].float().abs().sum()) == 0.0:              # guarded: exact zeros
            assert float(out[b].float().abs().sum()) == 0.0
    if rot_dims and not u8:                       # v and everything untouched bit for bit; a rotated k within tol
        assert _same_bits(cache[1], c_ref[1])
        torch.testing.assert_close(cache[0].float().nan_to_num(7.0), c_ref[0].float().nan_to_num(7.0),
                                   rtol=tol, atol=tol)
        changed = _bits_differ(cache[0], before[0])
        assert torch.equal(changed, _bits_differ(c_ref[0], before[0]))
    else:                                         # the appended rows and all the rest: the bits of 'ref'
        assert _same_bits(cache, c_ref)
    if table is not None:
        assert _spares_untouched(cache, before, table)
    return out, ref, cache, before


def _bits_differ(a, b):
    """Per row [..., D]: whether any bit changed."""
    from test_decode_paged import _bits
    return (_bits(a) != _bits(b)).any(-1)


_RT = [(1, 2), (1, 3), (1, 4), (1, 5), (1, 8), (2, 2), (2, 3), (2, 4), (4, 2)]
_SHAPES = [(r, T, 128, dt) for r, T in _RT for dt in (torch.bfloat16, torch.float32)] + \
          [(r, T, D, dt) for r, T in ((1, 4), (2, 2)) for D in (64, 256) for dt in (torch.bfloat16, torch.float32)] + \
          [(1, 3, 128, torch.float16), (2, 4, 64, torch.float16)]


@pytest.mark.gpu
@pytest.mark.parametrize('r,T,D,dtype', _SHAPES, ids=[f'r{r}-T{T}-D{D}-{str(d)[6:]}' for r, T, D, d in _SHAPES])
def test_multi_hip_kernel_gpu(r, T, D, dtype):
    for lens in _len_sets(T):
        out, ref, cache, before = _kernel_vs_ref(r, T, D, dtype, lens)
        for b, n in enumerate(lens):
            rows = slice(n, n + T)
            if n + T <= _L:                       # T rows appended, nothing else touched
                assert not _same_bits(cache[:, b, :, n + T - 1], before[:, b, :, n + T - 1])
                cache[:, b, :, rows] = before[:, b, :, rows]
        assert _same_bits(cache, before)


@pytest.mark.gpu
@pytest.mark.parametrize('t', [0, 63, 64, 130])
@pytest.mark.parametrize('r,T', [(1, 4), (2, 3)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_multi_host_time_step_gpu(r, T, t, dtype):
    _kernel_vs_ref(r, T, 128, dtype, None, t=t)                   # splits sized by t + T, no seq_lens
    _kernel_vs_ref(r, T, 128, dtype, (t, 0, t // 2), t=t)
    _kernel_vs_ref(r, T, 128, dtype, (t + 1, t, 0), t=t)          # past the host bound: guarded


@pytest.mark.gpu
@pytest.mark.parametrize('rot_dims', [1, 2])
@pytest.mark.parametrize('r,T,D', [(1, 4, 128), (2, 3, 128), (1, 5, 64), (2, 2, 256)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_multi_mask_and_rotary_gpu(r, T, D, rot_dims, dtype):
    for lens in _len_sets(T)[:2]:
        _kernel_vs_ref(r, T, D, dtype, lens, use_mask=True, rot_dims=rot_dims)
    # a mask that ends one column before t_b + T guards the sequence; one that ends at it does not
    out, ref, _, _ = _kernel_vs_ref(r, T, D, dtype, (100 - T, 101 - T, 50), use_mask=True, rot_dims=rot_dims,
                                    mask_len=100)
    assert float(out[1].float().abs().sum()) == 0.0 and float(out[0].float().abs().sum()) > 0.0
    # every token has its own rotary row: with token 0's row for all, 'ref' itself moves away
    B, H = _B, _KVH * r
    qkv, cache = _problem(B, T, H, _KVH, _L, D, seed=1, dtype=dtype)
    rot = _rot_rows(B, T, D, 9)
    lens = torch.tensor([5, 70, 130], dtype=torch.int32)
    f = R.get_kernel('mmha_decode_multi', 'ref')
    a = f(qkv, cache.clone(), torch.tensor([130], dtype=torch.int32), None, seq_lens=lens, rotary=rot,
          rotary_dims=rot_dims)
    b = f(qkv, cache.clone(), torch.tensor([130], dtype=torch.int32), None, seq_lens=lens,
          rotary=rot[:, :, :1].expand(2, B, T, D).contiguous(), rotary_dims=rot_dims)
    assert float((a[:, 1:].float() - b[:, 1:].float()).abs().max()) > 10 * _TOLS[dtype]


@pytest.mark.gpu
@pytest.mark.parametrize('round_type', [0, 1])
@pytest.mark.parametrize('dyn', [False, True], ids=['per_head', 'per_seq'])
@pytest.mark.parametrize('r,T,D', [(1, 4, 128), (2, 3, 128), (4, 2, 64), (1, 8, 256)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_multi_q8_gpu(r, T, D, dyn, round_type, dtype):
    for lens in _len_sets(T):
        _kernel_vs_ref(r, T, D, dtype, lens, dyn=dyn, round_type=round_type)     # bytes bit-equal inside
    _kernel_vs_ref(r, T, D, dtype, _len_sets(T)[0], dyn=dyn, round_type=round_type, use_mask=True)


@pytest.mark.gpu
@pytest.mark.parametrize('u8', [False, True], ids=['float', 'uint8'])
@pytest.mark.parametrize('BS', [16, 64])
@pytest.mark.parametrize('r,T', [(1, 4), (2, 3), (1, 8)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_multi_paged_gpu(r, T, BS, u8, dtype):
    dyn = True if u8 else None
    for lens in [(BS - 1, BS - T + 1, 0)] + _len_sets(T):         # the new tokens straddle a block boundary
        _kernel_vs_ref(r, T, 128, dtype, lens, dyn=dyn, BS=BS)
    _kernel_vs_ref(r, T, 128, dtype, (BS - 1, 70, 2 * BS), dyn=dyn, BS=BS, use_mask=True,
                   rot_dims=0 if u8 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize('u8', [False, True], ids=['float', 'uint8'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_multi_paged_untrusted_table_gpu(dtype, u8):
    BS, T, dyn = 16, 4, (False if u8 else None)
    lens = (3 * BS - 2, 5 * BS + 1, 2 * BS + 3)   # sequence 0 writes blocks 2 and 3, the others one block

    def read_only(tab, NB):                       # blocks that are only read: weight 0
        tab[0, 1], tab[1, 0], tab[2, 1] = -1, NB + 5, -1
        return tab

    out, ref, _, _ = _kernel_vs_ref(2, T, 128, dtype, lens, dyn=dyn, BS=BS, table_edit=read_only)
    assert all(float(out[b].float().abs().sum()) > 0.0 for b in range(_B))
    for col, bad in ((2, -1), (3, -1), (3, 'past')):              # either own block of sequence 0
        def own(tab, NB, col=col, bad=bad):
            tab[0, col] = NB + 5 if bad == 'past' else bad
            return tab
        out, ref, cache, before = _kernel_vs_ref(2, T, 128, dtype, lens, dyn=dyn, BS=BS, table_edit=own)
        assert float(out[0].float().abs().sum()) == 0.0 and float(out[1].float().abs().sum()) > 0.0
        assert not _same_bits(cache, before)      # the others wrote; 'ref' and the kernel agree on where


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32])
def test_multi_identity_table_is_the_contiguous_cache_gpu(dtype):
    B, KVH, T, D, L = _B, _KVH, 3, 128, 64
    qkv, cache = _problem(B, T, 2 * KVH, KVH, L, D, seed=8, dtype=dtype)
    qkv, cache = qkv.cuda(), cache.cuda()
    lens = torch.tensor([0, 33, L - T], dtype=torch.int32).cuda()
    t = torch.tensor([L - 1], dtype=torch.int32).cuda()
    table = torch.arange(B, dtype=torch.int32)[:, None].cuda()    # BS = L, MB = 1: the pool is the cache
    c1, c2 = cache.clone(), cache.clone()
    a = K.mmha_decode_multi(qkv, c1, t, seq_lens=lens)
    b = K.mmha_decode_multi(qkv, c2, t, seq_lens=lens, block_tables=table)
    assert _same_bits(a, b) and _same_bits(c1, c2) and not _same_bits(c1, cache)


@pytest.mark.gpu
def test_multi_dispatch_and_limits_gpu():
    D, L = 128, 64
    for r, T in ((2, 5), (4, 3), (8, 2), (1, 9), (3, 2)):
        qkv, cache = _problem(_B, T, _KVH * r, _KVH, L, D, seed=1, dtype=torch.bfloat16)
        before = cache.clone()
        with pytest.raises(ValueError, match='query rows per K/V row'):
            K.mmha_decode_multi(qkv.cuda(), cache.cuda(), 3)
        assert _same_bits(cache, before)
    qkv, cache = _problem(_B, 4, _KVH, _KVH, L, D, seed=1, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='CUDA int32'):
        K.mmha_decode_multi(qkv.cuda(), cache.cuda(), torch.tensor([3]).cuda())
    with pytest.raises(ValueError, match='time_step'):
        K.mmha_decode_multi(qkv.cuda(), cache.cuda(), L - 3)
    R.reset_stats()
    K.mmha_decode_multi(qkv.cuda(), cache.cuda(), 3)
    assert R.stats() == {('mmha_decode_multi', 'hip'): 1}


# ----------------------------------------------------------------------------- GPU: the runner from captured graphs
_GBS, _GMAX, _GLENS = 16, 48, (13, 5, 16)         # [13, 17) and [16, 20) cross a block boundary


@functools.lru_cache(None)
def _gpu_model():
    m = _case('cuda', torch.bfloat16, **_BIG)[0]   # 4 query heads over 2 K/V heads, head dim 128
    return (m,) + tuple(_tables(m.head_dim, _GMAX))


@pytest.mark.gpu
@pytest.mark.parametrize('kind,BS', [('float', None), ('float', _GBS), ('int8_static', None), ('int8_dynamic', _GBS)])
def test_runner_hip_graphs_gpu(kind, BS):
    paddle.set_device('gpu')
    m, cos, sin = _gpu_model()
    R.reset_stats()
    d = _speculative(m, cos, sin, _GLENS, _GMAX, [('multi', 4, [4, 2, 0]), ('step',), ('multi', 2, [1, 2, 0])],
                     device='cuda', dtype=torch.bfloat16, tol=2e-2, kind=kind, BS=BS, num_blocks=8)
    graphs = {T: e[1] for T, e in d._multi.items()}
    assert sorted(graphs) == [2, 4] and all(g is not None for g in graphs.values()) and d._graph is not None
    st = R.stats()
    assert st.get(('mmha_decode_multi', 'hip'), 0) > 0, st
    assert not [k for k in st if k[0].startswith('mmha_decode') and k[1] == 'ref'], st
    x = torch.zeros(len(_GLENS), 4, m.embed_dim, device='cuda', dtype=torch.bfloat16)
    calls = st[('mmha_decode_multi', 'hip')]
    d.step_multi(paddle.Tensor(x))
    d.commit([1, 1, 1])
    d.step_multi(paddle.Tensor(x[:, :2]))
    assert {T: e[1] for T, e in d._multi.items()} == graphs       # replayed: nothing captured again
    assert R.stats()[('mmha_decode_multi', 'hip')] == calls
