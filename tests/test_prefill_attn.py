"""Prefill attention over the KV cache: up to T new tokens per sequence appended to a cache that
may already hold positions, equal to that many consecutive single-token steps.

``'ref'`` is checked against the loop of public ``mmha_decode`` steps on the CPU, the HIP kernels
against ``'ref'`` on the GPU with the project's tolerances (``_TOL`` / ``_TOL_F16`` of
``test_decode_gqa``: bf16 2e-2, f16 2e-3), ``fused_multi_transformer`` and the decoder's ``extend``
against single-token steps of themselves. Appended uint8 bytes and un-rotated float rows are
compared bit for bit, a rotated k within the dtype's tolerance (as ``test_decode_multi``).

The attend kernel takes 128 query rows per workgroup, (128 / ratio) tokens, and 64 keys per tile:
T in {1, 63, 64, 65, 130} crosses the token tile at ratio 4 and 8 (32 and 16 tokens), T 128 / 129 /
130 at ratio 1; the prefixes put the diagonal on, next to and off a key-tile edge.
"""
import functools

import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import FusedMultiTransformerDecoder
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

from test_decode_ragged import LENS, MAXLEN, _tables
from test_fused_multi_transformer import _causal, _close
from test_decode_gqa import _case, _gqa_model
from test_decode_q8 import _scales
from test_decode_paged import _gathered, _paged, _same_bits, _spares_untouched
from test_decode_multi import _TOLS, _bits_differ, _mask_for, _problem, _rot_rows, _speculative


def _steps(qkv, cache, lens, news, mask=None, rotary=None, rot_dims=0, table=None, scales=None):
    """Sequence by sequence, ``news[b]`` single-token steps of the public ``mmha_decode``."""
    B, T, N, D = qkv.shape
    out = torch.zeros(B, T, N - 2 * cache.shape[2], D, dtype=qkv.dtype)
    for b in range(B):
        c = cache if table is not None else cache[:, b:b + 1].contiguous()
        kw = {} if table is None else dict(block_tables=table[b:b + 1])
        if scales is not None:
            kq, vq = (s[b:b + 1] if s.dim() == 2 else s for s in scales)
            kw.update(cache_k_quant_scales=kq, cache_v_quant_scales=vq)
        for j in range(news[b]):
            if rotary is not None:
                kw.update(rotary=rotary[:, b:b + 1, j], rotary_dims=rot_dims)
            out[b, j] = K.mmha_decode(qkv[b:b + 1, j].contiguous(), c, lens[b] + j,
                                      None if mask is None else mask[b:b + 1], seq_lens=[lens[b] + j], **kw)[0]
        if table is None:
            cache[:, b] = c[:, 0]
    return out


# ----------------------------------------------------------------------------- CPU: 'ref' is the loop
@pytest.mark.parametrize('variant', ['plain', 'mask_rotary', 'gqa2', 'gqa3', 'q8_per_head', 'q8_per_seq', 'paged',
                                     'paged_q8'])
def test_ref_is_the_loop_of_single_steps(variant):
    B, T, KVH, D, L = 3, 9, 2, 16, 32
    lens, news = (0, 5, 13), (9, 0, 6)
    H = KVH * {'gqa2': 2, 'gqa3': 3}.get(variant, 1)
    u8 = 'q8' in variant
    qkv, cache = _problem(B, T, H, KVH, L, D, seed=len(variant), u8=u8)
    mask, kw, lkw = None, dict(seq_lens=torch.tensor(lens), new_lens=torch.tensor(news)), {}
    if variant == 'mask_rotary':
        mask = _mask_for(B, 20, lens, T)                      # sequence 2 ends at 19
        lkw = dict(rotary=_rot_rows(B, T, D, 5), rot_dims=1)
        kw.update(rotary=lkw['rotary'], rotary_dims=1)
    if u8:
        lkw['scales'] = _scales(B, KVH, variant == 'q8_per_seq')
        kw.update(cache_k_quant_scales=lkw['scales'][0], cache_v_quant_scales=lkw['scales'][1])
    table = None
    if variant.startswith('paged'):
        cache, table = _paged(cache, 4, spare=3, seed=1)
        kw['block_tables'] = lkw['table'] = table
    before, c_loop = cache.clone(), cache.clone()
    want = _steps(qkv, c_loop, lens, news, mask, **lkw)
    got = K.mmha_prefill(qkv, cache, max(lens), mask, **kw)
    assert R.stats()[('mmha_prefill', 'ref')] >= 1
    assert got.shape == (B, T, H, D) and torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert float(got[1].abs().sum()) == 0.0 and float(got[2, 6:].abs().sum()) == 0.0
    assert _same_bits(cache, c_loop) and not _same_bits(cache, before)
    if table is not None:
        assert _spares_untouched(cache, before, table)


def test_ref_guard_is_per_sequence():
    B, T, KVH, D, L = 3, 4, 2, 16, 16
    ref = R.get_kernel('mmha_prefill', 'ref')
    qkv, cache = _problem(B, T, KVH, KVH, L, D, seed=3)
    dev_t = torch.tensor([L - 1], dtype=torch.int32)          # device-style position: nothing validated
    for lens, news, table_edit in (((L - 4, L - 3, 4), (4, 4, 4), None),      # fits exactly; one row too many
                                   ((2, 6, 9), (4, 3, 2), (1, 2))):           # [6, 9) needs block 2 of row 1
        c, table = cache.clone(), None
        if table_edit:
            c, table = _paged(cache, 4, spare=2, seed=2)
            table = table.clone()
            table[table_edit] = c.shape[1] + 3
        before, c_loop = c.clone(), c.clone()
        out = ref(qkv, c, dev_t, None, seq_lens=torch.tensor(lens, dtype=torch.int32),
                  new_lens=torch.tensor(news, dtype=torch.int32), tables=None if table is None else table.int())
        want = _steps(qkv[[0, 2]], c_loop if table is not None else c_loop[:, [0, 2]].contiguous(),
                      (lens[0], lens[2]), (news[0], news[2]), table=None if table is None else table[[0, 2]])
        assert torch.equal(out[[0, 2]], want) and float(out[1].abs().sum()) == 0.0
        if table is None:
            assert _same_bits(c[:, 1], before[:, 1]) and not _same_bits(c[:, 0], before[:, 0])
        else:
            assert _same_bits(c, c_loop) and _spares_untouched(c, before, table)


def test_host_validation():
    B, T, KVH, D, L = 3, 3, 2, 16, 16
    qkv, cache = _problem(B, T, KVH, KVH, L, D, seed=4)
    before = cache.clone()
    for bad in ([1, 4, 0], [1, -1, 0]):
        with pytest.raises(ValueError, match='new_lens'):
            K.mmha_prefill(qkv, cache, 3, new_lens=bad)
    with pytest.raises(ValueError, match='seq_lens'):
        K.mmha_prefill(qkv, cache, L - 2, seq_lens=[2, L - 2, 1])            # seq_lens + T > L
    K.mmha_prefill(qkv, cache.clone(), L - 2, seq_lens=[2, L - 2, 1], new_lens=[3, 2, 0])
    pool, table = _paged(before, 4, spare=2, seed=2)
    tab = table.clone()
    tab[2, 1] = tab[0, 0]                         # sequence 2 (positions 3..5) appends to sequence 0's block
    with pytest.raises(ValueError, match='same block'):
        K.mmha_prefill(qkv, pool, 9, seq_lens=[1, 9, 3], block_tables=tab)
    K.mmha_prefill(qkv, pool.clone(), 9, seq_lens=[1, 9, 3], new_lens=[3, 3, 1], block_tables=tab)   # 3 stays in its own
    assert _same_bits(cache, before)


# ----------------------------------------------------------------------------- CPU: functional and runner
def test_functional_new_lens_are_single_steps():
    m = _gqa_model()
    B, S0, S, Lc, news = 2, 5, 3, 12, (3, 2)
    x = torch.randn(B, S0 + S, m.embed_dim, generator=torch.Generator().manual_seed(1))
    caches = [paddle.Tensor(torch.zeros(2, B, m.kv_num_heads, Lc, m.head_dim)) for _ in m.qkv_weights]
    with torch.no_grad():
        m(paddle.Tensor(x[:, :S0]), attn_mask=paddle.Tensor(_causal(S0, B)), caches=caches)
        one = [paddle.Tensor(c._t.clone()) for c in caches]
        st = R.stats().get(('mmha_prefill', 'ref'), 0)
        got, _ = m(paddle.Tensor(x[:, S0:]), caches=caches, time_step=S0, new_lens=list(news))
        assert R.stats()[('mmha_prefill', 'ref')] == st + len(m.qkv_weights)
        want = torch.cat([m(paddle.Tensor(x[:, S0 + j:S0 + j + 1]), caches=one, time_step=S0 + j)[0]._t
                          for j in range(S)], 1)
    for b, n in enumerate(news):
        _close(got._t[b, :n], want[b, :n], 2e-5)
        for a, c in zip(caches, one):
            _close(a._t[:, b, :, :S0 + n], c._t[:, b, :, :S0 + n], 2e-5)
            assert float(a._t[:, b, :, S0 + n:].abs().sum()) == 0.0


def test_extend_in_chunks_is_single_steps_cpu():
    m, _, _, _, cos, sin = _case()
    B, E, chunks = len(LENS), m.embed_dim, (5, 1, 7)
    x = torch.randn(B, sum(chunks), E, generator=torch.Generator().manual_seed(2))

    def fresh(nb):
        d = FusedMultiTransformerDecoder(m, B, MAXLEN, block_size=4, num_blocks=nb)
        d.set_rotary(cos, sin, 1)
        return d
    d, one = fresh(12), fresh(12)
    want = torch.cat([one.step(paddle.Tensor(x[:, j:j + 1]))._t for j in range(x.shape[1])], 1)
    got, at = [], 0
    for n in chunks:
        got.append(d.extend(paddle.Tensor(x[:, at:at + n]))._t)
        at += n
    _close(torch.cat(got, 1), want, 2e-5)
    assert d._pos == [at] * B and d.lens.tolist() == [at] * B and int(d.t) == at
    for a, c in zip(d.caches, one.caches):
        _close(_gathered(a, d.tables)[:, :, :, :at], _gathered(c, one.tables)[:, :, :, :at], 2e-5)
    # ragged counts advance each slot by its own; a short free list raises before anything changes
    d = fresh(5)
    d.extend(paddle.Tensor(x[:, :4]), new_lens=[4, 0, 2])
    state = (d.lens.clone(), d.tables.clone(), list(d._pos), [list(b) for b in d._blocks], [c.clone() for c in d.caches])
    assert d._pos == [4, 0, 2] and d.free_blocks == 3
    with pytest.raises(RuntimeError, match='free'):
        d.extend(paddle.Tensor(x[:, :7]))                     # [4, 11), [0, 7), [2, 9): 2 + 2 + 2 new blocks
    assert d.free_blocks == 3 and torch.equal(d.tables, state[1]) and torch.equal(d.lens, state[0])
    assert d._pos == state[2] and d._blocks == state[3]
    assert all(torch.equal(a, b) for a, b in zip(d.caches, state[4]))


# ----------------------------------------------------------------------------- GPU: the HIP kernels
_KVH, _L = 2, 256
_PREFIX = (0, 1, 63, 64, 100)                     # empty; key-tile edge - 1 and on it; diagonal off the edge


def _ragged(T):
    return (T, 0, max(T // 2, 1), T, max(T - 1, 1))   # a full chunk, none, a partial tile


def _kernel_vs_ref(r, T, D, dtype, lens=_PREFIX, news='ragged', use_mask=False, rot_dims=0, dyn=None, BS=None,
                   table_edit=None, mask_len=None):
    """One prefill step of the HIP kernels and of ``'ref'`` on clones of the same cache."""
    B, KVH, L = len(lens), _KVH, _L
    H, u8 = KVH * r, dyn is not None
    news = _ragged(T)[:B] if news == 'ragged' else news
    qkv, cache = _problem(B, T, H, KVH, L, D, seed=D + T + H, dtype=dtype, u8=u8)
    table = None
    if BS is not None:
        cache, table = _paged(cache, BS, spare=3, seed=D + BS)
        if table_edit is not None:
            table = table_edit(table.clone(), cache.shape[1])
    qkv, cache = qkv.cuda(), cache.cuda()
    kw = dict(seq_lens=torch.tensor(lens, dtype=torch.int32).cuda())
    if news is not None:
        kw['new_lens'] = torch.tensor(news, dtype=torch.int32).cuda()
    tt = torch.tensor([max(lens)], dtype=torch.int32).cuda()
    mask = _mask_for(B, mask_len or L, lens, T).cuda() if use_mask else None
    if rot_dims:
        kw.update(rotary=_rot_rows(B, T, D, D + T).cuda(), rotary_dims=rot_dims)
    rkw, pub = dict(kw), {}
    if u8:
        kq, vq = (s.cuda() for s in _scales(B, KVH, dyn, base=(3.6, 3.9)))
        pub = dict(cache_k_quant_scales=kq, cache_v_quant_scales=vq)
        rkw['quant'] = K._kv_quant_args(B, cache, kq, vq, device=qkv.device)
    if table is not None:
        pub['block_tables'] = rkw['tables'] = table.int().cuda()  # a device table: never validated
    before, c_ref = cache.clone(), cache.clone()
    ref = R.get_kernel('mmha_prefill', 'ref')(qkv, c_ref, tt, mask, **rkw)
    R.reset_stats()
    out = K.mmha_prefill(qkv, cache, tt, mask, **kw, **pub)
    st = R.stats()
    assert st.get(('mmha_prefill', 'hip'), 0) == 1 and not [k for k in st if k[1] == 'ref'], st
    assert out.shape == (B, T, H, D) and bool(torch.isfinite(out.float()).all())
    tol = _TOLS[dtype]
    torch.testing.assert_close(out.float(), ref.float(), rtol=tol, atol=tol)
    assert torch.equal(out.float().abs().sum(-1) == 0, ref.float().abs().sum(-1) == 0)   # padded and guarded rows
    if rot_dims and not u8:                       # v and everything untouched bit for bit; a rotated k within tol
        assert _same_bits(cache[1], c_ref[1])
        torch.testing.assert_close(cache[0].float().nan_to_num(7.0), c_ref[0].float().nan_to_num(7.0),
                                   rtol=tol, atol=tol)
        assert torch.equal(_bits_differ(cache[0], before[0]), _bits_differ(c_ref[0], before[0]))
    else:
        assert _same_bits(cache, c_ref)
    if table is not None:
        assert _spares_untouched(cache, before, table)
    return out, cache, before


_RT = [(r, T) for r in (1, 4, 8) for T in (1, 63, 64, 65, 130)] + [(1, 128), (1, 129)]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('r,T', _RT)
def test_prefill_hip_kernel_gpu(r, T, D, dtype):
    _kernel_vs_ref(r, T, D, dtype)
    out, cache, before = _kernel_vs_ref(r, T, D, dtype, news=None)            # every sequence takes all T
    for b, n in enumerate(_PREFIX):               # T rows appended, nothing else touched
        assert not _same_bits(cache[:, b, :, n + T - 1], before[:, b, :, n + T - 1])
        cache[:, b, :, n:n + T] = before[:, b, :, n:n + T]
    assert _same_bits(cache, before)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('rot_dims', [1, 2])
@pytest.mark.parametrize('r,T,D', [(1, 65, 128), (4, 65, 64), (8, 63, 128), (2, 130, 64)])
def test_prefill_mask_and_rotary_gpu(r, T, D, rot_dims, dtype):
    _kernel_vs_ref(r, T, D, dtype, use_mask=True, rot_dims=rot_dims)
    _kernel_vs_ref(r, T, D, dtype, use_mask=True)
    _kernel_vs_ref(r, T, D, dtype, rot_dims=rot_dims)


@pytest.mark.gpu
@pytest.mark.parametrize('dyn', [False, True], ids=['per_head', 'per_seq'])
@pytest.mark.parametrize('BS', [None, 16, 64])
@pytest.mark.parametrize('r,T,D,dtype', [(1, 65, 128, torch.bfloat16), (4, 70, 64, torch.float16),
                                         (8, 33, 128, torch.float16)])
def test_prefill_q8_gpu(r, T, D, dtype, BS, dyn):
    _kernel_vs_ref(r, T, D, dtype, dyn=dyn, BS=BS)                            # bytes bit-equal inside
    _kernel_vs_ref(r, T, D, dtype, dyn=dyn, BS=BS, use_mask=True, news=None)


@pytest.mark.gpu
@pytest.mark.parametrize('BS', [16, 64])
@pytest.mark.parametrize('r,T,D,dtype', [(1, 70, 128, torch.bfloat16), (4, 70, 128, torch.float16),
                                         (2, 130, 64, torch.bfloat16)])
def test_prefill_paged_gpu(r, T, D, dtype, BS):
    lens = (BS - 1, 0, 2 * BS - 3, 64, 100)       # the new tokens straddle block boundaries
    _kernel_vs_ref(r, T, D, dtype, lens=lens, BS=BS)
    _kernel_vs_ref(r, T, D, dtype, lens=lens, BS=BS, use_mask=True, rot_dims=1)

    def read_only(tab, NB):                       # blocks that are only read: their keys carry weight 0
        tab[2, 0], tab[4, 0] = -1, NB + 5         # prefixes 2 BS - 3 and 100: block 0 holds no new position
        return tab
    out, _, _ = _kernel_vs_ref(r, T, D, dtype, lens=lens, BS=BS, table_edit=read_only)
    assert float(out[2].float().abs().sum()) > 0.0 and float(out[4].float().abs().sum()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('u8', [False, True], ids=['float', 'uint8'])
def test_prefill_device_guards_gpu(u8):
    dyn, T = (False if u8 else None), 70
    # overflow alone, no mask: 186 + 70 = L fits exactly, 187 + 70 is one row too many; then a mask one
    # column short of 100 + 70 with every sequence inside L: that sequence only, each time
    for lens, mask_len, bad in (((0, 187, 63, 186, 100), None, 1), (_PREFIX, 169, 4)):
        out, cache, before = _kernel_vs_ref(4, T, 128, torch.bfloat16, lens=lens, news=None, dyn=dyn,
                                            use_mask=mask_len is not None, mask_len=mask_len)
        for b in range(5):
            assert (float(out[b].float().abs().sum()) == 0.0) == (b == bad)
            assert _same_bits(cache[:, b], before[:, b]) == (b == bad)

    def own(tab, NB):                             # sequence 2 writes [63, 133): blocks 3..8 at BS 16
        tab[2, 5] = NB
        return tab
    out, cache, before = _kernel_vs_ref(4, T, 128, torch.bfloat16, news=None, dyn=dyn, BS=16, table_edit=own)
    assert float(out[2].float().abs().sum()) == 0.0 and float(out[3].float().abs().sum()) > 0.0
    assert not _same_bits(cache, before)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_prefill_meets_decode_multi_at_the_seam_gpu(dtype):
    B, T, D, L = 3, 4, 128, 256
    qkv, cache = _problem(B, T, _KVH, _KVH, L, D, seed=8, dtype=dtype)
    qkv, c1 = qkv.cuda(), cache.cuda()
    c2 = c1.clone()
    lens = torch.tensor([0, 62, 130], dtype=torch.int32).cuda()
    t = torch.tensor([130], dtype=torch.int32).cuda()
    a = K.mmha_prefill(qkv, c1, t, seq_lens=lens)
    b = K.mmha_decode_multi(qkv, c2, t, seq_lens=lens)
    torch.testing.assert_close(a.float(), b.float(), rtol=_TOLS[dtype], atol=_TOLS[dtype])
    assert _same_bits(c1, c2) and not _same_bits(c1, cache.cuda())


@pytest.mark.gpu
def test_prefill_hip_refuses_what_it_does_not_support_gpu():
    for r, D, match in ((3, 128, 'ratio'), (1, 256, 'head_dim')):
        qkv, cache = _problem(2, 40, _KVH * r, _KVH, 64, D, seed=1, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match=match):
            K.mmha_prefill(qkv.cuda(), cache.cuda(), 3)
    qkv, cache = _problem(2, 40, _KVH, _KVH, 64, 128, seed=1, dtype=torch.bfloat16)
    pool, table = _paged(cache, 8, spare=1)
    with pytest.raises(ValueError, match='block size'):
        K.mmha_prefill(qkv.cuda(), pool.cuda(), 3, block_tables=table)


# ----------------------------------------------------------------------------- GPU: the runner
@functools.lru_cache(None)
def _gpu_model():
    m = _case('cuda', torch.bfloat16, E=512, H=4, KVH=1)[0]       # 4 query heads over 1 K/V head, head dim 128
    return (m,) + tuple(_tables(m.head_dim, 128))


@pytest.mark.gpu
@pytest.mark.parametrize('kind,BS', [('float', None), ('int8_dynamic', 16)])
def test_step_multi_beyond_the_multi_kernel_runs_prefill_in_the_graph_gpu(kind, BS):
    """T 8 x 4 query heads per K/V head = 32 rows > MULTI_MAX_ROWS: the captured step_multi graph holds
    the prefill launches; three replays, every row against the sequence alone with eager steps."""
    paddle.set_device('gpu')
    m, cos, sin = _gpu_model()
    R.reset_stats()
    d = _speculative(m, cos, sin, (13, 5, 16), 128, [('multi', 8, [8, 3, 0]), ('step',), ('multi', 8, [1, 2, 0]),
                                                     ('multi', 8, [8, 8, 8])],
                     device='cuda', dtype=torch.bfloat16, tol=2e-2, kind=kind, BS=BS, num_blocks=9)
    st = R.stats()
    assert list(d._multi) == [8] and d._multi[8][1] is not None, d._multi
    assert st.get(('mmha_prefill', 'hip'), 0) > 0 and ('mmha_decode_multi', 'hip') not in st, st
    assert not [k for k in st if k[0].startswith('mmha_') and k[1] == 'ref'], st


@pytest.mark.gpu
def test_extend_on_a_prefilled_paged_decoder_gpu():
    paddle.set_device('gpu')
    m, cos, sin = _gpu_model()
    lens, news, T, maxlen, E = (13, 5, 16), (70, 33, 0), 70, 128, m.embed_dim
    g = torch.Generator().manual_seed(5)
    xp, xc, xs = (torch.randn(3, n, E, generator=g).cuda().bfloat16() for n in (max(lens), T, 1))

    def decoder(B):
        d = FusedMultiTransformerDecoder(m, B, maxlen, use_graph=False, block_size=16, num_blocks=8 * B)
        d.set_rotary(cos, sin, 1)
        return d
    d = decoder(3)
    d.prefill(paddle.Tensor(xp), seq_lens=list(lens))
    R.reset_stats()
    out = d.extend(paddle.Tensor(xc), new_lens=list(news))._t
    st = R.stats()
    assert st.get(('mmha_prefill', 'hip'), 0) == len(m.qkv_weights) and not [k for k in st if k[1] == 'ref'], st
    last = d.step(paddle.Tensor(xs))._t
    assert d._pos == [a + n + 1 for a, n in zip(lens, news)] and d.lens.tolist() == d._pos
    assert bool(torch.isfinite(out.float()).all())
    for b, (a, n) in enumerate(zip(lens, news)):  # the sequence alone, one step per token
        one = decoder(1)
        one.prefill(paddle.Tensor(xp[b:b + 1, :a]))
        want = [one.step(paddle.Tensor(xc[b:b + 1, j:j + 1]))._t[0, 0] for j in range(n)]
        want.append(one.step(paddle.Tensor(xs[b:b + 1]))._t[0, 0])
        if n:
            _close(out[b, :n], torch.stack(want[:-1]), 2e-2)
        _close(last[b, 0], want[-1], 2e-2)
        for c, c1 in zip(d.caches, one.caches):
            _close(_gathered(c, d.tables[b:b + 1])[:, :, :, :a + n + 1],
                   _gathered(c1, one.tables)[:, :, :, :a + n + 1], 2e-2)
