"""Paged KV cache on the decode path: a block pool ``[2, NB, KVH, BS, D]`` shared by the
sequences through ``block_tables`` ``[B, MB]``.

CPU: the paged ``'ref'`` kernel against the contiguous ``'ref'`` on the gathered cache (plain,
ragged with mask and rotary, guarded, uint8 pools), block-boundary positions, out-of-range
table entries, prefix sharing, the argument checks; a ``FusedMultiTransformer`` on pools against
itself on contiguous caches; the paged ``FusedMultiTransformerDecoder`` against the contiguous
one, its block accounting, exhaustion, and ``release`` / ``admit``. GPU: the PAGED HIP kernels
against ``'ref'`` on a cloned pool, boundary positions, untrusted tables, the identity table
against the contiguous kernel, dispatch, and the runner from one captured graph."""
import functools

import numpy as np
import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import FusedMultiTransformerDecoder
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

from test_decode_ragged import LENS, MAXLEN, STEPS, _i32, _rot, _tables, _tok
from test_fused_multi_transformer import _causal, _close
from test_decode_gqa import _BIG, _TOL, _TOL_F16, _case, _gqa_model
from test_decode_q8 import _scales, _static_scales

_TOLS = dict(_TOL)
_TOLS[torch.float16] = _TOL_F16


# ----------------------------------------------------------------------------- pools and tables
def _blocks(cache, BS):
    """[2, B, KVH, L, D] -> [2, B, MB, KVH, BS, D]."""
    _, B, KVH, L, D = cache.shape
    return cache.reshape(2, B, KVH, L // BS, BS, D).permute(0, 1, 3, 2, 4, 5)


def _paged(cache, BS, spare=3, seed=0):
    """A pool that holds the contiguous ``cache`` in shuffled physical blocks, the sequences'
    blocks interleaved, with ``spare`` unreferenced blocks: NaN in a float pool, byte 7 in a
    uint8 one. Returns the pool and the host table [B, MB]."""
    _, B, KVH, L, D = cache.shape
    MB = L // BS
    NB = B * MB + spare
    perm = torch.randperm(NB, generator=torch.Generator().manual_seed(seed))[:B * MB]
    table = perm.reshape(MB, B).t().contiguous()                  # (b, j) -> perm[j*B + b]
    if cache.dtype == torch.uint8:
        pool = torch.full((2, NB, KVH, BS, D), 7, dtype=torch.uint8, device=cache.device)
    else:
        pool = torch.full((2, NB, KVH, BS, D), float('nan'), dtype=cache.dtype, device=cache.device)
    pool[:, table.to(cache.device)] = _blocks(cache, BS)
    return pool, table


def _gathered(pool, table):
    """The contiguous cache [2, B, KVH, MB*BS, D] a table of valid entries describes."""
    _, _, KVH, BS, D = pool.shape
    B, MB = table.shape
    g = pool[:, table.to(pool.device).long()]                     # [2, B, MB, KVH, BS, D]
    return g.permute(0, 1, 3, 2, 4, 5).reshape(2, B, KVH, MB * BS, D).contiguous()


def _bits(x):
    """For comparisons that must hold bit for bit, NaN included."""
    return x.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _spares_untouched(pool, before, table):
    """Every block that ``table`` does not name is bit for bit as it was."""
    spare = torch.ones(pool.shape[1], dtype=torch.bool)
    t = table.reshape(-1).cpu().long()
    spare[t[(t >= 0) & (t < pool.shape[1])]] = False
    assert int(spare.sum()) > 0
    return _same_bits(pool[:, spare.to(pool.device)], before[:, spare.to(pool.device)])


def _problem(B, H, KVH, L, D, seed, dtype=torch.float32, u8=False):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, H + 2 * KVH, D, generator=g).to(dtype)
    if u8:
        cache = torch.randint(1, 256, (2, B, KVH, L, D), generator=g, dtype=torch.uint8)
    else:
        cache = torch.randn(2, B, KVH, L, D, generator=g).to(dtype)
    return qkv, cache


def _mask(B, n, lens):
    m = torch.zeros(B, n)
    m[:, ::7] = float('-inf')
    for b, t in enumerate(lens):
        if t < n:
            m[b, t] = 0.0
    return m


# ----------------------------------------------------------------------------- CPU: the ref kernel
_VARIANTS = ['plain', 'ragged_mask_rotary', 'guarded', 'q8_per_head', 'q8_per_seq']


@pytest.mark.parametrize('r', [1, 2, 3])
@pytest.mark.parametrize('variant', _VARIANTS)
def test_paged_ref_is_ref_on_the_gathered_cache(variant, r):
    B, KVH, D, BS, MB = 3, 2, 16, 4, 3
    L, H = MB * BS, KVH * r
    u8 = variant.startswith('q8')
    qkv, cache = _problem(B, H, KVH, L, D, seed=r, u8=u8)
    pool, table = _paged(cache, BS, spare=4, seed=r)
    assert pool.shape[1] > B * MB and _same_bits(_gathered(pool, table), cache)
    t, kw, mask, lens = 6, {}, None, (6, 6, 6)
    if variant == 'ragged_mask_rotary':
        lens = (0, 6, 3)
        ang = torch.rand(B, D, generator=torch.Generator().manual_seed(11)) * (2 * np.pi)
        kw = dict(seq_lens=torch.tensor(lens), rotary=torch.stack([ang.cos(), ang.sin()]), rotary_dims=1)
        mask = torch.zeros(B, t + 2)
        mask[:, 1::3] = float('-inf')
        for b, n in enumerate(lens):
            mask[b, n] = 0.0
    elif variant == 'guarded':      # device-style positions: the middle sequence is at t_b = L
        t = torch.tensor([L - 1], dtype=torch.int32)
        lens = (6, L, 2)
        kw = dict(seq_lens=torch.tensor(lens))
    pub = {}
    if u8:
        kq, vq = _scales(B, KVH, variant == 'q8_per_seq')
        kw['quant'] = K._kv_quant_args(B, cache, kq, vq)
        pub = dict(cache_k_quant_scales=kq, cache_v_quant_scales=vq)
    qrow = qkv if r > 1 else qkv.reshape(B, 3, H, D)
    c_ref, p_out, before = cache.clone(), pool.clone(), pool.clone()
    want = R.get_kernel('mmha_decode', 'ref')(qrow, c_ref, t, mask, **kw)
    got = R.get_kernel('mmha_decode_paged', 'ref')(qrow, p_out, t, mask, table, **kw)
    assert got.shape == (B, H, D) and torch.equal(got, want)
    assert bool(torch.isfinite(got).all())
    expect = before.clone()
    expect[:, table] = _blocks(c_ref, BS)         # the contiguous result scattered
    assert _same_bits(p_out, expect)
    assert not _same_bits(p_out, before)          # something was appended
    assert _spares_untouched(p_out, before, table)
    if variant == 'guarded':
        assert float(got[1].abs().sum()) == 0.0
        assert _same_bits(p_out[:, table[1]], before[:, table[1]])
    else:                                         # the public entry takes the same path
        p2 = pool.clone()
        st = R.stats().get(('mmha_decode_paged', 'ref'), 0)
        pkw = {k: v for k, v in kw.items() if k != 'quant'}
        out = K.mmha_decode(qkv, p2, t, mask, block_tables=table, **pkw, **pub)
        assert R.stats()[('mmha_decode_paged', 'ref')] == st + 1
        assert torch.equal(out, want) and _same_bits(p2, expect)


def test_paged_ref_at_block_boundaries():
    # t_b = 0; the last row of a block; the first row of a block that nothing has read yet
    B, H, KVH, D, BS, MB = 3, 4, 2, 16, 4, 3
    lens = (0, BS - 1, BS)
    qkv, cache = _problem(B, H, KVH, MB * BS, D, seed=5)
    for b, n in enumerate(lens):
        cache[:, b, :, n:] = float('nan')         # rows at and past t_b were never written
    pool, table = _paged(cache, BS)
    c_ref, before = cache.clone(), pool.clone()
    want = R.get_kernel('mmha_decode', 'ref')(qkv, c_ref, BS, None, seq_lens=torch.tensor(lens))
    got = K.mmha_decode(qkv, pool, BS, seq_lens=list(lens), block_tables=table.tolist())
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert torch.equal(got[0], qkv[0, H + KVH:].repeat_interleave(H // KVH, 0))   # one key of weight 1
    for b, n in enumerate(lens):                  # the row landed in the block the table names
        e = int(table[b, n // BS])
        assert torch.equal(pool[0, e, :, n % BS], qkv[b, H:H + KVH])
        assert torch.equal(pool[1, e, :, n % BS], qkv[b, H + KVH:])
        pool[:, e, :, n % BS] = before[:, e, :, n % BS]
    assert _same_bits(pool, before)               # and nothing else was written


def _untrusted(B, H, KVH, D, BS, MB, lens, seed, dtype=torch.float32, u8=False):
    """Sequence 1: an earlier block -1 and another one NB + 5; sequence 2: its own block -1.
    Returns the problem and what the contiguous ref gives with those positions masked."""
    L = MB * BS
    qkv, cache = _problem(B, H, KVH, L, D, seed, dtype, u8)
    pool, good = _paged(cache, BS, seed=seed)
    NB = pool.shape[1]
    table = good.clone()
    own = [n // BS for n in lens]
    assert own[1] >= 2
    lost = [0, own[1] - 1]
    table[1, lost[0]], table[1, lost[1]] = -1, NB + 5
    table[2, own[2]] = -1
    mask = torch.zeros(B, L)
    for j in lost:
        mask[1, j * BS:(j + 1) * BS] = float('-inf')
    guarded = torch.tensor([lens[0], lens[1], L])  # sequence 2 as the oracle guards it
    return qkv, cache, pool, table, good, mask, guarded


def test_paged_ref_out_of_range_entries():
    B, H, KVH, D, BS, MB = 3, 4, 2, 16, 4, 3
    lens = (6, 9, 5)
    qkv, cache, pool, table, good, mask, guarded = _untrusted(B, H, KVH, D, BS, MB, lens, seed=3)
    t = torch.tensor([MB * BS - 1], dtype=torch.int32)            # device-style: nothing validated
    c_ref, before = cache.clone(), pool.clone()
    want = R.get_kernel('mmha_decode', 'ref')(qkv, c_ref, t, mask, seq_lens=guarded)
    got = K.mmha_decode(qkv, pool, t, seq_lens=torch.tensor(lens), block_tables=table)
    torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-5)
    assert bool(torch.isfinite(got).all())
    assert float(got[2].abs().sum()) == 0.0 and float(got[1].abs().sum()) > 0
    # sequence 1 without the lost positions: they carried weight 0
    keep = torch.ones(MB * BS, dtype=torch.bool)
    keep[(mask[1] == float('-inf')).nonzero().reshape(-1)] = False
    keep[lens[1] + 1:] = False
    rep = H // KVH
    kk = c_ref[0, 1][:, keep].repeat_interleave(rep, 0)
    vv = c_ref[1, 1][:, keep].repeat_interleave(rep, 0)
    p = torch.softmax(torch.einsum('hd,hld->hl', qkv[1, :H], kk) / np.sqrt(D), -1)
    torch.testing.assert_close(got[1], torch.einsum('hl,hld->hd', p, vv), rtol=2e-5, atol=2e-5)
    expect = before.clone()
    expect[:, good] = _blocks(c_ref, BS)
    assert _same_bits(pool, expect)               # sequence 2 wrote nothing, the others one row each
    assert _same_bits(pool[:, good[2]], before[:, good[2]])
    assert not _same_bits(pool[:, good[1]], before[:, good[1]])


def test_paged_ref_prefix_sharing():
    B, H, KVH, D, BS, MB = 2, 4, 2, 16, 4, 3
    lens = (9, 10)
    qkv, cache = _problem(B, H, KVH, MB * BS, D, seed=8)
    cache[:, 1, :, :2 * BS] = cache[:, 0, :, :2 * BS]             # a common prefix of two blocks
    private, ptab = _paged(cache, BS, seed=1)
    shared, stab = private.clone(), ptab.clone()
    stab[1, :2] = stab[0, :2]
    shared[:, ptab[1, :2]] = float('nan')         # sequence 1's own copies are gone
    before = shared.clone()
    a = K.mmha_decode(qkv, private, 10, seq_lens=list(lens), block_tables=ptab)
    b = K.mmha_decode(qkv, shared, 10, seq_lens=list(lens), block_tables=stab)
    assert torch.equal(a, b) and bool(torch.isfinite(b).all())
    assert _same_bits(shared[:, stab[0, :2]], before[:, stab[0, :2]])
    for s in range(B):
        assert _same_bits(shared[:, stab[s, 2]], private[:, ptab[s, 2]])
        assert not _same_bits(shared[:, stab[s, 2]], before[:, stab[s, 2]])


def test_paged_validation():
    B, H, KVH, D, BS, MB = 2, 4, 2, 8, 4, 3
    qkv, cache = _problem(B, H, KVH, MB * BS, D, seed=2)
    pool, table = _paged(cache, BS)
    NB = pool.shape[1]
    K.mmha_decode(qkv, pool.clone(), 9, seq_lens=[5, 9], block_tables=table)
    K.mmha_decode(qkv, pool.clone(), 9, seq_lens=[5, 9], block_tables=table.numpy())
    uncovered = table.clone()
    uncovered[0, 2] = -1                          # sequence 0 at t_b = 5 never reaches block 2
    K.mmha_decode(qkv, pool.clone(), 9, seq_lens=[5, 9], block_tables=uncovered)
    bad_cover, bad_big, same = table.clone(), table.clone(), table.clone()
    bad_cover[1, 1] = -1                          # covers positions 4..7 of sequence 1 at t_b = 9
    bad_big[0, 0] = NB
    same[1, 2] = same[0, 1]                       # both append to one block (t_b = 5 and 9)
    bad = [
        (pool, dict(block_tables=bad_cover)),
        (pool, dict(block_tables=bad_big)),
        (pool, dict(block_tables=same)),
        (pool.reshape(2, NB, KVH, BS * D), dict(block_tables=table)),             # a pool is 5-D
        (pool, dict(block_tables=table[:1])),                                     # another batch
        (pool, dict(block_tables=torch.cat([table, table]))),
        (pool, dict(block_tables=table.reshape(-1))),
        (pool, dict(block_tables=table.float())),
        (torch.zeros(2, B + 1, KVH, D), dict(block_tables=table)),                # a 4-D cache of another B
        (pool[..., :4], dict(block_tables=table)),                                # another head dim
        (pool[:, :, :1].expand(2, NB, 3, BS, D), dict(block_tables=table)),       # 8 - 2*3 heads over 3
    ]
    for p, kw in bad:
        c = p.clone()
        with pytest.raises(ValueError):
            K.mmha_decode(qkv, c, 9, seq_lens=[5, 9], **kw)
        assert _same_bits(c, p)
    with pytest.raises(ValueError):               # positions are logical: L = MB*BS
        K.mmha_decode(qkv, pool.clone(), MB * BS, block_tables=table)
    with pytest.raises(ValueError):
        K.mmha_decode(qkv, pool.clone(), 9, seq_lens=[5, 10], block_tables=table)
    # shared blocks that are only read are fine; a uint8 pool wants its scales
    K.mmha_decode(qkv, pool.clone(), 9, seq_lens=[9, 5], block_tables=torch.stack([table[0], table[0]]))
    with pytest.raises(ValueError):
        K.mmha_decode(qkv, torch.full_like(pool, 128, dtype=torch.uint8), 9, block_tables=table)
    m = _case()[0]
    with pytest.raises(ValueError):               # the layers want pools with a table
        m(paddle.Tensor(torch.randn(2, 1, 32)), time_step=3, block_tables=table)
    with pytest.raises(ValueError):
        FusedMultiTransformerDecoder(m, 2, 16, num_blocks=4)
    with pytest.raises(ValueError):
        FusedMultiTransformerDecoder(m, 2, 16, block_size=0)
    with pytest.raises(RuntimeError):
        FusedMultiTransformerDecoder(m, 2, 16).release(0)


# ----------------------------------------------------------------------------- CPU: the layers
def test_paged_generation_matches_contiguous_caches():
    m, seqs, refs, xp, cos, sin = _case()
    B, S0, KVH, D, BS = len(LENS), max(LENS), m.kv_num_heads, m.head_dim, 4
    L = MAXLEN
    zero = torch.zeros(2, B, KVH, L, D)
    pools, tables = [], []
    for i in range(2):
        p, t = _paged(zero, BS, spare=2, seed=20)  # one table for all layers
        pools.append(p)
        tables.append(t)
    table = tables[0]
    caches = [paddle.Tensor(zero.clone()) for _ in range(2)]
    pcaches = [paddle.Tensor(p) for p in pools]
    spare_before = [p.clone() for p in pools]

    def both(xs, mask, lens, pos, **kw):
        args = dict(attn_mask=paddle.Tensor(mask), seq_lens=_i32(lens, 'cpu'),
                    rotary_embs=_rot(cos, sin, pos, 'cpu'), rotary_emb_dims=1, **kw)
        with torch.no_grad():
            a, _ = m(paddle.Tensor(xs), caches=caches, **args)
            b, _ = m(paddle.Tensor(xs), caches=pcaches, block_tables=table, **args)
        _close(b._t, a._t, 2e-5)
        return b._t
    out = both(xp, _causal(S0, B), LENS, torch.arange(S0).expand(B, S0))
    for b, n in enumerate(LENS):
        _close(out[b, :n], refs[b][:n], 2e-5)
    R.reset_stats()
    for i in range(STEPS):
        lens = [n + i for n in LENS]
        out = both(_tok(seqs, i), torch.zeros(B, 1, 1, S0 + i + 1), lens, torch.tensor(lens)[:, None],
                   time_step=S0 + i)
        for b, n in enumerate(LENS):
            _close(out[b, 0], refs[b][n + i], 2e-5)
        for c, p in zip(caches, pools):
            g = _gathered(p, table)
            for b, n in enumerate(lens):
                assert torch.equal(g[:, b, :, :n + 1], c._t[:, b, :, :n + 1])
                assert float(g[:, b, :, :n + 1].abs().sum()) > 0
    assert R.stats()[('mmha_decode_paged', 'ref')] == 2 * STEPS
    for p, s in zip(pools, spare_before):
        assert _spares_untouched(p, s, table)


def test_context_phase_skips_positions_without_a_block():
    m, _, _, xp, cos, sin = _case()
    B, S0, KVH, D, BS = len(LENS), max(LENS), m.kv_num_heads, m.head_dim, 4
    zero = torch.zeros(2, B, KVH, MAXLEN, D)
    pool, table = _paged(zero, BS, seed=4)
    table[0, 1] = -1                              # positions 4..7 of sequence 0 have no block
    lost = int(_paged(zero, BS, seed=4)[1][0, 1])
    pools = [paddle.Tensor(pool.clone()) for _ in range(2)]
    caches = [paddle.Tensor(zero.clone()) for _ in range(2)]
    args = dict(attn_mask=paddle.Tensor(_causal(S0, B)), rotary_emb_dims=1,
                rotary_embs=_rot(cos, sin, torch.arange(S0).expand(B, S0), 'cpu'))
    with torch.no_grad():
        a, _ = m(paddle.Tensor(xp), caches=caches, **args)
        b, _ = m(paddle.Tensor(xp), caches=pools, block_tables=table, **args)
    assert torch.equal(a._t, b._t)                # the context phase's own attention is unchanged
    for c, p in zip(caches, pools):
        assert float(p._t[:, lost].abs().sum()) == 0.0
        good = table.clone()
        good[0, 1] = lost
        g = _gathered(p._t, good)
        assert torch.equal(g[:, 1:, :, :S0], c._t[:, 1:, :, :S0])
        assert torch.equal(g[:, 0, :, :BS], c._t[:, 0, :, :BS])


# ----------------------------------------------------------------------------- CPU: the runner
_BS = 4


def _blocks_in_use(lens, steps_done):
    """Blocks a paged runner holds: the prompt's, plus one for every block an append started."""
    total = 0
    for n in lens:
        last = n + steps_done - 1                 # the last position written so far
        total += max(-(-n // _BS), last // _BS + 1 if steps_done else 0)
    return total


def _runners(kind, num_blocks=None, device='cpu', dtype=torch.float32, use_graph=True, BS=_BS, **size):
    m, seqs, refs, xp, cos, sin = _case(device, dtype, **size)
    kw = {}
    if kind != 'float':
        kw = dict(kv_cache_dtype='int8',
                  cache_scales=_static_scales(m, device=device) if kind == 'int8_static' else None)
    dp = FusedMultiTransformerDecoder(m, len(LENS), MAXLEN, use_graph=use_graph, block_size=BS,
                                      num_blocks=num_blocks, **kw)
    dc = FusedMultiTransformerDecoder(m, len(LENS), MAXLEN, use_graph=use_graph, **kw)
    for d in (dp, dc):
        d.set_rotary(cos, sin, 1)
    return dp, dc, seqs, refs, xp


@pytest.mark.parametrize('kind', ['float', 'int8_static', 'int8_dynamic'])
def test_paged_runner_matches_the_contiguous_runner_cpu(kind):
    B, MB = len(LENS), MAXLEN // _BS
    need = _blocks_in_use(LENS, STEPS)
    assert _blocks_in_use(LENS, 0) == 5 and need == 7 < B * MB    # 2->5, 5->8 and 7->10 cross boundaries
    for nb in (None, need):                       # the default pool, and one just large enough
        dp, dc, seqs, refs, xp = _runners(kind, nb)
        NB = B * MB if nb is None else nb
        assert all(tuple(c.shape) == (2, NB, 2, _BS, 8) for c in dp.caches)
        assert tuple(dp.tables.shape) == (B, MB) and dp.tables.dtype == torch.int32
        assert dp.free_blocks == NB and int((dp.tables != -1).sum()) == 0
        _close(dp.prefill(paddle.Tensor(xp), seq_lens=list(LENS))._t,
               dc.prefill(paddle.Tensor(xp), seq_lens=list(LENS))._t, 2e-5)
        assert dp.free_blocks == NB - _blocks_in_use(LENS, 0)
        for i in range(STEPS):
            tok = paddle.Tensor(_tok(seqs, i))
            a, b = dp.step(tok)._t, dc.step(tok)._t
            _close(a, b, 2e-5)
            if kind == 'float':
                for s, n in enumerate(LENS):
                    _close(a[s, 0], refs[s][n + i], 2e-5)
            assert dp.free_blocks == NB - _blocks_in_use(LENS, i + 1), i
        assert dp.lens.tolist() == dc.lens.tolist() == [n + STEPS for n in LENS]
        used = dp.tables[dp.tables >= 0].tolist()
        assert len(used) == need == len(set(used)) and dp._graph is None
        for p, c in zip(dp.caches, dc.caches):    # the same rows, wherever they live
            g = _gathered(p, dp.tables.clamp(min=0))
            for s, n in enumerate(LENS):
                assert torch.equal(g[:, s, :, :n + STEPS], c[:, s, :, :n + STEPS])
        if kind == 'int8_dynamic':
            for a, b in zip(dp.kv_scales, dc.kv_scales):
                assert torch.equal(a, b)


@pytest.mark.parametrize('kind', ['float', 'int8_static'])
def test_paged_runner_exhaustion_changes_nothing(kind):
    need = _blocks_in_use(LENS, STEPS)
    dp, _, seqs, _, xp = _runners(kind, need - 1)
    dp.prefill(paddle.Tensor(xp), seq_lens=list(LENS))
    for i in range(STEPS - 1):
        dp.step(paddle.Tensor(_tok(seqs, i)))
    assert dp.free_blocks == 0
    state = (dp.lens.clone(), dp.tables.clone(), list(dp._pos), [c.clone() for c in dp.caches])
    with pytest.raises(RuntimeError, match='free'):
        dp.step(paddle.Tensor(_tok(seqs, STEPS - 1)))
    assert torch.equal(dp.lens, state[0]) and torch.equal(dp.tables, state[1]) and dp._pos == state[2]
    assert all(torch.equal(a, b) for a, b in zip(dp.caches, state[3]))
    dp.release(1)                                 # room again: the step goes through
    dp.step(paddle.Tensor(_tok(seqs, STEPS - 1)))
    with pytest.raises(RuntimeError):             # prompts that do not fit raise before anything changes
        FusedMultiTransformerDecoder(_case()[0], len(LENS), MAXLEN, block_size=_BS, num_blocks=4).prefill(
            paddle.Tensor(xp), seq_lens=list(LENS))


def test_paged_runner_uniform_prefill_cpu():
    m, _, _, _, cos, sin = _case()
    B, S0 = 2, 5
    x = torch.randn(B, S0 + STEPS, m.embed_dim, generator=torch.Generator().manual_seed(3))
    dp = FusedMultiTransformerDecoder(m, B, MAXLEN, block_size=_BS)
    dc = FusedMultiTransformerDecoder(m, B, MAXLEN)
    for d in (dp, dc):
        d.set_rotary(cos, sin, 1)
    _close(dp.prefill(paddle.Tensor(x[:, :S0]))._t, dc.prefill(paddle.Tensor(x[:, :S0]))._t, 2e-5)
    assert dp.free_blocks == B * (MAXLEN // _BS) - B * 2 and dp.ragged
    for t in range(S0, S0 + STEPS):
        _close(dp.step(paddle.Tensor(x[:, t:t + 1]))._t, dc.step(paddle.Tensor(x[:, t:t + 1]))._t, 2e-5)
    assert dp.lens.tolist() == [S0 + STEPS] * B


class _Spy:
    """Records what ``mmha_decode`` returned, layer by layer."""

    def __init__(self):
        self.orig, self.outs = K.mmha_decode, []

    def __enter__(self):
        def spy(*a, **kw):
            self.outs.append(self.orig(*a, **kw))
            return self.outs[-1]
        K.mmha_decode = spy
        return self

    def __exit__(self, *exc):
        K.mmha_decode = self.orig


def _alone(m, x, cos, sin, device='cpu'):
    """A sequence [S, E] generated alone: the causal context phase over all its tokens."""
    S = x.shape[0]
    with torch.no_grad():
        return m(paddle.Tensor(x[None]), attn_mask=paddle.Tensor(_causal(S, 1).to(x.device, x.dtype)),
                 rotary_embs=_rot(cos, sin, torch.arange(S)[None], device), rotary_emb_dims=1)._t[0]


def _continuous_batching(kind, device='cpu', dtype=torch.float32, tol=2e-5, BS=_BS, maxlen=MAXLEN,
                         lens=LENS, **size):
    """prefill, two steps, release(0), a step, admit(0, new prompt), three steps. Slots 1 and 2
    against a runner in which nothing was released; the admitted sequence against itself alone
    (float pools) or against the same admission into a fresh contiguous-precision twin."""
    m = _case(device, dtype, **size)[0]
    D = m.head_dim
    cos, sin = _tables(D, maxlen)
    B, S0, SN, after = len(lens), max(lens), 3, 3
    g = torch.Generator().manual_seed(21)
    xp = torch.randn(B, S0, m.embed_dim, generator=g).to(device, dtype)
    toks = torch.randn(3 + after, B, 1, m.embed_dim, generator=g).to(device, dtype)
    new = torch.randn(SN + after, m.embed_dim, generator=g).to(device, dtype)
    kw = {}
    if kind != 'float':
        kw = dict(kv_cache_dtype='int8', cache_scales=None if kind == 'int8_dynamic' else
                  [tuple(s.to(device) for s in _scales(B, m.kv_num_heads, False, base=(5.0 + i, 4.0 + i)))
                   for i in range(len(m.qkv_weights))])
    dp = FusedMultiTransformerDecoder(m, B, maxlen, block_size=BS, **kw)
    dn = FusedMultiTransformerDecoder(m, B, maxlen, block_size=BS, **kw)      # nothing released
    for d in (dp, dn):
        d.set_rotary(cos, sin, 1)
        d.prefill(paddle.Tensor(xp), seq_lens=list(lens))
    NB = dp.free_blocks + sum(-(-n // BS) for n in lens)
    for i in range(2):
        _close(dp.step(paddle.Tensor(toks[i]))._t, dn.step(paddle.Tensor(toks[i]))._t, tol)
    graph = dp._graph
    held, free = len(dp._blocks[0]), dp.free_blocks
    assert held > 0
    dp.release(0)
    assert dp.free_blocks == free + held and dp.tables[0].tolist() == [-1] * dp.MB
    assert int(dp.lens[0]) == dp.MB * BS
    freed = sorted(dp._free[-held:])
    before = [c[:, freed].clone() for c in dp.caches]
    with _Spy() as spy:
        o = dp.step(paddle.Tensor(toks[2]))._t
    if device == 'cpu':                           # (a captured graph does not call the wrapper again)
        assert len(spy.outs) == len(dp.caches)
        for a in spy.outs:                        # the released slot: zeros out of the kernel
            assert float(a[0].float().abs().sum()) == 0.0 and float(a[1].float().abs().sum()) > 0
    for c, b in zip(dp.caches, before):           # and nothing written into the blocks it gave back
        assert torch.equal(c[:, freed], b)
    _close(o[1:], dn.step(paddle.Tensor(toks[2]))._t[1:], tol)
    free = dp.free_blocks
    out = dp.admit(0, paddle.Tensor(new[None, :SN]))._t
    assert tuple(out.shape) == (1, SN, m.embed_dim)
    assert dp.free_blocks == free - (-(-SN // BS)) and int(dp.lens[0]) == SN
    assert dp.lens[1:].tolist() == dn.lens[1:].tolist()
    ref = _alone(m, new, cos, sin, device)
    outs = [out[0]]
    for i in range(after):
        x = toks[3 + i].clone()
        x[0, 0] = new[SN + i]
        o = dp.step(paddle.Tensor(x))._t
        _close(o[1:], dn.step(paddle.Tensor(toks[3 + i]))._t[1:], tol)
        outs.append(o[0])
    got = torch.cat(outs)
    assert dp._graph is graph                     # release / admit keep the captured graph
    assert int(dp.lens[0]) == SN + after
    return dp, got, ref


def test_continuous_batching_cpu():
    dp, got, ref = _continuous_batching('float')
    _close(got, ref, 2e-5)                        # the admitted sequence, as generated alone
    with pytest.raises(RuntimeError):             # slot 1 still holds a sequence
        dp.admit(1, paddle.Tensor(torch.randn(1, 2, 32)))
    with pytest.raises(ValueError):
        dp.admit(0, paddle.Tensor(torch.randn(2, 2, 32)))


@pytest.mark.parametrize('kind', ['int8_static', 'int8_dynamic'])
def test_continuous_batching_int8_cpu(kind):
    dp, got, ref = _continuous_batching(kind)
    # against the unquantised sequence alone the 8-bit cache costs a few percent; the exact
    # checks are those of slots 1 and 2 above. What admit must get right is slot 0's scales:
    m = dp.model
    if kind == 'int8_dynamic':
        for s in dp.kv_scales:
            assert bool((s[:, 0] != 1.0).any()) and bool(torch.isfinite(s).all())
            torch.testing.assert_close(s[2:], 1.0 / s[:2])
    assert float((got - ref).abs().max()) / float(ref.abs().max()) < 0.1


# ----------------------------------------------------------------------------- GPU: the kernel
#        D   BS   MB  R  B  lens         time_step  mask
_PA = (64, 16, 3, 2, 3, (0, 17, 47), 47, False)     # one split; the last slot of the last block
_PB = (128, 64, 11, 4, 2, (5, 650), 650, False)     # 11 splits of 60 keys: split edges inside blocks
_PC = (64, 16, 44, 8, 2, (5, 650), 'dev', False)    # device time_step: the splits cover MB*BS
_PD = (256, 128, 6, 2, 2, (5, 650), 650, True)      # with a mask
_KVH = 2


def _paged_kernel_vs_ref(case, dtype, rot_dims=0, dyn=None, r1=False, device_table=False):
    """One step of the PAGED HIP kernel and of ``'ref'`` on clones of the same pool."""
    D, BS, MB, Rr, B, lens, t, use_mask = case
    KVH = _KVH
    H = KVH * Rr
    u8 = dyn is not None
    qkv, cache = _problem(B, H, KVH, MB * BS, D, seed=D + MB + H, dtype=dtype, u8=u8)
    pool, table = _paged(cache, BS, spare=3, seed=D + BS)
    qkv, pool = qkv.cuda(), pool.cuda()
    if r1:
        qkv = qkv.reshape(B, 3, H, D)
    kw, pub = {}, {}
    if lens is not None:
        kw['seq_lens'] = torch.tensor(lens, dtype=torch.int32).cuda()
    if t == 'dev':
        t = torch.tensor([max(lens)], dtype=torch.int32).cuda()
    mask = _mask(B, max(lens) + 1 + 3, lens).cuda() if use_mask else None
    if rot_dims:
        ang = torch.rand(B, D, generator=torch.Generator().manual_seed(D)) * (2 * np.pi)
        kw.update(rotary=torch.stack([ang.cos(), ang.sin()]).cuda(), rotary_dims=rot_dims)
    if u8:
        kq, vq = (s.cuda() for s in _scales(B, KVH, dyn, base=(3.6, 3.9)))
        pub = dict(cache_k_quant_scales=kq, cache_v_quant_scales=vq)
    before, p_ref = pool.clone(), pool.clone()
    rkw = dict(kw, quant=K._kv_quant_args(B, p_ref, kq, vq, device=qkv.device)) if u8 else kw
    ref = R.get_kernel('mmha_decode_paged', 'ref')(qkv, p_ref, t, mask, table, **rkw)
    R.reset_stats()
    out = K.mmha_decode(qkv, pool, t, mask, block_tables=table.int().cuda() if device_table else table,
                        **kw, **pub)
    st = R.stats()
    assert st.get(('mmha_decode_paged', 'hip'), 0) == 1 and not [k for k in st if k[1] == 'ref'], st
    assert out.shape == (B, H, D) and bool(torch.isfinite(out.float()).all())
    tol = _TOLS[dtype]
    torch.testing.assert_close(out.float(), ref.float(), rtol=tol, atol=tol)
    assert _spares_untouched(pool, before, table)
    assert not _same_bits(pool, before)
    return out, ref, pool, p_ref, before, table


_CASES = [(n, c, dt) for n, c in (('a', _PA), ('b', _PB), ('c', _PC), ('d', _PD))
          for dt in [torch.bfloat16, torch.float32] + ([torch.float16] if n == 'b' else [])]
_IDS = [f'{n}-{str(d)[6:]}' for n, _, d in _CASES]


@pytest.mark.gpu
@pytest.mark.parametrize('name,case,dtype', _CASES, ids=_IDS)
def test_paged_hip_kernel_gpu(name, case, dtype):
    out, ref, pool, p_ref, before, table = _paged_kernel_vs_ref(case, dtype, device_table=name == 'c')
    assert _same_bits(pool, p_ref)                # K/V appended at each t_b, through the table


@pytest.mark.gpu
@pytest.mark.parametrize('BS', [16, 64])
@pytest.mark.parametrize('D', [64, 128, 256])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_paged_r1_sweep_gpu(D, BS, dtype):
    # five splits of 52 keys, no multiple of the keys an iteration takes nor of a block
    case = (D, BS, 320 // BS, 1, 2, (5, 257), 257, False)
    out, ref, pool, p_ref, before, table = _paged_kernel_vs_ref(case, dtype, r1=True)
    assert _same_bits(pool, p_ref)


@pytest.mark.gpu
@pytest.mark.parametrize('name,case', [('a', _PA), ('b', _PB)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_paged_rotary_in_kernel_gpu(name, case, dtype):
    out, ref, pool, p_ref, before, table = _paged_kernel_vs_ref(case, dtype, rot_dims=1)
    assert R.stats().get(('mmha_decode_rotary', 'hip'), 0) == 1
    torch.testing.assert_close(pool[:, table], p_ref[:, table])   # a rotated row may differ by one rounding
    D, BS = case[0], case[1]
    for b, n in enumerate(case[5]):               # only the rows at each t_b changed
        e = int(table[b, n // BS])
        assert not _same_bits(pool[0, e, :, n % BS], before[0, e, :, n % BS])
        pool[:, e, :, n % BS] = before[:, e, :, n % BS]
    assert _same_bits(pool, before)


@pytest.mark.gpu
@pytest.mark.parametrize('dyn', [False, True], ids=['per_head', 'per_seq'])
@pytest.mark.parametrize('name,case', [('a', _PA), ('b', _PB), ('c', _PC)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_paged_q8_hip_kernel_gpu(name, case, dtype, dyn):
    out, ref, pool, p_ref, before, table = _paged_kernel_vs_ref(case, dtype, dyn=dyn)
    assert R.stats().get(('mmha_decode_q8', 'hip'), 0) == 1
    assert pool.dtype == torch.uint8 and torch.equal(pool, p_ref)  # the same bytes as 'ref' wrote


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_paged_block_boundaries_gpu(dtype):
    # t_b = 0, the last row of a block, the first row of the next one, and of the one after:
    # rows at and past t_b hold NaN, so a read of a row that nothing wrote shows in the output
    B, H, KVH, D, BS, MB = 4, 4, 2, 128, 16, 3
    lens = (0, BS - 1, BS, 2 * BS)
    qkv, cache = _problem(B, H, KVH, MB * BS, D, seed=9, dtype=dtype)
    for b, n in enumerate(lens):
        cache[:, b, :, n:] = float('nan')
    pool, table = _paged(cache, BS, seed=9)
    qkv, pool = qkv.cuda(), pool.cuda()
    before, p_ref = pool.clone(), pool.clone()
    sl = torch.tensor(lens, dtype=torch.int32).cuda()
    ref = R.get_kernel('mmha_decode_paged', 'ref')(qkv, p_ref, 2 * BS, None, table, seq_lens=sl)
    out = K.mmha_decode(qkv, pool, 2 * BS, seq_lens=sl, block_tables=table)
    assert bool(torch.isfinite(out.float()).all())
    tol = _TOLS[dtype]
    torch.testing.assert_close(out.float(), ref.float(), rtol=tol, atol=tol)
    assert torch.equal(out[0], qkv[0, H + KVH:].repeat_interleave(H // KVH, 0))
    assert _same_bits(pool, p_ref)
    for b, n in enumerate(lens):
        e = int(table[b, n // BS])
        assert torch.equal(pool[0, e, :, n % BS], qkv[b, H:H + KVH])
        assert torch.equal(pool[1, e, :, n % BS], qkv[b, H + KVH:])
        pool[:, e, :, n % BS] = before[:, e, :, n % BS]
    assert _same_bits(pool, before)


@pytest.mark.gpu
@pytest.mark.parametrize('u8', [False, True], ids=['float', 'uint8'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_paged_untrusted_table_gpu(dtype, u8):
    # the kernel is specified to handle these entries: it never makes an address of one. The
    # table is a device tensor, which is not synced and so not validated on the host
    B, H, KVH, D, BS, MB = 3, 4, 2, 64, 16, 4
    lens = (20, 60, 40)
    qkv, cache, pool, table, good, mask, guarded = _untrusted(B, H, KVH, D, BS, MB, lens, 6, dtype, u8)
    qkv, pool = qkv.cuda(), pool.cuda()
    pub, rkw = {}, {}
    if u8:
        kq, vq = (s.cuda() for s in _scales(B, KVH, True, base=(3.6, 3.9)))
        pub = dict(cache_k_quant_scales=kq, cache_v_quant_scales=vq)
        rkw = dict(quant=K._kv_quant_args(B, pool, kq, vq, device=qkv.device))
    before, p_ref = pool.clone(), pool.clone()
    sl = torch.tensor(lens, dtype=torch.int32).cuda()
    ref = R.get_kernel('mmha_decode_paged', 'ref')(qkv, p_ref, 60, None, table, seq_lens=sl, **rkw)
    R.reset_stats()
    out = K.mmha_decode(qkv, pool, 60, seq_lens=sl, block_tables=table.int().cuda(), **pub)
    assert R.stats().get(('mmha_decode_paged', 'hip'), 0) == 1
    assert bool(torch.isfinite(out.float()).all())
    assert float(out[2].float().abs().sum()) == 0.0 and float(out[1].float().abs().sum()) > 0
    tol = _TOLS[dtype]
    torch.testing.assert_close(out.float(), ref.float(), rtol=tol, atol=tol)
    assert _same_bits(pool, p_ref)
    assert _same_bits(pool[:, good[2]], before[:, good[2]])       # sequence 2 wrote nothing
    for b in (0, 1):                              # the others their own row and nothing else
        e, n = int(good[b, lens[b] // BS]), lens[b] % BS
        assert not _same_bits(pool[:, e, :, n], before[:, e, :, n])
        pool[:, e, :, n] = before[:, e, :, n]
    assert _same_bits(pool, before)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32])
def test_identity_table_is_the_contiguous_cache_gpu(dtype):
    B, H, KVH, D, L = 3, 8, 2, 128, 64
    qkv, cache = _problem(B, H, KVH, L, D, seed=4, dtype=dtype)
    qkv, cache = qkv.cuda(), cache.cuda()
    sl = torch.tensor([0, 33, 63], dtype=torch.int32).cuda()
    c1, c2 = cache.clone(), cache.clone()
    a = K.mmha_decode(qkv, c1, 63, seq_lens=sl)
    b = K.mmha_decode(qkv, c2, 63, seq_lens=sl, block_tables=torch.arange(B, dtype=torch.int32)[:, None])
    print(f'identity table {dtype}: outputs bit-equal {torch.equal(a, b)}, caches bit-equal {torch.equal(c1, c2)}')
    tol = _TOLS[dtype]
    torch.testing.assert_close(b.float(), a.float(), rtol=tol, atol=tol)
    assert torch.equal(c1, c2) and not torch.equal(c1, cache)


@pytest.mark.gpu
def test_paged_dispatch_counts_and_refusals_gpu():
    B, H, KVH, D, BS, MB = 2, 4, 2, 64, 16, 2
    qkv, cache = _problem(B, H, KVH, MB * BS, D, seed=1)
    pool, table = _paged(torch.zeros_like(cache), BS)
    qkv, pool = qkv.cuda(), pool.cuda()
    R.reset_stats()
    for n in (1, 2):
        K.mmha_decode(qkv, pool, 3 + n, block_tables=table)
        st = R.stats()
        assert st.get(('mmha_decode_paged', 'hip'), 0) == n == st.get(('mmha_decode_gqa', 'hip'), 0), st
    assert not [k for k in st if k[1] == 'ref'] and ('mmha_decode', 'hip') not in st, st
    before = pool.clone()
    pool24, table24 = _paged(torch.zeros(2, B, KVH, 48, D), 24)
    with pytest.raises(ValueError, match='24'):   # not a power of two
        K.mmha_decode(qkv, pool24.cuda(), 3, block_tables=table24)
    pool8, table8 = _paged(torch.zeros(2, B, KVH, 32, D), 8)
    with pytest.raises(ValueError):               # a power of two below 16
        K.mmha_decode(qkv, pool8.cuda(), 3, block_tables=table8)
    with pytest.raises(ValueError, match='2, 4, 8'):
        K.mmha_decode(torch.randn(B, 6 + 2 * KVH, D).cuda(), pool, 3, block_tables=table)
    assert _same_bits(pool, before)
    assert not [k for k in R.stats() if k[1] == 'ref'], R.stats()


# ----------------------------------------------------------------------------- GPU: end to end
_GBS, _GMAX, _GLENS, _GSTEPS = 16, 48, (13, 5, 16), 4     # 13->17 and 16->20 cross a block boundary


@functools.lru_cache(None)
def _gpu_case():
    """The bf16 grouped-query model at head dim 128, three sequences and each one alone."""
    m = _case('cuda', torch.bfloat16, **_BIG)[0]
    cos, sin = _tables(m.head_dim, _GMAX)
    g = torch.Generator().manual_seed(17)
    seqs = [torch.randn(n + _GSTEPS, m.embed_dim, generator=g).to('cuda', torch.bfloat16) for n in _GLENS]
    refs = [_alone(m, x, cos, sin, 'cuda') for x in seqs]
    S0 = max(_GLENS)
    xp = torch.randn(len(_GLENS), S0, m.embed_dim, generator=g).to('cuda', torch.bfloat16)
    for b, n in enumerate(_GLENS):
        xp[b, :n] = seqs[b][:n]
    return m, seqs, refs, xp, cos, sin


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['float', 'int8_static', 'int8_dynamic'])
def test_paged_runner_hip_graph_gpu(kind):
    paddle.set_device('gpu')
    m, seqs, refs, xp, cos, sin = _gpu_case()
    B = len(_GLENS)
    kw = {}
    if kind != 'float':
        kw = dict(kv_cache_dtype='int8', cache_scales=None if kind == 'int8_dynamic' else
                  [tuple(s.cuda() for s in _scales(B, m.kv_num_heads, False, base=(5.0 + i, 4.0 + i)))
                   for i in range(len(m.qkv_weights))])
    R.reset_stats()
    dp = FusedMultiTransformerDecoder(m, B, _GMAX, block_size=_GBS, num_blocks=7, **kw)
    dc = FusedMultiTransformerDecoder(m, B, _GMAX, **kw)
    for d in (dp, dc):
        d.set_rotary(cos, sin, 1)
    a = dp.prefill(paddle.Tensor(xp), seq_lens=list(_GLENS))._t
    b = dc.prefill(paddle.Tensor(xp), seq_lens=list(_GLENS))._t
    assert torch.equal(a, b) and dp.free_blocks == 7 - 3
    graph, worst = None, 0.0
    for i in range(_GSTEPS):
        tok = paddle.Tensor(torch.stack([seqs[s][n + i] for s, n in enumerate(_GLENS)])[:, None])
        a, b = dp.step(tok)._t, dc.step(tok)._t
        _close(a, b, 2e-2)                        # the contiguous runner with the same cache dtype
        for s, n in enumerate(_GLENS):
            ref = refs[s][n + i].float()
            worst = max(worst, float((a[s, 0].float() - ref).abs().max()) / float(ref.abs().max()))
            if kind == 'float':
                _close(a[s, 0], refs[s][n + i], 2e-2)
        graph = graph or dp._graph
        assert dp._graph is graph and graph is not None           # one graph, boundary steps included
    print(f'paged runner {kind}: worst deviation from each sequence alone {worst:.3e}')
    assert dp.free_blocks == 7 - 5 and dp.lens.tolist() == [n + _GSTEPS for n in _GLENS]
    st = R.stats()
    assert st.get(('mmha_decode_paged', 'hip'), 0) > 0 and st.get(('mmha_decode_rotary', 'hip'), 0) > 0, st
    assert not [k for k in st if k[0].startswith('mmha_decode') and k[1] == 'ref'], st
    for p, c in zip(dp.caches, dc.caches):
        g = _gathered(p, dp.tables.clamp(min=0))
        for s, n in enumerate(_GLENS):
            assert torch.equal(g[:, s, :, :n + _GSTEPS], c[:, s, :, :n + _GSTEPS])


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['float', 'int8_dynamic'])
def test_continuous_batching_hip_graph_gpu(kind):
    paddle.set_device('gpu')
    _gpu_case()
    dp, got, ref = _continuous_batching(kind, 'cuda', torch.bfloat16, 2e-2, BS=_GBS, maxlen=_GMAX,
                                        lens=_GLENS, **_BIG)
    assert dp._graph is not None
    dev = float((got.float() - ref.float()).abs().max()) / float(ref.float().abs().max())
    print(f'admitted sequence {kind}: deviation from itself alone {dev:.3e}')
    if kind == 'float':
        _close(got, ref, 2e-2)
    else:
        assert dev < 0.1
