"""Temperature / top-k / top-p token sampling: ``ops.fused.sample_top_p`` ('ref' and the HIP kernel),
``paddle.tensor.top_p_sampling`` and ``paddle.incubate.nn.TokenSampler``.

The float64 oracle below is independent of 'ref': ``lexsort`` on (-x, index), float64 cumulative
sums, the index-order draw. It also says which rows are *robust*: a row is left out of exact id
comparisons when a sorted cumulative ``c_j / Z`` (j < n_k, top_p < 1) lies within DELTA of top_p,
or a kept-set CDF edge lies within DELTA of u, because there an fp32 sum may legitimately land on
the other side. DELTA = 1e-4: the fp32 sequential cumulative sum of a 50304-entry softmax differs
from float64 by at most 5.3e-6 (measured), DELTA is about 20 times that. At most MAX_LEFT_OUT of 64
rows may be left out per case; the inputs are peaked (``randn * scale``), so few are.

The HIP kernel computes its weights in fp32 from the same inputs as 'ref' and sums them as
2^-40 fixed point, so ``probs`` of 16-bit inputs are held to the same 1e-5 as fp32 in practice;
the bound asserted for them is the 2e-3 the feature was specified with.
"""
import functools

import numpy as np
import pytest
import torch

import paddle_ray_amd as paddle
from paddle_ray_amd.incubate.nn import FusedMultiTransformerDecoder, TokenSampler
from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

DELTA = 1e-4
MAX_LEFT_OUT = 8
FLT_MAX = float(np.finfo(np.float32).max)

# V, scale, temperature, top_k, top_p
CASES = [(7, 1, 1.0, 0, 0.8), (1000, 4, 1.0, 0, 0.9), (1000, 4, 0.7, 0, 0.95), (1025, 4, 1.0, 8, 0.99),
         (4099, 3, 1.0, 50, 1.0), (50304, 4, 1.0, 64, 1.0), (50304, 8, 1.3, 40, 0.95), (131075, 8, 1.0, 0, 0.9)]
_IDS = [f'V{c[0]}-s{c[1]}-t{c[2]}-k{c[3]}-p{c[4]}' for c in CASES]
_DT = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float16': torch.float16}


def _oracle(x, T, k, p, u, probs=False):
    """(ids, probs, robust) of the definition in float64. x [R, V] float64 (the stored values),
    T / k / p scalars or [R], u [R]."""
    Rn, V = x.shape
    T, k, p = (np.broadcast_to(np.asarray(a, dtype=t), (Rn,)) for a, t in ((T, np.float64), (k, np.int64),
                                                                          (p, np.float64)))
    ids, pr, robust = np.zeros(Rn, np.int64), np.zeros(Rn), np.ones(Rn, bool)
    idx = np.arange(V)
    for r in range(Rn):
        xr = np.where(np.isnan(x[r]), -np.inf, x[r]) + 0.0
        order = np.lexsort((idx, -xr))
        mx = xr[order[0]]
        ids[r] = order[0]
        if mx == -np.inf or (probs and not mx > 0):
            continue
        cold = (not probs) and not T[r] > 0
        if cold:
            pr[r] = 1.0
            continue
        with np.errstate(invalid='ignore', over='ignore'):
            w = np.maximum(xr, 0) / mx if probs else np.exp((xr - mx) / T[r])
        w = np.where(xr == mx, 1.0, w)
        ws = w[order]
        c = np.cumsum(ws)
        Z = c[-1]
        if k[r] == 1 or not p[r] > 0:
            pr[r] = 1.0 / Z
            continue
        nk = k[r] if 1 <= k[r] < V else V
        n_p = V if p[r] >= 1 else min(V, int(np.searchsorted(c, p[r] * Z, side='left')) + 1)
        n = max(1, min(n_p, nk))
        if p[r] < 1 and np.any(np.abs(c[:nk] / Z - p[r]) < DELTA):
            robust[r] = False
        kept = np.sort(order[:n])
        ck = np.cumsum(w[kept])
        M = ck[-1]
        hit = np.nonzero(ck > u[r] * M)[0]
        ids[r] = kept[hit[0]] if len(hit) else kept[-1]
        # the last edge is 1: a u that close to it draws the last kept index either way
        if np.any(np.abs(ck[:-1] / M - u[r]) < DELTA):
            robust[r] = False
        pr[r] = w[ids[r]] / Z
    return ids, pr, robust


@functools.lru_cache(None)
def _table(ci, dtype_name):
    """One case of the table in one dtype, computed once: inputs, the oracle and 'ref' on the CPU."""
    V, scale, T, k, p = CASES[ci]
    g = torch.Generator().manual_seed(1000 + ci)
    x = (torch.randn(64, V, generator=g) * scale).to(_DT[dtype_name])
    u = torch.rand(64, generator=g)
    oid, opr, robust = _oracle(x.double().numpy(), T, k, p, u.double().numpy())
    rid, rpr = K.sample_top_p(x, T, k, p, uniform=u)
    return dict(x=x, u=u, oid=torch.from_numpy(oid), opr=torch.from_numpy(opr), robust=torch.from_numpy(robust),
                rid=rid, rpr=rpr, par=(T, k, p))


def _check_left_out(robust, what):
    left = int((~robust).sum())
    print(f"{what}: {left} of {robust.numel()} rows left out")
    assert left <= MAX_LEFT_OUT * max(1, robust.numel() // 64), (what, left)


# ------------------------------------------------------------------------------------- CPU
_CPU_TABLE = [(ci, 'float32') for ci in range(len(CASES))] + [(1, 'bfloat16'), (2, 'bfloat16'), (6, 'bfloat16')]


@pytest.mark.parametrize('ci,dtype', _CPU_TABLE, ids=[f'{_IDS[c]}-{d}' for c, d in _CPU_TABLE])
def test_ref_equals_oracle(ci, dtype):
    d = _table(ci, dtype)
    _check_left_out(d['robust'], _IDS[ci])
    ok = d['robust']
    assert d['rid'].dtype == torch.int64 and d['rpr'].dtype == torch.float32
    assert torch.equal(d['rid'][ok], d['oid'][ok])
    err = float((d['rpr'].double() - d['opr'])[ok].abs().max())
    print(f"probs: max error {err:.3g}")
    assert err < 1e-5


def test_greedy_forms_equal_first_argmax():
    x = torch.randn(6, 33, generator=torch.Generator().manual_seed(2))
    x[:, 5] = x[:, 20] = x[:, 31] = 9.0                     # repeated maxima: index 5 wins
    x[3, 2] = 9.0                                           # row 3: index 2
    want = torch.tensor([5, 5, 5, 2, 5, 5])
    u = torch.full((6,), 0.99)
    for kw in (dict(temperature=0.0), dict(top_k=1), dict(top_p=0.0), dict(temperature=-1.0)):
        ids, pr = K.sample_top_p(x, uniform=u, **kw)
        assert torch.equal(ids, want), kw
        oid, opr, _ = _oracle(x.double().numpy(), kw.get('temperature', 1.0), kw.get('top_k', 0),
                              kw.get('top_p', 1.0), u.numpy())
        assert torch.equal(ids, torch.from_numpy(oid))
        assert float((pr.double() - torch.from_numpy(opr)).abs().max()) < 1e-6
    ids, _ = K.sample_top_p(x.to(torch.bfloat16), top_k=1)
    assert torch.equal(ids, want)


def _all_equal_case():
    """33 rows of one all-equal V = 64 row, top_p = 0.5 + 1/256: p * Z = 32.25, so 33 entries stay,
    and of the 64-way tie they are indices 0..32. u = (j + 0.5) / 33 draws index j."""
    x = torch.full((34, 64), 1.5)
    u = torch.cat([(torch.arange(33) + 0.5) / 33, torch.tensor([1 - 2.0 ** -24])])
    return x, u, torch.cat([torch.arange(33), torch.tensor([32])])


def _five_value_case():
    """bf16 rows built from 5 distinct values: every limit cuts a large tie group."""
    g = torch.Generator().manual_seed(5)
    levels = torch.tensor([-2.0, 0.5, 1.0, 3.0, 3.5])
    x = levels[torch.randint(0, 5, (24, 257), generator=g)].to(torch.bfloat16)
    u = torch.rand(24, generator=g)
    T = [1.0, 0.5, 2.0] * 8
    k = [0, 0, 10, 10, 100, 100, 200, 3] * 3
    p = [0.9, 0.5, 1.0, 0.3] * 6
    oid, opr, robust = _oracle(x.double().numpy(), T, k, p, u.double().numpy())
    return x, u, (T, k, p), torch.from_numpy(oid), torch.from_numpy(robust)


def _masked_case():
    """-inf and NaN entries (never returned), a row with one finite entry, a row with none."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(40, 131, generator=g)
    dead = torch.rand(40, 131, generator=g) < 0.7
    x[dead] = float('-inf')
    x[dead & (torch.rand(40, 131, generator=g) < 0.5)] = float('nan')
    x[:, 7] = 0.25                                          # every row keeps at least one entry
    dead[:, 7] = False
    x[38] = float('nan')
    x[38, :60] = float('-inf')
    x[38, 77] = -3.0                                        # one finite entry
    x[39] = float('nan')
    x[39, ::2] = float('-inf')                              # none
    u = torch.rand(40, generator=g)
    return x, dead, u


def _check_ties_and_masks(device):
    x, u, want = _all_equal_case()
    ids, pr = K.sample_top_p(x.to(device), top_p=0.5 + 1 / 256, uniform=u.to(device))
    assert torch.equal(ids.cpu(), want)
    assert float((pr.cpu() - 1 / 64).abs().max()) < 1e-7
    x, u, (T, k, p), oid, robust = _five_value_case()
    ids, _ = K.sample_top_p(x.to(device), T, k, p, uniform=u.to(device))
    assert int(robust.sum()) >= 16
    assert torch.equal(ids.cpu()[robust], oid[robust])
    x, dead, u = _masked_case()
    for dt in (torch.float32, torch.float16):
        ids, pr = K.sample_top_p(x.to(device, dt), temperature=5.0, uniform=u.to(device))
        ids, pr = ids.cpu(), pr.cpu()
        assert not bool(dead[:38].gather(1, ids[:38, None]).any())
        assert int(ids[38]) == 77 and float(pr[38]) == 1.0
        assert int(ids[39]) == 0 and float(pr[39]) == 0.0
        assert bool(torch.isfinite(pr).all()) and int(ids.min()) >= 0 and int(ids.max()) < 131


def test_ties_and_masked_entries():
    _check_ties_and_masks('cpu')


def test_hash_uniform_reference():
    seed = 0x1234567890ABCDEF
    us = [K.sample_uniform_ref(seed, c, 4096) for c in (7, 8, 9)]
    for u in us:
        assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
        assert len(np.unique(u)) == 4096                     # all different across the rows
    assert np.array_equal(us[0], K.sample_uniform_ref(seed, 7, 4096))
    assert np.array_equal(us[0][:100], K.sample_uniform_ref(seed, 7, 100))          # a row's u ignores R
    hs = np.concatenate([K.sample_hash_ref(seed, c, 4096) for c in (7, 8, 9)])
    assert len(np.unique(hs)) == 3 * 4096                    # and across the counters
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert float(np.mean(us[a] == us[b])) < 0.01
    assert not np.array_equal(us[0], K.sample_uniform_ref(seed + (1 << 40), 7, 4096))
    assert not np.array_equal(us[0], K.sample_uniform_ref(seed, 7 + (1 << 32), 4096))
    assert abs(float(np.mean(np.concatenate(us))) - 0.5) < 0.01
    # the hash drives the op when no uniform is given: counter = offset + step
    x = torch.randn(50, 40, generator=torch.Generator().manual_seed(1))
    a, _ = K.sample_top_p(x, seed=seed, offset=3, step=torch.tensor([4]))
    b, _ = K.sample_top_p(x, uniform=torch.from_numpy(us[0][:50]))
    assert torch.equal(a, b)


# chi-square quantiles at 1 - 1e-6 by degrees of freedom (scipy.stats.chi2.ppf), used when scipy is
# not installed
_CHI2_Q = {1: 23.928, 2: 27.631, 3: 30.665, 4: 33.377, 5: 35.888, 6: 38.258, 7: 40.522, 8: 42.701, 9: 44.811,
           10: 46.863, 11: 48.866, 12: 50.825, 13: 52.747, 14: 54.635, 15: 56.493}


def test_distribution_chi_square():
    N, V, p = 8192, 16, 0.9
    logits = torch.randn(V, generator=torch.Generator().manual_seed(11))
    x = logits.expand(N, V).contiguous()
    ids, _ = K.sample_top_p(x, top_p=p, seed=2024, offset=5)
    xd = logits.double().numpy()
    order = np.lexsort((np.arange(V), -xd))
    w = np.exp(xd - xd.max())
    c = np.cumsum(w[order]) / w.sum()
    assert not np.any(np.abs(c - p) < DELTA)                # the kept set is not on a boundary
    n = int(np.searchsorted(c, p, side='left')) + 1
    kept = np.sort(order[:n])
    assert 8 <= n < V
    counts = np.bincount(ids.numpy(), minlength=V)
    assert counts.sum() == N and counts[np.setdiff1d(np.arange(V), kept)].sum() == 0
    expect = N * w[kept] / w[kept].sum()
    chi = float(((counts[kept] - expect) ** 2 / expect).sum())
    try:
        from scipy.stats import chi2
        q = float(chi2.ppf(1 - 1e-6, n - 1))
    except ImportError:
        q = _CHI2_Q[n - 1]
    print(f"chi-square {chi:.2f} with {n - 1} degrees of freedom, bound {q:.2f}")
    assert chi < q


def test_top_p_sampling_api():
    g = torch.Generator().manual_seed(3)
    probs = torch.softmax(torch.randn(5, 50, generator=g) * 2, -1)
    for dt in (torch.float32, torch.bfloat16):
        x = paddle.Tensor(probs.to(dt))
        for ps in (paddle.Tensor(torch.full((5,), 0.7)), paddle.Tensor(torch.full((5, 1), 0.7))):
            out, ids = paddle.tensor.top_p_sampling(x, ps, seed=9)
            assert tuple(out.shape) == (5, 1) and tuple(ids.shape) == (5, 1)
            assert out._t.dtype == dt and ids._t.dtype == torch.int64
            assert torch.equal(out._t, x._t.gather(1, ids._t))
        tiny, ids = paddle.tensor.top_p_sampling(x, paddle.Tensor(torch.full((5,), 1e-6)), seed=1)
        assert torch.equal(ids._t[:, 0], x._t.float().argmax(-1))
    x = paddle.Tensor(probs)
    ps = paddle.Tensor(torch.full((5,), 0.9))
    a = paddle.tensor.top_p_sampling(x, ps, seed=77)[1]._t
    assert torch.equal(a, paddle.tensor.top_p_sampling(x, ps, seed=77)[1]._t)
    draws = {tuple(paddle.tensor.top_p_sampling(x, ps, seed=s)[1]._t[:, 0].tolist()) for s in range(20)}
    assert len(draws) > 1
    paddle.seed(5)
    a = [paddle.tensor.top_p_sampling(x, ps)[1]._t for _ in range(2)]       # seed=None: host generator
    paddle.seed(5)
    b = [paddle.tensor.top_p_sampling(x, ps, seed=-1)[1]._t for _ in range(2)]
    assert all(torch.equal(i, j) for i, j in zip(a, b))
    with pytest.raises(NotImplementedError, match='threshold'):
        paddle.tensor.top_p_sampling(x, ps, threshold=paddle.Tensor(torch.full((5,), 0.1)))


def test_token_sampler():
    B, V = 6, 200
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, V, generator=g) * 2
    s = TokenSampler(B, temperature=1.0, top_k=0, top_p=0.95, seed=31, device='cpu')
    assert s.state() == (31, 0)
    s.set(2, temperature=0.0)
    s.set(4, top_k=3, top_p=1.0)
    assert s.temperature.tolist() == [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    assert s.top_k.tolist() == [0, 0, 0, 0, 3, 0]
    assert torch.allclose(s.top_p, torch.tensor([0.95, 0.95, 0.95, 0.95, 1.0, 0.95]))
    st0 = s.state()
    draws = [s(x) for _ in range(6)]
    assert s.state() == (31, 6) and draws[0].dtype == torch.int64 and tuple(draws[0].shape) == (B,)
    assert len({tuple(d.tolist()) for d in draws}) > 1
    top3 = set(x[4].topk(3).indices.tolist())
    for i, d in enumerate(draws):
        assert int(d[2]) == int(x[2].argmax()) and int(d[4]) in top3
        want, _ = K.sample_top_p(x, s.temperature, s.top_k, s.top_p, seed=31, offset=i)
        assert torch.equal(d, want)
    s.set_state(st0)
    again = [s(x) for _ in range(6)]
    assert all(torch.equal(a, b) for a, b in zip(draws, again))
    # [B, T, V]: every slot's T rows share its parameters; rows are numbered b * T + j
    T = 3
    x3 = torch.randn(B, T, V, generator=g) * 2
    s.set_state((31, 2))
    got = s(paddle.Tensor(x3))
    assert isinstance(got, paddle.Tensor) and tuple(got.shape) == (B, T)
    want, wpr = K.sample_top_p(x3.reshape(B * T, V), s.temperature.repeat_interleave(T),
                               s.top_k.repeat_interleave(T), s.top_p.repeat_interleave(T), seed=31, offset=2)
    assert torch.equal(got._t.reshape(-1), want) and torch.equal(s.last_probs.reshape(-1), wpr)
    with pytest.raises(ValueError, match='logits'):
        s(x[:3])
    with pytest.raises(ValueError, match='finite'):
        s.set(0, top_p=float('nan'))
    with pytest.raises(IndexError):
        s.set(B, top_k=2)


def test_host_validation():
    x = torch.randn(4, 10)
    with pytest.raises(ValueError, match='temperature has 3 values for 4 rows'):
        K.sample_top_p(x, temperature=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match='top_k has 5 values'):
        K.sample_top_p(x, top_k=np.arange(5))
    with pytest.raises(ValueError, match='temperature must be finite'):
        K.sample_top_p(x, temperature=float('inf'))
    with pytest.raises(ValueError, match='top_p must be finite'):
        K.sample_top_p(x, top_p=torch.tensor([0.5, float('nan'), 0.5, 0.5]))
    with pytest.raises(ValueError, match='uniform'):
        K.sample_top_p(x, uniform=torch.rand(3))
    with pytest.raises(ValueError, match='step'):
        K.sample_top_p(x, step=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match='floating'):
        K.sample_top_p(torch.zeros(4, 10, dtype=torch.int64))
    # scalars, lists, numpy arrays and tensors; leading dimensions are rows
    x3 = torch.randn(2, 3, 10, generator=torch.Generator().manual_seed(8))
    u = torch.rand(6)
    a, pa = K.sample_top_p(x3, [0.5] * 6, np.full(6, 4), torch.full((6,), 0.9), uniform=u)
    b, pb = K.sample_top_p(x3.reshape(6, 10), 0.5, 4, 0.9, uniform=u)
    assert tuple(a.shape) == (2, 3) and torch.equal(a.reshape(-1), b) and torch.equal(pa.reshape(-1), pb)
    assert ('sample_top_p', 'ref') in R.list_kernels() and ('sample_top_p', 'hip') in R.list_kernels()


# ------------------------------------------------------------------------------------- GPU
_TOL = {'float32': 1e-5, 'bfloat16': 2e-3, 'float16': 2e-3}


def _hip(x, *a, **kw):
    st = R.stats().get(('sample_top_p', 'hip'), 0)
    out = K.sample_top_p(x, *a, **kw)
    assert R.stats().get(('sample_top_p', 'hip'), 0) == st + 1
    return out[0].cpu(), out[1].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'float16'])
@pytest.mark.parametrize('ci', range(len(CASES)), ids=_IDS)
def test_hip_equals_ref_gpu(ci, dtype):
    d = _table(ci, dtype)
    _check_left_out(d['robust'], _IDS[ci])
    ok = d['robust']
    ids, pr = _hip(d['x'].cuda(), *d['par'], uniform=d['u'].cuda())
    assert int(ids.min()) >= 0 and int(ids.max()) < CASES[ci][0]
    assert torch.equal(ids[ok], d['rid'][ok])
    err = float((pr - d['rpr'])[ok].abs().max())
    print(f"probs: max error {err:.3g}")
    assert err < _TOL[dtype]
    if CASES[ci][0] in (7, 1025):                           # R = 1 and R = 3: rows 1, 2 start unaligned
        for Rn in (1, 3):
            ids, pr = _hip(d['x'][:Rn].cuda(), *d['par'], uniform=d['u'][:Rn].cuda())
            assert torch.equal(ids[ok[:Rn]], d['rid'][:Rn][ok[:Rn]])
            assert all(float(e) < _TOL[dtype] for e in (pr - d['rpr'][:Rn]).abs()[ok[:Rn]])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_hip_mixed_rows_gpu(dtype):
    """One launch whose rows cycle through greedy, top-k only, top-p only and both."""
    x, u = _table(3, dtype)['x'], _table(3, dtype)['u']
    r = np.arange(64)
    T = np.where(r % 8 == 0, 0.0, 1.0)
    k = np.select([r % 16 == 4, r % 4 == 1, r % 4 == 3], [1, 8, 8], 0)
    p = np.select([r % 16 == 12, r % 4 == 2, r % 4 == 3], [0.0, 0.9, 0.9], 1.0)    # greedy: T 0, k 1, p 0
    oid, _, robust = _oracle(x.double().numpy(), T, k, p, u.double().numpy())
    robust = torch.from_numpy(robust)
    _check_left_out(robust, 'mixed')
    rid, rpr = K.sample_top_p(x, T, k, p, uniform=u)
    assert torch.equal(rid[robust], torch.from_numpy(oid)[robust])
    ids, pr = _hip(x.cuda(), T, k, p, uniform=u.cuda())
    assert torch.equal(ids[robust], rid[robust])
    assert float((pr - rpr)[robust].abs().max()) < _TOL[dtype]


@pytest.mark.gpu
def test_hip_hash_equals_reference_gpu():
    for seed, counter in ((0, 0), (0x1234567890ABCDEF, 7), (5, (1 << 40) + 3)):
        got = K.sample_uniform_hip(seed, counter, 4096, 'cuda')
        assert np.array_equal(got.cpu().numpy(), K.sample_uniform_ref(seed, counter, 4096))
    step = torch.tensor([11], dtype=torch.int64, device='cuda')
    got = K.sample_uniform_hip(9, 30, 300, 'cuda', step=step)
    assert np.array_equal(got.cpu().numpy(), K.sample_uniform_ref(9, 41, 300))


@pytest.mark.gpu
def test_hip_ties_masks_and_untrusted_parameters_gpu():
    _check_ties_and_masks('cuda')
    # device parameters are not validated on the host: the kernel clamps them
    V = 257
    g = torch.Generator().manual_seed(12)
    x = torch.randn(8, V, generator=g) * 3
    x[7] = float('nan')
    u = torch.rand(8, generator=g)
    T = torch.tensor([1.0, float('inf'), 1.0, float('nan'), 1.0, -2.0, float('inf'), 1.0])
    k = torch.tensor([-5, 0, V + 1000, 4, 2 ** 31 - 1, 4, -2 ** 31, -1], dtype=torch.int32)
    p = torch.tensor([float('nan'), 0.9, 0.5, 0.5, float('inf'), 0.5, float('nan'), float('nan')])
    for dt in (torch.float32, torch.bfloat16):
        ids, pr = _hip(x.cuda().to(dt), T.cuda(), k.cuda(), p.cuda(), uniform=u.cuda())
        assert int(ids.min()) >= 0 and int(ids.max()) < V and bool(torch.isfinite(pr).all())
        Tc = [1.0, FLT_MAX, 1.0, 0.0, 1.0, 0.0, FLT_MAX, 1.0]
        kc = [0, 0, 0, 4, 0, 4, 0, 0]
        pc = [1.0, 0.9, 0.5, 0.5, 1.0, 0.5, 1.0, 1.0]
        rid, rpr = K.sample_top_p(x.to(dt), Tc, kc, pc, uniform=u)
        _, _, robust = _oracle(x.to(dt).double().numpy(), Tc, kc, pc, u.double().numpy())
        robust = torch.from_numpy(robust)
        assert int(robust.sum()) >= 6
        assert torch.equal(ids[robust], rid[robust])
        assert float((pr - rpr)[robust].abs().max()) < 2e-3
        assert int(ids[7]) == 0 and float(pr[7]) == 0.0
    # junk uniforms are clamped into [0, 1)
    junk = torch.tensor([float('nan'), -1.0, 2.0, float('inf'), 0.5, 1.0, -0.0, 1e-30])
    ids, _ = _hip(x.cuda(), uniform=junk.cuda())
    assert int(ids.min()) >= 0 and int(ids.max()) < V
    with pytest.raises(ValueError, match='sample_top_p'):
        K.sample_top_p(torch.zeros(1, K.SAMPLE_MAX_V + 1, device='cuda', dtype=torch.bfloat16))


@pytest.mark.gpu
def test_hip_is_reproducible_gpu():
    d = _table(6, 'bfloat16')
    x, u = d['x'].cuda(), d['u'].cuda()
    a = _hip(x, *d['par'], uniform=u)
    b = _hip(x, *d['par'], uniform=u)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = _hip(x, 1.0, 0, 0.999, seed=3, offset=1)            # a diffuse set: thousands of entries kept
    b = _hip(x, 1.0, 0, 0.999, seed=3, offset=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_token_sampler_graph_replays_draw_fresh_numbers_gpu():
    d = _table(1, 'float32')
    x = d['x'].cuda()
    T, k, p = d['par']
    s = TokenSampler(64, temperature=T, top_k=k, top_p=p, seed=99, device='cuda')
    s(x)
    s(x)                                                    # warm-up outside the capture
    torch.cuda.synchronize()
    seed, c = s.state()
    assert (seed, c) == (99, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = s(x)
    got = []
    for _ in range(3):
        graph.replay()
        got.append(out.clone())
    torch.cuda.synchronize()
    assert s.state() == (99, c + 3)
    got = [g.cpu() for g in got]
    for i, ids in enumerate(got):
        u = K.sample_uniform_ref(99, c + i, 64)
        _, _, robust = _oracle(d['x'].double().numpy(), T, k, p, u.astype(np.float64))
        robust = torch.from_numpy(robust)
        _check_left_out(robust, f'replay {i}')
        want, _ = K.sample_top_p(d['x'], T, k, p, seed=99, offset=c + i)
        assert torch.equal(ids[robust], want[robust])
    assert not (torch.equal(got[0], got[1]) and torch.equal(got[1], got[2]))


@pytest.mark.gpu
def test_decoder_loop_with_greedy_sampler_equals_argmax_gpu():
    from paddle_ray_amd.incubate.nn import FusedMultiTransformer
    paddle.set_device('gpu')
    paddle.seed(0)
    m = FusedMultiTransformer(256, 2, 512, num_layers=2)     # head dim 128
    rs = np.random.RandomState(0)
    for prm in m.parameters():
        prm.set_value((rs.randn(*prm.shape) * (0.1 if len(prm.shape) > 1 else 0.2)).astype('float32')
                      + (1.0 if 'scale' in prm.name else 0.0))
    m.eval()
    m.to(dtype='bfloat16')
    B, E, V, S0 = 3, m.embed_dim, 1001, 5
    g = torch.Generator().manual_seed(21)
    prompt = torch.randn(B, S0, E, generator=g).to('cuda', torch.bfloat16)
    emb = torch.randn(V, E, generator=g).to('cuda', torch.bfloat16)
    head = (torch.randn(E, V, generator=g) / E ** 0.5).to('cuda', torch.bfloat16)
    sampler = TokenSampler(B, temperature=0.8, top_k=1, top_p=0.9, seed=1, device='cuda')
    runs = []
    for pick in (lambda logits: logits.argmax(-1), sampler):
        dec = FusedMultiTransformerDecoder(m, B, 48)
        h = dec.prefill(paddle.Tensor(prompt))._t[:, -1:]
        toks = []
        for _ in range(4):
            tok = pick((h[:, 0] @ head).float())
            toks.append(tok)
            h = dec.step(paddle.Tensor(emb[tok][:, None]))._t
        runs.append(torch.stack(toks, 1).cpu())
    assert torch.equal(runs[0], runs[1]) and runs[0].dtype == torch.int64
    assert len(set(runs[0].reshape(-1).tolist())) > 1
