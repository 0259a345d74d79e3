"""Row-wise kernels (LayerNorm, RMSNorm, add+dropout+LayerNorm, softmax, softmax cross-entropy,
vocab-parallel cross-entropy) against a float64 reference, over every launcher path.

One case table, two groups of tests: the unmarked CPU tests run the ``ref`` backend over it, the
``gpu`` tests run the HIP kernels over it (and assert through ``registry.stats()`` that they did).

Reference: plain torch in float64 on the dtype-rounded inputs, written here; backward from
autograd on that expression. Error measure per output tensor ``t``:

    e_kernel = max|t_kernel - t64|
    e_round  = max|round_to_dtype(t64) - t64|      (irreducible output rounding)
    e_ref32  = the same for the project's ``ref`` backend on the same inputs

GPU assertion:  e_kernel <= K * max(e_round, e_ref32) + tiny, K = 4 unless ``K_TABLE`` says
otherwise (measured worst ratios and the reason for every entry: profiles/rowwise_numerics.md).
tiny = 2^-126 + 2^-24 * max|t64|: every kernel computes in fp32, so it may flush fp32 denormals
and no output can be asked to be better than the fp32 rounding of its own magnitude. e_round
understates that when an fp32 output has a single element (rows = 1: mean, rstd) or happens to be
exactly representable (a column sum of half-precision dy); for a half-precision output the term
is 2^-16 (bf16) / 2^-13 (f16) of e_round's own scale and changes nothing.

CPU assertion (the ``ref`` backend has no second implementation to lean on):
    e_ref32 <= 4 * e_round + 64 * 2^-24 * amp * max|t64| + TINY
``amp`` is the case's condition number for fp32 arithmetic: max over rows of max|x| * rstd for
the norms (the relative rounding of x and of the mean is amplified by |x| / sigma in x - mean),
1 for softmax / cross-entropy. 64 covers the dozen or so fp32 roundings between input and
output including a pairwise sum over up to 16392 columns (log2 = 14 levels).

Width -> instantiation map (from launch_fwd / launch_bwd / pick_threads in norm.hip,
ADL_DISPATCH_C in fused_ln.hip, _adl_ok in ops/fused.py; ``chunks = ceil(cols / 8 / nt)``):

  norm.hip, cols % 8 == 0, nt = clamp(ceil(cols/8/64)*64, 64, 256):
    8, 520 (nt 64, 128)        fwd norm_fwd_vec<C=1>   bwd norm_bwd_vec<C=1>     (rms only)
    2048                        fwd norm_fwd_vec<C=1>   bwd norm_bwd_vec<C=1>     (rms only)
    2056, 4096                  fwd norm_fwd_vec<C=2>   bwd norm_bwd_vec<C=2>     (rms only)
    4104, 8192                  fwd norm_fwd_vec<C=4>   bwd norm_bwd_vec<C=4>     (rms, ln)
    8200, 16384                 fwd norm_fwd_vec<C=8>   bwd norm_bwd_scalar       (rms, ln)
    16392                       fwd norm_fwd_scalar     bwd norm_bwd_scalar       (rms, ln)
  norm.hip, cols % 8 != 0:
    1, 7, 333, 4099             fwd norm_fwd_scalar     bwd norm_bwd_scalar       (rms; ln 7, 333, 4099)
  HAS_MEAN = false for rms_norm, true for layer_norm; W = T (weights in x's dtype) or float.
  rows = 259 > 256 partial blocks: three blocks of the backward take two rows.
  fused_ln.hip (layer_norm with cols % 8 == 0 and cols <= 4096; add_dropout_layer_norm):
    8, 512                      adl_fwd_k<C=1>   adl_bwd2_k<C=1>
    520, 1024                   adl_fwd_k<C=2>   adl_bwd2_k<C=2>
    1032, 2048                  adl_fwd_k<C=4>   adl_bwd2_k<C=4>
    2056, 4096                  adl_fwd_k<C=8>   adl_bwd2_k<C=8>
    rows 67 -> 9 blocks of 4 waves, two rows per wave; 6150 x 8 -> 768 blocks stride over rows.
    dW / dB partials: colsum4_k (layer_norm), colsum4_multi_k (add_dropout_layer_norm).
    PRA_ADL_BWD=1 (read once per process) selects the one-pass adl_bwd_k<C> instead: run in a
    child process over 512, 520, 2048, 4096. colsum16_k needs cols % 4 != 0: no caller has one.
  softmax.hip: cols % 8 == 0 -> the 8-wide branches (8, 512, 520, 2048, 2056, 16392; 16392 makes
    the 256-thread strided loops wrap once more for one lane), otherwise the scalar branches
    (1, 7, 333, 1001, 4099). ce_bwd_k: gx = min(8, ceil(V/8/256)) parts per row.
"""
import contextlib

import pytest
import torch

from paddle_ray_amd.ops import fused as K
from paddle_ray_amd.ops import registry as R

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
U32 = 2.0 ** -24
TINY = 2.0 ** -126
EPS = 1e-5
NAME = {F32: 'fp32', F16: 'f16', BF16: 'bf16'}
UNIT = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}   # unit roundoff

# (op, output, x dtype) -> K where the measured worst ratio on the MI355X needs more than 4
# (profiles/rowwise_numerics.md: about twice the worst ratio over the whole table).
K_TABLE = {
    # column sums over rows: the kernels add one row after the other per workgroup and then the
    # (up to 256) workgroup partials in order, torch sums pairwise
    ('layer_norm', 'dw', 'fp32'): 8.0, ('layer_norm', 'dw', 'bf16'): 8.0, ('layer_norm', 'dw', 'f16'): 8.0,
    ('layer_norm', 'db', 'fp32'): 14.0,
    ('rms_norm', 'dw', 'fp32'): 15.0, ('rms_norm', 'dw', 'bf16'): 13.0, ('rms_norm', 'dw', 'f16'): 8.0,
    # the mean of zero-mean rows is ~0: e_round and e_ref32 are relative to |mean|, the kernel's
    # (and any) summation error to mean|x|
    ('layer_norm', 'mean', 'fp32'): 40.0,
    # rsqrtf (1 ulp) on a single row, whose e_round happens to be small
    ('layer_norm', 'rstd', 'bf16'): 12.0,
    # __expf
    ('softmax', 'y', 'fp32'): 10.0,
}

# (x dtype, weight dtype): weights in x's dtype and, for half x, in fp32 (the AMP layout)
DTYPES = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32)]

RMS_COLS = [8, 520, 2048, 2056, 4096, 4104, 8192, 8200, 16384, 16392, 1, 7, 333, 4099]
LN_NORM_COLS = [4104, 8192, 8200, 16384, 16392, 7, 333, 4099]
LN_FUSED_COLS = [8, 512, 520, 1024, 1032, 2048, 2056, 4096]
ADL_COLS = [512, 4096]
SM_COLS = [1, 7, 8, 333, 512, 520, 2048, 2056, 4099, 16392]
CE_V = [1, 7, 8, 1001, 2048, 2056, 16392]
VP_PER = [1001, 1000]
NORM_KINDS = ['randn', 'offset', 'const', 'scale', 'dymean']


def _k(op, out, xdt):
    return K_TABLE.get((op, out, NAME[xdt]), 4.0)


@contextlib.contextmanager
def _backend(ref):
    """Run the public ops with the ``ref`` backend (also on device tensors) when ``ref``."""
    old = R._FORCE_REF
    R._FORCE_REF = old or bool(ref)
    try:
        yield
    finally:
        R._FORCE_REF = old


def _maxerr(t, t64):
    return float((t.double() - t64).abs().max()) if t64.numel() else 0.0


class Checker:
    """Collects every figure of one test, prints it, and fails once at the end."""

    def __init__(self, gpu):
        self.gpu, self.bad, self.n = gpu, [], 0

    def check(self, op, xdt, case, got, ref, amp=1.0, floor=0.0, extra=None):
        """got / ref: {output: (tensor, t64, output dtype)} of the backend under test and of the
        ``ref`` backend (None in the CPU tests, where ``got`` IS the ref backend). floor (a number
        or {output: number}): the magnitude of the terms an output is a difference of, where
        that exceeds max|t64|; extra {output: number}: error the op's definition brings with it,
        such as a backward that reads the forward's ROUNDED output (both CPU bound only)."""
        for out, (t, t64, odt) in got.items():
            assert t is not None, (op, out, case)
            assert t.dtype == odt, (op, out, case, t.dtype, odt)
            assert t.shape == t64.shape, (op, out, case, t.shape, t64.shape)
            rounded = t64.to(odt).double()
            assert bool(torch.isfinite(rounded).all()), f"{op}.{out} {case}: vacuous case (overflow)"
            e_round = _maxerr(rounded, t64)
            e = _maxerr(t, t64)
            if self.gpu:
                rt, rt64, _ = ref[out]
                e_ref = _maxerr(rt, rt64)
                den = max(e_round, e_ref)
                tiny = TINY + U32 * (float(t64.abs().max()) if t64.numel() else 0.0)
                bound = _k(op, out, xdt) * den + tiny
                ratio = 0.0 if e <= tiny else ((e - tiny) / den if den > 0 else float('inf'))
                print(f"RATIO {op} {out} {NAME[xdt]} {ratio:.3f} e={e:.3e} tiny={tiny:.3e} e_round={e_round:.3e} "
                      f"e_ref32={e_ref:.3e} {case}")
            else:
                fl = floor.get(out, 0.0) if isinstance(floor, dict) else floor
                scale = max(float(t64.abs().max()) if t64.numel() else 0.0, fl)
                bound = 4 * e_round + 64 * U32 * amp * scale + (extra or {}).get(out, 0.0) + TINY
                print(f"REF {op} {out} {NAME[xdt]} e={e:.3e} bound={bound:.3e} {case}")
            self.n += 1
            if not e <= bound:
                self.bad.append(f"{op}.{out} {case}: e={e:.3e} > bound={bound:.3e} (e_round={e_round:.3e})")

    def done(self):
        assert self.n > 0
        assert not self.bad, f"{len(self.bad)} of {self.n} checks failed:\n" + "\n".join(self.bad[:40])


def _assert_hip(*ops):
    st = R.stats()
    for op in ops:
        assert st.get((op, 'hip'), 0) > 0 and (op, 'ref') not in st, (op, st)


def _leaf(t):
    return None if t is None else t.detach().clone().requires_grad_(True)


def _grad(t):
    return None if t is None else t.grad


def _d(t):
    return None if t is None else t.detach().double().requires_grad_(True)


# ---------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------
def _norm_base(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g),
            1 + 0.5 * torch.randn(cols, generator=g), 0.5 * torch.randn(cols, generator=g),
            torch.randn(rows, cols, generator=g), 0.5 * torch.randn(cols, generator=g))


def _norm_inputs(base, kind, xdt, wdt, pres, dev):
    x, dy, w, b = (t.clone() for t in base[:4])
    if kind == 'offset':      # a one-pass variance E[x^2] - E[x]^2 loses its digits here
        x += 100.0 if xdt == F32 else 8.0
    elif kind == 'const':     # variance exactly 0 (sums of small integers are exact): eps decides
        x[0] = 3.0
    elif kind == 'scale':     # one row scaled by 1e3 beside rows scaled by 1e-3
        x[0] *= 1e3
        x[1:] *= 1e-3
    elif kind == 'dymean':    # the c2 (mean of dy * w) term of the backward
        dy += 2.0
    x, dy = x.to(xdt).to(dev), dy.to(xdt).to(dev)
    w = w.to(wdt).to(dev) if pres in ('w', 'wb') else None
    b = b.to(wdt).to(dev) if pres == 'wb' else None
    return x, w, b, dy


def _ln64(op, x, w, b):
    """float64 LayerNorm / RMSNorm of fp64 leaves -> (y, mean, rstd)."""
    if op == 'rms_norm':
        mean = None
        rstd = torch.rsqrt((x * x).mean(-1) + EPS)
        y = x * rstd[:, None]
    else:
        mean = x.mean(-1)
        xc = x - mean[:, None]
        rstd = torch.rsqrt((xc * xc).mean(-1) + EPS)
        y = xc * rstd[:, None]
    if w is not None:
        y = y * w
    if b is not None:
        y = y + b
    return y, mean, rstd


def _norm64(op, x, w, b, dy):
    x64, w64, b64 = _d(x), _d(w), _d(b)
    y, mean, rstd = _ln64(op, x64, w64, b64)
    y.backward(dy.double())
    det = lambda t: None if t is None else t.detach()
    return {'y': det(y), 'mean': det(mean), 'rstd': det(rstd), 'dx': x64.grad, 'dw': _grad(w64),
            'db': _grad(b64)}


def _norm_run(op, x, w, b, dy, ref):
    xl, wl, bl = _leaf(x), _leaf(w), _leaf(b)
    with _backend(ref):
        if op == 'rms_norm':
            y = K.rms_norm(xl, wl, EPS)
            mean, (_, rstd) = None, R.dispatch('rms_norm_fwd', x, x, w, EPS)
        else:
            y = K.layer_norm(xl, wl, bl, EPS)
            _, mean, rstd = R.dispatch('layer_norm_fwd', x, x, w, b, EPS)
        y.backward(dy)
    return {'y': y.detach(), 'mean': mean, 'rstd': rstd, 'dx': xl.grad, 'dw': _grad(wl), 'db': _grad(bl)}


def _norm_amp(x, w, dy, rstd64):
    """(amp, floor) of the CPU bound: dx = (g - c2 - xhat * c1) * rstd is a difference of terms of
    size |dy * w| * rstd (and cancels completely for a single column); the mean is a sum of terms
    of size |x|."""
    amp = max(1.0, float((x.double().abs().amax(-1) * rstd64).max()))
    wmax = float(w.double().abs().max()) if w is not None else 1.0
    return amp, {'dx': float((dy.double().abs().amax(-1) * rstd64).max()) * wmax,
                 'mean': float(x.double().abs().max())}


def _norm_pack(vals, t64, xdt, wdt):
    odt = {'y': xdt, 'dx': xdt, 'dw': wdt, 'db': wdt, 'mean': F32, 'rstd': F32}
    return {k: (v, t64[k], odt[k]) for k, v in vals.items() if t64[k] is not None}


def _norm_cases(op, rows_list, full_rows):
    """(rows, kind, pres): randn over every presence at the small row counts and with all
    parameters at the largest; the hard inputs at 5 rows with all parameters."""
    allp = ['none', 'w'] if op == 'rms_norm' else ['none', 'w', 'wb']
    for rows in rows_list:
        for pres in (allp if rows in full_rows else allp[-1:]):
            yield rows, 'randn', pres
    for kind in NORM_KINDS[1:]:
        yield 5, kind, allp[-1]


def _norm_sweep(ck, op, cols, dev, rows_list=(1, 5, 259), full_rows=(1, 5)):
    bases = {}
    for rows, kind, pres in _norm_cases(op, rows_list, full_rows):
        if rows not in bases:
            bases[rows] = _norm_base(rows, cols, 1000 * rows + cols)
        for xdt, wdt in DTYPES:
            x, w, b, dy = _norm_inputs(bases[rows], kind, xdt, wdt, pres, dev)
            t64 = _norm64(op, x, w, b, dy)
            amp, floor = _norm_amp(x, w, dy, t64['rstd'])
            case = f"{rows}x{cols} {NAME[xdt]}/w{NAME[wdt]} {pres} {kind}"
            refv = _norm_pack(_norm_run(op, x, w, b, dy, True), t64, xdt, wdt)
            if ck.gpu:
                R.reset_stats()
                got = _norm_pack(_norm_run(op, x, w, b, dy, False), t64, xdt, wdt)
                _assert_hip(op + '_fwd', op + '_bwd')
                ck.check(op, xdt, case, got, refv, amp)
            else:
                ck.check(op, xdt, case, refv, None, amp, floor)


# ---------------------------------------------------------------------------------------------
# add + dropout(p = 0) + LayerNorm: r = x + h + hbias, y = LN(r). The LayerNorm reference is taken
# on the r the backend returned (rounded to x's dtype): y, mean and rstd must be those of the
# ROUNDED residual, which is what backward re-reads.
# ---------------------------------------------------------------------------------------------
def _adl_run(x, h, hb, w, b, dy, dr, ref, stats=True):
    xl, hl, hbl, wl, bl = _leaf(x), _leaf(h), _leaf(hb), _leaf(w), _leaf(b)
    with _backend(ref):
        r, y = K.add_dropout_layer_norm(xl, hl, hbl, wl, bl, p=0.0, eps=EPS)
        mean = rstd = None
        if stats:   # mean / rstd are returned by the kernel entry only
            _, _, mean, rstd = R.dispatch('add_dropout_ln_fwd', x, x, h, hb, w, b, 0.0, EPS, 0)
        torch.autograd.backward([r, y], [dr, dy])
    vals = {'r': r.detach(), 'y': y.detach(), 'mean': mean, 'rstd': rstd, 'dx': xl.grad, 'dh': hl.grad,
            'dhb': _grad(hbl), 'dw': _grad(wl), 'db': _grad(bl)}
    # float64 reference around this backend's own r
    r64 = x.double() + h.double() + (hb.double() if hb is not None else 0)
    rl, w64, b64 = _d(r), _d(w), _d(b)
    y64, mean64, rstd64 = _ln64('layer_norm', rl, w64, b64)
    y64.backward(dy.double())
    dri = rl.grad + dr.double()
    t64 = {'r': r64, 'y': y64.detach(), 'mean': mean64.detach(), 'rstd': rstd64.detach(), 'dx': dri, 'dh': dri,
           'dhb': dri.sum(0) if hb is not None else None, 'dw': _grad(w64), 'db': _grad(b64)}
    lead = w if w is not None else b
    xdt, wdt = x.dtype, (lead.dtype if lead is not None else x.dtype)
    odt = {'r': xdt, 'y': xdt, 'mean': F32, 'rstd': F32, 'dx': xdt, 'dh': xdt, 'dhb': xdt, 'dw': wdt, 'db': wdt}
    amp = max(1.0, float((r.detach().double().abs().amax(-1) * rstd64.detach()).max()))
    return {k: (v, t64[k], odt[k]) for k, v in vals.items() if t64[k] is not None and (stats or k not in ('mean', 'rstd'))}, amp


def _adl_sweep(ck, cols, dev):
    for rows in (5, 67):
        base = _norm_base(rows, cols, 31 * rows + cols)
        for with_hb in (True, False):
            for pres in ('none', 'w', 'wb'):
                for xdt, wdt in DTYPES:
                    x, w, b, dy = _norm_inputs(base, 'randn', xdt, wdt, pres, dev)
                    h, dr = base[4].to(xdt).to(dev), base[0].flip(0).to(xdt).to(dev)
                    hb = base[5].to(xdt).to(dev) if with_hb else None
                    case = f"{rows}x{cols} {NAME[xdt]}/w{NAME[wdt]} {pres} hbias={with_hb}"
                    refv, amp = _adl_run(x, h, hb, w, b, dy, dr, True)
                    if ck.gpu:
                        R.reset_stats()
                        got, _ = _adl_run(x, h, hb, w, b, dy, dr, False)
                        _assert_hip('add_dropout_ln_fwd', 'add_dropout_ln_bwd')
                        ck.check('add_dropout_ln', xdt, case, got, refv, amp)
                    else:
                        ck.check('add_dropout_ln', xdt, case, refv, None, amp)


# ---------------------------------------------------------------------------------------------
# softmax over the last dim
# ---------------------------------------------------------------------------------------------
SM_KINDS = ['randn4', 'spike', 'inf_chunks', 'inf_allbut1', 'equal_big']


def _sm_inputs(rows, cols, kind, dt, dev):
    g = torch.Generator().manual_seed(7 * rows + cols)
    x = torch.randn(rows, cols, generator=g) * 4
    dy = torch.randn(rows, cols, generator=g)
    ninf = float('-inf')
    if kind == 'spike':
        for i in range(rows):
            x[i, (i * 7 + 3) % cols] += 30.0
    elif kind == 'inf_chunks':   # whole aligned chunks of 8 (first and last) and part of a chunk
        x[:, 0:min(8, cols - 1)] = ninf
        if cols >= 24:
            x[:, (cols // 8 - 1) * 8:(cols // 8) * 8] = ninf
            x[:, 10:13] = ninf
    elif kind == 'inf_allbut1':
        keep = torch.arange(rows) * 5 % cols
        v = x[torch.arange(rows), keep].clone()
        x[:] = ninf
        x[torch.arange(rows), keep] = v
    elif kind == 'equal_big':
        big = 3e4 if dt == F16 else 1e30
        x[:] = big
        x[1::2] = -big
    elif kind == 'inf_row':
        x[0] = ninf
    return x.to(dt).to(dev), dy.to(dt).to(dev)


def _sm_run(x, dy, ref):
    xl = _leaf(x)
    with _backend(ref):
        y = K.softmax_lastdim(xl)
        y.backward(dy)
    return {'y': y.detach(), 'dx': xl.grad}


def _sm_sweep(ck, cols, dev):
    for rows in (1, 19):
        for dt in (F32, BF16, F16):
            for kind in SM_KINDS:
                x, dy = _sm_inputs(rows, cols, kind, dt, dev)
                x64 = _d(x)
                y64 = torch.softmax(x64, -1)
                y64.backward(dy.double())
                t64 = {'y': y64.detach(), 'dx': x64.grad}
                pack = lambda v: {k: (v[k], t64[k], dt) for k in v}
                case = f"{rows}x{cols} {NAME[dt]} {kind}"
                refv = pack(_sm_run(x, dy, True))
                if ck.gpu:
                    R.reset_stats()
                    got = pack(_sm_run(x, dy, False))
                    _assert_hip('softmax_fwd', 'softmax_bwd')
                    ck.check('softmax', dt, case, got, refv)
                else:
                    # dx = y * (dy - sum(y * dy)) from the SAVED y (<= 1, rounded to dt): a difference
                    # of terms of size max|dy|, each off by y's rounding
                    dmax = float(dy.double().abs().max())
                    ck.check('softmax', dt, case, refv, None, floor={'dx': dmax},
                             extra={'dx': 4 * UNIT[dt] * dmax})
            # a fully -inf row: one policy on both backends -- the row is NaN (0 / 0), as in
            # torch.softmax; the other rows are unaffected
            x, _ = _sm_inputs(rows, cols, 'inf_row', dt, dev)
            with _backend(not ck.gpu):
                y = K.softmax_lastdim(x)
            assert bool(torch.isnan(y[0]).all()), (rows, cols, dt)
            if rows > 1:
                y64 = torch.softmax(x[1:].double(), -1)
                got = {'y': (y[1:], y64, dt)}
                with _backend(True):
                    refv = {'y': (K.softmax_lastdim(x)[1:], y64, dt)}
                ck.check('softmax', dt, f"{rows}x{cols} {NAME[dt]} inf_row", got, refv if ck.gpu else None)


# ---------------------------------------------------------------------------------------------
# softmax + cross-entropy. Policy on both backends: a label equal to ignore_index or outside
# [0, V) gives loss 0 and a zero gradient row.
# ---------------------------------------------------------------------------------------------
CE_KINDS = ['edges', 'edges_dloss0', 'one_ignored', 'all_ignored', 'ignore0', 'out_of_range']


def _ce_labels(rows, V, kind):
    edge = torch.tensor([min(v, V - 1) for v in (0, V - 1, 7, 8, V // 2)])
    lab = edge[torch.arange(rows) % 5].clone()
    ign = -100
    if kind == 'one_ignored':
        lab[rows // 2] = ign
    elif kind == 'all_ignored':
        lab[:] = ign
    elif kind == 'ignore0':
        ign = 0
    elif kind == 'out_of_range':
        lab[0] = V
        if rows > 1:
            lab[1] = -5
    return lab, ign


def _ce64(x, lab, ign, dloss):
    """loss, lse and dlogits in float64."""
    x64 = _d(x)
    V = x.shape[1]
    lse = torch.logsumexp(x64, -1)
    valid = (lab != ign) & (lab >= 0) & (lab < V)
    picked = x64.gather(-1, torch.where(valid, lab, torch.zeros_like(lab))[:, None]).squeeze(-1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
    (loss * dloss.double()).sum().backward()
    return {'loss': loss.detach(), 'lse': lse.detach(), 'dlogits': x64.grad}


def _ce_run(x, lab, ign, dloss, ref):
    xl = _leaf(x)
    with _backend(ref):
        loss = K.softmax_cross_entropy(xl, lab, ign)
        _, lse = R.dispatch('softmax_ce_fwd', x, x, lab, ign)
        loss.backward(dloss)
    return {'loss': loss.detach(), 'lse': lse, 'dlogits': xl.grad}


def _ce_sweep(ck, V, dev):
    for rows in (1, 67):
        g = torch.Generator().manual_seed(13 * rows + V)
        base = torch.randn(rows, V, generator=g) * 4
        dl = torch.randn(rows, generator=g)
        for dt in (F32, BF16, F16):
            x = base.to(dt).to(dev)
            for kind in CE_KINDS:
                lab, ign = _ce_labels(rows, V, kind)
                lab = lab.to(dev)
                dloss = (torch.zeros_like(dl) if kind == 'edges_dloss0' else dl).to(dev)
                t64 = _ce64(x, lab, ign, dloss)
                pack = lambda v: {k: (v[k], t64[k], dt if k == 'dlogits' else F32) for k in v}
                case = f"{rows}x{V} {NAME[dt]} {kind}"
                floor = float(x.double().abs().max())
                refv = pack(_ce_run(x, lab, ign, dloss, True))
                if ck.gpu:
                    R.reset_stats()
                    got = pack(_ce_run(x, lab, ign, dloss, False))
                    _assert_hip('softmax_ce_fwd', 'softmax_ce_bwd')
                    ck.check('softmax_ce', dt, case, got, refv, floor=floor)
                else:
                    ck.check('softmax_ce', dt, case, refv, None, floor=floor)
                if kind in ('all_ignored', 'out_of_range', 'ignore0'):   # the policy, exactly
                    out = (got if ck.gpu else refv)
                    dead = ~((lab != ign) & (lab >= 0) & (lab < V))
                    assert bool((out['loss'][0][dead] == 0).all()) and bool((out['dlogits'][0][dead] == 0).all()), case


# ---------------------------------------------------------------------------------------------
# vocab-parallel cross-entropy as the ranks of a 4-way split (partials of every rank by the same
# backend, stacked in place of the all-gather)
# ---------------------------------------------------------------------------------------------
def _vp_run(x, lab, dloss, per, world, ign, ref):
    with _backend(ref):
        sl = [x[:, r * per:(r + 1) * per].contiguous() for r in range(world)]
        parts = [R.dispatch('vp_ce_part_fwd', sl[r], sl[r], lab, r * per) for r in range(world)]
        allp = torch.stack(parts)
        loss, lse = R.dispatch('vp_ce_final', allp, allp, lab, world * per, ign)
        grads = [R.dispatch('vp_ce_bwd', sl[r], sl[r], lab, lse, dloss, r * per, world * per, ign)
                 for r in range(world)]
    return {'m': allp[..., 0], 's': allp[..., 1], 'picked': allp[..., 2], 'loss': loss, 'lse': lse,
            'dlogits': torch.cat(grads, -1)}


def _vp_sweep(ck, per, dev):
    world, rank, rows, ign = 4, 1, 37, -100
    V, start = world * per, rank * per
    g = torch.Generator().manual_seed(per)
    base = torch.randn(rows, V, generator=g) * 4
    base[5, 2 * per + 3] = base[5].max() + 60.0     # row 5: the maximum lives on rank 2 by a margin of 60
    lab = torch.randint(0, V, (rows,), generator=g)
    lab[:4] = torch.tensor([start - 1, start, start + per - 1, start + per])   # the middle rank's edges
    lab[6], lab[7], lab[8] = ign, V, -5
    dl = torch.randn(rows, generator=g)
    for dt in (F32, BF16, F16):
        x, labd, dloss = base.to(dt).to(dev), lab.to(dev), dl.to(dev)
        t64 = _ce64(x, labd, ign, dloss)
        xs = x.double().view(rows, world, per).transpose(0, 1)          # [world, rows, per]
        m64 = xs.amax(-1)
        loc = labd[None, :] - torch.arange(world, device=dev)[:, None] * per
        inr = (loc >= 0) & (loc < per)
        t64.update(m=m64, s=torch.exp(xs - m64[..., None]).sum(-1),
                   picked=xs.gather(-1, loc.clamp(0, per - 1)[..., None]).squeeze(-1) * inr)
        pack = lambda v: {k: (v[k], t64[k], dt if k == 'dlogits' else F32) for k in v}
        case = f"{rows}x4x{per} {NAME[dt]}"
        floor = float(x.double().abs().max())
        refv = pack(_vp_run(x, labd, dloss, per, world, ign, True))
        if ck.gpu:
            R.reset_stats()
            got = pack(_vp_run(x, labd, dloss, per, world, ign, False))
            _assert_hip('vp_ce_part_fwd', 'vp_ce_final', 'vp_ce_bwd')
            ck.check('vp_ce', dt, case, got, refv, floor=floor)
        else:
            ck.check('vp_ce', dt, case, refv, None, floor=floor)
        out = got if ck.gpu else refv
        assert bool((out['loss'][0][6:9] == 0).all()) and bool((out['dlogits'][0][6:9] == 0).all()), case


# ---------------------------------------------------------------------------------------------
# dtype policy: w / b of a dtype the kernels do not take are cast to fp32 (ops.fused._norm_params)
# ---------------------------------------------------------------------------------------------
def _policy_sweep(ck, dev, cols_list):
    for cols in cols_list:
        base = _norm_base(5, cols, cols)
        for xdt in (F32, F16, BF16):
            for wdt in (F32, F16, BF16):
                for pres in ('w', 'b', 'wb'):
                    x, dy = base[0].to(xdt).to(dev), base[1].to(xdt).to(dev)
                    w = base[2].to(wdt).to(dev) if 'w' in pres else None
                    b = base[3].to(wdt).to(dev) if 'b' in pres else None
                    h, hb, dr = base[4].to(xdt).to(dev), base[5].to(xdt).to(dev), base[0].flip(0).to(xdt).to(dev)
                    case = f"5x{cols} {NAME[xdt]}/w{NAME[wdt]} {pres} policy"
                    # what the op must compute: the parameters as given (rounded to wdt), in fp64;
                    # dw / db come back in the dtype of the tensors that were passed
                    runs = [('layer_norm', lambda ref: _norm_run('layer_norm', x, w, b, dy, ref),
                             lambda: _norm64('layer_norm', x, w, b, dy))]
                    if pres == 'w':
                        runs.append(('rms_norm', lambda ref: _norm_run('rms_norm', x, w, None, dy, ref),
                                     lambda: _norm64('rms_norm', x, w, None, dy)))
                    ok = wdt in (xdt, F32)
                    for op, run, r64 in runs:
                        t64 = r64()
                        amp, floor = _norm_amp(x, w, dy, t64['rstd'])

                        def go(ref):
                            with _backend(ref):
                                if ok:
                                    return _norm_pack(run(ref), t64, xdt, wdt)
                                # the direct fwd dispatch of _norm_run takes kernel dtypes only
                                xl, wl, bl = _leaf(x), _leaf(w), _leaf(b)
                                y = K.rms_norm(xl, wl, EPS) if op == 'rms_norm' else K.layer_norm(xl, wl, bl, EPS)
                                y.backward(dy)
                                v = {'y': y.detach(), 'dx': xl.grad, 'dw': _grad(wl), 'db': _grad(bl)}
                                return _norm_pack(v, t64, xdt, wdt)
                        refv = go(True)
                        if ck.gpu:
                            R.reset_stats()
                            ck.check(op, xdt, case, go(False), refv, amp)
                            _assert_hip(op + '_fwd', op + '_bwd')
                        else:
                            ck.check(op, xdt, case, refv, None, amp, floor)
                    if not K._adl_ok(cols):   # other widths take the ref kernels on every backend
                        continue
                    refv, amp = _adl_run(x, h, hb, w, b, dy, dr, True, stats=False)
                    if ck.gpu:
                        R.reset_stats()
                        got, _ = _adl_run(x, h, hb, w, b, dy, dr, False, stats=False)
                        _assert_hip('add_dropout_ln_fwd', 'add_dropout_ln_bwd')
                        ck.check('add_dropout_ln', xdt, case, got, refv, amp)
                    else:
                        ck.check('add_dropout_ln', xdt, case, refv, None, amp)


# =============================================================================================
# CPU tests: the ``ref`` backend over the table
# =============================================================================================
@pytest.mark.parametrize('cols', RMS_COLS)
def test_ref_rms_norm(cols):
    ck = Checker(False)
    _norm_sweep(ck, 'rms_norm', cols, 'cpu')
    ck.done()


@pytest.mark.parametrize('cols', LN_NORM_COLS + LN_FUSED_COLS)
def test_ref_layer_norm(cols):
    ck = Checker(False)
    _norm_sweep(ck, 'layer_norm', cols, 'cpu', *(((1, 5, 259), (1, 5)) if cols in LN_NORM_COLS else
                                                 ((1, 5, 67), (1, 5))))
    ck.done()


def test_ref_layer_norm_many_rows():
    ck = Checker(False)
    _norm_sweep(ck, 'layer_norm', 8, 'cpu', (6150,), ())
    ck.done()


@pytest.mark.parametrize('cols', ADL_COLS)
def test_ref_add_dropout_layer_norm(cols):
    ck = Checker(False)
    _adl_sweep(ck, cols, 'cpu')
    ck.done()


@pytest.mark.parametrize('cols', SM_COLS)
def test_ref_softmax(cols):
    ck = Checker(False)
    _sm_sweep(ck, cols, 'cpu')
    ck.done()


@pytest.mark.parametrize('V', CE_V)
def test_ref_softmax_ce(V):
    ck = Checker(False)
    _ce_sweep(ck, V, 'cpu')
    ck.done()


@pytest.mark.parametrize('per', VP_PER)
def test_ref_vp_ce(per):
    ck = Checker(False)
    _vp_sweep(ck, per, 'cpu')
    ck.done()


def test_dtype_policy():
    """Every (x dtype, w dtype) pair of {fp32, f16, bf16}^2 with w only, b only and both gives the
    float64 result of the parameters as passed (a dtype the kernels do not take is cast to fp32,
    nothing raises), and dw / db come back in the parameters' own dtype."""
    ck = Checker(False)
    _policy_sweep(ck, 'cpu', [24, 333])
    ck.done()


def test_norm_params_policy():
    x = torch.zeros(2, 8, dtype=BF16)
    for wdt, want in ((BF16, BF16), (F32, F32), (F16, F32)):
        w, b = K._norm_params(x, torch.ones(8, dtype=wdt), torch.ones(8, dtype=F16))
        assert w.dtype == want and b.dtype == want
        w, b = K._norm_params(x, None, torch.ones(8, dtype=wdt))
        assert w is None and b.dtype == want
    assert K._norm_params(x, None, None) == (None, None)
    with pytest.raises(TypeError):   # the guard in front of the launches
        K._wdt('layer_norm', x, torch.ones(8, dtype=F16))
    with pytest.raises(TypeError):
        K._wdt('layer_norm', x, None, torch.ones(8, dtype=F16))
    assert K._wdt('layer_norm', x, None, torch.ones(8)) == 0


def test_out_of_range_label_policy():
    """ref kernels: labels outside [0, V) that are not ignore_index give loss 0 and a zero row,
    as ce_fwd_k / ce_bwd_k and the vp_ce_* kernels do."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(6, 11, generator=g)
    lab = torch.tensor([11, -5, 3, -100, 0, 10])
    loss, lse = K._ce_fwd_ref(x, lab, -100)
    grad = K._ce_bwd_ref(x, lab, lse, torch.ones(6), -100)
    want = torch.nn.functional.cross_entropy(x[[2, 4, 5]], lab[[2, 4, 5]], reduction='none')
    torch.testing.assert_close(loss[[2, 4, 5]], want)
    assert bool((loss[[0, 1, 3]] == 0).all()) and bool((grad[[0, 1, 3]] == 0).all())
    assert bool((grad[[2, 4, 5]].abs().sum(-1) > 0).all())
    xl = x.clone().requires_grad_(True)
    K.softmax_cross_entropy(xl, lab, -100).sum().backward()
    assert bool((xl.grad[[0, 1, 3]] == 0).all())


def test_offset_rows_expose_one_pass_variance():
    """The offset of the 'offset' inputs keeps e_ref32 meaningful: an fp32 LayerNorm whose
    variance is E[x^2] - E[x]^2 misses the GPU bound K * max(e_round, e_ref32) on them. (For
    half inputs an fp32 one-pass variance is harmless -- its error is far below the output
    rounding -- so the offset there only has to keep the rounded inputs apart.)"""
    for cols in (333, 2048):
        x, w, b, dy = _norm_inputs(_norm_base(5, cols, cols), 'offset', F32, F32, 'wb', 'cpu')
        t64 = _norm64('layer_norm', x, w, b, dy)
        y_ref = _norm_run('layer_norm', x, w, b, dy, True)['y']
        var1 = (x * x).mean(-1) - x.mean(-1) ** 2
        y_one = (x - x.mean(-1, keepdim=True)) * torch.rsqrt(var1 + EPS)[:, None] * w + b
        den = max(_maxerr(t64['y'].float(), t64['y']), _maxerr(y_ref, t64['y']))
        kmax = max([4.0] + [v for (op, out, _), v in K_TABLE.items() if out == 'y'])
        assert _maxerr(y_one, t64['y']) > kmax * den


# =============================================================================================
# GPU tests: the HIP kernels over the table
# =============================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('cols', RMS_COLS)
def test_hip_rms_norm(cols):
    ck = Checker(True)
    _norm_sweep(ck, 'rms_norm', cols, 'cuda')
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize('cols', LN_NORM_COLS + LN_FUSED_COLS)
def test_hip_layer_norm(cols):
    ck = Checker(True)
    _norm_sweep(ck, 'layer_norm', cols, 'cuda', *(((1, 5, 259), (1, 5)) if cols in LN_NORM_COLS else
                                                  ((1, 5, 67), (1, 5))))
    ck.done()


@pytest.mark.gpu
def test_hip_layer_norm_many_rows():
    """6150 x 8: the fused backward's 768 workgroups of 4 waves stride over the rows."""
    ck = Checker(True)
    _norm_sweep(ck, 'layer_norm', 8, 'cuda', (6150,), ())
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize('cols', ADL_COLS)
def test_hip_add_dropout_layer_norm(cols):
    ck = Checker(True)
    _adl_sweep(ck, cols, 'cuda')
    ck.done()


_ONE_PASS = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import test_rowwise_numerics as T
ck = T.Checker(True)
for cols in T.ADL_COLS:                      # adl_bwd_k<C=1>, <C=8>, colsum4_multi_k
    T._adl_sweep(ck, cols, 'cuda')
for cols in (520, 2048):                     # adl_bwd_k<C=2>, <C=4>
    T._norm_sweep(ck, 'layer_norm', cols, 'cuda', (5, 67), (5,))
ck.done()
print('one-pass ok', ck.n)
"""


@pytest.mark.gpu
def test_hip_add_dropout_layer_norm_one_pass_backward():
    """The one-pass backward ``adl_bwd_k`` (PRA_ADL_BWD=1, read once per process: hence the child
    process) over the fused widths of every C, same bound as the default two-pass kernel."""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _ONE_PASS.format(root=os.path.dirname(tests), tests=tests)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PRA_ADL_BWD='1'),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and 'one-pass ok' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize('cols', SM_COLS)
def test_hip_softmax(cols):
    ck = Checker(True)
    _sm_sweep(ck, cols, 'cuda')
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize('V', CE_V)
def test_hip_softmax_ce(V):
    ck = Checker(True)
    _ce_sweep(ck, V, 'cuda')
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize('per', VP_PER)
def test_hip_vp_ce(per):
    ck = Checker(True)
    _vp_sweep(ck, per, 'cuda')
    ck.done()


@pytest.mark.gpu
def test_hip_dtype_policy():
    """The same policy on the hip backend: a weight dtype the kernels do not take never reaches
    them (it is cast to fp32), and the result is the reference result. 24 columns reach
    fused_ln.hip, 333 norm.hip."""
    ck = Checker(True)
    _policy_sweep(ck, 'cuda', [24, 333])
    ck.done()


@pytest.mark.gpu
def test_hip_entry_points_refuse_dtype_pairs():
    """The six C entry points launch nothing and report a dtype pair they have no instantiation
    for (the binding raises) instead of returning silently."""
    L = K._native.lib()
    t = torch.zeros(4, 8, device='cuda')
    v = torch.zeros(8, device='cuda')
    p, s = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    for dt, dtw in ((0, 2), (0, 1), (2, 1), (1, 2), (7, 0), (0, 7)):
        with pytest.raises(ValueError):
            L.layernorm_fwd(p, v.data_ptr(), 0, p, v.data_ptr(), v.data_ptr(), 4, 8, EPS, dt, dtw, s)
        with pytest.raises(ValueError):
            L.layernorm_bwd(p, p, v.data_ptr(), v.data_ptr(), v.data_ptr(), p, p, p, 1, 8, 1, dt, dtw, s)
        with pytest.raises(ValueError):
            L.rmsnorm_fwd(p, v.data_ptr(), p, v.data_ptr(), 4, 8, EPS, dt, dtw, s)
        with pytest.raises(ValueError):
            L.rmsnorm_bwd(p, p, v.data_ptr(), v.data_ptr(), p, p, 1, 8, 1, dt, dtw, s)
        with pytest.raises(ValueError):
            L.adl_fwd(p, 0, 0, v.data_ptr(), 0, 0, p, v.data_ptr(), v.data_ptr(), 4, 8, EPS, 0.0, 0, 0, 0, dt, dtw, s)
        with pytest.raises(ValueError):
            L.adl_bwd(p, 0, p, v.data_ptr(), v.data_ptr(), v.data_ptr(), p, 0, 0, 0, 0, 1, 8, 1, 0.0, 0, 0, 0,
                      dt, dtw, s)
    torch.cuda.synchronize()
    assert bool((t == 0).all())
