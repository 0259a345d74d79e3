"""Weight-only quantised linear (parity: python/paddle/nn/quant/quantized_linear.py): int8 / int4
weights with fp32 scales, activations in bf16 / fp16, over ``ops.fused.weight_only_linear``."""
from ...framework.core import Tensor, _u, convert_dtype
from ...ops import fused as K

_ALGOS = ('weight_only_int8', 'weight_only_int4')


def _arch(arch):
    if arch is not None and int(arch) != 950:
        raise ValueError(f"weight-only quantisation: arch must be None or 950 (the weight layout is "
                         f"gfx950's), got {arch!r}")


def _algo(algo):
    if algo not in _ALGOS:
        raise ValueError(f"weight-only quantisation: algo must be one of {_ALGOS}, got {algo!r}")
    return algo


def weight_quantize(x, algo='weight_only_int8', arch=None, group_size=-1):
    """Quantise a ``[K, N]`` weight: returns ``(weight, scale)`` for ``weight_only_linear``;
    ``weight`` is int8 ``[N, K]`` (``[N, K // 2]`` for int4) in the kernel's own tile order and
    ``scale`` fp32 ``[N]`` or ``[K / group_size, N]`` (``ops.fused.weight_quantize``)."""
    _arch(arch)
    q, s = K.weight_quantize(_u(x), _algo(algo), group_size)
    return Tensor(q), Tensor(s)


def weight_dequantize(x, scale, algo='weight_only_int8', out_dtype='float16', group_size=-1):
    """The ``[K, N]`` weight a ``weight_quantize`` pair stands for, in ``out_dtype``."""
    return Tensor(K.weight_dequantize(_u(x), _u(scale), _algo(algo), group_size, convert_dtype(out_dtype)))


def weight_only_linear(x, weight, bias=None, weight_scale=None, weight_dtype='int8', arch=None, group_size=-1):
    """``x @ dequantize(weight, weight_scale) + bias`` for ``x`` [..., K] in bf16 / fp16 (fp32 on the
    reference path): on the GPU one HIP kernel that never builds the floating-point weight
    (``ops.fused.weight_only_linear``), streaming the integer weight once up to
    ``ops.fused.WO_MAX_ROWS`` rows and running 128 x 128 MFMA tiles over the same bytes above."""
    _arch(arch)
    if weight_dtype not in ('int8', 'int4'):
        raise ValueError(f"weight_only_linear: weight_dtype must be 'int8' or 'int4', got {weight_dtype!r}")
    if weight_scale is None:
        raise ValueError("weight_only_linear: weight_scale is required")
    return Tensor(K.weight_only_linear(_u(x), _u(weight), _u(weight_scale), None if bias is None else _u(bias),
                                       None, weight_dtype, group_size))
