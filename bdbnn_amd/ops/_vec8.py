"""Which tensors the "8 channels per thread" NHWC kernels can take
(csrc/vec8.h: bn_act, bn_pool, prelu, pool).

A thread owns 8 consecutive channels and a block covers 256 / (C/8) pixel
rows, so C must be a power of two in [8, 1024]; the kernels exist for
fp32 and bf16 only.  The bindings raise on anything else; the Python ops
ask this predicate first and take the torch composition instead.
"""

import torch

_DTYPES = (torch.float32, torch.bfloat16)


def vec8_supported(is_cuda, dim, C, dtype):
    """Pure: no tensor is touched.  C is ignored unless dim == 4."""
    if not is_cuda or dim != 4 or dtype not in _DTYPES:
        return False
    return 8 <= C <= 1024 and (C & (C - 1)) == 0


def tensor_vec8_supported(x):
    """vec8_supported of a tensor; x.size(1) is read only when it is 4-D."""
    dim = x.dim()
    return vec8_supported(x.is_cuda, dim, x.size(1) if dim == 4 else 0,
                          x.dtype)
