"""Fused BatchNorm (+ residual add) (+ activation) — K8.

``fused_bn_act(x, bn, act=None, skip=None)`` runs the whole
conv-output -> BN -> (+skip) -> PReLU/ReLU tail of a BD-BNN block as two
kernels forward (stats + normalize/add/act) and two backward (reduce +
apply) on the GPU, replacing the MIOpen BN pipeline + separate add +
activation (profiles/r01_bench_b256_kernel_stats.md).  Parameters stay
in the ordinary ``nn.BatchNorm2d`` / ``ChannelPReLU`` modules, so
checkpoints are unchanged.

CPU (and any tensor ops/_vec8.py rules out: not 4-D, C not a power of two
in [8, 1024], dtype other than fp32 / bf16): exact composition fallback.
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _C
from ._vec8 import tensor_vec8_supported
from .activations import ChannelPReLU, RPReLU
from .pool import FusedMaxPool2d

_ACT_NONE, _ACT_PRELU, _ACT_RELU, _ACT_RPRELU = 0, 1, 2, 3

# BDBNN_FUSE_RPRELU=1: an RPReLU tail (ReAct models) runs inside the BN
# kernels as act_kind 3 instead of as three elementwise modules after them.
# Off by default: under autocast the fused output keeps the conv output's
# dtype (bf16), where the composition's fp32 shift parameters promote every
# block activation to fp32 — a numerics change the user opts into
# (docs/TUNING.md).
_FUSE_RPRELU = os.environ.get("BDBNN_FUSE_RPRELU", "0") == "1"


class _BNActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip, gamma, beta, a, running_mean, running_var,
                momentum, eps, act_kind, training, s1=None, s2=None,
                want_pack=False, defer_cell=None, b1=None, b2=None):
        nat = _C.native_required()
        res = nat.bn_act_fwd_train(
            x, skip, gamma, beta, a, running_mean, running_var,
            momentum, eps, act_kind, s1, s2, want_pack, b1, b2)
        out, z, mean, invstd = res[:4]
        # RPReLU's shifts (kind 3): backward never reads them (the saved
        # plane z already holds u = z + b1); their grads go back in the
        # parameters' own shape and dtype
        ctx.shift_like = ((b1.shape, b1.dtype), (b2.shape, b2.dtype)) \
            if act_kind == _ACT_RPRELU else None
        ctx.save_for_backward(x, z, mean, invstd, gamma,
                              a if a is not None else torch.empty(0))
        ctx.act_kind = act_kind
        ctx.has_skip = skip is not None
        ctx.has_a = a is not None
        # deferred skip grad: instead of returning dskip (which autograd
        # would add to the conv's dx in a separate full-tensor pass), the
        # backward stashes it in this cell; the conv that produced the
        # skip tensor's other consumer fuses it into its dgrad epilogue.
        ctx.defer_cell = defer_cell if skip is not None else None
        if want_pack:
            # next conv's sign/mask bitplanes, packed in the epilogue
            xpk, mpk = res[4], res[5]
            ctx.mark_non_differentiable(xpk, mpk)
            return out, xpk, mpk
        dummy = out.new_empty(0)
        ctx.mark_non_differentiable(dummy)
        return out, dummy, dummy

    @staticmethod
    def backward(ctx, dy, _gxpk=None, _gmpk=None):
        x, z, mean, invstd, gamma, a = ctx.saved_tensors
        nat = _C.native_required()
        res = nat.bn_act_bwd(
            dy, z, x, mean, invstd, gamma,
            a if ctx.has_a else None, ctx.act_kind, ctx.has_skip)
        dx, dskip, dgamma, dbeta, da = res[:5]
        db1 = db2 = None
        if ctx.shift_like is not None:
            (sh1, dt1), (sh2, dt2) = ctx.shift_like
            db1 = res[5].to(dt1).view(sh1)
            db2 = res[6].to(dt2).view(sh2)
        skip_grad = dskip if ctx.has_skip else None
        if ctx.defer_cell is not None and skip_grad is not None:
            ctx.defer_cell["g"] = skip_grad
            skip_grad = None
        return (dx, skip_grad,
                dgamma, dbeta,
                da if ctx.has_a else None,
                None, None, None, None, None, None, None, None, None,
                None, db1, db2)


class _BNReluPoolFn(torch.autograd.Function):
    """bn -> ReLU -> maxpool as one op (csrc/bn_pool.hip).  Neither the
    ReLU output nor the pool's input gradient is materialised: forward
    saves the BN input x and the u8 argmax plane, backward recomputes the
    ReLU mask from x and gathers dy through the argmax plane."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum,
                eps, ks, stride, pad, want_pack):
        nat = _C.native_required()
        res = nat.bn_relu_maxpool_fwd_train(
            x, gamma, beta, running_mean, running_var, momentum, eps,
            ks, stride, pad, None, None, want_pack)
        out, idx, mean, invstd = res[:4]
        ctx.save_for_backward(x, idx, mean, invstd, gamma, beta)
        ctx.pool = (ks, stride, pad)
        if want_pack:
            xpk, mpk = res[4], res[5]
            ctx.mark_non_differentiable(xpk, mpk)
            return out, xpk, mpk
        dummy = out.new_empty(0)
        ctx.mark_non_differentiable(dummy)
        return out, dummy, dummy

    @staticmethod
    def backward(ctx, dy, _gxpk=None, _gmpk=None):
        x, idx, mean, invstd, gamma, beta = ctx.saved_tensors
        ks, stride, pad = ctx.pool
        dx, dgamma, dbeta = _C.native_required().bn_relu_maxpool_bwd(
            dy, idx, x, mean, invstd, gamma, beta, ks, stride, pad)
        return (dx, dgamma, dbeta, None, None, None, None, None, None,
                None, None)


def fused_bn_relu_maxpool(x, bn: nn.BatchNorm2d, pool, pack=False):
    """pool(relu(bn(x))) — the ImageNet stem tail.

    One fused op when bn is training with grad enabled, x is a CUDA 4-D
    tensor with C a power of two in [8, 1024], and pool is a
    FusedMaxPool2d; every other case (eval, no_grad, CPU, any other pool
    module) is the composition ``pool(fused_bn_act(x, bn, "relu"))``.

    pack=True: returns (out, (xp, mp) | None) like fused_bn_act — the
    consuming binary conv's bitplanes of the pooled output, produced only
    by the fused path with C % 32 == 0."""
    if (bn.training and torch.is_grad_enabled() and tensor_vec8_supported(x)
            and isinstance(pool, FusedMaxPool2d) and _C.has_native()):
        C = x.size(1)
        if bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        want_pack = bool(pack) and C % 32 == 0
        out, xpk, mpk = _BNReluPoolFn.apply(
            x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
            bn.momentum if bn.momentum is not None else 0.1, bn.eps,
            pool.kernel_size, pool.stride, pool.padding, want_pack)
        if pack:
            return out, ((xpk, mpk) if want_pack else None)
        return out
    out = pool(fused_bn_act(x, bn, "relu"))
    return (out, None) if pack else out


def fused_bn_act(x, bn: nn.BatchNorm2d, act=None, skip=None, stats=None,
                 pack=False, defer_skip_cell=None):
    """BN(x) (+skip) then act.  act: None | ChannelPReLU | 'relu' | RPReLU
    (fused only with BDBNN_FUSE_RPRELU=1; any other module runs unfused
    after BN+add).

    stats: optional (sum, sumsq) per channel of x, pre-accumulated by the
    producing conv's epilogue — skips BN's own stats read pass.

    pack=True: also return the consuming binary conv's (sign, mask)
    bitplanes, packed in the epilogue (the conv then skips its own pack
    read pass).  Returns (out, (xp, mp) | None); only the fused training
    path with C % 32 == 0 produces a pack — callers must handle None."""
    b1 = b2 = None
    if isinstance(act, ChannelPReLU):
        act_kind, a = _ACT_PRELU, act.weight
    elif (_FUSE_RPRELU and isinstance(act, RPReLU)
          and tensor_vec8_supported(x) and _C.has_native()):
        act_kind, a = _ACT_RPRELU, act.prelu.weight
        b1, b2 = act.move1.bias, act.move2.bias
    elif act == "relu":
        act_kind, a = _ACT_RELU, None
    elif act is None:
        act_kind, a = _ACT_NONE, None
    else:  # generic module: apply unfused after BN+add
        out = fused_bn_act(x, bn, None, skip, stats=stats,
                           defer_skip_cell=defer_skip_cell)
        out = act(out)
        return (out, None) if pack else out

    use_fused = tensor_vec8_supported(x) and _C.has_native()
    C = x.size(1) if use_fused else 0
    if use_fused and bn.training:
        if bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        s1, s2 = stats if stats is not None else (None, None)
        want_pack = bool(pack) and C % 32 == 0
        out, xpk, mpk = _BNActFn.apply(
            x, skip, bn.weight, bn.bias, a, bn.running_mean, bn.running_var,
            bn.momentum if bn.momentum is not None else 0.1, bn.eps,
            act_kind, True, s1, s2, want_pack, defer_skip_cell, b1, b2)
        if pack:
            return out, ((xpk, mpk) if want_pack else None)
        return out
    if use_fused and not torch.is_grad_enabled() \
            and bn.running_mean is not None:
        nat = _C.native_required()
        out = nat.bn_act_eval(x, skip, bn.weight, bn.bias, a,
                              bn.running_mean, bn.running_var, bn.eps,
                              act_kind, b1, b2)
        return (out, None) if pack else out

    # composition fallback (CPU / oracle)
    z = bn(x)
    if skip is not None:
        z = z + skip
    if act_kind in (_ACT_PRELU, _ACT_RPRELU):
        out = act(z)
    elif act_kind == _ACT_RELU:
        out = F.relu(z)
    else:
        out = z
    return (out, None) if pack else out
