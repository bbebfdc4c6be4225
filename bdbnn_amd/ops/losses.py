"""Fused classification losses (K4 logit-KD, K6 cross-entropy) over
(B, C) logits — csrc/loss.hip; exact reference semantics
(ref:utils/KD_loss.py:10-43, ref:train.py:318)."""

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _C


def native_logits(logits):
    """True when the loss.hip kernels take these logits: a (B, C) CUDA
    tensor in fp32 or bf16, the two types they have a template for.  Any
    other dtype (fp16, fp64) goes to the torch formula; the binding
    raises on it, since it would be read as fp32."""
    return (logits.is_cuda and logits.dim() == 2
            and logits.dtype in (torch.float32, torch.bfloat16)
            and _C.has_native())


def _scale_grad(ds, g):
    """ds * g for the 0-dim fp32 upstream gradient g, formed in fp32: torch
    would round g itself to a bf16 ds's type before the product."""
    if ds.dtype == torch.float32:
        return ds * g
    return (ds.float() * g).to(ds.dtype)


class _LogitKDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t):
        nat = _C.native_required()
        out, stats, tc = nat.kd_logit_fwd(s, t)
        ctx.save_for_backward(s, tc, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        s, tc, stats = ctx.saved_tensors
        ds = _C.native_required().kd_logit_bwd(s, tc, stats, 1.0)
        return _scale_grad(ds, g), None


def fused_logit_kd(stud_logits, teacher_logits):
    """mean_n(-sum_c softmax(t) * log_softmax(s)); differentiable wrt s."""
    return _LogitKDFn.apply(stud_logits, teacher_logits)


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, y):
        nat = _C.native_required()
        out, stats = nat.ce_fwd(s, y)
        ctx.save_for_backward(s, y, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        s, y, stats = ctx.saved_tensors
        ds = _C.native_required().ce_bwd(s, y, stats, 1.0)
        return _scale_grad(ds, g), None


class FusedCrossEntropy(nn.Module):
    """nn.CrossEntropyLoss(mean) with a fused HIP kernel on the GPU."""

    def forward(self, logits, target):
        if (native_logits(logits) and target.dtype == torch.long
                and target.dim() == 1):
            return _CEFn.apply(logits, target)
        return F.cross_entropy(logits, target)
