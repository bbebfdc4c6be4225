"""1-bit (1W/1A) convolution modules — the compute core of BD-BNN.

The reference's ``models`` package (HardBinaryConv / HardBinaryConv_react /
HardBinaryConv_cifar) is missing from its snapshot; the module contract is
reconstructed from call sites (ref:train.py:30-32,392,
ref:utils/KD_loss.py:6-7,60):

* expose a 4-D ``weight`` nn.Parameter (latent fp weights — kurtosis and
  layer-KD read it directly),
* forward = conv(sign(x), alpha * sign(W)) with straight-through backward,
* accept per-epoch EDE (t, k) injection as module attributes,
* first conv + final FC of a model stay real-valued.

GPU path (CUDA tensors): bit-packed XNOR+popcount convolution via the
in-tree HIP extension (csrc/xnor_conv.hip), activations packed on the fly
(csrc/pack.hip), backward as hand-written MFMA-bf16 dgrad/wgrad
(csrc/conv_bwd.hip) with the clip-STE / ReAct / EDE mask fused into the
dgrad epilogue on stride-1 3x3 bf16 convs; elsewhere dense conv on the
decoded +-1 operands (MIOpen) with separate mask kernels.  Requires NHWC
(channels_last) activations and C % 32 == 0 for the packed path; the
engine puts models in channels_last.

CPU path: the pure-PyTorch oracle (also the numerics reference for the
kernels' tests).
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .binarize import binsign, weight_scale
from .. import _C

_CONV_STATS = os.environ.get("BDBNN_CONV_STATS", "0") == "1"
# hand-written MFMA backward kernels (default ON; BDBNN_MFMA_BWD=0 falls
# back to MIOpen igemm on decoded operands for A/B comparison)
_MFMA_BWD = os.environ.get("BDBNN_MFMA_BWD", "1") != "0"
# the stride-2 kernels of that backward (3x3/s2/p1 and 1x1/s2/p0,
# csrc/conv_bwd_s2.hip) alone: BDBNN_MFMA_BWD_S2=0 sends just those convs
# back to the MIOpen path while stride 1 stays on the owned kernels
_MFMA_BWD_S2 = os.environ.get("BDBNN_MFMA_BWD_S2", "1") != "0"
# the stride-1 weight gradient straight from the NHWC sign plane
# (csrc/conv_wgrad3.hip, default ON); BDBNN_WGRAD3=0 keeps repack_cplane +
# conv_wgrad2, its A/B partner
_WGRAD3 = os.environ.get("BDBNN_WGRAD3", "1") != "0"
# the 16/32-channel stride-1 kernels of that backward (the first two stages
# of CIFAR ResNet-20, csrc/conv_bwd_small.hip) alone: BDBNN_MFMA_BWD_SMALL=0
# sends just those convs back to the MIOpen path
_MFMA_BWD_SMALL = os.environ.get("BDBNN_MFMA_BWD_SMALL", "1") != "0"


def _act_grad_mask(x: torch.Tensor, mode: str, t, k) -> torch.Tensor:
    """d sign(x) / dx surrogate used by the backward pass (matches binarize.py)."""
    if t is not None and k is not None:
        th = torch.tanh(float(t) * x)
        return float(k) * float(t) * (1.0 - th * th)
    if mode == "approx":
        neg = (x >= -1) & (x < 0)
        pos = (x >= 0) & (x < 1)
        g = torch.zeros_like(x)
        g = torch.where(neg, 2.0 + 2.0 * x, g)
        g = torch.where(pos, 2.0 - 2.0 * x, g)
        return g
    return (x.abs() <= 1).to(x.dtype)


def _owned_route(nat, *, g_dtype, x_dtype, stride, padding, ks, H_in, W_in,
                 H_out, W_out, C, K, mask_mode, valmask):
    """Which owned MFMA backward runs a binary conv: "s1" (3x3/s1/p1,
    csrc/conv_bwd.hip), "s1small" (3x3/s1/p1 with C and K in {16, 32},
    csrc/conv_bwd_small.hip), "s2" (3x3/s2/p1 and 1x1/s2/p0,
    csrc/conv_bwd_s2.hip) or None (MIOpen on decoded operands).  The whole
    routing decision: knobs, dtypes, geometry, and the native shape
    predicates.  ks is the
    (square) kernel size; a value-mask context that carries the clip-STE
    mask (mask_mode 0) has no owned kernel."""
    if not _MFMA_BWD or (valmask and mask_mode == 0):
        return None
    if g_dtype != torch.bfloat16 or x_dtype != torch.bfloat16:
        return None
    if (ks, stride, padding) == (3, 1, 1):
        if nat.dgrad2_supported(H_out, W_out, C, K):
            return "s1"
        if _MFMA_BWD_SMALL and nat.bwd_small_supported(H_out, W_out, C, K):
            return "s1small"
        return None
    if _MFMA_BWD_S2 and stride == 2 and (ks, padding) in ((3, 1), (1, 0)):
        return "s2" if nat.dgrad2_s2_supported(H_in, W_in, C, K, ks) else None
    return None


def _owned_backward(nat, route, g, w, xp, wp, alpha, C, mode, mp, x, t, k,
                    acc):
    """The owned backward of either route and either mask kind (mode 0:
    bitplane mp; 1/2: value mask of the saved activation x).  dgrad: halo
    (s1) / parity-phase (s2) implicit GEMM with the mask and the deferred
    skip grad, if any, in its epilogue.  wgrad: all-tap block GEMM straight
    from the sign BITS (the dense +-1 activation is never materialized):
    stride 1 reads the NHWC sign plane as saved (conv_wgrad3,
    conv_wgrad_small), stride 2 and the BDBNN_WGRAD3=0 path a per-channel
    repack of it; then slab sum + transpose + |w|<=1 mask in one pass."""
    s2 = route == "s2"
    H, W, ks = xp.shape[1], xp.shape[2], w.shape[2]
    wd = (nat.dgrad_weight_decode_1x1 if ks == 1
          else nat.dgrad_weight_decode)(wp, alpha, C)
    if s2:
        dx = nat.conv_dgrad2_s2(g, wd, H, W, C, mode, mp, x, t, k, acc)
        planes = nat.repack_cplane_s2(xp, C, H, W)
        dwT = nat.conv_wgrad2_s2(g, planes, C, H, W, ks)
        dw = nat.wgrad_finish_s2(dwT, w.float())
    elif route == "s1small":
        dx = nat.conv_dgrad_small(g, wd, C, mode, mp, x, t, k, acc)
        dwT = nat.conv_wgrad_small(g, xp, C)
        dw = nat.wgrad_finish(dwT, w.float())
    else:
        dx = (nat.conv_dgrad2(g, wd, mp, C, acc) if mode == 0
              else nat.conv_dgrad2_x(g, wd, x, C, mode, t, k, acc))
        if _WGRAD3 and nat.wgrad3_supported(H, W, C, w.shape[0]):
            dwT = nat.conv_wgrad3(g, xp, C)
        else:
            planes = nat.repack_cplane(xp, C, W)
            dwT = nat.conv_wgrad2(g, planes, C)
        dw = nat.wgrad_finish(dwT, w.float())
    return dx, dw


def _conv_backward(g, xb, wb, stride, padding):
    return torch.ops.aten.convolution_backward(
        g, xb, wb, None, [stride, stride], [padding, padding], [1, 1], False,
        [0, 0], 1, [True, True, False])[:2]


def _packed_fallback(nat, g, w, xp, mp, wp, alpha, C, x_dtype, stride,
                     padding):
    """MIOpen on operands decoded from the bit planes, separate mask
    kernels; g is channels_last."""
    bf16 = g.dtype == torch.bfloat16
    xb = nat.decode_packed(xp, C, bf16)
    wb = nat.weight_decode(wp, alpha, C, bf16)
    dxb, dwb = _conv_backward(g, xb, wb, stride, padding)
    dx = nat.mask_mul_packed(dxb, mp, C, x_dtype == torch.bfloat16)
    return dx, nat.ste_mask_mul(dwb, w, 0, 0.0, 0.0)


def _value_fallback(g, x, w, stride, padding, act_mode, t, k):
    """Dense conv on +-1 operands decoded from the saved activation, then
    the activation-gradient mask of x: native kernels on the GPU (g is
    channels_last there), the pure-torch oracle on the CPU."""
    if not x.is_cuda:
        dxb, dwb = _conv_backward(g, binsign(x), weight_scale(w) * binsign(w),
                                  stride, padding)
        return (dxb * _act_grad_mask(x, act_mode, t, k),
                dwb * (w.abs() <= 1).to(w.dtype))
    nat = _C.native_required()
    # decode +-1 operands in the compute dtype for the dense MFMA pass
    xb = nat.binsign_decode(x, 1 if g.dtype == torch.bfloat16 else 0)
    wb = (weight_scale(w) * binsign(w)).to(g.dtype)
    dxb, dwb = _conv_backward(g, xb, wb, stride, padding)
    if t is not None and k is not None:
        mode_id, t, k = 2, float(t), float(k)
    else:
        mode_id, t, k = {"ste": 0, "approx": 1}[act_mode], 0.0, 0.0
    return (nat.ste_mask_mul(dxb, x, mode_id, t, k),
            nat.ste_mask_mul(dwb, w, 0, 0.0, 0.0))


class BinaryConvFunction(torch.autograd.Function):
    """Fused 1W/1A conv: XNOR+popcount forward, dense-MFMA backward.

    forward:  out = conv2d(sign(x), alpha * sign(w), stride, padding)
    backward: dx = conv_dgrad(g, alpha*sign(w)) * act_mask(x)
              dw = conv_wgrad(sign(x), g) * 1(|w| <= 1)
    (alpha = per-out-channel mean|W|, detached.)
    """

    @staticmethod
    def forward(ctx, x, w, stride, padding, act_mode, t, k,
                want_stats=False, xp_pre=None, mp_pre=None, skip_cell=None):
        ctx.stride = stride
        ctx.padding = padding
        ctx.act_mode = act_mode
        ctx.t = t
        ctx.k = k
        ctx.packed = False
        ctx.valmask = False
        # deferred residual-skip gradient: the consuming BN's backward
        # (which runs first) stashes its dskip here instead of returning
        # it, and this conv's dgrad adds it in the epilogue — removing
        # autograd's separate grad-accumulation pass over dx
        ctx.skip_cell = skip_cell
        if x.is_cuda:
            nat = _C.native_required()
            wp, alpha, stab = nat.weight_pack(w)  # bits, alpha[K], S[K][T]
            # (grad mode is always off inside Function.forward; use
            # needs_input_grad to detect inference/no-grad calls)
            if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
                # inference/validation: no mask plane, nothing saved
                xp = (xp_pre if xp_pre is not None else nat.sign_pack_nhwc(
                    x.contiguous(memory_format=torch.channels_last)))
                ctx.packed = None  # backward must never run
            elif act_mode == "ste" and t is None:
                # packed fast path: sign + clip-STE mask bitplanes (either
                # pre-packed by the producing BN's epilogue, or in one
                # pass here); the fp activations are NOT saved — backward
                # works entirely from the 1-bit planes (32x less read
                # traffic)
                if xp_pre is not None and mp_pre is not None:
                    xp, mp = xp_pre, mp_pre
                else:
                    xp, mp = nat.sign_mask_pack_nhwc(
                        x.contiguous(memory_format=torch.channels_last))
                ctx.packed = True
                ctx.x_dtype = x.dtype
                ctx.in_channels = x.shape[1]
                ctx.save_for_backward(w, xp, mp, wp, alpha)
            else:
                # value-mask modes (ReAct polynomial / EDE): the mask
                # depends on the value of x, so the fp activation IS
                # saved (channels_last, the copy made for packing) next
                # to the tiny sign plane / packed weights that the owned
                # MFMA backward consumes.  The kernel reads x at dx's
                # NHWC address, so the saved copy is channels_last even
                # when xp_pre spares the pack: free for the engine's
                # channels_last tensors (contiguous() returns x itself),
                # one layout copy per forward for an NCHW caller — the
                # copy the fallback's decode/mask ops made in backward
                x_cl = x.contiguous(memory_format=torch.channels_last)
                xp = (xp_pre if xp_pre is not None
                      else nat.sign_pack_nhwc(x_cl))
                ctx.valmask = True
                if t is not None and k is not None:
                    ctx.mask_mode, ctx.mask_t, ctx.mask_k = (
                        2, float(t), float(k))
                else:
                    ctx.mask_mode, ctx.mask_t, ctx.mask_k = (
                        {"ste": 0, "approx": 1}[act_mode], 0.0, 0.0)
                ctx.save_for_backward(w, xp, x_cl, wp, alpha)
            res = nat.xnor_conv_fwd(
                xp, wp, alpha, stab, x.shape[1], stride, padding,
                x.dtype == torch.bfloat16, want_stats)
            if want_stats:
                # per-channel (sum, sumsq) of the output, accumulated in
                # the conv epilogue — consumed by the fused BN (its stats
                # pass is skipped entirely)
                ctx.mark_non_differentiable(res[1], res[2])
                return res[0], res[1], res[2]
            dummy = res[0].new_empty(0)
            ctx.mark_non_differentiable(dummy)
            return res[0], dummy, dummy
        ctx.save_for_backward(x, w)
        xb = binsign(x)
        wb = weight_scale(w) * binsign(w)
        out = F.conv2d(xb, wb, None, stride=stride, padding=padding)
        dummy = out.new_empty(0)
        ctx.mark_non_differentiable(dummy)
        return out, dummy, dummy

    @staticmethod
    def backward(ctx, g, _gs1=None, _gs2=None):
        stride, padding = ctx.stride, ctx.padding
        acc = ctx.skip_cell.pop("g", None) if ctx.skip_cell else None
        if ctx.packed or ctx.valmask:
            nat = _C.native_required()
            if ctx.packed:
                w, xp, mp, wp, alpha = ctx.saved_tensors
                x, x_dtype, C = None, ctx.x_dtype, ctx.in_channels
                mode, t, k = 0, 0.0, 0.0
            else:
                w, xp, x, wp, alpha = ctx.saved_tensors
                mp, x_dtype, C = None, x.dtype, x.shape[1]
                mode, t, k = ctx.mask_mode, ctx.mask_t, ctx.mask_k
            g = g.contiguous(memory_format=torch.channels_last)
            route = _owned_route(
                nat, g_dtype=g.dtype, x_dtype=x_dtype, stride=stride,
                padding=padding,
                ks=w.shape[2] if w.shape[2] == w.shape[3] else 0,
                H_in=xp.shape[1], W_in=xp.shape[2], H_out=g.shape[2],
                W_out=g.shape[3], C=C, K=w.shape[0], mask_mode=mode,
                valmask=ctx.valmask)
            if route:
                dx, dw = _owned_backward(nat, route, g, w, xp, wp, alpha, C,
                                         mode, mp, x, t, k, acc)
                acc = None  # added in the dgrad epilogue
            elif ctx.packed:
                dx, dw = _packed_fallback(nat, g, w, xp, mp, wp, alpha, C,
                                          x_dtype, stride, padding)
            else:
                dx, dw = _value_fallback(g, x, w, stride, padding,
                                         ctx.act_mode, ctx.t, ctx.k)
        else:
            x, w = ctx.saved_tensors
            dx, dw = _value_fallback(g, x, w, stride, padding, ctx.act_mode,
                                     ctx.t, ctx.k)
        if acc is not None:
            dx = dx + acc.to(dx.dtype)
        return (dx, dw.to(w.dtype)) + (None,) * 9


class _HardBinaryConvBase(nn.Module):
    """Shared implementation; subclasses fix the activation-STE default."""

    act_mode = "ste"

    def __init__(self, in_chn, out_chn, kernel_size=3, stride=1, padding=1):
        super().__init__()
        self.in_channels = in_chn
        self.out_channels = out_chn
        self.kernel_size = kernel_size
        self.stride = stride
        self.padding = padding
        self.weight = nn.Parameter(
            torch.empty(out_chn, in_chn, kernel_size, kernel_size))
        # ReActNet-style init scale for latent binary weights
        nn.init.normal_(self.weight, mean=0.0, std=0.1)
        # EDE schedule attrs, injected per-epoch by the engine (ref:train.py:412-415)
        self.t = None
        self.k = None

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, "
                f"kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, act={self.act_mode}")

    def _apply(self, fn, recurse=True):
        # keep the latent weight NCHW-contiguous even when the model is
        # converted to channels_last: only our own kernels consume it
        # (pack expects NCHW) and a channels_last weight would force a
        # layout copy every step.
        super()._apply(fn, recurse)
        if not self.weight.data.is_contiguous():
            self.weight.data = self.weight.data.contiguous()
        return self

    def _check_prepack(self, x, prepack):
        """Validate a (xp, mp) pair packed by the producing BN's epilogue
        against this conv's input; returns (xp, mp) or (None, None)."""
        if prepack is None or not x.is_cuda:
            return None, None
        xp, mp = prepack
        if (xp.shape[0] == x.shape[0] and xp.shape[1] == x.shape[2]
                and xp.shape[2] == x.shape[3]
                and xp.shape[3] * 32 == self.in_channels):
            return xp, mp
        return None, None

    def forward(self, x, prepack=None, skip_cell=None):
        t = float(self.t) if self.t is not None else None
        k = float(self.k) if self.k is not None else None
        xp, mp = self._check_prepack(x, prepack)
        out, _, _ = BinaryConvFunction.apply(
            x, self.weight, self.stride, self.padding, self.act_mode, t, k,
            False, xp, mp, skip_cell)
        return out

    def forward_with_stats(self, x, prepack=None, skip_cell=None):
        """(out, (s1, s2)|None): per-out-channel sum/sumsq accumulated in
        the conv epilogue, for the fused BN that consumes the output.

        OFF by default, MEASURED twice (r1 flat-[K] atomics, r2 32-way
        sliced + LDS accumulation): any stats work in this epilogue
        costs the conv kernel 1.4-4x (profiles/, bn_bench.md r2) —
        far more than the separate bn_stats read pass it saves, which
        after the 4-deep MLP unroll costs ~0.07 ms/layer at b512.
        BDBNN_CONV_STATS=1 re-enables for experiments."""
        t = float(self.t) if self.t is not None else None
        k = float(self.k) if self.k is not None else None
        want = (x.is_cuda and self.training and _CONV_STATS)
        xp, mp = self._check_prepack(x, prepack)
        out, s1, s2 = BinaryConvFunction.apply(
            x, self.weight, self.stride, self.padding, self.act_mode, t, k,
            want, xp, mp, skip_cell)
        return out, ((s1, s2) if want else None)


class HardBinaryConv(_HardBinaryConvBase):
    """BD-BNN ImageNet binary conv (ref name: models.imagenet.resnet_bi_imagenet_set_2_2)."""
    act_mode = "ste"


class HardBinaryConv_react(_HardBinaryConvBase):
    """ReActNet-style binary conv (ref name: models.imagenet.resnet_bi_imagenet_set_2)."""
    act_mode = "approx"


class HardBinaryConv_cifar(_HardBinaryConvBase):
    """CIFAR binary conv (ref name: models.bin_module.binarized_modules)."""
    act_mode = "ste"
