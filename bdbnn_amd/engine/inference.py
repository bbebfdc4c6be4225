"""Binary inference path (BASELINE config 5): persistent packed 1-bit
weights + hipGraph-captured eval loop.

``PackedInference(model)`` snapshots every HardBinaryConv's packed
weights once (bit-pack + alpha + pad table survive across calls instead
of being recomputed per forward), switches the model to eval, and
``capture(batch_shape)`` records the whole forward into a hipGraph so
steady-state inference replays with near-zero launch overhead
(SURVEY.md K11).

With ``fuse`` on (the default, ``BDBNN_INFER_FUSE=0`` turns it off) every
BiBasicBlock whose two 3x3 convs the i8 MFMA kernel covers also runs its
BN + residual + activation tail, and the sign pack of the next conv,
inside the conv kernel's epilogue (csrc/xnor_conv_mfma.hip, EPI mode):
two launches per block, 1-bit activations handed from conv to conv.  The
outputs are bit-identical to the unfused path.
"""

import os

import torch
import torch.nn as nn

from .. import _C
from ..models.resnet_common import (BiBasicBlock, CifarResNet,
                                    FusedDownsample, ResNet, _act_fuses_pack)
from ..ops.activations import ChannelPReLU, RPReLU
from ..ops.binary_conv import _HardBinaryConvBase


def _infer_fuse_default():
    return os.environ.get("BDBNN_INFER_FUSE", "1") != "0"


class _PackedConvForward:
    """Replacement forward for HardBinaryConv in inference: cached packed
    weights, no autograd, no repack."""

    def __init__(self, conv):
        nat = _C.native_required()
        self.stride = conv.stride
        self.padding = conv.padding
        self.C = conv.in_channels
        self.wp, self.alpha, self.stab = nat.weight_pack(conv.weight.detach())

    def __call__(self, x):
        nat = _C.native_required()
        xc = x.contiguous(memory_format=torch.channels_last)
        xp = nat.sign_pack_nhwc(xc)
        return nat.xnor_conv_fwd(xp, self.wp, self.alpha, self.stab,
                                 self.C, self.stride, self.padding,
                                 x.dtype == torch.bfloat16, False)[0]


def _conv_fuses(nat, conv, bn, act):
    """conv -> bn -> (+skip) -> act as one fused launch: a conv the MFMA
    kernel covers, an eval BN that the unfused path runs on bn_act_eval
    (running stats, C a power of two <= 1024), and an activation whose
    final value that kernel writes (_act_fuses_pack)."""
    K = conv.out_channels
    return (isinstance(conv, _HardBinaryConvBase)
            and isinstance(conv.kernel_size, int)
            and nat.xnor_mfma_supported(conv.in_channels, K,
                                        conv.kernel_size, conv.kernel_size,
                                        conv.stride, conv.padding)
            and isinstance(bn, nn.BatchNorm2d)
            and bn.running_mean is not None and bn.weight is not None
            and bn.num_features == K and _vec8_channels(K)
            and _act_fuses_pack(act))


def block_fuses(block):
    """True when PackedInference(fuse=True) replaces this block's forward."""
    nat = _C.native_required()
    return (isinstance(block, BiBasicBlock)
            and _conv_fuses(nat, block.conv1, block.bn1, block.act1)
            and _conv_fuses(nat, block.conv2, block.bn2, block.act2)
            and block.conv1.out_channels == block.conv2.in_channels)


def _chan(t):
    # private fp32 [C] copy: the kernel reads it through float4 loads
    return t.detach().reshape(-1).to(torch.float32, copy=True)


class _FusedConvTail:
    """One conv + bn + act of a block, everything the launch needs folded
    once: packed weights, alpha, (sc, sh) by bn_fold, slopes and shifts."""

    def __init__(self, conv, bn, act):
        nat = _C.native_required()
        self.C = conv.in_channels
        self.stride = conv.stride
        self.padding = conv.padding
        self.wp, self.alpha, _ = nat.weight_pack(conv.weight.detach())
        self.a = self.b2 = b1 = None
        if isinstance(act, ChannelPReLU):
            self.kind, self.a = 1, _chan(act.weight)
        else:
            assert isinstance(act, RPReLU)
            self.kind, self.a = 3, _chan(act.prelu.weight)
            b1, self.b2 = _chan(act.move1.bias), _chan(act.move2.bias)
        self.sc, self.sh = nat.bn_fold(bn.weight.detach(), bn.bias.detach(),
                                       bn.running_mean, bn.running_var,
                                       bn.eps, b1)

    def __call__(self, xp, skip, want_pack):
        return _C.native_required().xnor_conv_bn_act_fwd(
            xp, self.wp, self.alpha, self.sc, self.sh, self.a, self.b2, skip,
            self.C, self.stride, self.padding, self.kind,
            skip.dtype == torch.bfloat16, want_pack)


def _vec8_channels(K):
    # what ops/_vec8.py asks of C: a power of two in [8, 1024]
    return 8 <= K <= 1024 and K & (K - 1) == 0


class _PackedDownsample:
    """downsample.0 / downsample.1 of a fused block on the plane conv1
    consumes: the kernels FusedDownsample runs in eval (xnor_conv_fwd, then
    bn_act_eval without activation), with the weights packed once and
    without a second pack of x."""

    def __init__(self, ds):
        nat = _C.native_required()
        conv, self.bn = ds[0], ds[1]
        self.C = conv.in_channels
        self.stride = conv.stride
        self.padding = conv.padding
        self.wp, self.alpha, self.stab = nat.weight_pack(conv.weight.detach())

    @staticmethod
    def covers(ds):
        return (isinstance(ds, FusedDownsample) and len(ds) == 2
                and isinstance(ds[0], _HardBinaryConvBase)
                and ds[0].in_channels % 32 == 0
                and isinstance(ds[1], nn.BatchNorm2d)
                and ds[1].running_mean is not None
                and ds[1].weight is not None
                and ds[1].num_features == ds[0].out_channels
                and _vec8_channels(ds[0].out_channels))

    def __call__(self, xp, bf16):
        nat = _C.native_required()
        bn = self.bn
        out = nat.xnor_conv_fwd(xp, self.wp, self.alpha, self.stab, self.C,
                                self.stride, self.padding, bf16, False)[0]
        return nat.bn_act_eval(out, None, bn.weight, bn.bias, None,
                               bn.running_mean, bn.running_var, bn.eps, 0,
                               None, None)


class _FusedBlockForward:
    """Replacement forward of a qualifying BiBasicBlock: two launches.
    Takes x or (x, (sign plane, _)) like the block's own forward and hands
    (out, (plane, None)) on when a fused block follows."""

    def __init__(self, block, pack_out):
        self.block = block
        self.pack_out = pack_out
        self.tail1 = _FusedConvTail(block.conv1, block.bn1, block.act1)
        self.tail2 = _FusedConvTail(block.conv2, block.bn2, block.act2)
        self.ds = (_PackedDownsample(block.downsample)
                   if _PackedDownsample.covers(block.downsample) else None)

    def __call__(self, x):
        nat = _C.native_required()
        blk = self.block
        pk_in = None
        if isinstance(x, tuple):
            x, pk_in = x
        assert x.dtype in (torch.bfloat16, torch.float32), x.dtype
        x = x.contiguous(memory_format=torch.channels_last)
        xp, _ = blk.conv1._check_prepack(x, pk_in)
        if xp is None:   # first block after the stem / after an unfused one
            xp = nat.sign_pack_nhwc(x)
        if self.ds is not None:
            # downsample.0 consumes the same plane as conv1
            identity = self.ds(xp, x.dtype == torch.bfloat16)
        elif blk.downsample is not None:
            identity = blk.downsample(x, prepack=(xp, None)).to(
                x.dtype).contiguous(memory_format=torch.channels_last)
        else:
            identity = x
        out1, p1 = self.tail1(xp, identity, True)
        out2, p2 = self.tail2(p1, out1, self.pack_out)
        return (out2, (p2, None)) if p2 is not None else out2


class PackedInference:
    """Inference wrapper: packed weights resident in HBM + hipGraph replay.

    fuse: run qualifying BiBasicBlocks as two fused conv+BN+act launches
    (bit-identical outputs); None reads BDBNN_INFER_FUSE (default on)."""

    def __init__(self, model, dtype=torch.bfloat16, fuse=None):
        assert torch.cuda.is_available(), "PackedInference needs a GPU"
        _C.native_required()
        self.dtype = dtype
        self.fuse = _infer_fuse_default() if fuse is None else bool(fuse)
        self.model = model.cuda().to(memory_format=torch.channels_last).eval()
        self._orig_forwards = {}
        for mod in self.model.modules():
            if isinstance(mod, _HardBinaryConvBase):
                packed = _PackedConvForward(mod)
                self._orig_forwards[mod] = mod.forward
                mod.forward = packed
        self.fused_blocks = []
        if self.fuse:
            # the trunks whose blocks run as one chain and whose forward
            # drops a trailing (out, pack) tuple; elsewhere a fused block
            # never hands a plane on
            chained = isinstance(self.model, (ResNet, CifarResNet))
            blocks = [m for m in self.model.modules()
                      if isinstance(m, BiBasicBlock)]
            fuses = [block_fuses(b) for b in blocks]
            for i, blk in enumerate(blocks):
                if not fuses[i]:
                    continue
                nxt = (chained and i + 1 < len(blocks) and fuses[i + 1]
                       and blocks[i + 1].conv1.in_channels
                       == blk.conv2.out_channels)
                self._orig_forwards[blk] = blk.forward
                blk.forward = _FusedBlockForward(blk, nxt)
                self.fused_blocks.append(blk)
        self.graph = None
        self._static_in = None
        self._static_out = None

    @torch.no_grad()
    def __call__(self, x):
        x = x.to("cuda", self.dtype).contiguous(
            memory_format=torch.channels_last)
        if self.graph is not None and x.shape == self._static_in.shape:
            self._static_in.copy_(x)
            self.graph.replay()
            return self._static_out
        with torch.autocast("cuda", dtype=torch.bfloat16,
                            enabled=self.dtype == torch.bfloat16):
            return self.model(x)

    @torch.no_grad()
    def capture(self, batch_shape, warmup=3):
        """Record one forward of the given shape into a hipGraph."""
        self._static_in = torch.zeros(
            batch_shape, device="cuda", dtype=self.dtype).contiguous(
            memory_format=torch.channels_last)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                with torch.autocast("cuda", dtype=torch.bfloat16,
                                    enabled=self.dtype == torch.bfloat16):
                    out = self.model(self._static_in)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            with torch.autocast("cuda", dtype=torch.bfloat16,
                                enabled=self.dtype == torch.bfloat16):
                self._static_out = self.model(self._static_in)
        return self

    def release(self):
        for mod, fwd in self._orig_forwards.items():
            mod.forward = fwd
        self._orig_forwards.clear()
        self.graph = None
