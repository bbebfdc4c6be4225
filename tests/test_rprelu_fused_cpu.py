"""RPReLU's home (ops/activations.py), its checkpoint layout, the
BDBNN_FUSE_RPRELU knob's latch, and the fused-path selection rules that
need no GPU: on CPU tensors the knob changes nothing, and the block's
pack/fuse flag follows (knob, activation type)."""

import pytest
import torch
import torch.nn as nn

from bdbnn_amd.models import resnet_common as rc
from bdbnn_amd.ops import activations, bn_act
from bdbnn_amd.ops.activations import ChannelPReLU
from bdbnn_amd.ops.binary_conv import HardBinaryConv_react


def test_rprelu_is_one_class_in_both_modules():
    assert activations.RPReLU is rc.RPReLU
    assert bn_act.RPReLU is activations.RPReLU
    assert activations.RPReLU.__module__ == "bdbnn_amd.ops.activations"
    assert isinstance(rc._make_act("rprelu", 16), activations.RPReLU)


def test_knob_is_latched_off_by_default():
    import os
    assert isinstance(bn_act._FUSE_RPRELU, bool)
    if "BDBNN_FUSE_RPRELU" not in os.environ:
        assert bn_act._FUSE_RPRELU is False
    assert bn_act._ACT_RPRELU == 3


def test_react_block_state_dict_names_and_shapes():
    blk = rc.BiBasicBlock(16, 16, conv_cls=HardBinaryConv_react, act="rprelu")
    sd = blk.state_dict()
    for act in ("act1", "act2"):
        want = {f"{act}.move1.bias": (1, 16, 1, 1),
                f"{act}.prelu.weight": (16,),
                f"{act}.move2.bias": (1, 16, 1, 1)}
        got = {k: tuple(v.shape) for k, v in sd.items()
               if k.startswith(act + ".")}
        assert got == want
        assert all(sd[k].dtype == torch.float32 for k in want)


def _rprelu(C, seed):
    g = torch.Generator().manual_seed(seed)
    act = activations.RPReLU(C)
    with torch.no_grad():
        act.move1.bias.copy_(torch.rand(1, C, 1, 1, generator=g) - 0.5)
        act.prelu.weight.copy_(torch.rand(C, generator=g) - 0.4)
        act.move2.bias.copy_(torch.rand(1, C, 1, 1, generator=g) - 0.5)
    return act


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("with_skip", [False, True], ids=["noskip", "skip"])
def test_cpu_knob_on_equals_the_composition(monkeypatch, train, with_skip):
    """CPU tensors never reach the fused path: with the knob on, out and
    every gradient are torch.equal to bn -> (+skip) -> move1 -> prelu ->
    move2 written out by hand, and pack=True yields no pack."""
    monkeypatch.setattr(bn_act, "_FUSE_RPRELU", True)
    C = 16
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, C, 5, 5, generator=g)
    s0 = torch.randn(2, C, 5, 5, generator=g) if with_skip else None
    dy = torch.randn(2, C, 5, 5, generator=g)

    def make():
        bn = nn.BatchNorm2d(C).train(train)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C))
            bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
            bn.running_mean.copy_(torch.linspace(-1, 1, C))
            bn.running_var.copy_(torch.linspace(0.5, 2, C))
        x = x0.clone().requires_grad_(True)
        s = None if s0 is None else s0.clone().requires_grad_(True)
        return bn, _rprelu(C, 4), x, s

    bn, act, x, s = make()
    out, pk = bn_act.fused_bn_act(x, bn, act, skip=s, pack=True)
    assert pk is None
    out.backward(dy)

    bn2, act2, x2, s2 = make()
    z = bn2(x2)
    if s2 is not None:
        z = z + s2
    want = act2.move2(act2.prelu(act2.move1(z)))
    want.backward(dy)

    assert torch.equal(out, want)
    assert torch.equal(x.grad, x2.grad)
    if with_skip:
        assert torch.equal(s.grad, s2.grad)
    for (n, p), (_, q) in zip(
            list(bn.named_parameters()) + list(act.named_parameters()),
            list(bn2.named_parameters()) + list(act2.named_parameters())):
        assert p.grad is not None and p.grad.shape == p.shape, n
        assert torch.equal(p.grad, q.grad), n
    assert torch.equal(bn.running_var, bn2.running_var)
    # without pack the same call returns the bare tensor
    bn3, act3, x3, s3 = make()
    assert torch.equal(bn_act.fused_bn_act(x3, bn3, act3, skip=s3), want)


@pytest.mark.parametrize("knob,act,want", [
    (False, "prelu", True), (True, "prelu", True),
    (False, "rprelu", False), (True, "rprelu", True),
    (False, "relu", False), (True, "relu", False),
], ids=lambda v: str(v))
def test_block_fuse_flag_table(monkeypatch, knob, act, want):
    """(knob, act type) -> does the block ask fused_bn_act for a pack"""
    monkeypatch.setattr(bn_act, "_FUSE_RPRELU", knob)
    mod = rc._make_act(act, 16)
    assert rc._act_fuses_pack(mod) is want
    assert isinstance(mod, ChannelPReLU) == (act == "prelu")

    # and the block passes exactly that flag on, for both of its tails
    seen = []
    real = rc.fused_bn_act

    def spy(*a, **kw):
        seen.append(kw.get("pack"))
        return real(*a, **kw)
    monkeypatch.setattr(rc, "fused_bn_act", spy)
    blk = rc.BiBasicBlock(16, 16, conv_cls=HardBinaryConv_react, act=act)
    out = blk(torch.randn(2, 16, 6, 6))
    assert seen == [want, want]
    assert isinstance(out, torch.Tensor) and out.shape == (2, 16, 6, 6)
