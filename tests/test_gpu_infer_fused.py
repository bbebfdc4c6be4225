"""PackedInference(fuse=True): qualifying BiBasicBlocks run as two fused
conv + BN + residual + activation launches (csrc/xnor_conv_mfma.hip EPI
mode) with the sign plane handed from conv to conv.  The logits must be
bit for bit those of the unfused engine, eagerly and from a captured
graph; the launch counter says which path a model took."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.engine import PackedInference
from bdbnn_amd.models import cifar10, imagenet
from bdbnn_amd.models import resnet_common as rc
from bdbnn_amd.ops import bn_act
from bdbnn_amd.ops.activations import ChannelPReLU, RPReLU

FP32, BF16 = torch.float32, torch.bfloat16

MODELS = {
    "resnet18_bi": (lambda: rc.resnet18_bi(num_classes=10), (2, 3, 64, 64)),
    "resnet34_bi": (lambda: rc.resnet34_bi(num_classes=10), (2, 3, 64, 64)),
    "resnet20": (lambda: cifar10.resnet20(), (2, 3, 32, 32)),
    "resnet18_react": (lambda: imagenet.resnet18_react(False),
                       (2, 3, 64, 64)),
}


def _randomised(name, seed=0):
    """The model with BN statistics, BN affine, PReLU slopes and RPReLU
    shifts away from their defaults (a default BN makes the tail an
    identity and hides errors)."""
    torch.manual_seed(seed)
    model = MODELS[name][0]()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g))
                m.running_var.copy_(10 ** (torch.rand(n, generator=g) * 2 - 1))
                m.weight.copy_(torch.randn(n, generator=g) * 0.5 + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.5)
            elif isinstance(m, ChannelPReLU):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.4)
            elif isinstance(m, RPReLU):
                for b in (m.move1.bias, m.move2.bias):
                    b.copy_(torch.randn(b.shape, generator=g) * 0.3)
    return model


def _expected_fused_convs(model):
    """Convs in qualifying blocks, from the predicates the issue names."""
    nat = _C.native_required()

    def ok(conv, act):
        return (nat.xnor_mfma_supported(
            conv.in_channels, conv.out_channels, conv.kernel_size,
            conv.kernel_size, conv.stride, conv.padding)
            and rc._act_fuses_pack(act))

    return sum(2 for b in model.modules() if isinstance(b, rc.BiBasicBlock)
               and ok(b.conv1, b.act1) and ok(b.conv2, b.act2))


def _check_model(name, dtype, expect=None):
    nat = _C.native_required()
    shape = MODELS[name][1]
    base = _randomised(name)
    n_fused = _expected_fused_convs(base)
    if expect is not None:
        assert n_fused == expect, n_fused
    g = torch.Generator().manual_seed(7)
    x1 = torch.randn(shape, generator=g).cuda()
    x2 = torch.randn(shape, generator=g).cuda()

    # the module's own eval forward, before any engine touches it
    plain = copy.deepcopy(base).cuda().to(
        memory_format=torch.channels_last).eval()
    with torch.no_grad():
        own = plain(x1.contiguous(memory_format=torch.channels_last)).clone()

    off = PackedInference(copy.deepcopy(base), dtype=dtype, fuse=False)
    c0 = nat.xnor_fused_calls()
    want1, want2 = off(x1).clone(), off(x2).clone()
    assert nat.xnor_fused_calls() == c0          # knob off: counter rests
    assert not off.fused_blocks

    on = PackedInference(plain, dtype=dtype, fuse=True)
    assert len(on.fused_blocks) * 2 == n_fused
    c0 = nat.xnor_fused_calls()
    got1 = on(x1).clone()
    assert nat.xnor_fused_calls() - c0 == n_fused
    got2 = on(x2).clone()
    assert nat.xnor_fused_calls() - c0 == 2 * n_fused
    assert torch.isfinite(got1).all()
    assert torch.equal(got1, want1), (got1 - want1).abs().max().item()
    assert torch.equal(got2, want2), (got2 - want2).abs().max().item()
    assert not torch.equal(got1, got2)

    on.capture(shape)
    rep1 = on(x1).clone()
    rep2 = on(x2).clone()
    assert torch.equal(rep1, want1), (rep1 - want1).abs().max().item()
    assert torch.equal(rep2, want2), (rep2 - want2).abs().max().item()
    assert not torch.equal(rep1, rep2)

    on.release()
    c0 = nat.xnor_fused_calls()
    with torch.no_grad():
        again = plain(x1.contiguous(memory_format=torch.channels_last))
    assert nat.xnor_fused_calls() == c0
    assert torch.equal(again, own), (again - own).abs().max().item()
    return n_fused


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_resnet18_bi_fused_equals_unfused(dtype):
    assert _check_model("resnet18_bi", dtype, expect=16) == 16


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_resnet34_bi_fused_equals_unfused(dtype):
    assert _check_model("resnet34_bi", dtype, expect=32) == 32


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_cifar_resnet20_fuses_its_64_channel_blocks_only(dtype):
    """16- and 32-channel stages and layer3.0 (conv1 has C = 32) keep the
    unfused path; layer3.1 and layer3.2 fuse."""
    assert _check_model("resnet20", dtype, expect=4) == 4


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("knob", [False, True], ids=["rprelu_off", "rprelu_on"])
def test_resnet18_react_follows_the_rprelu_knob(knob, dtype):
    """RPReLU tails fuse only with BDBNN_FUSE_RPRELU on: without it the
    unfused model keeps fp32 activations after the shifts."""
    saved = bn_act._FUSE_RPRELU
    bn_act._FUSE_RPRELU = knob
    try:
        _check_model("resnet18_react", dtype, expect=16 if knob else 0)
    finally:
        bn_act._FUSE_RPRELU = saved
