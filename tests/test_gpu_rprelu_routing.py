"""What BDBNN_FUSE_RPRELU=1 unlocks for the ReAct models under bf16
autocast: block activations stay bf16, the BN epilogue hands the next conv
its sign plane, and every binary conv the ChannelPReLU ResNet-18 runs on
the owned MFMA backward (conv_dgrad2_x stride 1, conv_dgrad2_s2 stride 2)
runs there for resnet18_react too.  Knob off: the routing on record in
test_gpu_bwd_modes.py / test_gpu_bwd_s2_routing.py (fp32 activations)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.models import resnet_common as rc
from bdbnn_amd.ops import bn_act
from bdbnn_amd.ops.binary_conv import HardBinaryConv_react, _HardBinaryConvBase


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _count(monkeypatch, name):
    nat = _nat()
    real = getattr(nat, name)
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(nat, name, counted)
    return calls


def _react_block():
    torch.manual_seed(90)
    blk = rc.BiBasicBlock(64, 64, conv_cls=HardBinaryConv_react,
                          act="rprelu").cuda().to(
        memory_format=torch.channels_last)
    with torch.no_grad():   # shifts and slopes that are not their init
        for act in (blk.act1, blk.act2):
            act.move1.bias.uniform_(-0.3, 0.3)
            act.move2.bias.uniform_(-0.3, 0.3)
            act.prelu.weight.uniform_(-0.2, 0.6)
    x = _cl(torch.randn(2, 64, 14, 14, device="cuda", dtype=torch.bfloat16))
    return blk, x


def test_react_block_knob_on_stays_bf16_and_hands_the_pack_on(monkeypatch):
    monkeypatch.setattr(bn_act, "_FUSE_RPRELU", True)
    blk, x0 = _react_block()
    packs = _count(monkeypatch, "sign_pack_nhwc")
    dgrad = _count(monkeypatch, "conv_dgrad2_x")
    # conv2's prepack, as the conv sees it
    seen = {}
    real_fws = blk.conv2.forward_with_stats

    def spy(x, prepack=None, skip_cell=None):
        seen["prepack"] = prepack
        return real_fws(x, prepack=prepack, skip_cell=skip_cell)
    monkeypatch.setattr(blk.conv2, "forward_with_stats", spy)

    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        res = blk(x)
    assert isinstance(res, tuple) and len(res) == 2
    out, pack = res
    assert out.dtype == torch.bfloat16 and out.shape == x.shape
    assert pack is not None and pack[0].shape == (2, 14, 14, 2)
    assert torch.equal(pack[0], _nat().sign_pack_nhwc(out.detach()))
    packs.clear()   # the line above is this test's own call
    assert seen["prepack"] is not None
    # conv1 packs the block input itself (no producer here); conv2 must not
    with torch.autocast("cuda", dtype=torch.bfloat16):
        blk(x0.clone())
    assert len(packs) == 1, "conv2 packed its input despite the prepack"

    out.backward(_cl(torch.randn_like(out)))
    torch.cuda.synchronize()
    assert len(dgrad) == 2, "both stride-1 convs on conv_dgrad2_x"
    assert x.grad is not None and torch.isfinite(x.grad).all()
    for n, p in blk.named_parameters():
        assert p.grad is not None, n
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype, n
        assert torch.isfinite(p.grad).all(), n
    # the shifts' and slopes' gradients are real numbers, not zeros
    for act in (blk.act1, blk.act2):
        for p in act.parameters():
            assert p.grad.abs().sum() > 0


def test_react_block_knob_off_is_fp32_as_before(monkeypatch):
    monkeypatch.setattr(bn_act, "_FUSE_RPRELU", False)
    blk, x0 = _react_block()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x0.clone().requires_grad_(True))
    assert isinstance(out, torch.Tensor)
    assert out.dtype == torch.float32


def test_react_block_knob_on_close_to_knob_off(monkeypatch):
    """fp32, no autocast: both paths compute the same function, so the
    fused block output is the composition's to fp32 accumulation noise
    (1e-4 relative to the output's scale: ~100 fp32 roundings of O(1)
    values per element through two BN tails)."""
    blk, x0 = _react_block()
    x0 = x0.float()
    gout = _cl(torch.randn_like(x0))
    outs, grads = [], []
    for knob in (True, False):
        monkeypatch.setattr(bn_act, "_FUSE_RPRELU", knob)
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        res = blk(x)
        out = res[0] if isinstance(res, tuple) else res
        out.backward(gout)
        outs.append(out.detach())
        grads.append([x.grad] + [p.grad.clone() for p in blk.parameters()])
    err = (outs[0] - outs[1]).abs().max().item()
    scale = outs[1].abs().max().item()
    print(f"fp32 block, knob on vs off: max diff {err:.3g} at scale "
          f"{scale:.3g}")
    # a sign flip of a conv2 input at |x| ~ 1e-7 changes one output by
    # O(alpha); none is expected at 25 k elements, and the bound says so
    assert err <= 1e-4 * scale, (err, scale)
    # every gradient (input, conv weights, BN, shifts, slopes), by norm:
    # the same fp32 formulas summed in another order; 1e-3 leaves room for
    # the conv2 input sitting within 1e-6 of a breakpoint of the polynomial
    # STE mask (slope 2 there, so the mask itself moves by ~2e-6)
    names = ["x"] + [n for n, _ in blk.named_parameters()]
    rels = {n: ((a - b).norm() / (b.norm() + 1e-12)).item()
            for n, a, b in zip(names, grads[0], grads[1])}
    print("grad rel. diff: " + " ".join(f"{n}:{v:.2g}"
                                        for n, v in rels.items()))
    for n, v in rels.items():
        assert v <= 1e-3, (n, v)


def _stride2_supported_count(model, x):
    """how many of the model's stride-2 binary convs dgrad2_s2_supported
    routes, from the input shapes the convs really see"""
    nat = _nat()
    want = []
    wrapped_mods = []
    # the blocks call conv.forward_with_stats, not forward: wrap that
    for mod in model.modules():
        if isinstance(mod, _HardBinaryConvBase) and mod.stride == 2:
            def wrapped(xin, *a, _m=mod, _r=mod.forward_with_stats, **kw):
                want.append(bool(nat.dgrad2_s2_supported(
                    xin.shape[2], xin.shape[3], _m.in_channels,
                    _m.out_channels, _m.kernel_size)))
                return _r(xin, *a, **kw)
            mod.forward_with_stats = wrapped
            wrapped_mods.append(mod)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model(x)
    for mod in wrapped_mods:
        del mod.forward_with_stats
    return sum(want), len(want)


def test_resnet18_react_knob_on_routes_like_the_prelu_model(monkeypatch):
    """One bf16-autocast step of resnet18_react at 8x3x64x64: all 13
    stride-1 3x3 binary convs on conv_dgrad2_x (the ChannelPReLU model's
    count in test_gpu_bwd_modes.py) and as many stride-2 convs on
    conv_dgrad2_s2 as dgrad2_s2_supported admits (4 of 6 for the
    ChannelPReLU model in test_gpu_bwd_s2_routing.py)."""
    from bdbnn_amd.models import imagenet as im
    monkeypatch.setattr(bn_act, "_FUSE_RPRELU", True)
    torch.manual_seed(91)
    m = im.resnet18_react(False, num_classes=10).cuda().to(
        memory_format=torch.channels_last)
    x = _cl(torch.randn(8, 3, 64, 64, device="cuda"))
    y = torch.randint(0, 10, (8,), device="cuda")
    m.eval()    # shape survey: leaves the running stats alone
    n_s2, n_s2_all = _stride2_supported_count(m, x)
    m.train()
    assert n_s2_all == 6 and 0 < n_s2 <= 6
    n_s1 = sum(1 for mod in m.modules()
               if isinstance(mod, _HardBinaryConvBase)
               and (mod.kernel_size, mod.stride, mod.padding) == (3, 1, 1))
    assert n_s1 == 13
    s1 = _count(monkeypatch, "conv_dgrad2_x")
    s2 = _count(monkeypatch, "conv_dgrad2_s2")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(x)
        loss = F.cross_entropy(out.float(), y)
    loss.backward()
    torch.cuda.synchronize()
    print(f"react, knob on: conv_dgrad2_x calls = {len(s1)}, "
          f"conv_dgrad2_s2 calls = {len(s2)} (predicate admits {n_s2})")
    assert torch.isfinite(loss)
    assert len(s1) == n_s1
    assert len(s2) == n_s2
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        assert torch.isfinite(p.grad).all(), n


def test_short_training_run_descends_knob_on_and_off(monkeypatch):
    """CIFAR-stem ReAct ResNet-18 on one fixed synthetic batch of 32 at
    32x32, 30 SGD steps under bf16 autocast, knob on and knob off from one
    seed: each run ends below its own starting loss.  Both curves are
    printed; no cross-run threshold.  Plain SGD at lr 0.01: the real fc
    layer on top of +-1 feature maps takes large steps, and at lr 0.05
    with momentum both runs (and the CPU composition) climb to a loss of
    ~30 before they come back."""
    curves = {}
    for knob in (True, False):
        monkeypatch.setattr(bn_act, "_FUSE_RPRELU", knob)
        torch.manual_seed(92)
        m = rc.resnet18_bi(conv_cls=HardBinaryConv_react, act="rprelu",
                           stem="cifar", num_classes=10).cuda().to(
            memory_format=torch.channels_last)
        x = _cl(torch.randn(32, 3, 32, 32, device="cuda"))
        y = torch.randint(0, 10, (32,), device="cuda")
        opt = torch.optim.SGD(m.parameters(), lr=0.01)
        losses = []
        for _ in range(30):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = F.cross_entropy(m(x).float(), y)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        curves[knob] = losses
        print(f"knob {'on ' if knob else 'off'}: "
              + " ".join(f"{v:.3f}" for v in losses))
    for knob, losses in curves.items():
        assert all(v == v and abs(v) != float("inf") for v in losses), knob
        assert losses[-1] < losses[0], (knob, losses[0], losses[-1])
