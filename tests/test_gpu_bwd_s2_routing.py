"""Routing of the stride-2 binary convs (3x3/s2/p1, 1x1/s2/p0) through
BinaryConvFunction.backward onto the owned parity kernels
(conv_dgrad2_s2 / conv_wgrad2_s2), and the BDBNN_MFMA_BWD_S2 knob."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops import binary_conv as bc
from bdbnn_amd.ops.binary_conv import BinaryConvFunction


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


# (act_mode, t, k, maximum of the mask)
MODES = [("ste", None, None, 1.0), ("approx", None, None, 2.0),
         ("ste", 1.0, 1.0, 1.0)]
MODE_IDS = ["ste", "approx", "ede"]
# (kernel size, padding)
KSP = [(3, 1), (1, 0)]
KSP_IDS = ["3x3", "1x1"]


def _raiser(name):
    def f(*a, **kw):
        raise AssertionError(f"{name} called on the owned backward path")
    return f


def _count(monkeypatch, name):
    nat = _nat()
    real = getattr(nat, name)
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(nat, name, counted)
    return calls


def _fwd_bwd(act, t, k, ks, pad, dtype=torch.bfloat16, C=64, seed=71):
    torch.manual_seed(seed)
    x = _cl(torch.randn(2, C, 14, 14, device="cuda", dtype=dtype))
    w = torch.randn(64, C, ks, ks, device="cuda")
    xl = x.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    out, _, _ = BinaryConvFunction.apply(xl, wl, 2, pad, act, t, k, False)
    (out.float() * torch.randn_like(out.float())).sum().backward()
    torch.cuda.synchronize()
    return xl.grad, wl.grad


@pytest.mark.parametrize("ks,pad", KSP, ids=KSP_IDS)
@pytest.mark.parametrize("act,t,k,mx", MODES, ids=MODE_IDS)
def test_stride2_backward_takes_owned_path(monkeypatch, act, t, k, mx, ks,
                                           pad):
    nat = _nat()
    for name in ("decode_packed", "binsign_decode", "weight_decode",
                 "mask_mul_packed"):
        monkeypatch.setattr(nat, name, _raiser(name))
    calls = _count(monkeypatch, "conv_dgrad2_s2")
    wcalls = _count(monkeypatch, "conv_wgrad2_s2")
    xcalls = _count(monkeypatch, "conv_dgrad2_x")
    dx, dw = _fwd_bwd(act, t, k, ks, pad)
    assert len(calls) == 1 and len(wcalls) == 1 and len(xcalls) == 0
    assert dx.shape == (2, 64, 14, 14) and dw.shape == (64, 64, ks, ks)
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all()


@pytest.mark.parametrize("ks,pad", KSP, ids=KSP_IDS)
@pytest.mark.parametrize("act,t,k,mx", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("why", ["knob_s2_off", "knob_bwd_off", "fp32",
                                 "c32"])
def test_stride2_backward_fallback_cases(monkeypatch, why, act, t, k, mx, ks,
                                         pad):
    calls = _count(monkeypatch, "conv_dgrad2_s2")
    kw = {}
    if why == "knob_s2_off":
        monkeypatch.setattr(bc, "_MFMA_BWD_S2", False)
    elif why == "knob_bwd_off":
        monkeypatch.setattr(bc, "_MFMA_BWD", False)
    elif why == "fp32":
        kw["dtype"] = torch.float32
    else:
        kw["C"] = 32
    dx, dw = _fwd_bwd(act, t, k, ks, pad, **kw)
    assert len(calls) == 0
    assert dx is not None and dw is not None
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all()


@pytest.mark.parametrize("ks,pad", KSP, ids=KSP_IDS)
@pytest.mark.parametrize("act,t,k,mx", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N,C,H,K", [(2, 64, 28, 128), (2, 128, 14, 256)])
def test_stride2_backward_owned_vs_knob_off(monkeypatch, N, C, H, K, act, t,
                                            k, mx, ks, pad):
    """dx and dw of the owned path vs the BDBNN_MFMA_BWD_S2=0 path, at the
    tolerances of test_value_mask_backward_owned_vs_fallback."""
    torch.manual_seed(74)
    x = _cl(torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16))
    w = torch.randn(K, C, ks, ks, device="cuda")
    calls = _count(monkeypatch, "conv_dgrad2_s2")

    def run(flag):
        monkeypatch.setattr(bc, "_MFMA_BWD_S2", flag)
        torch.manual_seed(75)
        xl = x.clone().requires_grad_(True)
        wl = w.clone().requires_grad_(True)
        out, _, _ = BinaryConvFunction.apply(xl, wl, 2, pad, act, t, k,
                                             False)
        (out.float() * torch.randn_like(out.float())).sum().backward()
        return xl.grad.float(), wl.grad.float()
    # the deep 3x3 (C >= 128, K >= 256) is routed to the fallback by the
    # predicate itself (measured slower, benchmarks/RESULTS.md)
    want = 1 if _nat().dgrad2_s2_supported(H, H, C, K, ks) else 0
    assert want == (0 if (ks == 3 and C == 128) else 1)
    dx2, dw2 = run(True)
    assert len(calls) == want
    dx1, dw1 = run(False)
    assert len(calls) == want
    print(f"dx max diff {(dx2 - dx1).abs().max().item():.4g}, "
          f"dw max diff {(dw2 - dw1).abs().max().item():.4g}")
    assert torch.allclose(dx2, dx1, atol=5e-2 * mx, rtol=2e-2), \
        (dx2 - dx1).abs().max().item()
    assert torch.allclose(dw2, dw1, atol=5e-1, rtol=2e-2), \
        (dw2 - dw1).abs().max().item()


def _train_step(m):
    m = m.cuda().to(memory_format=torch.channels_last)
    x = _cl(torch.randn(8, 3, 64, 64, device="cuda"))
    y = torch.randint(0, 10, (8,), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(x)
        loss = torch.nn.functional.cross_entropy(out.float(), y)
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        assert torch.isfinite(p.grad).all(), n


@pytest.mark.parametrize("recipe", ["plain", "ede"])
def test_bf16_training_step_resnet18_stride2_convs(monkeypatch, recipe):
    """One bf16-autocast step of ResNet-18 (stride-2 inputs 16x16, 8x8 and
    4x4 at this image size), with the clip-STE bitplane mask (plain) and
    the EDE value mask.  All six stride-2 convs are shapes the kernels
    run, but dgrad2_s2_supported routes only 4 of them: the three 1x1/s2
    downsample.0 and layer2.0.conv1 (64 -> 128).  The 3x3/s2 conv1 of
    layer3.0 (128 -> 256) and layer4.0 (256 -> 512) measured 10-35% slower
    per backward than the MIOpen pipeline at batch 256
    (benchmarks/RESULTS.md), so the predicate keeps them on the fallback;
    the count returns to 6 when those two shapes are tuned."""
    from bdbnn_amd.engine.trainer import ede_inject
    from bdbnn_amd.models import imagenet as im
    torch.manual_seed(76)
    calls = _count(monkeypatch, "conv_dgrad2_s2")
    m = im.resnet18(False, num_classes=10)
    if recipe == "ede":
        ede_inject(m, 10, 100)
    _train_step(m)
    print(f"{recipe}: conv_dgrad2_s2 calls = {len(calls)}")
    assert len(calls) == 4


def test_bf16_training_step_resnet18_react_stride2_convs(monkeypatch):
    """resnet18_react takes the stride-2 path 0 times under bf16 autocast:
    RPReLU's fp32 shift parameters (LearnableBias) promote every block
    output to fp32, so the inputs of layer{2,3,4}.0 — each fed by the
    previous stage's last block — are fp32 and miss the bf16 predicate.
    Those six convs keep the fp32 fallback, as they did before (see the
    "Binary conv backward" section of ARCHITECTURE.md)."""
    from bdbnn_amd.models import imagenet as im
    torch.manual_seed(77)
    calls = _count(monkeypatch, "conv_dgrad2_s2")
    _train_step(im.resnet18_react(False, num_classes=10))
    print(f"react: conv_dgrad2_s2 calls = {len(calls)}")
    assert len(calls) == 0


def test_downsampling_block_owned_vs_knob_off(monkeypatch):
    """BiBasicBlock(64 -> 128, stride 2) with its 1x1/s2 downsample, bf16
    autocast: conv1 and downsample.0 on the owned stride-2 kernels vs the
    knob-off path."""
    from bdbnn_amd.models import resnet_common as rc
    from bdbnn_amd.ops.binary_conv import HardBinaryConv
    torch.manual_seed(78)
    ds = rc.FusedDownsample(HardBinaryConv(64, 128, 1, 2, 0),
                            torch.nn.BatchNorm2d(128))
    blk = rc.BiBasicBlock(64, 128, stride=2, downsample=ds).cuda().to(
        memory_format=torch.channels_last)
    x0 = torch.randn(2, 64, 14, 14, device="cuda", dtype=torch.bfloat16)
    gout = torch.randn(2, 128, 7, 7, device="cuda", dtype=torch.bfloat16)
    calls = _count(monkeypatch, "conv_dgrad2_s2")

    def run(flag):
        monkeypatch.setattr(bc, "_MFMA_BWD_S2", flag)
        blk.zero_grad(set_to_none=True)
        x = _cl(x0.clone()).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = blk(x)
        if isinstance(out, tuple):
            out = out[0]
        out.backward(_cl(gout))
        return ([p.grad.clone() for p in blk.parameters()], x.grad.clone())

    pg_o, xg_o = run(True)
    assert len(calls) == 2
    pg_f, xg_f = run(False)
    assert len(calls) == 2
    err = (xg_o.float() - xg_f.float()).abs().max().item()
    print(f"input grad max diff {err:.4g}")
    assert torch.allclose(xg_o.float(), xg_f.float(), atol=3e-2,
                          rtol=2e-2), err
    for a, b in zip(pg_o, pg_f):
        rel = (a.float() - b.float()).norm() / (b.float().norm() + 1e-12)
        assert rel.item() < 0.05, rel.item()
