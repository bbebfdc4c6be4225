"""The deferred residual-skip gradient (skip_cell) on every branch of
BinaryConvFunction.backward: dx with the cell must be dx without it plus
the stashed tensor, whether the dgrad epilogue fuses the add (owned
kernels) or backward adds it after a fallback, and the cell must come back
empty."""

import pytest
import torch

from bdbnn_amd.ops.binary_conv import BinaryConvFunction


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _dx_pair(x, w, stride, pad, act, s):
    """(dx without skip_cell, dx with skip_cell={"g": s}), same gout."""
    gout = None
    dxs = []
    for cell in (None, {"g": s}):
        xl = x.clone().requires_grad_(True)
        wl = w.clone().requires_grad_(True)
        out, _, _ = BinaryConvFunction.apply(xl, wl, stride, pad, act, None,
                                             None, False, None, None, cell)
        if gout is None:
            gout = torch.randn_like(out)
        out.backward(gout)
        if cell is not None:
            assert cell == {}, "backward must pop the stashed gradient"
        dxs.append(xl.grad)
    return dxs


def test_skip_grad_cpu_exact():
    torch.manual_seed(91)
    x = torch.randn(2, 8, 9, 9)
    w = torch.randn(8, 8, 3, 3)
    s = torch.randn(2, 8, 9, 9)
    for act in ("ste", "approx"):
        base, fused = _dx_pair(x, w, 1, 1, act, s)
        assert torch.equal(fused, base + s)


def _count(monkeypatch, name):
    from bdbnn_amd import _C
    nat = _C.native_required()
    real = getattr(nat, name)
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(nat, name, counted)
    return calls


def _check_gpu(monkeypatch, marker, C, K, ks, H, stride, pad, act):
    """marker: the native call that only this branch makes (once per
    backward).  Bound: that of test_conv_dgrad2_acc_fuses_skip_grad
    (tests/test_gpu_kernels.py), the same comparison at kernel level."""
    torch.manual_seed(92)
    calls = _count(monkeypatch, marker)
    x = _cl(torch.randn(2, C, H, H, device="cuda", dtype=torch.bfloat16))
    w = torch.randn(K, C, ks, ks, device="cuda")
    s = _cl(torch.randn(2, C, H, H, device="cuda", dtype=torch.bfloat16))
    base, fused = _dx_pair(x, w, stride, pad, act, s)
    torch.cuda.synchronize()
    assert len(calls) == 2, f"{marker}: {len(calls)} calls in 2 backwards"
    want = (base.float() + s.float()).to(torch.bfloat16)
    err = (fused.float() - want.float()).abs().max().item()
    print(f"{marker} C={C} ks={ks} H={H} {act}: max err {err}")
    assert torch.allclose(fused.float(), want.float(), atol=2e-2,
                          rtol=1e-2), err


@pytest.mark.gpu
@pytest.mark.parametrize("act,marker", [("ste", "conv_dgrad2"),
                                        ("approx", "conv_dgrad2_x")])
def test_skip_grad_owned_s1(monkeypatch, act, marker):
    _check_gpu(monkeypatch, marker, 64, 64, 3, 9, 1, 1, act)


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["ste", "approx"])
@pytest.mark.parametrize("H", [14, 13])
@pytest.mark.parametrize("ks,pad", [(3, 1), (1, 0)], ids=["3x3", "1x1"])
def test_skip_grad_owned_s2(monkeypatch, ks, pad, H, act):
    _check_gpu(monkeypatch, "conv_dgrad2_s2", 64, 64, ks, H, 2, pad, act)


@pytest.mark.gpu
def test_skip_grad_packed_fallback(monkeypatch):
    _check_gpu(monkeypatch, "mask_mul_packed", 32, 64, 3, 9, 1, 1, "ste")


@pytest.mark.gpu
def test_skip_grad_value_fallback(monkeypatch):
    _check_gpu(monkeypatch, "binsign_decode", 32, 64, 3, 9, 1, 1, "approx")
