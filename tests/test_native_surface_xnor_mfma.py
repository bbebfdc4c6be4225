"""The i8 MFMA forward conv's entry points (csrc/xnor_conv_mfma.hip) must
be part of the built extension — checked on a CPU-only machine too, where
a source file missing from setup.py would otherwise only show up as an
undefined symbol on the GPU box."""

import pytest


EXPECTED = ["xnor_mfma_supported", "xnor_conv_mfma_fwd", "xnor_conv_valu_fwd",
            "xnor_route_calls"]


def test_native_extension_exposes_xnor_mfma():
    _native = pytest.importorskip("bdbnn_amd._native")
    missing = [n for n in EXPECTED if not hasattr(_native, n)]
    assert not missing, missing


def test_xnor_mfma_predicate_needs_no_gpu():
    """The routing predicate is pure host code: (C, K, KH, KW, stride,
    pad)."""
    _native = pytest.importorskip("bdbnn_amd._native")
    if not hasattr(_native, "xnor_mfma_supported"):
        pytest.fail("xnor_mfma_supported missing")
    ok = _native.xnor_mfma_supported
    # the 16 3x3 convs of ResNet-18/34
    for c in (64, 128, 256, 512):
        assert ok(c, c, 3, 3, 1, 1)
    for c in (64, 128, 256):
        assert ok(c, 2 * c, 3, 3, 2, 1)
    for c in (16, 48, 96):
        assert not ok(c, 64, 3, 3, 1, 1)       # C % 64
    assert not ok(64, 96, 3, 3, 1, 1)          # K % 64
    assert not ok(64, 64, 5, 5, 1, 2)          # kernel size
    assert not ok(64, 64, 3, 3, 1, 0)          # pad
    assert not ok(64, 64, 3, 3, 1, 2)
    assert not ok(64, 64, 3, 3, 3, 1)          # stride
    assert not ok(64, 128, 1, 1, 2, 0)         # 1x1/s2 stays on the VALU kernel
    assert len(_native.xnor_route_calls()) == 2    # (MFMA, VALU) counters
