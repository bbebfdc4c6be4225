"""The wgrad3 entry points (csrc/conv_wgrad3.hip) must be part of the built
extension — checked on a CPU-only machine too, where a source file missing
from setup.py would otherwise only show up as an undefined symbol on the
GPU box."""

import pytest


EXPECTED_WGRAD3 = ["conv_wgrad3", "wgrad3_supported"]


def test_native_extension_exposes_wgrad3():
    _native = pytest.importorskip("bdbnn_amd._native")
    missing = [n for n in EXPECTED_WGRAD3 if not hasattr(_native, n)]
    assert not missing, missing


def test_wgrad3_shape_predicate_needs_no_gpu():
    """Pure host code: 3x3/s1/p1 with C % 64 == 0, K % 64 == 0, W <= 64."""
    _native = pytest.importorskip("bdbnn_amd._native")
    if not hasattr(_native, "wgrad3_supported"):
        pytest.fail("wgrad3_supported missing")
    ok = _native.wgrad3_supported
    assert not ok(14, 14, 96, 64)          # C % 64
    assert not ok(14, 14, 64, 32)          # K % 64
    assert not ok(14, 65, 64, 64)          # W > 64
    assert not ok(14, 14, 0, 64) and not ok(0, 14, 64, 64)
    # the four classes of the flagship, all routed
    for H, C in ((56, 64), (28, 128), (14, 256), (7, 512)):
        assert ok(H, H, C, C)
