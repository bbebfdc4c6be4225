"""The stride-2 MFMA backward's entry points (csrc/conv_bwd_s2.hip) must
be part of the built extension — checked on a CPU-only machine too, where
a source file missing from setup.py would otherwise only show up as an
undefined symbol on the GPU box."""

import pytest


EXPECTED_S2 = [
    "dgrad2_s2_supported", "conv_dgrad2_s2", "repack_cplane_s2",
    "conv_wgrad2_s2",
    # siblings: 1x1 weight decode, finish for ks*ks in {1, 9} taps
    "dgrad_weight_decode_1x1", "wgrad_finish_s2",
]


def test_native_extension_exposes_stride2_backward():
    _native = pytest.importorskip("bdbnn_amd._native")
    missing = [n for n in EXPECTED_S2 if not hasattr(_native, n)]
    assert not missing, missing


def test_stride2_shape_predicate_needs_no_gpu():
    """The routing predicate is pure host code: H, W are the INPUT size."""
    _native = pytest.importorskip("bdbnn_amd._native")
    if not hasattr(_native, "dgrad2_s2_supported"):
        pytest.fail("dgrad2_s2_supported missing")
    ok = _native.dgrad2_s2_supported
    for ks in (3, 1):
        assert ok(56, 56, 64, 128, ks)
        assert ok(7, 7, 64, 64, ks) and ok(10, 14, 64, 128, ks)
        assert ok(64, 64, 64, 64, ks) and ok(200, 64, 64, 64, ks)
        assert not ok(14, 66, 64, 64, ks)      # W > 64
        assert not ok(14, 14, 96, 64, ks)      # C % 64
        assert not ok(14, 14, 64, 32, ks)      # K % 64
    assert not ok(14, 14, 64, 64, 5)           # kernel size
    # measured slower than the fallback: deep 3x3 stays unrouted
    assert not ok(28, 28, 128, 256, 3) and not ok(14, 14, 256, 512, 3)
    assert ok(28, 28, 128, 256, 1) and ok(18, 18, 128, 64, 3)
