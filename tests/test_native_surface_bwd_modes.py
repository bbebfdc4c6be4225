"""The value-mask dgrad op (ReAct-polynomial / EDE backward) must be part
of the built extension's surface — checked on a CPU-only machine too,
like tests/test_native_surface.py."""

import pytest


def test_native_extension_exposes_conv_dgrad2_x():
    _native = pytest.importorskip("bdbnn_amd._native")
    assert hasattr(_native, "conv_dgrad2_x")
    # the clip-STE entry point and the shared shape predicate stay
    assert hasattr(_native, "conv_dgrad2")
    assert hasattr(_native, "dgrad2_supported")
