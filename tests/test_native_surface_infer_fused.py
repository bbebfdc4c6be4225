"""The fused inference conv's entry points (csrc/xnor_conv_mfma.hip EPI
mode, bn_fold of csrc/bn_act.hip) must be part of the built extension, and
the engine must expose its knob — checked on a CPU-only machine too."""

import inspect

import pytest


EXPECTED = ["bn_fold", "xnor_conv_bn_act_fwd", "xnor_fused_calls"]


def test_native_extension_exposes_fused_inference_conv():
    _native = pytest.importorskip("bdbnn_amd._native")
    missing = [n for n in EXPECTED if not hasattr(_native, n)]
    assert not missing, missing
    # the launch counter is host state: readable without a GPU
    assert isinstance(_native.xnor_fused_calls(), int)


def test_packed_inference_has_fuse_parameter():
    from bdbnn_amd.engine.inference import PackedInference
    params = inspect.signature(PackedInference.__init__).parameters
    assert "fuse" in params
    assert params["fuse"].default is None      # None reads BDBNN_INFER_FUSE
    assert list(params)[:3] == ["self", "model", "dtype"]
