"""The entry points of the 16/32-channel stride-1 backward
(csrc/conv_bwd_small.hip) must be part of the built extension, with the
documented signatures -- checked on a CPU-only machine too, where a source
file missing from setup.py would otherwise only show up as an undefined
symbol on the GPU box."""

import pytest


EXPECTED = {
    "conv_dgrad_small": ["g", "wd", "C", "mode", "mp", "x", "t", "k", "acc"],
    "conv_wgrad_small": ["g", "xp", "C", "fold"],
    "bwd_small_supported": ["H", "W", "C", "K"],
}


def test_native_extension_exposes_bwd_small():
    _native = pytest.importorskip("bdbnn_amd._native")
    missing = [n for n in EXPECTED if not hasattr(_native, n)]
    assert not missing, missing


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_bwd_small_signatures(name):
    _native = pytest.importorskip("bdbnn_amd._native")
    if not hasattr(_native, name):
        pytest.fail(f"{name} missing")
    doc = getattr(_native, name).__doc__
    sig = doc.splitlines()[0]
    args = [a.split(":")[0].strip()
            for a in sig[sig.index("(") + 1:sig.index(")")].split(",")]
    assert args == EXPECTED[name], sig
    if name == "conv_wgrad_small":
        assert "fold: bool = True" in sig
    if name == "conv_dgrad_small":
        # acc is the one optional argument
        assert sig.count("= None") == 1 and sig.rstrip().endswith("Tensor")
        assert sig.index("acc:") < sig.index("= None")


def test_bwd_small_shape_predicate_needs_no_gpu():
    """Pure host code: 3x3/s1/p1 with C, K in {16, 32} and W <= 64."""
    _native = pytest.importorskip("bdbnn_amd._native")
    if not hasattr(_native, "bwd_small_supported"):
        pytest.fail("bwd_small_supported missing")
    ok = _native.bwd_small_supported
    assert ok(32, 32, 16, 16) and ok(16, 16, 32, 32)
    assert ok(16, 16, 16, 32) and ok(16, 16, 32, 16)
    assert not ok(16, 16, 32, 64) and not ok(16, 16, 64, 32)
    assert not ok(16, 16, 48, 48) and not ok(16, 16, 8, 16)
    assert not ok(16, 65, 16, 16) and not ok(0, 16, 16, 16)
    assert ok(H=8, W=8, C=32, K=32)


def test_dgrad_weight_decode_accepts_16_channels_on_the_host_side():
    """The argument check runs before any GPU work: a CPU tensor must fail
    on the device check, not on C % 32."""
    torch = pytest.importorskip("torch")
    _native = pytest.importorskip("bdbnn_amd._native")
    wp = torch.zeros(16, 3, 3, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="wp must be packed"):
        _native.dgrad_weight_decode(wp, torch.ones(16), 16)
