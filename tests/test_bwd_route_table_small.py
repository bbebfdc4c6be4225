"""The "s1small" rows of BinaryConvFunction.backward's routing table: the
3x3/s1/p1 convs with C and K both in {16, 32} (csrc/conv_bwd_small.hip)
under the BDBNN_MFMA_BWD_SMALL knob.  Host predicates only: no GPU."""

import pytest
import torch

nat = pytest.importorskip("bdbnn_amd._native")

from bdbnn_amd.ops import binary_conv as bc

BF16, FP32 = torch.bfloat16, torch.float32

CONTEXTS = [dict(valmask=False, mask_mode=0), dict(valmask=True, mask_mode=1),
            dict(valmask=True, mask_mode=2)]
CONTEXT_IDS = ["packed", "value-approx", "value-ede"]


def _route(ctx, ks=3, stride=1, pad=1, C=16, K=16, H=32, W=None, g=BF16,
           x=BF16):
    W = H if W is None else W
    return bc._owned_route(
        nat, g_dtype=g, x_dtype=x, stride=stride, padding=pad, ks=ks,
        H_in=H, W_in=W, H_out=(H + 2 * pad - ks) // stride + 1,
        W_out=(W + 2 * pad - ks) // stride + 1, C=C, K=K, **ctx)


SMALL = [dict(C=16, K=16, H=32), dict(C=32, K=32, H=16),
         dict(C=16, K=32, H=16), dict(C=32, K=16, H=16)]
SMALL_IDS = ["16-16-32", "32-32-16", "16-32-16", "32-16-16"]

NOT_SMALL = [
    ("C32-K64", dict(C=32, K=64, H=16)),
    ("C64-K32", dict(C=64, K=32, H=16)),
    ("C48-K48", dict(C=48, K=48, H=16)),
    ("W66", dict(H=32, W=66)),
    ("fp32-g", dict(g=FP32)),
    ("fp32-x", dict(x=FP32)),
    ("3x3s2-16-32", dict(stride=2, C=16, K=32, H=32)),
    ("1x1s1", dict(ks=1, pad=0)),
    ("1x1s2-16-32", dict(ks=1, stride=2, pad=0, C=16, K=32, H=32)),
]

# the 64-channel rows of tests/test_bwd_route_table.py
BIG = [
    (dict(C=64, K=64, H=56), "s1"),
    (dict(C=64, K=64, H=56, W=66), None),
    (dict(C=64, K=64, H=9, W=8), None),
    (dict(C=64, K=64, H=56, ks=1, pad=0), None),
    (dict(C=64, K=128, H=56, stride=2), "s2"),
    (dict(C=128, K=256, H=28, ks=1, stride=2, pad=0), "s2"),
    (dict(C=128, K=256, H=28, stride=2), None),
]


def test_knob_is_on_by_default_and_read_at_import():
    assert isinstance(bc._MFMA_BWD_SMALL, bool)


@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
@pytest.mark.parametrize("conv", SMALL, ids=SMALL_IDS)
def test_small_convs_take_the_small_route(monkeypatch, ctx, conv):
    monkeypatch.setattr(bc, "_MFMA_BWD", True)
    monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", True)
    assert _route(ctx, **conv) == "s1small"


@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
@pytest.mark.parametrize("conv", [t[1] for t in NOT_SMALL],
                         ids=[t[0] for t in NOT_SMALL])
def test_everything_else_stays_unrouted(monkeypatch, ctx, conv):
    monkeypatch.setattr(bc, "_MFMA_BWD", True)
    monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", True)
    assert _route(ctx, **conv) is None


@pytest.mark.parametrize("conv", SMALL, ids=SMALL_IDS)
def test_value_context_with_bitplane_mode_is_never_owned(monkeypatch, conv):
    monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", True)
    assert _route(dict(valmask=True, mask_mode=0), **conv) is None


@pytest.mark.parametrize("knob", ["_MFMA_BWD", "_MFMA_BWD_SMALL"])
@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
@pytest.mark.parametrize("conv", SMALL, ids=SMALL_IDS)
def test_either_knob_off_routes_nothing_small(monkeypatch, ctx, conv, knob):
    monkeypatch.setattr(bc, "_MFMA_BWD", True)
    monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", True)
    monkeypatch.setattr(bc, knob, False)
    assert _route(ctx, **conv) is None


@pytest.mark.parametrize("small", [True, False], ids=["on", "off"])
@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
def test_64_channel_rows_do_not_depend_on_the_knob(monkeypatch, ctx, small):
    monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", small)
    for conv, want in BIG:
        assert _route(ctx, **conv) == want, conv


def test_predicate_admits_only_16_and_32():
    ok = nat.bwd_small_supported
    for C in (16, 32):
        for K in (16, 32):
            assert ok(32, 32, C, K) and ok(1, 1, C, K) and ok(40, 64, C, K)
            assert not ok(32, 65, C, K) and not ok(0, 8, C, K)
            assert not ok(8, 0, C, K)
    for C, K in ((64, 16), (16, 64), (48, 48), (8, 16), (32, 64), (64, 64),
                 (0, 16), (16, 24)):
        assert not ok(16, 16, C, K), (C, K)


def _resnet20_binary_convs():
    """(name, ks, stride, pad, C, K, input H) of the 20 binary convs of
    CIFAR ResNet-20 at 32x32, from the model itself"""
    from bdbnn_amd.models import cifar10
    from bdbnn_amd.ops.binary_conv import _HardBinaryConvBase
    H = {16: 32, 32: 16, 64: 8}       # input size of a stage by its width
    convs = []
    for name, m in cifar10.resnet20().named_modules():
        if isinstance(m, _HardBinaryConvBase):
            convs.append((name, m.kernel_size, m.stride, m.padding,
                          m.in_channels, m.out_channels, H[m.in_channels]))
    return convs


@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
def test_resnet20_routed_counts(monkeypatch, ctx):
    monkeypatch.setattr(bc, "_MFMA_BWD", True)
    monkeypatch.setattr(bc, "_MFMA_BWD_S2", True)
    monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", True)
    convs = _resnet20_binary_convs()
    assert len(convs) == 20
    routes = {name: _route(ctx, ks=ks, stride=s, pad=p, C=C, K=K, H=H)
              for name, ks, s, p, C, K, H in convs}
    by = {}
    for name, r in routes.items():
        by.setdefault(r, []).append(name)
    assert len(by["s1small"]) == 11 and len(by["s1"]) == 5
    assert sorted(by[None]) == ["layer2.0.conv1", "layer2.0.downsample.0",
                                "layer3.0.conv1", "layer3.0.downsample.0"]
    assert all(n.startswith(("layer1.", "layer2.")) for n in by["s1small"])
    assert all(n.startswith("layer3.") for n in by["s1"])
