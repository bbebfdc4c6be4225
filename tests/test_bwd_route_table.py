"""The routing decision of BinaryConvFunction.backward as a table:
_owned_route over shapes, dtypes, contexts and knobs.  The predicates are
host code, so this runs without a GPU."""

import pytest
import torch

nat = pytest.importorskip("bdbnn_amd._native")

from bdbnn_amd.ops import binary_conv as bc

BF16, FP32 = torch.bfloat16, torch.float32

# the two contexts forward can save: packed clip-STE bit planes, or the fp
# activation with a value mask (ReAct polynomial 1 / EDE 2)
CONTEXTS = [dict(valmask=False, mask_mode=0), dict(valmask=True, mask_mode=1),
            dict(valmask=True, mask_mode=2)]
CONTEXT_IDS = ["packed", "value-approx", "value-ede"]


def _route(ctx, ks=3, stride=1, pad=1, C=64, K=64, H=56, W=None, g=BF16,
           x=BF16):
    W = H if W is None else W
    return bc._owned_route(
        nat, g_dtype=g, x_dtype=x, stride=stride, padding=pad, ks=ks,
        H_in=H, W_in=W, H_out=(H + 2 * pad - ks) // stride + 1,
        W_out=(W + 2 * pad - ks) // stride + 1, C=C, K=K, **ctx)


# (id, conv, expected route)
TABLE = [
    ("3x3s1-64-56", dict(), "s1"),
    ("W66", dict(H=56, W=66), None),
    ("W8-H9", dict(H=9, W=8), None),
    ("C32", dict(C=32), None),
    ("fp32-g", dict(g=FP32), None),
    ("fp32-x", dict(x=FP32), None),
    ("1x1s1", dict(ks=1, pad=0), None),
    ("3x3s2-64-128-56", dict(stride=2, K=128), "s2"),
    ("1x1s2-128-256-28", dict(ks=1, stride=2, pad=0, C=128, K=256, H=28),
     "s2"),
    ("3x3s2-128-256-28", dict(stride=2, C=128, K=256, H=28), None),
    ("3x3s2-256-512-14", dict(stride=2, C=256, K=512, H=14), None),
    ("3x3s2p0", dict(stride=2, pad=0, K=128), None),
]


@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
@pytest.mark.parametrize("conv,want", [t[1:] for t in TABLE],
                         ids=[t[0] for t in TABLE])
def test_route_table(ctx, conv, want):
    assert _route(ctx, **conv) == want


@pytest.mark.parametrize("conv", [t[1] for t in TABLE],
                         ids=[t[0] for t in TABLE])
def test_value_context_with_bitplane_mode_is_never_owned(conv):
    assert _route(dict(valmask=True, mask_mode=0), **conv) is None


@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
@pytest.mark.parametrize("conv", [t[1] for t in TABLE],
                         ids=[t[0] for t in TABLE])
def test_knob_bwd_off_routes_nothing(monkeypatch, ctx, conv):
    monkeypatch.setattr(bc, "_MFMA_BWD", False)
    assert _route(ctx, **conv) is None


@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
@pytest.mark.parametrize("conv,want", [t[1:] for t in TABLE],
                         ids=[t[0] for t in TABLE])
def test_knob_s2_off_keeps_stride1(monkeypatch, ctx, conv, want):
    monkeypatch.setattr(bc, "_MFMA_BWD_S2", False)
    assert _route(ctx, **conv) == (None if want == "s2" else want)


# every binary conv of the ImageNet ResNet-18 at 224x224 (the stem and the
# FC are real-valued): (name, ks, stride, pad, C, K, input H)
def _resnet18_binary_convs():
    convs = []
    H = 56
    for li, (C, K) in enumerate([(64, 64), (64, 128), (128, 256),
                                 (256, 512)], start=1):
        s = 1 if li == 1 else 2
        convs.append((f"layer{li}.0.conv1", 3, s, 1, C, K, H))
        if s == 2:
            convs.append((f"layer{li}.0.downsample", 1, 2, 0, C, K, H))
            H //= 2
        convs.append((f"layer{li}.0.conv2", 3, 1, 1, K, K, H))
        convs.append((f"layer{li}.1.conv1", 3, 1, 1, K, K, H))
        convs.append((f"layer{li}.1.conv2", 3, 1, 1, K, K, H))
    return convs


@pytest.mark.parametrize("ctx", CONTEXTS, ids=CONTEXT_IDS)
def test_resnet18_routed_counts(ctx):
    """The counts ARCHITECTURE.md states for a bf16 ResNet-18."""
    convs = _resnet18_binary_convs()
    routes = {name: _route(ctx, ks=ks, stride=s, pad=p, C=C, K=K, H=H)
              for name, ks, s, p, C, K, H in convs}
    s1 = [n for n, ks, s, p, C, K, H in convs if s == 1]
    s2 = [n for n, ks, s, p, C, K, H in convs if s == 2]
    assert len(s1) == 13 and len(s2) == 6
    assert all(routes[n] == "s1" for n in s1)
    fallback = sorted(n for n in s2 if routes[n] is None)
    assert fallback == ["layer3.0.conv1", "layer4.0.conv1"]
    assert sum(routes[n] == "s2" for n in s2) == 4
