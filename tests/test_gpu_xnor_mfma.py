"""The i8 MFMA binary conv forward (csrc/xnor_conv_mfma.hip) against the
XNOR+popcount kernel it replaces (bit for bit) and the fp32 conv oracle."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops.binarize import binsign, weight_scale


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


# (N, C, H, W, K, ksize, stride, pad)
SHAPES = [
    (3, 64, 7, 7, 64, 3, 1, 1),        # M = 147: partial tile, tiles cross images
    (2, 64, 9, 11, 64, 3, 1, 1),       # odd, non-square
    (1, 64, 1, 1, 64, 3, 1, 1),        # 8 of 9 taps are padding
    (2, 128, 6, 6, 128, 3, 1, 1),      # two channel chunks
    (1, 512, 7, 7, 512, 3, 1, 1),      # deepest layer, 8 chunks, 8 K tiles
    (2, 64, 9, 11, 128, 3, 2, 1),      # stride 2, odd sizes
    (2, 256, 8, 8, 512, 3, 2, 1),      # stride 2, widest
    (300, 64, 4, 4, 64, 3, 1, 1),      # many images per tile
    (1, 64, 3, 70, 64, 3, 1, 1),       # rows wider than one 64-column segment
    (1, 64, 5, 131, 64, 3, 2, 1),      # the same at stride 2 (Wo = 66)
    (16, 64, 56, 56, 64, 3, 1, 1),     # more blocks than CUs: XCD remap
]


def _inputs(shape, seed=1):
    N, C, H, W, K, ks, stride, pad = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, C, H, W, device="cuda", generator=g)
    w = torch.randn(K, C, ks, ks, device="cuda", generator=g) * 0.5
    return x, w


def _packed(x, w):
    nat = _nat()
    xp = nat.sign_pack_nhwc(_cl(x))
    wp, alpha, stab = nat.weight_pack(w)
    return xp, wp, alpha, stab


def _ref(x, w, stride, pad):
    return F.conv2d(binsign(x), weight_scale(w) * binsign(w), None,
                    stride=stride, padding=pad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mfma_equals_valu_and_matches_reference(shape):
    N, C, H, W, K, ks, stride, pad = shape
    nat = _nat()
    assert nat.xnor_mfma_supported(C, K, ks, ks, stride, pad)
    x, w = _inputs(shape)
    xp, wp, alpha, stab = _packed(x, w)
    for bf16 in (False, True):
        new = nat.xnor_conv_mfma_fwd(xp, wp, alpha, C, stride, pad, bf16)
        old = nat.xnor_conv_valu_fwd(xp, wp, alpha, stab, C, stride, pad,
                                     bf16, False)[0]
        assert new.dtype == (torch.bfloat16 if bf16 else torch.float32)
        assert new.shape == old.shape
        assert torch.equal(new, old), \
            (new.float() - old.float()).abs().max().item()
        if not bf16:
            ref = _ref(x, w, stride, pad)
            assert new.shape == ref.shape
            assert torch.allclose(_cl(new), _cl(ref), atol=1e-3, rtol=1e-4), \
                (new - ref).abs().max().item()


@pytest.mark.parametrize("stride", [1, 2])
def test_all_positive_counts_valid_taps(stride):
    """x > 0 and w > 0 everywhere: an output is alpha * C * (valid taps),
    9C in the interior — zero padding needs no correction."""
    nat = _nat()
    N, C, H, W, K = 2, 64, 9, 11, 64
    x = torch.rand(N, C, H, W, device="cuda") + 0.1
    w = torch.rand(K, C, 3, 3, device="cuda") + 0.1
    xp, wp, alpha, stab = _packed(x, w)
    out = nat.xnor_conv_mfma_fwd(xp, wp, alpha, C, stride, 1, False)
    taps = F.conv2d(torch.ones(1, 1, H, W, device="cuda"),
                    torch.ones(1, 1, 3, 3, device="cuda"), None, stride, 1)
    want = alpha.view(1, K, 1, 1) * (C * taps)
    assert taps.max().item() == 9 and taps.min().item() == 4
    assert torch.equal(out, _cl(want.expand_as(out)))


def test_single_flip_moves_nine_outputs():
    """One channel of one pixel changes sign: exactly the 9 neighbouring
    outputs of every channel k move, each by 2 * alpha_k."""
    nat = _nat()
    N, C, H, W, K = 2, 128, 8, 8, 64
    x, w = _inputs((N, C, H, W, K, 3, 1, 1), seed=5)
    n0, c0, y0, x0 = 1, 77, 3, 4
    x2 = x.clone()
    x2[n0, c0, y0, x0] = -x2[n0, c0, y0, x0]
    xp, wp, alpha, stab = _packed(x, w)
    xp2 = nat.sign_pack_nhwc(_cl(x2))
    a = nat.xnor_conv_mfma_fwd(xp, wp, alpha, C, 1, 1, False)
    b = nat.xnor_conv_mfma_fwd(xp2, wp, alpha, C, 1, 1, False)
    d = b - a
    moved = d != 0
    assert moved.sum().item() == 9 * K
    assert moved[n0, :, y0 - 1:y0 + 2, x0 - 1:x0 + 2].all()
    # the dot product moves by exactly 2; alpha * int rounds once per side
    want = (2 * alpha).view(1, K, 1, 1).expand(1, K, 3, 3)
    got = d[n0:n0 + 1, :, y0 - 1:y0 + 2, x0 - 1:x0 + 2].abs()
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("shape", [
    (2, 16, 8, 8, 64, 3, 1, 1),        # C = 16
    (2, 48, 8, 8, 64, 3, 1, 1),        # C = 48
    (2, 96, 8, 8, 64, 3, 1, 1),        # C = 96
    (2, 64, 8, 8, 96, 3, 1, 1),        # K = 96
    (2, 64, 8, 8, 64, 5, 1, 2),        # 5x5
    (2, 64, 8, 8, 64, 3, 1, 0),        # 3x3 without padding
    (2, 64, 8, 8, 64, 3, 1, 2),        # 3x3 with pad 2
], ids=lambda s: "x".join(map(str, s)))
def test_unsupported_shapes_stay_on_the_valu_kernel(shape):
    N, C, H, W, K, ks, stride, pad = shape
    nat = _nat()
    assert not nat.xnor_mfma_supported(C, K, ks, ks, stride, pad)
    x, w = _inputs(shape, seed=9)
    xp, wp, alpha, stab = _packed(x, w)
    with pytest.raises(RuntimeError):
        nat.xnor_conv_mfma_fwd(xp, wp, alpha, C, stride, pad, False)
    before = nat.xnor_route_calls()
    out = nat.xnor_conv_fwd(xp, wp, alpha, stab, C, stride, pad, False,
                            False)[0]
    after = nat.xnor_route_calls()
    assert after[0] == before[0] and after[1] == before[1] + 1
    ref = _ref(x, w, stride, pad)
    assert torch.allclose(_cl(out), _cl(ref), atol=1e-3, rtol=1e-4), \
        (out - ref).abs().max().item()
