"""conv_wgrad3 (csrc/conv_wgrad3.hip): the stride-1 3x3 weight gradient
from the NHWC sign plane, against an fp64 weight gradient of (sign(x), g)
computed on the CPU.

Shapes are (N, C, H, W, K), the smallest that reach every branch: one per
padded-width class, W < WP, H % RB != 0 with odd N, odd slot counts where
two bands share a chunk, C != K, a single chunk, per ring class one
height at which every block walks its plane ring round at least twice
(C = K = 512 makes the m-split 4, so 4 x 6..9 chunks are enough), and two
shapes that leave a block WITHOUT a chunk: the m-split is clamped to the
chunk count, so that needs ceil(chunks / split) * (split - 1) >= chunks.
(5,512,8,14,512) has 5 chunks over 4 blocks of 2, block 3 would start at
chunk 6; (18,512,7,7,512) has 9 chunks (two images each) over 4 blocks of
3, block 3 starts at chunk 9.  Such a block must still write a zero slab:
the slabs are allocated uninitialised."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops import binary_conv as bc
from bdbnn_amd.ops.binary_conv import BinaryConvFunction


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


SHAPES = [
    (2, 64, 56, 56, 64),       # WP 64 / RB 2
    (2, 128, 28, 28, 128),     # WP 32 / RB 4
    (2, 256, 14, 14, 256),     # WP 16 / RB 8
    (4, 512, 7, 7, 512),       # WP 8 / RB 8, two bands per chunk
    (1, 64, 9, 9, 64),         # W < WP
    (3, 64, 30, 30, 64),       # H % RB != 0, odd N
    (1, 512, 7, 7, 512),       # odd slot count, two bands per chunk
    (3, 512, 7, 7, 512),
    (1, 64, 8, 8, 128),        # C != K
    (1, 128, 8, 8, 64),
    (1, 64, 4, 4, 64),         # one chunk
    (5, 512, 8, 14, 512),      # WP 16: 5 chunks, split 4: block 3 has none
    (18, 512, 7, 7, 512),      # WP 8: 9 chunks, split 4: block 3 has none
    # ring wraps: chunks per block x RB planes >= 2 x ring (2 RB + 4)
    (1, 512, 72, 33, 512),     # WP 64: 9 chunks x 2 = 18 >= 16
    (1, 512, 112, 17, 512),    # WP 32: 7 x 4 = 28 >= 24
    (1, 512, 192, 9, 512),     # WP 16: 6 x 8 = 48 >= 40
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _ref_dw(x, g):
    """fp64 dw[K][C][3][3] of (sign(x), g) on the CPU, sign(0) = +1"""
    N, C, H, W = x.shape
    K = g.shape[1]
    s = torch.where(x.cpu() >= 0, 1.0, -1.0).double()
    sp = F.pad(s, (1, 1, 1, 1)).permute(0, 2, 3, 1)      # [N][H+2][W+2][C]
    G = g.cpu().double().permute(0, 2, 3, 1).reshape(-1, K)
    out = torch.empty(K, C, 3, 3, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            S = sp[:, dy:dy + H, dx:dx + W, :].reshape(-1, C)
            out[:, :, dy, dx] = G.t() @ S
    return out


_CASES = {}


def _case(shape):
    """inputs and references of a shape, computed once for all tests"""
    if shape not in _CASES:
        N, C, H, W, K = shape
        gen = torch.Generator().manual_seed(1000 + sum(shape))
        x = torch.randn(N, C, H, W, generator=gen).bfloat16()
        g_int = torch.randint(-3, 4, (N, K, H, W), generator=gen).bfloat16()
        g_rnd = torch.randn(N, K, H, W, generator=gen).bfloat16()
        xd = _cl(x.cuda())
        _CASES[shape] = dict(
            xp=_nat().sign_pack_nhwc(xd),
            g_int=_cl(g_int.cuda()), g_rnd=_cl(g_rnd.cuda()),
            ref_int=_ref_dw(x, g_int), ref_rnd=_ref_dw(x, g_rnd),
            # sum_m |g[m, k]|, fp64
            absg=g_rnd.double().abs().sum(dim=(0, 2, 3)))
    return _CASES[shape]


def _kc33(dwT):
    """sum of the slabs [nslab][9][C][K] in [K][C][3][3] order"""
    C, K = dwT.shape[2], dwT.shape[3]
    return dwT.sum(0).permute(2, 1, 0).reshape(K, C, 3, 3)


def _bound(shape, absg):
    """fp32 summation bound per k: n * 2^-24 * sum_m |g[m, k]|"""
    N, C, H, W, K = shape
    return (N * H * W) * 2.0 ** -24 * absg.view(K, 1, 1, 1)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wgrad3_exact_on_integer_g(shape):
    """g integer in [-3, 3]: every partial sum is an integer below 2^24,
    so any accumulation order is exact"""
    N, C, H, W, K = shape
    c = _case(shape)
    # the slabs come from an uninitialised allocation: leave NaNs in the
    # block the caching allocator hands out next, so a word the kernel
    # does not write cannot pass as a zero
    poison = _nat().conv_wgrad3(c["g_int"], c["xp"], C)
    poison.fill_(float("nan"))
    del poison
    dwT = _nat().conv_wgrad3(c["g_int"], c["xp"], C)
    assert dwT.shape[1:] == (9, C, K) and dwT.dtype == torch.float32
    assert torch.isfinite(dwT).all(), "a slab was not (fully) written"
    got = _kc33(dwT).cpu().double()
    bad = (got != c["ref_int"]).sum().item()
    assert torch.equal(got, c["ref_int"]), f"{bad} of {got.numel()} differ"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wgrad3_random_g_within_fp32_sum_bound(shape):
    N, C, H, W, K = shape
    nat = _nat()
    c = _case(shape)
    bound = _bound(shape, c["absg"])
    dwT = nat.conv_wgrad3(c["g_rnd"], c["xp"], C)
    assert torch.isfinite(dwT).all(), "a slab was not (fully) written"
    old = nat.conv_wgrad2(c["g_rnd"], nat.repack_cplane(c["xp"], C, W), C)
    assert dwT.shape == old.shape
    r3 = ((_kc33(dwT).cpu().double() - c["ref_rnd"]).abs() / bound).max()
    r2 = ((_kc33(old).cpu().double() - c["ref_rnd"]).abs() / bound).max()
    print(f"{shape}: max err/bound wgrad3 {r3.item():.3g}, "
          f"wgrad2 {r2.item():.3g}")
    assert r3.item() <= 1.0
    assert r2.item() <= 1.0, "the bound must be reachable by wgrad2 too"


def test_wgrad3_predicate_and_rejection():
    nat = _nat()
    for (C, K, W) in [(96, 64, 14), (64, 32, 14), (64, 64, 65)]:
        assert not nat.wgrad3_supported(14, W, C, K)
        g = _cl(torch.zeros(1, K, 14, W, device="cuda",
                            dtype=torch.bfloat16))
        xp = torch.zeros(1, 14, W, (C + 31) // 32, device="cuda",
                         dtype=torch.int32)
        with pytest.raises(RuntimeError, match="conv_wgrad3"):
            nat.conv_wgrad3(g, xp, C)
    # a sign plane that does not belong to g
    g = _cl(torch.zeros(1, 64, 14, 14, device="cuda", dtype=torch.bfloat16))
    xp = torch.zeros(1, 14, 13, 2, device="cuda", dtype=torch.int32)
    with pytest.raises(RuntimeError, match="conv_wgrad3"):
        nat.conv_wgrad3(g, xp, 64)


# (act_mode, t, k)
MODES = [("ste", None, None), ("approx", None, None), ("ste", 1.0, 1.0)]
MODE_IDS = ["ste", "approx", "ede"]


@pytest.mark.parametrize("act,t,k", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N,C,H,W", [(2, 64, 16, 16), (2, 128, 8, 8)])
def test_binary_conv_function_knob_on_vs_off(monkeypatch, N, C, H, W, act,
                                             t, k):
    """out and dx are the same code on either setting (torch.equal); dw of
    each setting is within the fp32 summation bound of the fp64 weight
    gradient of (sign(x), g), masked by |w| <= 1."""
    nat = _nat()
    torch.manual_seed(300 + C)
    x = _cl(torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16))
    w = torch.randn(C, C, 3, 3, device="cuda")
    gout = _cl(torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16))
    calls = {}
    for name in ("conv_wgrad3", "conv_wgrad2"):
        real = getattr(nat, name)
        calls[name] = []

        def counted(*a, _r=real, _c=calls[name], **kw):
            _c.append(1)
            return _r(*a, **kw)
        monkeypatch.setattr(nat, name, counted)

    def run(knob):
        monkeypatch.setattr(bc, "_WGRAD3", knob)
        xl = x.clone().requires_grad_(True)
        wl = w.clone().requires_grad_(True)
        out, _, _ = BinaryConvFunction.apply(xl, wl, 1, 1, act, t, k, False)
        out.backward(gout)
        torch.cuda.synchronize()
        return out.detach(), xl.grad, wl.grad

    out1, dx1, dw1 = run(True)
    routed = bool(nat.wgrad3_supported(H, W, C, C))
    assert (len(calls["conv_wgrad3"]), len(calls["conv_wgrad2"])) == (
        (1, 0) if routed else (0, 1))
    out0, dx0, dw0 = run(False)
    assert len(calls["conv_wgrad2"]) == (1 if routed else 2)
    assert torch.equal(out1, out0) and torch.equal(dx1, dx0)
    mask = (w.abs() <= 1).cpu().double()
    ref = _ref_dw(x, gout) * mask
    absg = gout.cpu().double().abs().sum(dim=(0, 2, 3))
    bound = _bound((N, C, H, W, C), absg)
    for name, dw in (("on", dw1), ("off", dw0)):
        assert dw.dtype == torch.float32
        r = ((dw.cpu().double() - ref).abs() / bound).max().item()
        print(f"knob {name}: max err/bound {r:.3g}")
        assert r <= 1.0, name
