"""Owned MFMA backward for the stride-2 binary convs (3x3/s2/p1 and
1x1/s2/p0): conv_dgrad2_s2 (dx by pixel parity, mask in the epilogue),
repack_cplane_s2 + conv_wgrad2_s2 + wgrad_finish_s2 (dw from the sign bits
split by column parity).  Kernel numerics; routing is tested in
test_gpu_bwd_s2_routing.py."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops.binarize import binsign, weight_scale
from bdbnn_amd.ops.binary_conv import _act_grad_mask


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


# (ks, N, C, H, W, K): the smallest case of each failure class
SHAPES = [
    (3, 4, 64, 8, 8, 64),     # Wo=4; even sizes (zero halo); images share a block
    (3, 2, 64, 7, 7, 64),     # odd sizes, no halo
    (3, 1, 64, 14, 14, 128),  # Wo=7, dummy columns; two K chunks
    (3, 1, 128, 18, 18, 64),  # Wo=9, next width class; 2nd C tile; partial band
    (3, 3, 64, 34, 34, 64),   # Wo=17; odd N
    (3, 1, 64, 64, 64, 64),   # Wo=32, full width
    (3, 1, 64, 10, 14, 64),   # H != W
    (1, 4, 64, 8, 8, 64),     # 1x1 shortcut
    (1, 2, 64, 7, 7, 64),
    (1, 1, 128, 18, 18, 64),
    (1, 1, 64, 10, 14, 128),
]
SHAPE_IDS = [f"k{s[0]}_n{s[1]}_c{s[2]}_{s[3]}x{s[4]}_k{s[5]}" for s in SHAPES]

# (kernel mode, act_mode string, t, k)
MASKS = [
    (0, "ste", None, None),
    (1, "approx", None, None),
    (2, "ste", 0.01, 100.0),
    (2, "ste", 1.0, 1.0),
    (2, "ste", 10.0, 1.0),
]
MASK_IDS = ["ste", "approx", "ede_t0.01_k100", "ede_t1_k1", "ede_t10_k1"]

# the EDGE probes of tests/test_gpu_bwd_modes.py: the polynomial's
# half-open boundaries, both zeros, and |t*x| = 500 at t = 10
EDGE = [-1.0, -0.0, 0.0, 1.0, 0.5, -0.5, 50.0, -50.0]


def _max_mask(mode, t, k):
    return 1.0 if mode == 0 else 2.0 if mode == 1 else float(k) * float(t)


def _out_size(H, W):
    return (H + 1) // 2, (W + 1) // 2


def _dgrad_oracle(g, wb, ks, H, W):
    """fp32 conv_transpose2d with the output_padding that restores (H, W)."""
    p = 1 if ks == 3 else 0
    Ho, Wo = g.shape[2], g.shape[3]
    op = (H - ((Ho - 1) * 2 - 2 * p + ks), W - ((Wo - 1) * 2 - 2 * p + ks))
    return _cl(F.conv_transpose2d(g.float(), wb.float(), None, stride=2,
                                  padding=p, output_padding=op))


def _wgrad_oracle(g, xb, K, C, ks):
    """aten.convolution_backward in fp32 on the +-1 activation."""
    p = 1 if ks == 3 else 0
    return torch.ops.aten.convolution_backward(
        g.float(), _cl(xb.float()),
        torch.empty(K, C, ks, ks, device="cuda"), None,
        [2, 2], [p, p], [1, 1], False, [0, 0], 1,
        [False, True, False])[1]               # [K][C][ks][ks]


def _decode(nat, wp, alpha, C, ks):
    return (nat.dgrad_weight_decode(wp, alpha, C) if ks == 3
            else nat.dgrad_weight_decode_1x1(wp, alpha, C))


def _dx(nat, c, mode, t, k, acc=None):
    mp = c["mp"] if mode == 0 else None
    x = None if mode == 0 else c["x"]
    return nat.conv_dgrad2_s2(c["g"], c["wd"], c["H"], c["W"], c["C"], mode,
                              mp, x, 0.0 if t is None else t,
                              0.0 if k is None else k, acc)


@functools.lru_cache(maxsize=None)
def _case(ks, N, C, H, W, K):
    """Inputs and mask-independent references of one shape, built once and
    shared (read-only) by every test that uses the shape."""
    gen = torch.Generator(device="cuda").manual_seed(
        10000 * ks + 1000 * N + 100 * H + W + C + 7 * K)
    nat = _nat()
    Ho, Wo = _out_size(H, W)
    assert nat.dgrad2_s2_supported(H, W, C, K, ks)
    g = _cl(torch.randn(N, K, Ho, Wo, device="cuda", dtype=torch.bfloat16,
                        generator=gen))
    w = torch.randn(K, C, ks, ks, device="cuda", generator=gen)
    x = torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16,
                    generator=gen)
    probes = torch.tensor(EDGE, device="cuda", dtype=torch.bfloat16)
    x[0, :len(EDGE), 0, 0] = probes       # even row, even column
    x[0, :len(EDGE), 1, 1] = probes       # odd row, odd column
    x = _cl(x)
    skip_g = _cl(torch.randn(N, C, H, W, device="cuda",
                             dtype=torch.bfloat16, generator=gen))
    xp, mp = nat.sign_mask_pack_nhwc(x)
    wp, alpha, _ = nat.weight_pack(w)
    wd = _decode(nat, wp, alpha, C, ks)
    wb = (weight_scale(w) * binsign(w)).to(torch.bfloat16)
    ref_raw = _dgrad_oracle(g, wb, ks, H, W)
    ref_dw = _wgrad_oracle(g, binsign(x.float()), K, C, ks)
    # exact-arithmetic operands: g in {-1,0,1}, w = +-0.5, alpha = 0.5
    gi = _cl(torch.randint(-1, 2, (N, K, Ho, Wo), device="cuda",
                           generator=gen).to(torch.bfloat16))
    wh = (torch.randint(0, 2, (K, C, ks, ks), device="cuda",
                        generator=gen).float() - 0.5)
    return dict(ks=ks, N=N, C=C, H=H, W=W, K=K, g=g, w=w, x=x, xp=xp, mp=mp,
                wd=wd, skip_g=skip_g, ref_raw=ref_raw, ref_dw=ref_dw,
                gi=gi, wh=wh)


# ---------------- dgrad ----------------

@pytest.mark.parametrize("mode,act,t,k", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv_dgrad2_s2_matches_fp32_oracle(shape, mode, act, t, k):
    c = _case(*shape)
    dx = _dx(_nat(), c, mode, t, k)
    ref = c["ref_raw"] * _act_grad_mask(c["x"].float(), act, t, k)
    assert dx.shape == ref.shape and dx.dtype == torch.bfloat16
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert torch.isfinite(dx).all()
    err = (dx.float() - ref).abs().max().item()
    print(f"max abs err vs fp32 oracle: {err:.4g}")
    # the project's tolerance for the dgrad kernels; the oracle's error
    # scales with the mask, so atol is multiplied by the mode's maximum
    assert torch.allclose(dx.float(), ref, atol=0.5 * _max_mask(mode, t, k),
                          rtol=2e-2), err


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[5] == 64],
                         ids=[i for s, i in zip(SHAPES, SHAPE_IDS)
                              if s[5] == 64])
def test_conv_dgrad2_s2_exact_on_half_integers(shape):
    """g in {-1,0,1}, w = +-0.5 (alpha = 0.5 given explicitly), all-ones
    mask plane, K = 64: every dx value is a half-integer with |dx| <= 128,
    exact in bf16 — a wrong tap, phase or pad cannot hide in a tolerance."""
    ks, N, C, H, W, K = shape
    c = _case(*shape)
    nat = _nat()
    wp, _, _ = nat.weight_pack(c["wh"])
    alpha = torch.full((K,), 0.5, device="cuda")
    wd = _decode(nat, wp, alpha, C, ks)
    ones = torch.full((N, H, W, C // 32), -1, device="cuda",
                      dtype=torch.int32)
    dx = nat.conv_dgrad2_s2(c["gi"], wd, H, W, C, 0, ones, None, 0.0, 0.0)
    wb = (weight_scale(c["wh"]) * binsign(c["wh"])).to(torch.bfloat16)
    assert torch.equal(wb.float(), c["wh"])
    ref = _dgrad_oracle(c["gi"], wb, ks, H, W)
    assert ref.abs().max().item() <= 128
    nbad = (dx.float() != ref).sum().item()
    print(f"mismatching elements: {nbad}")
    assert torch.equal(dx.float(), ref), nbad


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] == 1],
                         ids=[i for s, i in zip(SHAPES, SHAPE_IDS)
                              if s[0] == 1])
@pytest.mark.parametrize("mode,act,t,k", [MASKS[0], MASKS[1], MASKS[3]],
                         ids=["ste", "approx", "ede_t1_k1"])
def test_conv_dgrad2_s2_1x1_empty_phases(shape, mode, act, t, k):
    """The three tap-less phases of the 1x1/p0 dx are written: exactly 0
    without acc, exactly acc with it — over an allocation pre-filled with
    NaN, so an unwritten pixel shows."""
    ks, N, C, H, W, K = shape
    c = _case(*shape)
    nat = _nat()

    def poison():
        junk = _cl(torch.full((N, C, H, W), float("nan"), device="cuda",
                              dtype=torch.bfloat16))
        del junk

    empty = torch.ones(H, W, dtype=torch.bool, device="cuda")
    empty[0::2, 0::2] = False
    poison()
    dx = _dx(nat, c, mode, t, k)
    assert torch.isfinite(dx).all()
    assert (dx[:, :, empty] == 0).all()
    poison()
    dxa = _dx(nat, c, mode, t, k, c["skip_g"])
    assert torch.isfinite(dxa).all()
    assert torch.equal(dxa[:, :, empty], c["skip_g"][:, :, empty])


@pytest.mark.parametrize("mode,act,t,k", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[7],
                                   SHAPES[8]],
                         ids=[SHAPE_IDS[i] for i in (0, 1, 7, 8)])
def test_conv_dgrad2_s2_acc_fuses_skip_grad(shape, mode, act, t, k):
    """acc adds the (unmasked) skip gradient in the epilogue."""
    c = _case(*shape)
    nat = _nat()
    plain = _dx(nat, c, mode, t, k)
    fused = _dx(nat, c, mode, t, k, c["skip_g"])
    want = (plain.float() + c["skip_g"].float()).to(torch.bfloat16)
    err = (fused.float() - want.float()).abs().max().item()
    print(f"max abs err fused vs separate add: {err:.4g}")
    assert torch.allclose(fused.float(), want.float(),
                          atol=2e-2 * _max_mask(mode, t, k), rtol=1e-2), err


def test_dgrad_weight_decode_1x1_values():
    torch.manual_seed(61)
    nat = _nat()
    w = torch.randn(64, 128, 1, 1, device="cuda")
    wp, alpha, _ = nat.weight_pack(w)
    wd = nat.dgrad_weight_decode_1x1(wp, alpha, 128)
    assert wd.shape == (1, 128, 64) and wd.dtype == torch.bfloat16
    want = (alpha[:, None] * binsign(w[:, :, 0, 0])).to(torch.bfloat16)
    assert torch.equal(wd[0], want.t())


# ---------------- wgrad ----------------

def _dw(nat, g, xp, C, H, W, ks):
    planes = nat.repack_cplane_s2(xp, C, H, W)
    dwT = nat.conv_wgrad2_s2(g, planes, C, H, W, ks)
    assert dwT.dim() == 4 and dwT.shape[1:] == (ks * ks, C, g.shape[1])
    assert dwT.dtype == torch.float32
    K = g.shape[1]
    return dwT, dwT.sum(0).permute(2, 1, 0).reshape(K, C, ks, ks)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv_wgrad2_s2_matches_reference(shape):
    ks, N, C, H, W, K = shape
    c = _case(*shape)
    _, got = _dw(_nat(), c["g"], c["xp"], C, H, W, ks)
    err = (got - c["ref_dw"]).abs().max().item()
    print(f"max abs err vs fp32 convolution_backward: {err:.4g}")
    assert torch.allclose(got, c["ref_dw"], atol=2.0, rtol=2e-2), err


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv_wgrad2_s2_exact_on_integers(shape):
    """g in {-1,0,1}: dwT is an integer sum, exact in fp32 in any order."""
    ks, N, C, H, W, K = shape
    c = _case(*shape)
    _, got = _dw(_nat(), c["gi"], c["xp"], C, H, W, ks)
    xb = binsign(c["x"].float())
    ref = _wgrad_oracle(c["gi"], xb, K, C, ks)
    # the same sum spelled out in fp64, independent of any conv library
    p = 1 if ks == 3 else 0
    cols = F.unfold(xb.double(), ks, padding=p, stride=2)   # [N, C*T, L]
    ref64 = torch.einsum("nkl,njl->kj", c["gi"].double().flatten(2),
                         cols).reshape(K, C, ks, ks)
    nbad = (got != ref).sum().item()
    nbad64 = (got.double() != ref64).sum().item()
    print(f"mismatching elements: {nbad} (fp32 oracle), {nbad64} (fp64)")
    assert torch.equal(got.double(), ref64), nbad64
    assert torch.equal(got, ref), nbad


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[9]],
                         ids=[SHAPE_IDS[2], SHAPE_IDS[9]])
def test_wgrad_finish_s2_transpose_and_mask(shape):
    ks, N, C, H, W, K = shape
    c = _case(*shape)
    nat = _nat()
    dwT, summed = _dw(nat, c["g"], c["xp"], C, H, W, ks)
    w = (c["w"] * 2.0).contiguous()          # plenty of |w| > 1
    dw = nat.wgrad_finish_s2(dwT, w)
    keep = (w.abs() <= 1)
    assert keep.any() and (~keep).any()
    assert dw.shape == w.shape
    assert (dw[~keep] == 0).all()
    assert torch.allclose(dw[keep], summed[keep], atol=1e-3, rtol=1e-5)


def test_repack_cplane_s2_bits():
    torch.manual_seed(62)
    nat = _nat()
    N, C, H, W = 2, 64, 5, 9
    x = torch.randn(N, C, H, W, device="cuda")
    xp = nat.sign_pack_nhwc(_cl(x))
    planes = nat.repack_cplane_s2(xp, C, H, W)
    assert planes.shape == (C, N * H) and planes.dtype == torch.int64
    pl = planes.cpu().numpy().astype("uint64")
    xs = x.permute(0, 2, 3, 1).cpu()
    for c in range(0, C, 17):
        for n in range(N):
            for y in range(H):
                row = int(pl[c][n * H + y])
                for pos in range(64):
                    xx = 2 * (pos & 31) + (pos >> 5)   # even low, odd high
                    want = (1 if xs[n, y, xx, c].item() >= 0 else 0) \
                        if xx < W else 0
                    assert (row >> pos) & 1 == want, (c, n, y, pos)


# ---------------- argument checks ----------------

def test_stride2_supported_predicate():
    ok = _nat().dgrad2_s2_supported
    assert ok(14, 14, 64, 64, 3) and ok(14, 14, 64, 64, 1)
    assert not ok(14, 66, 64, 64, 3)
    assert not ok(14, 14, 96, 64, 3)
    assert not ok(14, 14, 64, 32, 3)
    assert not ok(14, 14, 64, 64, 5)


def test_conv_dgrad2_s2_rejects_bad_arguments():
    c = _case(*SHAPES[2])          # 3x3, 1x64x14x14 -> K=128, g 7x7
    nat = _nat()
    g, wd, mp, x = c["g"], c["wd"], c["mp"], c["x"]

    def call(g=g, wd=wd, H=14, W=14, C=64, mode=0, mp=mp, x=None, acc=None):
        return nat.conv_dgrad2_s2(g, wd, H, W, C, mode, mp, x, 1.0, 1.0, acc)

    call()                                            # the good call
    with pytest.raises(RuntimeError, match="g must be"):       # dtype
        call(g=_cl(g.float()))
    with pytest.raises(RuntimeError, match="g must be channels_last"):
        call(g=g.contiguous())
    with pytest.raises(RuntimeError, match="wd"):              # dtype
        call(wd=wd.float())
    with pytest.raises(RuntimeError, match="g spatial size"):
        call(H=16, W=16, mp=torch.zeros(1, 16, 16, 2, device="cuda",
                                        dtype=torch.int32))
    with pytest.raises(RuntimeError, match="g spatial size"):
        call(H=12)
    with pytest.raises(RuntimeError, match="mode 0 needs mp"):
        call(mode=0, mp=None, x=x)
    with pytest.raises(RuntimeError, match="mode 0 needs mp"):
        call(mode=0, mp=mp, x=x)
    with pytest.raises(RuntimeError, match="modes 1/2 need x"):
        call(mode=1, mp=mp, x=None)
    with pytest.raises(RuntimeError, match="mode must be"):
        call(mode=3)
    with pytest.raises(RuntimeError, match="mp must be"):      # wrong size
        call(mp=mp[:, :7].contiguous())
    with pytest.raises(RuntimeError, match="x must be"):       # fp32 x
        call(mode=1, mp=None, x=x.float())
    with pytest.raises(RuntimeError, match="x must be channels_last"):
        call(mode=2, mp=None, x=x.contiguous())
    with pytest.raises(RuntimeError, match="x shape"):
        call(mode=1, mp=None, x=_cl(x[:, :, :13].clone()))
    with pytest.raises(RuntimeError, match="acc shape"):
        call(acc=c["skip_g"][:, :, :13])
    # unsupported shapes: W = 66, C = 96, K = 32
    g66 = _cl(torch.zeros(1, 128, 7, 33, device="cuda",
                          dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        call(g=g66, W=66)
    wd96 = torch.zeros(9, 96, 128, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        call(wd=wd96, C=96)
    g32 = _cl(torch.zeros(1, 32, 7, 7, device="cuda", dtype=torch.bfloat16))
    wd32 = torch.zeros(9, 64, 32, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        call(g=g32, wd=wd32)
    wd25 = torch.zeros(25, 64, 128, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="wd.size"):         # ks = 5
        call(wd=wd25)


def test_conv_wgrad2_s2_rejects_bad_arguments():
    c = _case(*SHAPES[2])
    nat = _nat()
    g, xp = c["g"], c["xp"]
    planes = nat.repack_cplane_s2(xp, 64, 14, 14)
    nat.conv_wgrad2_s2(g, planes, 64, 14, 14, 3)      # the good call
    with pytest.raises(RuntimeError, match="g must be"):
        nat.conv_wgrad2_s2(_cl(g.float()), planes, 64, 14, 14, 3)
    with pytest.raises(RuntimeError, match="g must be channels_last"):
        nat.conv_wgrad2_s2(g.contiguous(), planes, 64, 14, 14, 3)
    with pytest.raises(RuntimeError, match="g spatial size"):
        nat.conv_wgrad2_s2(g, planes, 64, 16, 14, 3)
    with pytest.raises(RuntimeError, match="planes must be"):
        nat.conv_wgrad2_s2(g, planes[:, :13].contiguous(), 64, 14, 14, 3)
    with pytest.raises(RuntimeError, match="planes must be"):
        nat.conv_wgrad2_s2(g, planes.int(), 64, 14, 14, 3)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        nat.conv_wgrad2_s2(g, planes, 64, 14, 14, 5)
    with pytest.raises(RuntimeError, match="H, W do not match"):
        nat.repack_cplane_s2(xp, 64, 14, 13)
    with pytest.raises(RuntimeError, match="C does not match"):
        nat.repack_cplane_s2(xp, 128, 14, 14)
    with pytest.raises(RuntimeError, match="xp must be"):
        nat.repack_cplane_s2(xp.float(), 64, 14, 14)
    with pytest.raises(RuntimeError, match="dwT must be"):
        nat.wgrad_finish_s2(torch.zeros(1, 9, 64, 64, device="cuda"),
                            torch.zeros(64, 64, 1, 1, device="cuda"))
    with pytest.raises(RuntimeError, match="w must be"):
        nat.wgrad_finish_s2(torch.zeros(1, 4, 64, 64, device="cuda"),
                            torch.zeros(64, 64, 2, 2, device="cuda"))
