"""conv_dgrad_small / conv_wgrad_small (csrc/conv_bwd_small.hip): the owned
backward of the 3x3/s1/p1 binary convs with C and K in {16, 32}, at kernel,
function and model level.

Shapes are (N, C, H, W, K), the smallest that reach every branch.  A tile is
RB rows of one image at WP = W rounded up to 8 columns, RB = min(128 / WP, H):
the two real classes of ResNet-20, the narrowest (WP 8) and widest (WP 64,
RB 2) class, W < WP with H % RB != 0 and odd N, C != K both ways, one pixel,
(2,16,20,20,32) whose RB*WP = 5*24 = 120 pixels are no multiple of the 16-
pixel MFMA column group nor of the wgrad's 32-pixel step (the last group /
step is part dummy), and (5000,16,1,1,16): 5000 tiles over the dgrad's grid
cap of 2048 blocks are 3 tiles per block with a last block of 2, and for the
wgrad 17 blocks of up to 295 chunks (the two LDS stages alternate; the m-
split is rounded so that no block is left without a chunk, so there is no
empty-block shape to test)."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops import binary_conv as bc
from bdbnn_amd.ops.binarize import binsign, weight_scale
from bdbnn_amd.ops.binary_conv import BinaryConvFunction, _act_grad_mask


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


SHAPES = [
    (2, 16, 32, 32, 16),
    (2, 32, 16, 16, 32),
    (4, 32, 8, 8, 32),
    (1, 16, 40, 64, 16),
    (3, 16, 5, 7, 16),
    (1, 16, 9, 9, 32),
    (1, 32, 9, 9, 16),
    (1, 16, 1, 1, 16),
    (2, 16, 20, 20, 32),
    (5000, 16, 1, 1, 16),
]
IDS = ["x".join(map(str, s)) for s in SHAPES]

# (kernel mode, act_mode string, t, k) of tests/test_gpu_bwd_modes.py
MASKS = [
    (1, "approx", None, None),
    (2, "ste", 0.01, 100.0),
    (2, "ste", 1.0, 1.0),
    (2, "ste", 10.0, 1.0),
]
MASK_IDS = ["approx", "ede_t0.01_k100", "ede_t1_k1", "ede_t10_k1"]

# bf16-exact probes: the polynomial's half-open boundaries, both zeros,
# and |t*x| = 500 at t = 10 (EDE overflow)
EDGE = [-1.0, -0.0, 0.0, 1.0, 0.5, -0.5, 50.0, -50.0]


def _max_mask(mode, t, k):
    return 1.0 if mode == 0 else 2.0 if mode == 1 else float(k) * float(t)


def _tk(t, k):
    return (0.0 if t is None else t, 0.0 if k is None else k)


def _ref_dgrad(g, wd):
    """fp64 sum_{t,k} g[n, y+dy-1, x+dx-1, k] * wd[t][c][k] on the CPU,
    NCHW result"""
    N, K, H, W = g.shape
    gp = F.pad(g.cpu().double(), (1, 1, 1, 1)).permute(0, 2, 3, 1)
    wdd = wd.cpu().double()
    out = torch.zeros(N, H, W, wd.shape[1], dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            out += gp[:, dy:dy + H, dx:dx + W, :] @ wdd[dy * 3 + dx].t()
    return out.permute(0, 3, 1, 2)


def _ref_dw(x, g):
    """fp64 dw[K][C][3][3] of (sign(x), g) on the CPU, sign(0) = +1"""
    N, C, H, W = x.shape
    K = g.shape[1]
    s = torch.where(x.cpu() >= 0, 1.0, -1.0).double()
    sp = F.pad(s, (1, 1, 1, 1)).permute(0, 2, 3, 1)
    G = g.cpu().double().permute(0, 2, 3, 1).reshape(-1, K)
    out = torch.empty(K, C, 3, 3, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            S = sp[:, dy:dy + H, dx:dx + W, :].reshape(-1, C)
            out[:, :, dy, dx] = G.t() @ S
    return out


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs and references of a shape, computed once, read-only"""
    N, C, H, W, K = shape
    nat = _nat()
    gen = torch.Generator().manual_seed(2000 + sum(shape))
    x = torch.randn(N, C, H, W, generator=gen).bfloat16()
    x[0, :len(EDGE), 0, 0] = torch.tensor(EDGE).bfloat16()
    xm = (1.5 * torch.randn(N, C, H, W, generator=gen)).bfloat16()
    g_int = torch.randint(-3, 4, (N, K, H, W), generator=gen).bfloat16()
    g_rnd = torch.randn(N, K, H, W, generator=gen).bfloat16()
    s_int = torch.randint(-3, 4, (N, C, H, W), generator=gen).bfloat16()
    s_rnd = torch.randn(N, C, H, W, generator=gen).bfloat16()
    wd_pm = (torch.randint(0, 2, (9, C, K), generator=gen) * 2 - 1).bfloat16()
    w = torch.randn(K, C, 3, 3, generator=gen)
    c = dict(x=_cl(x.cuda()), g_int=_cl(g_int.cuda()), g_rnd=_cl(g_rnd.cuda()),
             s_int=_cl(s_int.cuda()), s_rnd=_cl(s_rnd.cuda()),
             wd_pm=wd_pm.cuda(), w=w.cuda())
    c["xp"] = nat.sign_pack_nhwc(c["x"])
    _, c["mp"] = nat.sign_mask_pack_nhwc(_cl(xm.cuda()))
    assert c["mp"].shape == (N, H, W, 1)
    c["clip"] = (xm.float().abs() <= 1).double()          # CPU, NCHW
    c["ref_int"] = _ref_dgrad(g_int, wd_pm)               # CPU fp64
    c["skip_int"] = s_int.double()
    wp, alpha, _ = nat.weight_pack(c["w"])
    c["wd"] = nat.dgrad_weight_decode(wp, alpha, C)
    wb = (weight_scale(c["w"]) * binsign(c["w"])).to(torch.bfloat16)
    c["ref_raw"] = _cl(F.conv_transpose2d(
        c["g_rnd"].float(), wb.float(), None, stride=1, padding=1))
    ones = torch.full((N, H, W, 1), -1, device="cuda", dtype=torch.int32)
    c["base"] = nat.conv_dgrad_small(c["g_rnd"], c["wd"], C, 0, ones, None,
                                     0.0, 0.0)
    c["dw_int"] = _ref_dw(x, g_int)
    c["dw_rnd"] = _ref_dw(x, g_rnd)
    c["absg"] = g_rnd.double().abs().sum(dim=(0, 2, 3))
    return c


def test_dgrad_weight_decode_at_16_channels():
    """wd[t][c][k] = alpha_k * sign(w[k, c, 2-dy, 2-dx]) with one mask word
    of which bits 16..31 are unused"""
    torch.manual_seed(3)
    nat = _nat()
    for C, K in ((16, 16), (16, 32), (32, 16)):
        w = torch.randn(K, C, 3, 3, device="cuda")
        wp, alpha, _ = nat.weight_pack(w)
        wd = nat.dgrad_weight_decode(wp, alpha, C)
        assert wd.shape == (9, C, K) and wd.dtype == torch.bfloat16
        want = (weight_scale(w) * binsign(w)).flip(2, 3).permute(
            2, 3, 1, 0).reshape(9, C, K).to(torch.bfloat16)
        assert torch.equal(wd, want)


@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dgrad_small_mode0_exact_on_integers(shape, acc):
    """integer g in [-3, 3] and +-1 weights: every partial sum is an integer
    of magnitude <= 9*32*3 = 864 (+3 with the skip gradient), exact in fp32,
    so the result is the fp64 reference rounded once to bf16"""
    N, C, H, W, K = shape
    nat = _nat()
    c = _case(shape)
    want = c["ref_int"] * c["clip"]
    skip = None
    if acc:
        want = want + c["skip_int"]
        skip = c["s_int"]
    want = want.to(torch.bfloat16)

    def run():
        return nat.conv_dgrad_small(c["g_int"], c["wd_pm"], C, 0, c["mp"],
                                    None, 0.0, 0.0, skip)
    # dx comes from an uninitialised allocation: leave NaNs in the block
    # the caching allocator hands out next
    poison = run()
    poison.fill_(float("nan"))
    del poison
    dx = run()
    assert dx.shape == (N, C, H, W) and dx.dtype == torch.bfloat16
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert torch.isfinite(dx).all(), "a pixel was not written"
    got = dx.cpu()
    bad = (got != want).sum().item()
    assert torch.equal(got, want), f"{bad} of {got.numel()} differ"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dgrad_small_mode0_real_weights_vs_fp32_oracle(shape):
    N, C, H, W, K = shape
    c = _case(shape)
    dx = _nat().conv_dgrad_small(c["g_rnd"], c["wd"], C, 0, c["mp"], None,
                                 0.0, 0.0)
    ref = c["ref_raw"] * c["clip"].cuda().float()
    assert torch.isfinite(dx).all()
    err = (dx.float() - ref).abs().max().item()
    print(f"{shape}: max abs err vs fp32 oracle: {err:.4g}")
    assert torch.allclose(dx.float(), ref, atol=0.5, rtol=2e-2), err
    # the all-ones-mask run is the unmasked dgrad: masking is a select
    assert torch.equal(dx.float(), c["base"].float() *
                       c["clip"].cuda().float())


@pytest.mark.parametrize("mode,act,t,k", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dgrad_small_value_masks(shape, mode, act, t, k):
    """modes 1 and 2: against the fp32 oracle (the project's tolerance,
    atol scaled by the mode's largest mask), and tightly against the
    mode-0 kernel's unmasked output times the oracle mask (one extra bf16
    rounding of `base` plus the final rounding, each <= 2^-8 relative; the
    bound is 2x that plus an absolute term for the EDE tails)"""
    N, C, H, W, K = shape
    c = _case(shape)
    got = _nat().conv_dgrad_small(c["g_rnd"], c["wd"], C, mode, None, c["x"],
                                  *_tk(t, k))
    assert got.dtype == torch.bfloat16 and torch.isfinite(got).all()
    got = got.float()
    mask = _act_grad_mask(c["x"].float(), act, t, k)
    ref = c["ref_raw"] * mask
    err = (got - ref).abs().max().item()
    print(f"{shape}: max abs err vs fp32 oracle: {err:.4g}")
    assert torch.allclose(got, ref, atol=0.5 * _max_mask(mode, t, k),
                          rtol=2e-2), err
    want = c["base"].float() * mask
    bound = 2.0 ** -6 * want.abs() + 2.0 ** -10 * want.abs().max()
    excess = ((got - want).abs() - bound).max().item()
    print(f"{shape}: max (|got-want| - bound): {excess:.4g}")
    assert excess <= 0, excess
    if mode == 1:
        zero = mask == 0
        # the probes guarantee |x| >= 1 and x == -1 are present
        assert zero[0, 0, 0, 0] and zero[0, 3, 0, 0] and zero[0, 6, 0, 0]
        assert (got[zero] == 0).all()


@pytest.mark.parametrize("mode,act,t,k", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("shape", [(3, 16, 5, 7, 16), (2, 32, 16, 16, 32)])
def test_dgrad_small_value_masks_acc(shape, mode, act, t, k):
    """acc adds the (unmasked) skip gradient in the epilogue; bound of
    test_conv_dgrad2_x_acc_fuses_skip_grad"""
    N, C, H, W, K = shape
    c = _case(shape)
    nat = _nat()
    a = (c["g_rnd"], c["wd"], C, mode, None, c["x"]) + _tk(t, k)
    plain = nat.conv_dgrad_small(*a)
    fused = nat.conv_dgrad_small(*a, c["s_rnd"])
    want = (plain.float() + c["s_rnd"].float()).to(torch.bfloat16)
    err = (fused.float() - want.float()).abs().max().item()
    print(f"max abs err fused vs separate add: {err:.4g}")
    assert torch.allclose(fused.float(), want.float(),
                          atol=2e-2 * _max_mask(mode, t, k), rtol=1e-2), err


def _kc33(dwT):
    """sum of the slabs [nslab][9][C][K] in [K][C][3][3] order"""
    C, K = dwT.shape[2], dwT.shape[3]
    return dwT.sum(0).permute(2, 1, 0).reshape(K, C, 3, 3)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wgrad_small_exact_on_integer_g(shape):
    """g integer in [-3, 3]: every partial sum is an integer below 2^24
    (at most 3 * N*H*W <= 15360 here), so any accumulation order is exact"""
    N, C, H, W, K = shape
    nat = _nat()
    c = _case(shape)
    # fold=False: the block slabs as the kernel wrote them, from an
    # uninitialised allocation: leave NaNs in the block the caching
    # allocator hands out next
    poison = nat.conv_wgrad_small(c["g_int"], c["xp"], C, fold=False)
    poison.fill_(float("nan"))
    del poison
    dwT = nat.conv_wgrad_small(c["g_int"], c["xp"], C, fold=False)
    assert dwT.shape[1:] == (9, C, K) and dwT.dtype == torch.float32
    # the slabs written stay below the bytes of g read (one slab always)
    assert dwT.shape[0] == 1 or dwT.numel() * 4 <= c["g_int"].numel() * 2
    assert torch.isfinite(dwT).all(), "a slab was not (fully) written"
    got = _kc33(dwT).cpu().double()
    bad = (got != c["dw_int"]).sum().item()
    assert torch.equal(got, c["dw_int"]), f"{bad} of {got.numel()} differ"
    # the default call: more than 8 slabs come back folded into one
    folded = nat.conv_wgrad_small(c["g_int"], c["xp"], C)
    assert folded.shape[0] == (dwT.shape[0] if dwT.shape[0] <= 8 else 1)
    assert torch.equal(_kc33(folded).cpu().double(), c["dw_int"])
    # through wgrad_finish at these widths: transpose + |w| <= 1 mask
    want = c["dw_int"] * (c["w"].abs() <= 1).cpu().double()
    for slabs in (dwT, folded):
        dw = nat.wgrad_finish(slabs, c["w"]).cpu().double()
        assert torch.equal(dw, want)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wgrad_small_random_g_within_fp32_sum_bound(shape):
    """the project's bound: N*H*W * 2^-24 * sum_m |g[m, k]| per k"""
    N, C, H, W, K = shape
    c = _case(shape)
    bound = (N * H * W) * 2.0 ** -24 * c["absg"].view(K, 1, 1, 1)
    for fold in (False, True):
        dwT = _nat().conv_wgrad_small(c["g_rnd"], c["xp"], C, fold=fold)
        assert torch.isfinite(dwT).all(), "a slab was not (fully) written"
        r = ((_kc33(dwT).cpu().double() - c["dw_rnd"]).abs() / bound).max()
        print(f"{shape}: fold {fold}: {dwT.shape[0]} slabs, max err/bound "
              f"{r.item():.3g}")
        assert r.item() <= 1.0


def test_multi_tile_shape_walks_three_tiles_per_block():
    """the geometry the (5000,16,1,1,16) case relies on"""
    total, cap = 5000, 2048
    per_block = -(-total // cap)
    blocks = -(-total // per_block)
    assert per_block == 3 and total - (blocks - 1) * per_block == 2


def test_bwd_small_predicate_and_rejection():
    nat = _nat()
    dev = dict(device="cuda")

    def operands(N, C, H, W, K):
        g = _cl(torch.zeros(N, K, H, W, dtype=torch.bfloat16, **dev))
        wd = torch.zeros(9, C, K, dtype=torch.bfloat16, **dev)
        mp = torch.zeros(N, H, W, (C + 31) // 32, dtype=torch.int32, **dev)
        x = _cl(torch.zeros(N, C, H, W, dtype=torch.bfloat16, **dev))
        return g, wd, mp, x

    for (C, K, W) in [(64, 16, 14), (16, 64, 14), (48, 48, 14), (8, 16, 14),
                      (16, 16, 65)]:
        assert not nat.bwd_small_supported(14, W, C, K)
        g, wd, mp, x = operands(1, C, 14, W, K)
        with pytest.raises(RuntimeError, match="conv_dgrad_small"):
            nat.conv_dgrad_small(g, wd, C, 0, mp, None, 0.0, 0.0)
        with pytest.raises(RuntimeError, match="conv_dgrad_small"):
            nat.conv_dgrad_small(g, wd, C, 1, None, x, 0.0, 0.0)
        with pytest.raises(RuntimeError, match="conv_wgrad_small"):
            nat.conv_wgrad_small(g, mp, C)

    assert nat.bwd_small_supported(9, 9, 16, 32)
    g, wd, mp, x = operands(2, 16, 9, 9, 32)
    ok = nat.conv_dgrad_small(g, wd, 16, 0, mp, None, 0.0, 0.0)
    assert ok.shape == (2, 16, 9, 9)
    bad = [
        dict(mp=mp[:, :8].contiguous()),                  # mp of another H
        dict(mp=mp.float()),                              # mp dtype
        dict(mp=None),                                    # mode 0 without mp
        dict(mp=mp, x=x),                                 # both
        dict(mode=1, mp=None, x=_cl(x[:, :, :8].clone())),  # x of another H
        dict(mode=1, mp=None, x=x.float()),               # x dtype
        dict(mode=1, mp=None, x=x.contiguous()),          # NCHW x
        dict(mode=1, mp=mp, x=None),                      # mode 1 without x
        dict(mode=3, mp=None, x=x),                       # bad mode
        dict(acc=_cl(x[:, :, :, :8].clone())),            # acc of another W
        dict(acc=x[:, :8]),                               # acc of another C
        dict(wd=wd.float()),                              # wd dtype
        dict(wd=wd.transpose(1, 2).contiguous()),         # wd [9][K][C]
        dict(g=g.float()),                                # g dtype
        dict(g=g.contiguous()),                           # NCHW g
    ]
    for kw in bad:
        a = dict(g=g, wd=wd, mode=0, mp=mp, x=None, acc=None)
        a.update(kw)
        with pytest.raises(RuntimeError, match="conv_dgrad_small"):
            nat.conv_dgrad_small(a["g"], a["wd"], 16, a["mode"], a["mp"],
                                 a["x"], 0.0, 0.0, a["acc"])
    with pytest.raises(RuntimeError, match="conv_wgrad_small"):
        nat.conv_wgrad_small(g, mp[:, :, :8].contiguous(), 16)
    with pytest.raises(RuntimeError, match="conv_wgrad_small"):
        nat.conv_wgrad_small(g, mp.long(), 16)
    with pytest.raises(RuntimeError, match="conv_wgrad_small"):
        nat.conv_wgrad_small(g.float(), mp, 16)


# ---------------- function level ----------------

# (act_mode, t, k, largest mask)
MODES = [("ste", None, None, 1.0), ("approx", None, None, 2.0),
         ("ste", 10.0, 1.0, 10.0)]
MODE_IDS = ["ste", "approx", "ede_t10_k1"]


def _count(monkeypatch, names):
    nat = _nat()
    calls = {}
    for name in names:
        real = getattr(nat, name)
        calls[name] = []

        def counted(*a, _r=real, _c=calls[name], **kw):
            _c.append(1)
            return _r(*a, **kw)
        monkeypatch.setattr(nat, name, counted)
    return calls


@pytest.mark.parametrize("act,t,k,mx", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N,C,H,K", [(2, 16, 9, 16), (2, 32, 9, 32)])
def test_binary_conv_function_owned_vs_fallback(monkeypatch, N, C, H, K, act,
                                                t, k, mx):
    """dx and dw of the owned path vs the BDBNN_MFMA_BWD_SMALL=0 path, the
    tolerances of test_value_mask_backward_owned_vs_fallback"""
    torch.manual_seed(44)
    x = _cl(torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16))
    w = torch.randn(K, C, 3, 3, device="cuda")
    calls = _count(monkeypatch, ["conv_dgrad_small", "conv_wgrad_small"])

    def run(flag):
        monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", flag)
        torch.manual_seed(45)
        xl = x.clone().requires_grad_(True)
        wl = w.clone().requires_grad_(True)
        out, _, _ = BinaryConvFunction.apply(xl, wl, 1, 1, act, t, k, False)
        (out.float() * torch.randn_like(out.float())).sum().backward()
        torch.cuda.synchronize()
        return xl.grad.float(), wl.grad.float()
    dx2, dw2 = run(True)
    assert (len(calls["conv_dgrad_small"]),
            len(calls["conv_wgrad_small"])) == (1, 1)
    dx1, dw1 = run(False)
    assert (len(calls["conv_dgrad_small"]),
            len(calls["conv_wgrad_small"])) == (1, 1)
    print(f"dx max diff {(dx2 - dx1).abs().max().item():.4g}, "
          f"dw max diff {(dw2 - dw1).abs().max().item():.4g}")
    assert torch.allclose(dx2, dx1, atol=5e-2 * mx, rtol=2e-2), \
        (dx2 - dx1).abs().max().item()
    assert torch.allclose(dw2, dw1, atol=5e-1, rtol=2e-2), \
        (dw2 - dw1).abs().max().item()


@pytest.mark.parametrize("act", ["ste", "approx"])
@pytest.mark.parametrize("C,K", [(16, 16), (32, 32), (16, 32)])
def test_skip_grad_owned_small(monkeypatch, C, K, act):
    """the statement of tests/test_bwd_skip_grad_branches.py (_check_gpu):
    dx with the skip cell is dx without it plus the stashed tensor, the
    cell comes back empty, and conv_dgrad_small ran once per backward"""
    monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", True)
    torch.manual_seed(92)
    calls = _count(monkeypatch, ["conv_dgrad_small"])["conv_dgrad_small"]
    x = _cl(torch.randn(2, C, 9, 9, device="cuda", dtype=torch.bfloat16))
    w = torch.randn(K, C, 3, 3, device="cuda")
    s = _cl(torch.randn(2, C, 9, 9, device="cuda", dtype=torch.bfloat16))
    gout, dxs = None, []
    for cell in (None, {"g": s}):
        xl = x.clone().requires_grad_(True)
        wl = w.clone().requires_grad_(True)
        out, _, _ = BinaryConvFunction.apply(xl, wl, 1, 1, act, None, None,
                                             False, None, None, cell)
        if gout is None:
            gout = torch.randn_like(out)
        out.backward(gout)
        if cell is not None:
            assert cell == {}, "backward must pop the stashed gradient"
        dxs.append(xl.grad)
    torch.cuda.synchronize()
    assert len(calls) == 2
    base, fused = dxs
    want = (base.float() + s.float()).to(torch.bfloat16)
    err = (fused.float() - want.float()).abs().max().item()
    print(f"C={C} K={K} {act}: max err {err}")
    assert torch.allclose(fused.float(), want.float(), atol=2e-2,
                          rtol=1e-2), err


# ---------------- model level ----------------

@pytest.mark.parametrize("knob,want", [(True, (11, 11, 5, 4)),
                                       (False, (0, 0, 5, 15))],
                         ids=["on", "off"])
@pytest.mark.parametrize("recipe", ["clip-ste", "ede"])
def test_resnet20_native_call_counts(monkeypatch, recipe, knob, want):
    """One bf16-autocast forward + backward of CIFAR ResNet-20: the eleven
    16/32-channel stride-1 convs on the new kernels, the five 64-channel
    ones on conv_dgrad2(_x) + conv_wgrad3, the four stride-2 convs on the
    fallback (whose decode is the marker: decode_packed for clip-STE,
    binsign_decode for EDE)."""
    from bdbnn_amd.engine.trainer import ede_inject
    from bdbnn_amd.models import cifar10
    monkeypatch.setattr(bc, "_MFMA_BWD_SMALL", knob)
    torch.manual_seed(36)
    m = cifar10.resnet20()
    if recipe == "ede":
        ede_inject(m, 10, 100)
    m = m.cuda().to(memory_format=torch.channels_last)
    marker = "decode_packed" if recipe == "clip-ste" else "binsign_decode"
    calls = _count(monkeypatch, ["conv_dgrad_small", "conv_wgrad_small",
                                 "conv_wgrad3", marker])
    x = _cl(torch.randn(4, 3, 32, 32, device="cuda"))
    y = torch.randint(0, 10, (4,), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(x)
        loss = F.cross_entropy(out.float(), y)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    got = tuple(len(calls[n]) for n in ("conv_dgrad_small",
                                        "conv_wgrad_small", "conv_wgrad3",
                                        marker))
    print(f"{recipe} knob {knob}: {got}")
    assert got == want
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        assert torch.isfinite(p.grad).all(), n
