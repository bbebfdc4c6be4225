"""The inference epilogue of the i8 MFMA conv (csrc/xnor_conv_mfma.hip,
EPI mode): conv + folded eval BN (+ skip) + activation (+ sign plane) in
one launch, against

  * the composition it replaces, bit for bit:
      bn_act_eval(xnor_conv_mfma_fwd(...), skip, ...)  and  sign_pack_nhwc
    (that composition has its own oracles: test_gpu_xnor_mfma.py and
    test_gpu_bn_act_oracle.py),
  * host-computed plane words (bit order, zero packs as +1),
  * an fp64 formula written out here (fp32 output).

Bound of the fp64 comparison.  With u = 2^-24 the epilogue rounds
  v  = fl(alpha * dot)            1   (dot is an exact integer)
  z  = fma(sc, v, sh)             1
  z += skip                       1   (with a skip)
  a * z                           1   (kinds 1, 3, negative branch)
  + b2                            1   (kind 3)
so R = 2 + skip + {0: 0, 1: 1, 2: 0, 3: 2}[kind] roundings, each of a
quantity no larger than S = L (|sc v| + |sh| + |skip|) + |b2| with
L = max(1, |a|) the Lipschitz constant of the activation (1 for kinds 0
and 2); an element whose z changes branch at the kink stays within the
bound because PReLU and ReLU are continuous.  The oracle takes alpha, sc
and sh as the kernels produced them (fp32 values, widened), so
  |out - ref| <= R u S (1 + 2^-10)      (the last factor: second order).

bn_fold.  sc = gamma * rsq(fl(rv + eps)): the add rounds once (u, halved by
the inverse root), v_rsq_f32 is accurate to 1 ulp = 2 u, the product rounds
once: 3.5 u, asserted as 4 u |sc|.  sh = fma(-rm, sc, beta) (+ b1): sc's
error times |rm| plus one rounding each: asserted as
5 u (|rm sc| + |beta| + |b1|).

Measured on an MI355X (largest over the cases of this file; every test
prints its own before it asserts): bn_fold err / bound sc 0.50, sh 0.44,
and 0 elements differing from bn_act_eval_kernel's own constants; epilogue
against fp64 err / bound 0.88 (kind 2 without skip, R = 2), 0.53 at R = 5;
share of negative pre-activations 0.49 - 0.61.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C

U = 2.0 ** -24
BN_EPS = 1e-5
FP32, BF16 = torch.float32, torch.bfloat16

# (N, C, H, W, K, stride): 3x3 / pad 1, the small shapes of
# test_gpu_xnor_mfma.py
SHAPES = [
    (3, 64, 7, 7, 64, 1),        # partial tile, tiles cross images
    (2, 64, 9, 11, 64, 1),       # odd, non-square
    (1, 64, 1, 1, 64, 1),        # 8 of 9 taps are padding
    (2, 128, 6, 6, 128, 1),      # two channel chunks, two K tiles
    (2, 64, 9, 11, 128, 2),      # stride 2, odd sizes
    (1, 64, 3, 70, 64, 1),       # rows wider than one 64-column segment
    (1, 64, 5, 131, 64, 2),      # the same at stride 2 (Wo = 66)
    (2, 256, 8, 8, 512, 2),      # stride 2, widest
]
CROSS = [SHAPES[0], SHAPES[3], SHAPES[4]]
_ids = lambda s: "x".join(map(str, s))   # noqa: E731


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs of one shape, made once and left unchanged: activations,
    weights, a skip per dtype, and per-channel operands that are not the
    modules' defaults."""
    N, C, H, W, K, stride = shape
    nat = _nat()
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    x = rnd(N, C, H, W)
    w = rnd(K, C, 3, 3) * 0.5
    xp = nat.sign_pack_nhwc(_cl(x))
    wp, alpha, _ = nat.weight_pack(w)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    skip = _cl(rnd(N, K, Ho, Wo) * 4)
    c = dict(
        shape=shape, x=x, w=w, xp=xp, wp=wp, alpha=alpha,
        skip={FP32: skip, BF16: _cl(skip.to(BF16))},
        # gamma and a of both signs, running_var over 1e-3 .. 10, shifts != 0
        gamma=rnd(K) + 0.2, beta=rnd(K), rm=rnd(K) * 2,
        rv=10 ** (torch.rand(K, device="cuda", generator=g) * 4 - 3),
        a=rnd(K) * 0.5, b1=rnd(K) + 0.1, b2=rnd(K) - 0.1)
    assert (c["gamma"] < 0).any() and (c["gamma"] > 0).any()
    assert (c["a"] < 0).any() and (c["a"] > 0).any()
    assert c["rv"].min() >= 1e-3 and c["rv"].max() <= 10
    assert (c["b1"] != 0).all() and (c["b2"] != 0).all()
    return c


def _fused(c, kind, skip, bf16, pack, sc=None, sh=None):
    nat = _nat()
    N, C, H, W, K, stride = c["shape"]
    if sc is None:
        sc, sh = nat.bn_fold(c["gamma"], c["beta"], c["rm"], c["rv"], BN_EPS,
                             c["b1"] if kind == 3 else None)
    return nat.xnor_conv_bn_act_fwd(
        c["xp"], c["wp"], c["alpha"], sc, sh,
        c["a"] if kind in (1, 3) else None, c["b2"] if kind == 3 else None,
        skip, C, stride, 1, kind, bf16, pack)


def _composition(c, kind, skip, bf16):
    nat = _nat()
    N, C, H, W, K, stride = c["shape"]
    conv = nat.xnor_conv_mfma_fwd(c["xp"], c["wp"], c["alpha"], C, stride, 1,
                                  bf16)
    return nat.bn_act_eval(
        conv, skip, c["gamma"], c["beta"], c["a"] if kind in (1, 3) else None,
        c["rm"], c["rv"], BN_EPS, kind, c["b1"] if kind == 3 else None,
        c["b2"] if kind == 3 else None)


def _check_against_composition(c, kind, with_skip, dtype, pack):
    nat = _nat()
    bf16 = dtype == BF16
    skip = c["skip"][dtype] if with_skip else None
    out, plane = _fused(c, kind, skip, bf16, pack)
    want = _composition(c, kind, skip, bf16)
    tag = (c["shape"], kind, with_skip, dtype, pack)
    assert out.dtype == dtype and out.shape == want.shape, tag
    assert out.is_contiguous(memory_format=torch.channels_last), tag
    assert torch.equal(out, want), \
        (tag, (out.float() - want.float()).abs().max().item())
    if pack:
        assert plane.dtype == torch.int32, tag
        assert torch.equal(plane, nat.sign_pack_nhwc(out)), tag
    else:
        assert plane is None, tag
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_prelu_tail_equals_composition(shape):
    """Every shape with ChannelPReLU, skip and plane, both dtypes; about
    half of the pre-activations are negative so both branches run."""
    c = _case(shape)
    for dtype in (FP32, BF16):
        _check_against_composition(c, 1, True, dtype, True)
        z = _composition(c, 0, c["skip"][dtype], dtype == BF16)
        share = (z < 0).float().mean().item()
        print(f"{_ids(shape)} {dtype}: negative share of z {share:.3f}")
        assert 0.2 <= share <= 0.8, share


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", CROSS, ids=_ids)
def test_kinds_skip_dtype_pack_equal_composition(shape, kind):
    c = _case(shape)
    for with_skip in (False, True):
        for dtype in (FP32, BF16):
            for pack in (False, True):
                _check_against_composition(c, kind, with_skip, dtype, pack)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[6]], ids=_ids)
def test_plane_bit_order(shape):
    """sc = 0, no skip, kind 0: out is sh exactly, +1 on a channel set that
    no permutation of bytes or nibbles maps to itself, -1 elsewhere.  Bit
    j of word w is channel 32 w + j, computed here on the host."""
    c = _case(shape)
    K = shape[4]
    chosen = [k for k in (0, 5, 9, 30, 33, 63, 66, 127) if k < K]
    sh = torch.full((K,), -1.0, device="cuda")
    sh[chosen] = 1.0
    sc = torch.zeros(K, device="cuda")
    words = [0] * (K // 32)
    for k in chosen:
        words[k // 32] |= 1 << (k % 32)
    assert len(set(words)) == len(words)     # the words differ from each other
    signed = [wd - (1 << 32) if wd >= (1 << 31) else wd for wd in words]
    for bf16 in (False, True):
        out, plane = _fused(c, 0, None, bf16, True, sc=sc, sh=sh)
        assert torch.equal(out.float(),
                           sh.view(1, K, 1, 1).expand_as(out))
        assert plane.shape == (out.shape[0], out.shape[2], out.shape[3],
                               K // 32)
        want = torch.tensor(signed, dtype=torch.int32, device="cuda")
        assert torch.equal(plane, want.expand_as(plane)), \
            [hex(v & 0xffffffff) for v in plane.reshape(-1, K // 32)[0].tolist()]


@pytest.mark.parametrize("kind", [0, 1])
def test_zero_packs_as_plus_one(kind):
    """sc = sh = 0: every output is zero (-0.0 through a negative PReLU
    slope) and every plane bit is 1."""
    c = _case(SHAPES[3])
    K = SHAPES[3][4]
    zero = torch.zeros(K, device="cuda")
    for bf16 in (False, True):
        out, plane = _fused(c, kind, None, bf16, True, sc=zero, sh=zero)
        assert (out == 0).all()
        assert (plane == -1).all()


def test_bn_fold_equals_eval_kernel_constants_and_fp64():
    """bn_fold is bn_act_eval_kernel's own (sc, sh): with beta = rm = 0 the
    eval kernel maps x = 1 to sc exactly, and with any beta, rm it maps
    x = 0 to sh exactly.  Both also lie within the derived bounds of the
    fp64 formula."""
    nat = _nat()
    for shape in (SHAPES[0], SHAPES[7]):
        c = _case(shape)
        K = shape[4]
        gam, bet, rm, rv, b1 = (c[k] for k in ("gamma", "beta", "rm", "rv",
                                               "b1"))
        zero = torch.zeros(K, device="cuda")
        ones = torch.ones(1, K, 1, 1, device="cuda")
        for kind, shift in ((0, None), (3, b1)):
            sc, sh = nat.bn_fold(gam, bet, rm, rv, BN_EPS, shift)
            assert sc.dtype == FP32 and sc.shape == (K,) and sh.shape == (K,)
            # kind 0 of the eval kernel exposes its constants; b1 is added
            # to sh after the fold, checked against the fp32 sum
            k_sc = nat.bn_act_eval(ones, None, gam, zero, None, zero, rv,
                                   BN_EPS, 0, None, None).view(K)
            assert torch.equal(sc, k_sc), (sc != k_sc).sum().item()
            if kind == 0:
                k_sh = nat.bn_act_eval(0 * ones, None, gam, bet, None, rm, rv,
                                       BN_EPS, 0, None, None).view(K)
                assert torch.equal(sh, k_sh), (sh != k_sh).sum().item()
            else:
                sh0 = nat.bn_fold(gam, bet, rm, rv, BN_EPS, None)[1]
                assert torch.equal(sh, sh0 + b1)
            sc_ref = gam.double() / torch.sqrt(rv.double() + BN_EPS)
            sh_ref = bet.double() - rm.double() * sc_ref
            mags = (rm.double() * sc_ref).abs() + bet.double().abs()
            if shift is not None:
                sh_ref = sh_ref + shift.double()
                mags = mags + shift.double().abs()
            q_sc = ((sc.double() - sc_ref).abs() / (4 * U * sc_ref.abs())).max()
            q_sh = ((sh.double() - sh_ref).abs() / (5 * U * mags)).max()
            print(f"bn_fold K={K} kind={kind}: err/bound sc {q_sc.item():.3f} "
                  f"sh {q_sh.item():.3f}")
            assert q_sc.item() <= 1.0 and q_sh.item() <= 1.0


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[7]], ids=_ids)
def test_fp32_output_against_fp64_formula(shape, kind):
    nat = _nat()
    c = _case(shape)
    N, C, H, W, K, stride = shape
    sign = lambda t: torch.where(t >= 0, 1.0, -1.0).double().cpu()   # noqa: E731
    dot = F.conv2d(sign(c["x"]), sign(c["w"]), None, stride=stride,
                   padding=1).cuda()
    assert torch.equal(dot, dot.round())
    sc, sh = nat.bn_fold(c["gamma"], c["beta"], c["rm"], c["rv"], BN_EPS,
                         c["b1"] if kind == 3 else None)
    col = lambda t: t.double().view(1, K, 1, 1)   # noqa: E731
    for with_skip in (False, True):
        skip = c["skip"][FP32] if with_skip else None
        out, _ = _fused(c, kind, skip, False, False)
        v = col(c["alpha"]) * dot
        z = col(sc) * v + col(sh)
        mag = (col(sc) * v).abs() + col(sh).abs()
        if with_skip:
            z = z + skip.double()
            mag = mag + skip.double().abs()
        lip = torch.ones_like(col(sc))
        if kind in (1, 3):
            ref = torch.where(z > 0, z, col(c["a"]) * z)
            lip = col(c["a"]).abs().clamp(min=1.0)
        elif kind == 2:
            ref = z.clamp(min=0)
        else:
            ref = z
        mag = lip * mag
        if kind == 3:
            ref = ref + col(c["b2"])
            mag = mag + col(c["b2"]).abs()
        R = 2 + int(with_skip) + {0: 0, 1: 1, 2: 0, 3: 2}[kind]
        bound = R * U * mag * (1 + 2.0 ** -10)
        err = (out.double() - ref).abs()
        q = (err / bound).max().item()
        print(f"{_ids(shape)} kind {kind} skip {with_skip}: R = {R}, "
              f"max err / bound {q:.3f}, max |err| {err.max().item():.3g}")
        assert q <= 1.0, q


def _raw(C, K, ks, H=8, W=8):
    nat = _nat()
    x = torch.randn(2, C, H, W, device="cuda")
    w = torch.randn(K, C, ks, ks, device="cuda")
    xp = nat.sign_pack_nhwc(_cl(x))
    wp, alpha, _ = nat.weight_pack(w)
    return xp, wp, alpha


@pytest.mark.parametrize("C,K,ks,pad", [(48, 64, 3, 1), (64, 96, 3, 1),
                                        (64, 64, 1, 0), (64, 64, 5, 2)])
def test_unsupported_geometry_raises(C, K, ks, pad):
    nat = _nat()
    xp, wp, alpha = _raw(C, K, ks)
    one = torch.ones(K, device="cuda")
    before = nat.xnor_fused_calls()
    with pytest.raises(RuntimeError):
        nat.xnor_conv_bn_act_fwd(xp, wp, alpha, one, one, None, None, None,
                                 C, 1, pad, 0, False, False)
    assert nat.xnor_fused_calls() == before


def test_malformed_operands_raise():
    nat = _nat()
    C = K = 64
    xp, wp, alpha = _raw(C, K, 3)
    one = torch.ones(K, device="cuda")
    args = lambda **kw: [kw.get(n, d) for n, d in (   # noqa: E731
        ("xp", xp), ("wp", wp), ("alpha", alpha), ("sc", one), ("sh", one),
        ("a", one), ("b2", one), ("skip", None), ("C", C), ("stride", 1),
        ("pad", 1), ("kind", 1), ("bf16", False), ("pack", True))]
    before = nat.xnor_fused_calls()
    out, plane = nat.xnor_conv_bn_act_fwd(*args())          # well-formed
    assert nat.xnor_fused_calls() == before + 1
    bad = [
        dict(sc=torch.ones(K + 1, device="cuda")),          # wrong length
        dict(sh=torch.ones(K // 2, device="cuda")),
        dict(sc=one.double()),                               # not fp32
        dict(a=None),                                        # kind 1 needs a
        dict(kind=3, b2=None),                               # kind 3 needs b2
        dict(kind=3, a=None),
        dict(kind=4),
        dict(skip=out.to(BF16)),                             # skip dtype
        dict(skip=out[:, :, :-1]),                           # skip shape
        dict(skip=out.contiguous()),                         # skip layout
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            nat.xnor_conv_bn_act_fwd(*args(**kw))
    assert nat.xnor_fused_calls() == before + 1
