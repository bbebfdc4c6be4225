"""Owned MFMA backward for the ReAct-polynomial ("approx") and EDE
activation-gradient modes: conv_dgrad2_x (value mask of the saved bf16
activation in the dgrad2 epilogue) and its routing through
BinaryConvFunction.backward."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops import binary_conv as bc
from bdbnn_amd.ops.binarize import binsign, weight_scale
from bdbnn_amd.ops.binary_conv import BinaryConvFunction, _act_grad_mask


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


# smallest shape per padded-width class plus its edge cases
SHAPES = [
    (4, 64, 7, 64),     # Wp=8, multi-image blocks
    (1, 64, 9, 64),     # Wp=16, dummy columns, partial band
    (3, 64, 30, 64),    # Wp=32, H % RB != 0, odd N
    (1, 64, 33, 64),    # Wp=64, smallest width of the class, partial band
    (1, 128, 9, 64),    # C != K: second 64-channel tile
    (1, 64, 9, 128),    # C != K: two g-channel chunks
]

# (kernel mode, act_mode string, t, k): mode 1 and the ends + middle of the
# EDE (t, k) schedule (T_MIN=1e-2, T_MAX=1e1)
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
    return 2.0 if mode == 1 else float(k) * float(t)


def _args(mode, t, k):
    return (mode, 0.0 if t is None else t, 0.0 if k is None else k)


@functools.lru_cache(maxsize=None)
def _case(N, C, H, K):
    """Inputs and mask-independent references of one shape, built once and
    shared (read-only) by every test that uses the shape."""
    gen = torch.Generator(device="cuda").manual_seed(
        1000 * N + 100 * H + C + 7 * K)
    nat = _nat()
    g = _cl(torch.randn(N, K, H, H, device="cuda", dtype=torch.bfloat16,
                        generator=gen))
    w = torch.randn(K, C, 3, 3, device="cuda", generator=gen)
    x = torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16,
                    generator=gen)
    x[0, :len(EDGE), 0, 0] = torch.tensor(EDGE, device="cuda",
                                          dtype=torch.bfloat16)
    x = _cl(x)
    skip_g = _cl(torch.randn(N, C, H, H, device="cuda",
                             dtype=torch.bfloat16, generator=gen))
    wp, alpha, _ = nat.weight_pack(w)
    assert nat.dgrad2_supported(H, H, C, K)
    wd = nat.dgrad_weight_decode(wp, alpha, C)
    # fp32 oracle of the unmasked dgrad (wb as in _dgrad2_ref of
    # tests/test_gpu_kernels.py)
    wb = (weight_scale(w) * binsign(w)).to(torch.bfloat16)
    ref_raw = _cl(torch.nn.functional.conv_transpose2d(
        g.float(), wb.float(), None, stride=1, padding=1))
    # mode-0 kernel with an all-ones mask plane: the unmasked dgrad as the
    # kernel itself computes it, rounded once to bf16
    ones = torch.full((N, H, H, C // 32), -1, device="cuda",
                      dtype=torch.int32)
    base = nat.conv_dgrad2(g, wd, ones, C)
    return dict(g=g, w=w, x=x, wd=wd, skip_g=skip_g, ref_raw=ref_raw,
                base=base)


@pytest.mark.parametrize("mode,act,t,k", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("N,C,H,K", SHAPES)
def test_conv_dgrad2_x_matches_fp32_oracle(N, C, H, K, mode, act, t, k):
    c = _case(N, C, H, K)
    dx = _nat().conv_dgrad2_x(c["g"], c["wd"], c["x"], C, *_args(mode, t, k))
    ref = c["ref_raw"] * _act_grad_mask(c["x"].float(), act, t, k)
    assert dx.shape == ref.shape and dx.dtype == torch.bfloat16
    assert torch.isfinite(dx).all()
    err = (dx.float() - ref).abs().max().item()
    print(f"max abs err vs fp32 oracle: {err:.4g}")
    # the project's tolerance for this kernel; the oracle's error scales
    # with the mask, so atol is multiplied by the mode's maximum mask
    assert torch.allclose(dx.float(), ref, atol=0.5 * _max_mask(mode, t, k),
                          rtol=2e-2), err


@pytest.mark.parametrize("mode,act,t,k", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("N,C,H,K", SHAPES)
def test_conv_dgrad2_x_matches_mode0_kernel_times_mask(N, C, H, K, mode,
                                                       act, t, k):
    """Tight check of the mask math: the mode-0 kernel's unmasked output
    times the oracle mask.  The two differ by one extra bf16 rounding of
    `base` plus the final rounding of `got`, each <= 2^-8 relative; the
    bound is 2x that, plus an absolute term for the EDE tails where the
    mask underflows toward 0."""
    c = _case(N, C, H, K)
    mask = _act_grad_mask(c["x"].float(), act, t, k)
    want = c["base"].float() * mask
    got = _nat().conv_dgrad2_x(c["g"], c["wd"], c["x"], C,
                               *_args(mode, t, k)).float()
    assert torch.isfinite(got).all()
    bound = 2.0 ** -6 * want.abs() + 2.0 ** -10 * want.abs().max()
    excess = ((got - want).abs() - bound).max().item()
    print(f"max (|got-want| - bound): {excess:.4g}")
    assert excess <= 0, excess
    if mode == 1:
        zero = mask == 0
        # the probes guarantee |x| >= 1 and x == -1 are present
        assert zero[0, 0, 0, 0] and zero[0, 3, 0, 0] and zero[0, 6, 0, 0]
        assert (got[zero] == 0).all()


@pytest.mark.parametrize("mode,act,t,k", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("N,C,H,K", [(4, 64, 7, 64), (1, 64, 33, 64)])
def test_conv_dgrad2_x_acc_fuses_skip_grad(N, C, H, K, mode, act, t, k):
    """acc adds the (unmasked) skip gradient in the epilogue."""
    c = _case(N, C, H, K)
    nat = _nat()
    a = _args(mode, t, k)
    plain = nat.conv_dgrad2_x(c["g"], c["wd"], c["x"], C, *a)
    fused = nat.conv_dgrad2_x(c["g"], c["wd"], c["x"], C, *a, c["skip_g"])
    want = (plain.float() + c["skip_g"].float()).to(torch.bfloat16)
    err = (fused.float() - want.float()).abs().max().item()
    print(f"max abs err fused vs separate add: {err:.4g}")
    assert torch.allclose(fused.float(), want.float(),
                          atol=2e-2 * _max_mask(mode, t, k), rtol=1e-2), err


def test_conv_dgrad2_x_rejects_bad_arguments():
    c = _case(1, 64, 9, 64)
    nat = _nat()
    for bad_mode in (0, 3):
        with pytest.raises(RuntimeError):
            nat.conv_dgrad2_x(c["g"], c["wd"], c["x"], 64, bad_mode, 1.0, 1.0)
    with pytest.raises(RuntimeError):       # fp32 activation
        nat.conv_dgrad2_x(c["g"], c["wd"], c["x"].float(), 64, 1, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="x shape"):   # wrong H
        nat.conv_dgrad2_x(c["g"], c["wd"], _cl(c["x"][:, :, :8].clone()),
                          64, 1, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="channels_last"):  # NCHW x
        nat.conv_dgrad2_x(c["g"], c["wd"], c["x"].contiguous(), 64, 1,
                          0.0, 0.0)


# ---------------- routing ----------------

def _raiser(name):
    def f(*a, **kw):
        raise AssertionError(f"{name} called on the owned backward path")
    return f


def _count_dgrad2_x(monkeypatch):
    nat = _nat()
    real = nat.conv_dgrad2_x
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(nat, "conv_dgrad2_x", counted)
    return calls


def _fwd_bwd(act, t, k, dtype=torch.bfloat16, stride=1, seed=51):
    torch.manual_seed(seed)
    x = _cl(torch.randn(2, 64, 14, 14, device="cuda", dtype=dtype))
    w = torch.randn(64, 64, 3, 3, device="cuda")
    xl = x.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    out, _, _ = BinaryConvFunction.apply(xl, wl, stride, 1, act, t, k, False)
    (out.float() * torch.randn_like(out.float())).sum().backward()
    torch.cuda.synchronize()
    return xl.grad, wl.grad


@pytest.mark.parametrize("act,t,k", [("approx", None, None),
                                     ("ste", 1.0, 1.0)],
                         ids=["approx", "ede"])
def test_value_mask_backward_takes_owned_path(monkeypatch, act, t, k):
    nat = _nat()
    for name in ("binsign_decode", "decode_packed", "ste_mask_mul"):
        monkeypatch.setattr(nat, name, _raiser(name))
    calls = _count_dgrad2_x(monkeypatch)
    dx, dw = _fwd_bwd(act, t, k)
    assert len(calls) == 1
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all()


@pytest.mark.parametrize("act,t,k", [("approx", None, None),
                                     ("ste", 1.0, 1.0)],
                         ids=["approx", "ede"])
def test_value_mask_backward_knob_off_takes_fallback(monkeypatch, act, t, k):
    calls = _count_dgrad2_x(monkeypatch)
    old = bc._MFMA_BWD
    bc._MFMA_BWD = False
    try:
        dx, dw = _fwd_bwd(act, t, k)
    finally:
        bc._MFMA_BWD = old
    assert len(calls) == 0
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all()


@pytest.mark.parametrize("kw", [dict(dtype=torch.float32), dict(stride=2)],
                         ids=["fp32", "stride2"])
@pytest.mark.parametrize("act,t,k", [("approx", None, None),
                                     ("ste", 1.0, 1.0)],
                         ids=["approx", "ede"])
def test_value_mask_backward_unsupported_takes_fallback(monkeypatch, act, t,
                                                        k, kw):
    calls = _count_dgrad2_x(monkeypatch)
    dx, dw = _fwd_bwd(act, t, k, **kw)
    assert len(calls) == 0
    assert dx is not None and dw is not None
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all()


@pytest.mark.parametrize("act,t,k,mx", [("approx", None, None, 2.0),
                                        ("ste", 10.0, 1.0, 10.0)],
                         ids=["approx", "ede_t10_k1"])
@pytest.mark.parametrize("N,C,H,K", [(2, 64, 28, 64), (2, 64, 7, 128)])
def test_value_mask_backward_owned_vs_fallback(N, C, H, K, act, t, k, mx):
    """dx and dw of the owned path vs the BDBNN_MFMA_BWD=0 path."""
    torch.manual_seed(44)
    x = _cl(torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16))
    w = torch.randn(K, C, 3, 3, device="cuda")

    def run(flag):
        old = bc._MFMA_BWD
        bc._MFMA_BWD = flag
        try:
            xl = x.clone().requires_grad_(True)
            wl = w.clone().requires_grad_(True)
            out, _, _ = BinaryConvFunction.apply(
                xl, wl, 1, 1, act, t, k, False)
            (out.float() * torch.randn_like(out.float())).sum().backward()
            return xl.grad.float(), wl.grad.float()
        finally:
            bc._MFMA_BWD = old
    torch.manual_seed(45)
    dx2, dw2 = run(True)
    torch.manual_seed(45)
    dx1, dw1 = run(False)
    print(f"dx max diff {(dx2 - dx1).abs().max().item():.4g}, "
          f"dw max diff {(dw2 - dw1).abs().max().item():.4g}")
    assert torch.allclose(dx2, dx1, atol=5e-2 * mx, rtol=2e-2), \
        (dx2 - dx1).abs().max().item()
    assert torch.allclose(dw2, dw1, atol=5e-1, rtol=2e-2), \
        (dw2 - dw1).abs().max().item()


def test_react_block_defer_skip_grad_rides_dgrad2_x(monkeypatch):
    """BiBasicBlock with ReAct convs, bf16 autocast: the deferred skip
    gradient through conv_dgrad2_x's acc operand vs plain autograd
    accumulation (criteria of test_bi_block_defer_skip_grad_bf16_dgrad2_path)."""
    from bdbnn_amd.models import resnet_common as rc
    from bdbnn_amd.ops.binary_conv import HardBinaryConv_react
    torch.manual_seed(35)
    blk = rc.BiBasicBlock(64, 64, conv_cls=HardBinaryConv_react,
                          act="rprelu").cuda().to(
        memory_format=torch.channels_last)
    x0 = torch.randn(2, 64, 14, 14, device="cuda", dtype=torch.bfloat16)
    gout = torch.randn(2, 64, 14, 14, device="cuda", dtype=torch.bfloat16)
    calls = _count_dgrad2_x(monkeypatch)

    def run(defer):
        old = rc._FUSE_SKIP_GRAD
        rc._FUSE_SKIP_GRAD = defer
        try:
            blk.zero_grad(set_to_none=True)
            x = _cl(x0.clone()).requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = blk(x)
            if isinstance(out, tuple):
                out = out[0]
            out.backward(_cl(gout))
            return ([p.grad.clone() for p in blk.parameters()],
                    x.grad.clone())
        finally:
            rc._FUSE_SKIP_GRAD = old

    pg_d, xg_d = run(True)
    pg_p, xg_p = run(False)
    # conv1 sees the bf16 block input in both runs and owns the deferred
    # skip gradient of run(True); conv2's input comes out of RPReLU, whose
    # fp32 shift parameters promote it to fp32 under autocast (fallback)
    assert len(calls) >= 2
    assert torch.allclose(xg_d.float(), xg_p.float(), atol=3e-2,
                          rtol=2e-2), (xg_d.float() -
                                       xg_p.float()).abs().max().item()
    for a, b in zip(pg_d, pg_p):
        rel = (a.float() - b.float()).norm() / (b.float().norm() + 1e-12)
        assert rel.item() < 0.05, rel.item()


@pytest.mark.parametrize("recipe", ["react", "ede"])
def test_bf16_training_step_value_mask_models(monkeypatch, recipe):
    """One bf16-autocast step; also puts the owned path's real coverage
    on record.  ResNet-18 has 13 stride-1 3x3 binary convs (4 in layer1,
    3 in each later stage), all of dgrad2-supported shape here.

    EDE on the ChannelPReLU model: activations stay bf16, all 13 convs
    take conv_dgrad2_x.

    resnet18_react: RPReLU's fp32 shift parameters (LearnableBias)
    promote every block activation to fp32 under autocast, so only
    layer1.0.conv1 (fed by the bf16 stem) meets the bf16 predicate; the
    other 12 convs run the fp32 fallback, as they did before."""
    from bdbnn_amd.engine.trainer import ede_inject
    from bdbnn_amd.models import imagenet as im
    torch.manual_seed(36)
    calls = _count_dgrad2_x(monkeypatch)
    if recipe == "react":
        m = im.resnet18_react(False, num_classes=10)
    else:
        m = im.resnet18(False, num_classes=10)
        ede_inject(m, 10, 100)
    m = m.cuda().to(memory_format=torch.channels_last)
    x = _cl(torch.randn(8, 3, 64, 64, device="cuda"))
    y = torch.randint(0, 10, (8,), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(x)
        loss = torch.nn.functional.cross_entropy(out.float(), y)
    loss.backward()
    assert torch.isfinite(loss)
    print(f"{recipe}: conv_dgrad2_x calls = {len(calls)}")
    assert len(calls) == (1 if recipe == "react" else 13)
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        assert torch.isfinite(p.grad).all(), n
