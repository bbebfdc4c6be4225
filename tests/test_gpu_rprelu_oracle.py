"""The fused BN (+skip) + RPReLU tail (act_kind 3 of csrc/bn_act.hip)
against fp64 formulas, in the manner of test_gpu_bn_act_oracle.py and with
its inputs, shapes and constants (C_BOUND = 64, EPS24, BF16_RND,
KINK_CAP), but driven through the public op: fused_bn_act(x, bn, RPReLU,
skip=..., pack=...) with bn_act._FUSE_RPRELU patched on, gradients taken
by autograd, so which gradient lands on which parameter, and in what
shape, is under the oracle too.

  z = BN(x) (+ skip);  u = z + b1;  out = (u > 0 ? u : a u) + b2

Bounds, on top of that file's B_z and amp = c eps (1 + r^2):
  B_u  = B_z + amp |b1|
  out  |out - ref| <= B_u + amp |b2|          (|a| <= 1: PReLU 1-Lipschitz)
  dx, dskip, dgamma, dbeta, da: that file's PReLU bounds with u, B_u in
        place of z, B_z (kink band |u_ref| < B_u, in bf16 as in fp32: the
        saved plane holds u itself and rounding keeps its sign, so no
        element outside the band may take the other branch)
  db1  the dbeta bound, and bit-for-bit equal to the returned dbeta
  db2  amp sum|dy|
  each bf16-stored tensor adds 2^-8 |ref|; da in bf16 adds 2^-8 sum|dy u|
  eval (running stats, no variance is formed, so no (1 + r^2)):
        c eps (|g| (|x - rm| + |rm|) / sqrt(rv + eps) + |beta| + |skip|
               + |b1| + |b2|)
Elements in the kink band are left out of the elementwise dx / dskip
comparison, enter the sum bounds as in that file, and may be at most
KINK_CAP = 0.1 % of a tensor.

Measured on an MI355X (largest figure over all cases of this file and two
runs; the atomics make them vary from run to run; every test prints its
own before it asserts):
  err / bound, fp32: out 0.065, eval out 0.050, dx 0.12, dskip 0.016,
      dbeta = db1 0.096, dgamma 0.13, db2 0.021, da 0.30
  err / bound, bf16: out 0.995, eval out 0.993, dx 0.995, dskip 0.987 (the
      2^-8 rounding term is attained), dbeta = db1 0.026, dgamma 0.033,
      db2 0.004, da 0.78
  elements left out at the kink: at most 0.030 % of a tensor ((2, 64, 33),
      the same figure from the reference alone on the CPU)
  No case needed a kernel change.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_bn_act_oracle as bo
from test_gpu_bn_act_oracle import (BF16, BF16_RND, BN_EPS, C_BOUND, EPS24,
                                    FP32, KINK_CAP, LARGE, SMALL, _Case,
                                    _Ref, _ratio, _rows)

from bdbnn_amd import _C
from bdbnn_amd.ops import bn_act
from bdbnn_amd.ops.activations import RPReLU
from bdbnn_amd.ops.bn_act import fused_bn_act

_MEASURED = {}


def _note(key, value):
    value = float(value)
    if not (value <= _MEASURED.get(key, -1.0)):
        _MEASURED[key] = value


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _MEASURED:
        print("\n[rprelu oracle] largest measured figures")
        for k in sorted(_MEASURED):
            print(f"  {k:28s} {_MEASURED[k]:.4g}")


@pytest.fixture(autouse=True)
def _knob_on(monkeypatch):
    monkeypatch.setattr(bn_act, "_FUSE_RPRELU", True)


# ---------------------------------------------------------------- inputs

class _RCase(_Case):
    """_Case's PReLU inputs plus the two shifts: b1, b2 in [-0.5, 0.5],
    mixed signs, from a generator of their own (x, dy, a ... stay what
    _Case makes of the seed)."""

    def __init__(self, shape, dtype, with_skip, seed):
        super().__init__(shape, dtype, "prelu", with_skip, seed=seed)
        g = torch.Generator().manual_seed(5000 + seed)
        self.b1 = torch.rand(self.C, generator=g) - 0.5
        self.b2 = torch.rand(self.C, generator=g) - 0.5
        for b in (self.b1, self.b2):
            assert (b > 0).any() and (b < 0).any()


class _RRef(_Ref):
    """fp64 RPReLU tail on top of _Ref's BN (+skip).  After __init__,
    self.z / self.Bz hold u / B_u, so that _Ref.backward computes the
    PReLU backward and its bounds "with u in place of z" unchanged."""

    def __init__(self, case, dev):
        super().__init__(case, dev)
        self.b1 = case.b1.to(dev).double()
        self.b2 = case.b2.to(dev).double()
        self.z = self.z + self.b1
        self.Bz = self.Bz + self.amp * self.b1.abs()
        u = self.z
        self.out = torch.where(u > 0, u, self.a * u) + self.b2
        self.B_out = self.Bz + self.amp * self.b2.abs()

    def backward(self, case):
        super().backward(case)
        DY = _rows(case.dy.to(self.dev)).double()
        self.db2 = DY.sum(0)
        self.B_db2 = self.amp * DY.abs().sum(0)


def _modules(case):
    bn = torch.nn.BatchNorm2d(case.C, eps=BN_EPS, momentum=bo.MOMENTUM).cuda()
    act = RPReLU(case.C).cuda()
    with torch.no_grad():
        bn.weight.copy_(case.gamma)
        bn.bias.copy_(case.beta)
        bn.running_mean.copy_(case.rm0)
        bn.running_var.copy_(case.rv0)
        act.move1.bias.copy_(case.b1.view(1, -1, 1, 1))
        act.prelu.weight.copy_(case.a)
        act.move2.bias.copy_(case.b2.view(1, -1, 1, 1))
    return bn, act


def _run(case, want_pack, ref_dev, tag):
    """training forward + autograd backward of one case, checked"""
    nat = _C.native_required()
    bf = case.dtype == BF16
    sfx = "bf16" if bf else "fp32"
    bn, act = _modules(case)
    bn.train()
    x = case.x.cuda().requires_grad_(True)
    skip = None if case.skip is None else case.skip.cuda().requires_grad_(True)
    res = fused_bn_act(x, bn, act, skip=skip, pack=want_pack)
    out, pk = res if want_pack else (res, None)
    assert out.dtype == case.dtype and out.shape == x.shape
    assert out.is_contiguous(memory_format=torch.channels_last)
    # the fused op, not the composition: one autograd node made `out`
    assert type(out.grad_fn).__name__ == "_BNActFnBackward"
    out.backward(case.dy.cuda())

    ref = _RRef(case, ref_dev)
    # ---- forward
    k = _rows(out.detach()).to(ref.dev).double()
    B = ref.B_out + (BF16_RND * ref.out.abs() if bf else 0)
    q_out = _ratio((k - ref.out).abs(), B)
    _note(f"err/bound out {sfx}", q_out)
    print(f"[{tag}] fwd err/bound out:{q_out:.3g}")
    assert q_out <= 1.0, q_out
    assert bn.num_batches_tracked.item() == 1
    if want_pack:
        assert pk is not None, "C % 32 == 0 must produce a pack"
        xpk, mpk = pk
        o = out.detach()
        assert torch.equal(xpk, nat.sign_pack_nhwc(o)), "sign plane"
        assert torch.equal(mpk, nat.sign_mask_pack_nhwc(o)[1]), "mask plane"

    # ---- backward
    ref.backward(case)
    share = ref.kink.double().mean().item()
    _note("kink share", share)
    keep = ~ref.kink
    figs = {}
    for name, got, r, Bd in (("dx", x.grad, ref.dx, ref.B_dx),
                             ("dskip", None if skip is None else skip.grad,
                              ref.dz, ref.B_dz)):
        if got is None:
            continue
        assert got.dtype == case.dtype and got.shape == x.shape
        kk = _rows(got).to(ref.dev).double()
        Bd = Bd + (BF16_RND * r.abs() if bf else 0)
        figs[name] = _ratio((kk - r).abs()[keep], Bd[keep])
    d = lambda t: t.detach().reshape(-1).to(ref.dev).double()
    p_b1, p_a, p_b2 = act.move1.bias, act.prelu.weight, act.move2.bias
    for p in (bn.weight, bn.bias, p_b1, p_a, p_b2):
        assert p.grad is not None
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype
    figs["dbeta"] = _ratio((d(bn.bias.grad) - ref.dbeta).abs(), ref.B_dbeta)
    figs["dgamma"] = _ratio((d(bn.weight.grad) - ref.dgamma).abs(),
                            ref.B_dgamma)
    figs["db1"] = _ratio((d(p_b1.grad) - ref.dbeta).abs(), ref.B_dbeta)
    figs["db2"] = _ratio((d(p_b2.grad) - ref.db2).abs(), ref.B_db2)
    B_da = ref.B_da + (BF16_RND * ref.S_dyz if bf else 0)
    figs["da"] = _ratio((d(p_a.grad) - ref.da).abs(), B_da)
    for name, v in figs.items():
        _note(f"err/bound {name} {sfx}", v)
    print(f"[{tag}] bwd err/bound "
          + " ".join(f"{n}:{v:.3g}" for n, v in figs.items())
          + f" | kink share {100 * share:.4f} %")
    assert share <= KINK_CAP, share
    for name, v in figs.items():
        assert v <= 1.0, (name, v)
    assert torch.equal(p_b1.grad.reshape(-1), bn.bias.grad), \
        "db1 is the number dbeta is"


def _case_id(shape, dtype, skip, pack=False):
    return (f"{shape[0]}x{shape[1]}x{shape[2]}-"
            f"{'bf16' if dtype == BF16 else 'fp32'}"
            f"{'-skip' if skip else ''}{'-pack' if pack else ''}")


# one skip setting per dtype on each large shape, rotated so that fp32 and
# bf16 each run with and without skip: (shape, dtype, skip, pack)
LARGE_CASES = [
    (LARGE[0], FP32, True, False),
    (LARGE[0], BF16, False, False),
    (LARGE[1], FP32, False, True),
    (LARGE[1], BF16, True, True),
    (LARGE[2], FP32, True, True),
    (LARGE[2], BF16, False, True),
]


@pytest.mark.parametrize("shape,dtype,skip,pack", LARGE_CASES,
                         ids=[_case_id(*c) for c in LARGE_CASES])
def test_rprelu_main_loops(shape, dtype, skip, pack):
    """~18.8 M elements: the grid is capped at 2048 blocks, so the 2x
    unrolled bodies of both backward kernels and their tails run."""
    N, C, HW = shape
    rows = 256 // (C // 8)
    n_pix = N * HW * HW
    assert (n_pix + rows - 1) // rows > 2048 and n_pix % rows != 0
    case = _RCase(shape, dtype, skip, seed=100 + LARGE.index(shape))
    _run(case, pack, "cuda", _case_id(shape, dtype, skip, pack))


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("shape", SMALL, ids=[f"{n}x{c}x{h}"
                                              for n, c, h in SMALL])
def test_rprelu_small_shapes(shape, skip, dtype):
    """Both ends of chan_map8, one partial block, and 35 / 69 / 38 blocks
    for the wrap of the 32-way sliced four-row partial sums."""
    C = shape[1]
    case = _RCase(shape, dtype, skip, seed=110 + SMALL.index(shape))
    _run(case, C % 32 == 0, "cpu", _case_id(shape, dtype, skip))


def test_kink_cap_holds_for_the_reference_alone():
    """The cap means something only if the fp64 reference by itself marks
    fewer elements: every small case, on the CPU (the large cases
    recompute the share on the device; it depends on the reference
    alone)."""
    worst = 0.0
    for shape in SMALL:
        for skip in (False, True):
            for dtype in (FP32, BF16):
                case = _RCase(shape, dtype, skip,
                              seed=110 + SMALL.index(shape))
                ref = _RRef(case, "cpu")
                ref.backward(case)
                worst = max(worst, ref.kink.double().mean().item())
    print(f"[kink] reference-only share, small cases: {100 * worst:.4f} %")
    assert worst < KINK_CAP


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("shape", SMALL, ids=[f"{n}x{c}x{h}"
                                              for n, c, h in SMALL])
def test_rprelu_eval_against_running_stats_formula(shape, skip, dtype):
    """no_grad + eval mode: bn_act_eval with kind 3 against the fp64
    running-stats formula."""
    bf = dtype == BF16
    case = _RCase(shape, dtype, skip, seed=120 + SMALL.index(shape))
    bn, act = _modules(case)
    bn.eval()
    x = case.x.cuda()
    s = None if case.skip is None else case.skip.cuda()
    with torch.no_grad():
        out, pk = fused_bn_act(x, bn, act, skip=s, pack=True)
    assert pk is None and out.dtype == dtype and out.shape == x.shape
    assert torch.equal(bn.running_mean.cpu(), case.rm0)   # untouched
    D = lambda t: t.double()
    X = _rows(case.x).double()
    S = None if case.skip is None else _rows(case.skip).double()
    g, be, a = D(case.gamma), D(case.beta), D(case.a)
    b1, b2, rm = D(case.b1), D(case.b2), D(case.rm0)
    istd = 1.0 / (D(case.rv0) + BN_EPS).sqrt()
    u = g * (X - rm) * istd + be + b1
    if S is not None:
        u = u + S
    ref = torch.where(u > 0, u, a * u) + b2
    B = C_BOUND * EPS24 * (g.abs() * ((X - rm).abs() + rm.abs()) * istd
                           + be.abs() + b1.abs() + b2.abs()
                           + (S.abs() if S is not None else 0))
    if bf:
        B = B + BF16_RND * ref.abs()
    q = _ratio((_rows(out).cpu().double() - ref).abs(), B)
    _note(f"err/bound eval out {'bf16' if bf else 'fp32'}", q)
    print(f"[eval {_case_id(shape, dtype, skip)}] err/bound out:{q:.3g}")
    assert q <= 1.0, q


def test_kind3_bindings_reject_missing_or_short_vectors():
    """bn_act_fwd_train / bn_act_eval with kind 3 raise without a, b1 or
    b2, or with one of them not C long; bn_act_bwd without a; and on a
    channel count the vec8 kernels cannot index."""
    nat = _C.native_required()
    C = 16
    x = torch.randn(2, C, 4, 4, device="cuda").contiguous(
        memory_format=torch.channels_last)
    v = lambda n=C: torch.ones(n, device="cuda")
    fwd = lambda a, b1, b2, xx=x: nat.bn_act_fwd_train(
        xx, None, v(xx.shape[1]), v(xx.shape[1]), a, None, None, 0.1, BN_EPS,
        3, None, None, False, b1, b2)
    ev = lambda a, b1, b2: nat.bn_act_eval(
        x, None, v(), v(), a, v(), v(), BN_EPS, 3, b1, b2)
    for call in (fwd, ev):
        for args in ((None, v(), v()), (v(), None, v()), (v(), v(), None),
                     (v(8), v(), v()), (v(), v(8), v()), (v(), v(), v(8))):
            with pytest.raises(RuntimeError):
                call(*args)
    with pytest.raises(RuntimeError):       # trailing arguments left out
        nat.bn_act_fwd_train(x, None, v(), v(), v(), None, None, 0.1, BN_EPS,
                             3, None, None, False)
    with pytest.raises(RuntimeError):
        nat.bn_act_bwd(x, x, x, v(), v(), v(), None, 3, False)
    x48 = torch.randn(2, 48, 4, 4, device="cuda").contiguous(
        memory_format=torch.channels_last)
    with pytest.raises(RuntimeError):
        fwd(v(48), v(48), v(48), x48)
    # the valid call: four results, then seven from backward
    res = fwd(v() * 0.25, v() * 0.1, v() * -0.1)
    assert len(res) == 4
    back = nat.bn_act_bwd(x, res[1], x, res[2], res[3], v(), v() * 0.25, 3,
                          False)
    assert len(back) == 7 and all(t.shape == (C,) for t in back[2:])
    assert torch.equal(back[5], back[3])
