"""The "8 channels per thread" elementwise family (csrc/bn_act.hip,
csrc/prelu.hip, indexed by csrc/vec8.h) against fp64 formulas written out
here, at the shapes where its unrolled main loops, both ends of chan_map8
and the wrap of the 32-way sliced partial sums run, on channels whose
mean is not zero, within bounds derived from the number formats.

Bounds.  eps = 2^-24 (fp32 unit roundoff), c = C_BOUND, r = |mean| / std
of a channel in the fp64 reference.  bn_finalize forms the variance as
E[x^2] - mean^2 in fp32, whose relative error grows like (1 + r^2), so
every bound that depends on invstd carries that factor:

  var      |var - ref| / ref          <= c eps (1 + r^2)
  mean     |mean - ref|               <= c eps (|mean| + std)   (a sum)
  out, z   |out - ref| <= c eps (1 + r^2) (|g| (|x - mean| + |mean|) / std
                                           + |beta| + |skip|)   [B_z]
  dx       same form with |g| / std (|dz| + mean|dz| + |xhat| mean|dz xhat|)
  dbeta, dgamma, da   c eps (1 + r^2) sum|terms|
  bf16 stores add 2^-8 |ref| (one rounding); da in bf16 adds
  2^-8 sum|dy z| because the saved z is rounded.

Activation kink: an element with |z_ref| < B_z may take the other branch
in the kernel.  PReLU with |a| <= 1 and ReLU are 1-Lipschitz, so `out`
keeps its bound there; dz does not, so such elements are left out of the
elementwise dx / dskip comparison, their |1 - a| |dy| (times 1 or |xhat|)
is added to the sum bounds and, through the sums, to the dx bound, and
they may be at most 0.1 % of a tensor.

The forward bound B_z is used as stated above; it has no term of its own
for the error of the mean (see _Case on beta).

Measured on an MI355X (the largest figure over all cases of this file and
two runs; the atomics make them vary from run to run; every test prints
its own before it asserts):
  variance constant |var - ref| / (ref eps (1 + r^2)) per nominal r:
      r=0: 8.4   r=1: 7.5   r=4: 10.4   r=32: 7.3   r=256: 7.6
    on the mean-offset case alone (fp32): 3.0 / 5.3 / 8.6 / 5.3 / 7.6, and
    torch's own GPU BatchNorm on that input, for comparison only:
      r=0: 2.0   r=1: 1.0   r=4: 0.10   r=32: 0.006   r=256: 0.0006
    (it centres before squaring, so its error does not grow with r; ours
    stays within c = 64 up to r = 256 because eps (1 + r^2) is the model)
  err / bound, fp32: var 0.16, mean 0.07, running stats 0.22, out 0.074,
      z 0.074, dskip 0.016, da 0.067, PReLU-alone da 0.021, conv s1 0.004,
      conv s2 0.03; dx 0.96, dbeta 0.96, dgamma 0.91 where an element at
      the kink did flip (its own |1 - a| |dy| is then error and bound
      alike), a few percent otherwise
  err / bound, bf16: 0.99 for every stored tensor (the 2^-8 rounding term
      is attained), da 0.52
  elements left out at the activation kink: at most 0.010 % of a tensor
  No case, r <= 4 or above, needed a kernel change.
"""

import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops.activations import ChannelPReLU
from bdbnn_amd.ops.binarize import binsign, weight_scale
from bdbnn_amd.ops.bn_act import fused_bn_act

EPS24 = 2.0 ** -24
# c: a CPU model of the sliced single-pass accumulation gave 0.8-4.0, so 64
# leaves 16x over the model.  Largest measured on an MI355X: 10.4 (r = 4;
# 8.4 at r = 0, 7.6 at r = 256), which leaves 6x.  torch's own GPU
# BatchNorm on the mean-offset input: 2.0 at r = 0, 0.10 at r = 4, 0.0006
# at r = 256 (comparison only, nothing here asserts it).
C_BOUND = 64.0
BF16_RND = 2.0 ** -8
BN_EPS = 1e-5
MOMENTUM = 0.1
KINK_CAP = 1e-3

FP32, BF16 = torch.float32, torch.bfloat16
ACTS = {"none": 0, "prelu": 1, "relu": 2}

# (N, C, H=W).  LARGE: grid capped at 2048 blocks and n_pix ~ 4.5 pstep,
# not a multiple of rows = 256 / (C/8): one thread runs the 4x stats body
# and its tail, the 2x backward bodies twice and their tail.
LARGE = [(9, 8, 511), (5, 64, 243), (1, 1024, 135)]
# SMALL: 9 pixels < rows = 256 (one block, most threads idle); 35 / 69 /
# 38 blocks (the slice index blockIdx & 31 wraps, last block partial)
SMALL = [(1, 8, 3), (1, 32, 47), (2, 64, 33), (3, 1024, 5)]
RATIOS = (0.0, 1.0, 4.0)
HIGH_RATIOS = (0.0, 1.0, 4.0, 32.0, 256.0)

_MEASURED = {}


def _nat():
    return _C.native_required()


def _rows(t):
    """logical (N,C,H,W), channels_last memory -> the [pixels, C] view"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(rows, N, C, HW):
    """[pixels, C] -> logical (N,C,H,W) in channels_last memory"""
    return rows.reshape(N, HW, HW, C).permute(0, 3, 1, 2)


def _note(key, value):
    value = float(value)
    if not (value <= _MEASURED.get(key, -1.0)):
        _MEASURED[key] = value


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _MEASURED:
        print("\n[bn_act oracle] largest measured figures")
        for k in sorted(_MEASURED):
            print(f"  {k:28s} {_MEASURED[k]:.4g}")


def _ratio(err, bound):
    """max err / bound, nan-safe: a nan error is an infinite ratio"""
    q = err / bound
    q = torch.where(err == 0, torch.zeros_like(q), q)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return q.max().item() if q.numel() else 0.0


# ---------------------------------------------------------------- inputs

class _Case:
    """Inputs of one BN(+skip)(+act) case, made on the CPU from a seed so
    that the same data is there with and without a GPU.  Channel c is
    mu_c + sigma_c * randn with |mu_c| / sigma_c cycling over `ratios`."""

    def __init__(self, shape, dtype, act, with_skip, ratios=RATIOS, seed=0):
        N, C, HW = shape
        self.shape, self.dtype, self.act = shape, dtype, act
        self.N, self.C, self.HW = N, C, HW
        self.P = N * HW * HW
        g = torch.Generator().manual_seed(1000 + seed)
        ch = torch.arange(C)
        self.nominal_r = torch.tensor(ratios)[ch % len(ratios)]
        sigma = 0.5 + 1.5 * torch.rand(C, generator=g)
        mu = self.nominal_r * sigma * torch.where(ch % 2 == 0, 1.0, -1.0)
        x = torch.randn(self.P, C, generator=g).mul_(sigma).add_(mu)
        self.x = _nchw(x.to(dtype), N, C, HW)
        self.skip = None
        if with_skip:
            self.skip = _nchw(torch.randn(self.P, C, generator=g).to(dtype),
                              N, C, HW)
        self.dy = _nchw(torch.randn(self.P, C, generator=g).to(dtype),
                        N, C, HW)
        self.gamma = (0.5 + torch.rand(C, generator=g)) * \
            torch.where(ch % 5 == 3, -1.0, 1.0)
        # |beta| >= 0.25: B_z has no term of its own for the error of the
        # mean (|g| d_mean / std <= c eps |g| (1 + r)); |beta|, |skip| or
        # |mean| cover it.  With all three ~0 the bound vanishes at x = mean
        # and only the kernel's arithmetic, not the bound, would be at fault.
        self.beta = (0.25 + 0.25 * torch.rand(C, generator=g)) * \
            torch.where(ch % 3 == 1, -1.0, 1.0)
        # |a| <= 1 keeps PReLU 1-Lipschitz (see the module docstring)
        self.a = (torch.rand(C, generator=g) - 0.4) if act == "prelu" else None
        self.rm0 = 2 * torch.rand(C, generator=g) - 1
        self.rv0 = 0.5 + 1.5 * torch.rand(C, generator=g)


class _Ref:
    """The fp64 formulas, from the kernel's exact inputs, on device dev."""

    def __init__(self, case, dev):
        d = lambda t: None if t is None else t.to(dev).double()
        X = _rows(case.x.to(dev)).double()
        S = None if case.skip is None else _rows(case.skip.to(dev)).double()
        self.dev, self.act, self.n = dev, case.act, X.shape[0]
        self.gamma, self.beta, self.a = d(case.gamma), d(case.beta), d(case.a)
        n = self.n
        self.mean = X.mean(0)
        xc = X - self.mean
        self.var = (xc * xc).mean(0)                      # biased
        self.std = self.var.sqrt()
        self.invstd = 1.0 / (self.var + BN_EPS).sqrt()
        self.xhat = xc * self.invstd
        self.z = self.gamma * self.xhat + self.beta
        if S is not None:
            self.z = self.z + S
        if case.act == "prelu":
            self.out = torch.where(self.z > 0, self.z, self.a * self.z)
        elif case.act == "relu":
            self.out = self.z.clamp_min(0)
        else:
            self.out = self.z
        self.run_mean = (1 - MOMENTUM) * d(case.rm0) + MOMENTUM * self.mean
        self.var_unb = self.var * n / max(n - 1, 1)
        self.run_var = (1 - MOMENTUM) * d(case.rv0) + MOMENTUM * self.var_unb
        self.rm0, self.rv0 = d(case.rm0), d(case.rv0)
        # bounds
        self.r2 = self.mean ** 2 / self.var
        self.amp = C_BOUND * EPS24 * (1 + self.r2)                     # [C]
        self.Bz = self.amp * (self.gamma.abs() * (xc.abs() + self.mean.abs())
                              / self.std + self.beta.abs()
                              + (S.abs() if S is not None else 0))

    def backward(self, case):
        """fills dz, dx, dskip, dbeta, dgamma, da and their bounds"""
        DY = _rows(case.dy.to(self.dev)).double()
        n, z, xhat = self.n, self.z, self.xhat
        if self.act == "prelu":
            slope = torch.where(z > 0, torch.ones_like(z), self.a.expand_as(z))
            one_minus_a = (1 - self.a).abs()
        elif self.act == "relu":
            slope = (z > 0).double()
            one_minus_a = torch.ones_like(self.mean)
        else:
            slope = torch.ones_like(z)
            one_minus_a = torch.zeros_like(self.mean)
        dz = DY * slope
        if self.act == "none":
            self.kink = torch.zeros_like(z, dtype=torch.bool)
        else:
            self.kink = z.abs() < self.Bz
        kd = self.kink.double() * DY.abs() * one_minus_a
        K0, K1 = kd.sum(0), (kd * xhat.abs()).sum(0)
        self.dz = dz
        self.dbeta = dz.sum(0)
        self.dgamma = (dz * xhat).sum(0)
        gis = self.gamma * self.invstd
        self.dx = gis * (dz - self.dbeta / n - xhat * self.dgamma / n)
        self.B_dbeta = self.amp * dz.abs().sum(0) + K0
        self.B_dgamma = self.amp * (dz * xhat).abs().sum(0) + K1
        g_std = self.gamma.abs() / self.std
        self.B_dx = (self.amp * g_std * (dz.abs() + dz.abs().mean(0)
                                         + xhat.abs() * (dz * xhat).abs().mean(0))
                     + g_std * (K0 / n + xhat.abs() * K1 / n))
        self.B_dz = self.amp * dz.abs()
        if self.act == "prelu":
            neg = (z <= 0).double()
            self.da = (neg * DY * z).sum(0)
            self.S_dyz = (neg * (DY * z).abs()).sum(0)
            # a kinked element enters with z_ref, with the kernel's z
            # (|z_k| < 2 B_z), or not at all
            self.B_da = (self.amp * self.S_dyz
                         + (self.kink.double() * DY.abs() * 2 * self.Bz).sum(0))


def _per_r(case, const):
    """largest variance constant per nominal r of the case"""
    out = {}
    for r in sorted(set(case.nominal_r.tolist())):
        sel = (case.nominal_r == r).to(const.device)
        out[r] = const[sel].max().item()
    return out


def _check_stats(case, ref, mean, invstd, tag, key="var const"):
    """mean / invstd as the kernel returns them; prints, then asserts"""
    var_k = 1.0 / invstd.to(ref.dev).double() ** 2 - BN_EPS
    const = (var_k - ref.var).abs() / (ref.var * EPS24 * (1 + ref.r2))
    per_r = _per_r(case, const)
    for r, v in per_r.items():
        _note(f"{key} r={r:g}", v)
    e_mean = (mean.to(ref.dev).double() - ref.mean).abs()
    B_mean = C_BOUND * EPS24 * (ref.mean.abs() + ref.std)
    q_mean = _ratio(e_mean, B_mean)
    _note("err/bound var", const.max().item() / C_BOUND)
    _note("err/bound mean", q_mean)
    print(f"[{tag}] var const per r "
          + " ".join(f"r={r:g}:{v:.3g}" for r, v in per_r.items())
          + f" | mean err/bound {q_mean:.3g}")
    assert (const <= C_BOUND).all(), per_r
    assert (e_mean <= B_mean).all(), q_mean
    return per_r


def _check_fwd(case, ref, got, tag):
    """got: out, and optionally z, run_mean, run_var (device tensors)"""
    bf = case.dtype == BF16
    figs = {}
    for name, r in (("out", ref.out), ("z", ref.z)):
        if got.get(name) is None:
            continue
        k = _rows(got[name]).to(ref.dev).double()
        B = ref.Bz + (BF16_RND * r.abs() if bf else 0)
        figs[name] = _ratio((k - r).abs(), B)
        _note(f"err/bound {name} {'bf16' if bf else 'fp32'}", figs[name])
    # (1 - m) r0 + m stat in fp32 is at most 6 roundings on top of the
    # stat's own error (1 - m, two products, the sum; var_unb adds a
    # product and a quotient): 8 eps of the two terms covers them
    for name, k, r, r0, stat, B_stat in (
            ("run_mean", got.get("run_mean"), ref.run_mean, ref.rm0,
             ref.mean, C_BOUND * EPS24 * (ref.mean.abs() + ref.std)),
            ("run_var", got.get("run_var"), ref.run_var, ref.rv0,
             ref.var_unb, ref.amp * ref.var_unb)):
        if k is None:
            continue
        B = MOMENTUM * B_stat + 8 * EPS24 * ((1 - MOMENTUM) * r0.abs()
                                             + MOMENTUM * stat.abs())
        figs[name] = _ratio((k.to(ref.dev).double() - r).abs(), B)
        _note("err/bound running stats", figs[name])
    print(f"[{tag}] fwd err/bound "
          + " ".join(f"{k}:{v:.3g}" for k, v in figs.items()))
    for name, v in figs.items():
        assert v <= 1.0, (name, v)


def _check_bwd(case, ref, got, tag):
    """got: dx, dgamma, dbeta and optionally dskip, da"""
    bf = case.dtype == BF16
    ref.backward(case)
    share = ref.kink.double().mean().item()
    _note("kink share", share)
    keep = ~ref.kink
    figs = {}
    for name, r, B in (("dx", ref.dx, ref.B_dx), ("dskip", ref.dz, ref.B_dz)):
        if got.get(name) is None:
            continue
        k = _rows(got[name]).to(ref.dev).double()
        B = B + (BF16_RND * r.abs() if bf else 0)
        figs[name] = _ratio((k - r).abs()[keep], B[keep])
    figs["dbeta"] = _ratio((got["dbeta"].to(ref.dev).double() - ref.dbeta).abs(),
                           ref.B_dbeta)
    figs["dgamma"] = _ratio((got["dgamma"].to(ref.dev).double()
                             - ref.dgamma).abs(), ref.B_dgamma)
    if case.act == "prelu":
        B = ref.B_da + (BF16_RND * ref.S_dyz if bf else 0)
        figs["da"] = _ratio((got["da"].to(ref.dev).double() - ref.da).abs(), B)
    for name, v in figs.items():
        _note(f"err/bound {name} {'bf16' if bf else 'fp32'}", v)
    print(f"[{tag}] bwd err/bound "
          + " ".join(f"{k}:{v:.3g}" for k, v in figs.items())
          + f" | kink share {100 * share:.4f} %")
    assert share <= KINK_CAP, share
    for name, v in figs.items():
        assert v <= 1.0, (name, v)


def _planes(out):
    """(sign, mask) bit planes of a stored activation, built on the CPU:
    bit c%32 of word c//32 is out >= 0, resp. |out| <= 1"""
    o = _rows(out).float().cpu()
    P, C = o.shape
    sh = torch.arange(32, dtype=torch.int64)
    pk = lambda b: (b.view(P, C // 32, 32).to(torch.int64) << sh).sum(-1)
    return pk(o >= 0), pk(o.abs() <= 1)


def _words(t):
    return t.cpu().reshape(-1, t.shape[-1]).to(torch.int64) & 0xffffffff


def _run_native(case, want_pack, ref_dev, tag):
    """bn_act_fwd_train + bn_act_bwd called directly on one case"""
    nat = _nat()
    cu = lambda t: None if t is None else t.cuda()
    x, skip, dy = cu(case.x), cu(case.skip), cu(case.dy)
    gamma, beta, a = cu(case.gamma), cu(case.beta), cu(case.a)
    rm, rv = cu(case.rm0).clone(), cu(case.rv0).clone()
    kind = ACTS[case.act]
    res = nat.bn_act_fwd_train(x, skip, gamma, beta, a, rm, rv, MOMENTUM,
                               BN_EPS, kind, None, None, want_pack)
    out, z, mean, invstd = res[:4]
    assert out.dtype == case.dtype and out.shape == x.shape
    assert out.is_contiguous(memory_format=torch.channels_last)
    ref = _Ref(case, ref_dev)
    _check_stats(case, ref, mean, invstd, tag)
    _check_fwd(case, ref, dict(out=out, z=z if kind == 1 else None,
                               run_mean=rm, run_var=rv), tag)
    if want_pack:
        sp, mp = _planes(out)
        assert torch.equal(_words(res[4]), sp), "sign plane"
        assert torch.equal(_words(res[5]), mp), "mask plane"
    dx, dskip, dgamma, dbeta, da = nat.bn_act_bwd(
        dy, z, x, mean, invstd, gamma, a, kind, skip is not None)
    assert dx.dtype == case.dtype
    _check_bwd(case, ref, dict(dx=dx, dskip=dskip if skip is not None else None,
                               dgamma=dgamma, dbeta=dbeta, da=da), tag)


# ------------------------------------------------- the CPU side of the cap

def _reference_kink_share(case):
    ref = _Ref(case, "cpu")
    ref.backward(case)
    return ref.kink.double().mean().item()


# one act/skip combination per dtype on each large shape, rotated so that
# every act kind and want_pack occur: (shape, dtype, act, skip, pack)
LARGE_CASES = [
    (LARGE[0], FP32, "prelu", True, False),
    (LARGE[0], BF16, "relu", False, False),
    (LARGE[1], FP32, "relu", True, True),
    (LARGE[1], BF16, "prelu", False, True),
    (LARGE[2], FP32, "none", True, False),
    (LARGE[2], BF16, "prelu", True, True),
]


def _case_id(shape, dtype, act, skip, pack=False):
    return (f"{shape[0]}x{shape[1]}x{shape[2]}-"
            f"{'bf16' if dtype == BF16 else 'fp32'}-{act}"
            f"{'-skip' if skip else ''}{'-pack' if pack else ''}")


# ------------------------------------------------------------ BN, direct

@pytest.mark.parametrize("shape,dtype,act,skip,pack", LARGE_CASES,
                         ids=[_case_id(*c) for c in LARGE_CASES])
def test_bn_act_main_loops(shape, dtype, act, skip, pack):
    """~18.8 M elements: the unrolled bodies of bn_stats (4x) and of both
    backward kernels (2x), their tails, the capped grid."""
    N, C, HW = shape
    rows = 256 // (C // 8)
    n_pix = N * HW * HW
    pstep = 2048 * rows
    assert (n_pix + rows - 1) // rows > 2048 and n_pix % rows != 0
    assert 4 * pstep < n_pix < 5 * pstep
    case = _Case(shape, dtype, act, skip, seed=LARGE.index(shape))
    _run_native(case, pack, "cuda", _case_id(shape, dtype, act, skip, pack))


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("shape", SMALL, ids=[f"{n}x{c}x{h}"
                                              for n, c, h in SMALL])
def test_bn_act_small_shapes(shape, act, skip, dtype):
    """Both ends of chan_map8 (C=8: 256 rows per block, C=1024: 2), one
    partial block, and 35 / 69 / 38 blocks for the slice wrap."""
    N, C, HW = shape
    rows = 256 // (C // 8)
    blocks = (N * HW * HW + rows - 1) // rows
    assert blocks == {8: 1, 32: 35, 64: 69, 1024: 38}[C]
    case = _Case(shape, dtype, act, skip, seed=10 + SMALL.index(shape))
    _run_native(case, C % 32 == 0, "cpu", _case_id(shape, dtype, act, skip))


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_bn_act_mean_offset(dtype):
    """r = |mean| / std up to 256 on (2, 64, 33): the single-pass variance
    against its (1 + r^2) bound, beside torch's own GPU BatchNorm (printed
    for comparison, not asserted).  Identity activation, so that no
    element sits at a kink whatever the bound is."""
    shape = (2, 64, 33)
    case = _Case(shape, dtype, "none", True, ratios=HIGH_RATIOS, seed=20)
    _run_native(case, True, "cpu", f"mean-offset-{dtype}")
    # torch: momentum 1 leaves the unbiased batch variance in running_var
    x = case.x.cuda()
    rm = torch.zeros(case.C, device="cuda")
    rv = torch.ones(case.C, device="cuda")
    F.batch_norm(x, rm, rv, None, None, True, 1.0, BN_EPS)
    ref = _Ref(case, "cpu")
    var_t = rv.cpu().double() * (case.P - 1) / case.P
    const_t = (var_t - ref.var).abs() / (ref.var * EPS24 * (1 + ref.r2))
    per_r = _per_r(case, const_t)
    for r, v in per_r.items():
        _note(f"torch var const r={r:g}", v)
    print(f"[mean-offset-{dtype}] torch var const per r "
          + " ".join(f"r={r:g}:{v:.3g}" for r, v in per_r.items()))


def test_kink_cap_holds_for_the_reference_alone():
    """The 0.1 % cap on elements left out at the activation kink is
    meaningful only if the fp64 reference by itself marks fewer: checked
    here for every small case and, on the device, recomputed inside each
    large case (the mark depends on the reference alone)."""
    worst = 0.0
    for shape in SMALL:
        for act in ("prelu", "relu"):
            for skip in (False, True):
                for dtype in (FP32, BF16):
                    case = _Case(shape, dtype, act, skip,
                                 seed=10 + SMALL.index(shape))
                    worst = max(worst, _reference_kink_share(case))
    print(f"[kink] reference-only share, small cases: {100 * worst:.4f} %")
    assert worst < KINK_CAP


# ------------------------------------------------ BN, through autograd

@pytest.mark.parametrize("act", list(ACTS))
def test_fused_bn_act_autograd_against_fp64(act):
    shape = (2, 64, 33)
    case = _Case(shape, FP32, act, True, seed=30 + ACTS[act])
    bn = torch.nn.BatchNorm2d(case.C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(case.gamma)
        bn.bias.copy_(case.beta)
        bn.running_mean.copy_(case.rm0)
        bn.running_var.copy_(case.rv0)
    mod = None
    if act == "prelu":
        mod = ChannelPReLU(case.C).cuda()
        with torch.no_grad():
            mod.weight.copy_(case.a)
    elif act == "relu":
        mod = "relu"
    x = case.x.cuda().requires_grad_(True)
    skip = case.skip.cuda().requires_grad_(True)
    out = fused_bn_act(x, bn, mod, skip=skip)
    out.backward(case.dy.cuda())
    ref = _Ref(case, "cpu")
    tag = f"autograd-{act}"
    _check_fwd(case, ref, dict(out=out.detach(), run_mean=bn.running_mean,
                               run_var=bn.running_var), tag)
    _check_bwd(case, ref, dict(
        dx=x.grad, dskip=skip.grad, dgamma=bn.weight.grad,
        dbeta=bn.bias.grad,
        da=mod.weight.grad if act == "prelu" else None), tag)
    assert bn.num_batches_tracked.item() == 1


# ------------------------------------------------------- pack epilogue

def _probes(dtype):
    one = torch.tensor(1.0)
    vals = [1.0, -1.0, 0.0, -0.0,
            1 + 2.0 ** -7, 1 - 2.0 ** -8,          # bf16 neighbours of 1
            -(1 + 2.0 ** -7), -(1 - 2.0 ** -8)]
    if dtype == FP32:
        up = torch.nextafter(one, one * 2).item()
        dn = torch.nextafter(one, one * 0).item()
        vals += [up, dn, -up, -dn]
    return torch.tensor(vals, dtype=torch.float32)


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("shape", [(1, 32, 47), (2, 64, 33), (3, 1024, 5)],
                         ids=["C32", "C64", "C1024"])
def test_pack_epilogue_planes_and_planted_edges(shape, act, dtype):
    """xpk / mpk bit for bit against planes built on the CPU from the
    stored `out`, with out values of exactly +-1, +-0 and the neighbours
    of 1 planted: gamma = 1, beta = 0 and x constant 0 on two channels
    make z = skip there exactly."""
    N, C, HW = shape
    case = _Case(shape, dtype, act, True, seed=40)
    probes = _probes(dtype)
    chans = [5, C - 1]                 # a low byte and the last word's top bit
    xr, sr = _rows(case.x), _rows(case.skip)
    for i, c in enumerate(chans):
        xr[:, c] = 0
        reps = (case.P + len(probes) - 1) // len(probes)
        sr[:, c] = probes.roll(i).repeat(reps)[:case.P].to(dtype)
        case.gamma[c], case.beta[c] = 1.0, 0.0
    assert case.P >= len(probes)
    x, skip = case.x.cuda(), case.skip.cuda()
    res = _nat().bn_act_fwd_train(
        x, skip, case.gamma.cuda(), case.beta.cuda(), None,
        case.rm0.cuda(), case.rv0.cuda(), MOMENTUM, BN_EPS, ACTS[act],
        None, None, True)
    out = res[0]
    want = _rows(skip)[:, chans].float()
    if act == "relu":
        want = want.clamp_min(0)
    got = _rows(out)[:, chans].float()
    assert torch.equal(got, want), "planted values did not reach out"
    assert (got == 1).any() and (got.abs() == 1).sum() >= 2
    sp, mp = _planes(out)
    assert torch.equal(_words(res[4]), sp), "sign plane"
    assert torch.equal(_words(res[5]), mp), "mask plane"
    # the planted edge itself, spelled out: |out| == 1 is inside the mask
    c = chans[0]
    word, bit = c // 32, c % 32
    at_one = (_rows(out)[:, c].float().abs() == 1).cpu()
    mask_bits = (_words(res[5])[:, word] >> bit) & 1
    assert at_one.any() and (mask_bits[at_one] == 1).all()


# ------------------------------------------- conv-epilogue statistics

CONV_STATS_SHAPES = [
    # (N, C, H, W, K, ks, stride, pad)
    (8, 64, 28, 28, 96, 3, 1, 1),    # 98 blocks: slice wrap, partial k-tile
    (3, 48, 15, 15, 64, 3, 2, 1),    # tail channel word, partial last m-tile
    # K = 96 is no width bn_act_fwd_train takes (not a power of two), so
    # the wrapped slices reach bn_finalize through this one
    (8, 64, 28, 28, 128, 3, 1, 1),   # 98 blocks, K a power of two
]


@pytest.mark.parametrize("out_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", CONV_STATS_SHAPES,
                         ids=["8x64x28-K96", "3x48x15-K64-s2", "8x64x28-K128"])
def test_conv_epilogue_stats_against_fp64(shape, out_bf16):
    """The STATS epilogue of xnor_conv: sliced sums of the STORED output
    (bf16: of the rounded value) against fp64 sums, scale-aware; then,
    where K is a width the BN kernels take, bn_act_fwd_train fed those
    sums against the fp64 mean / variance."""
    N, C, H, W, K, ks, stride, pad = shape
    g = torch.Generator().manual_seed(50)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    w = (torch.randn(K, C, ks, ks, generator=g) * 0.5).cuda()
    nat = _nat()
    xp = nat.sign_pack_nhwc(x.contiguous(memory_format=torch.channels_last))
    wp, alpha, stab = nat.weight_pack(w)
    out, s1, s2 = nat.xnor_conv_fwd(xp, wp, alpha, stab, C, stride, pad,
                                    out_bf16, True)
    assert s1.shape == (32, K) and s2.shape == (32, K)
    # the stored output is the conv (checked here loosely; its own tests
    # are in test_gpu_kernels.py), so the sums below are of real data
    conv = F.conv2d(binsign(x), weight_scale(w) * binsign(w), None, stride,
                    pad)
    assert torch.allclose(out.float(), conv, atol=0.05 if out_bf16 else 1e-3,
                          rtol=0.02 if out_bf16 else 1e-4)
    v = _rows(out).double()
    e1 = (s1.double().sum(0) - v.sum(0)).abs()
    e2 = (s2.double().sum(0) - (v * v).sum(0)).abs()
    B1 = C_BOUND * EPS24 * v.abs().sum(0)
    B2 = C_BOUND * EPS24 * (v * v).sum(0)
    q1, q2 = _ratio(e1, B1), _ratio(e2, B2)
    _note("err/bound conv s1", q1)
    _note("err/bound conv s2", q2)
    print(f"[conv-stats {shape}] err/bound s1:{q1:.3g} s2:{q2:.3g}")
    assert (e1 <= B1).all() and (e2 <= B2).all(), (q1, q2)
    if N * out.shape[2] * out.shape[3] >= 32 * 128:
        # >= 32 row tiles: every slice received a block (sum of squares
        # of a block's outputs cannot be zero)
        assert (s2.sum(1) > 0).all()

    if K & (K - 1):
        with pytest.raises(RuntimeError):
            nat.bn_act_fwd_train(out, None, torch.ones(K, device="cuda"),
                                 torch.zeros(K, device="cuda"), None, None,
                                 None, MOMENTUM, BN_EPS, 0, s1, s2, False)
        return
    # the conv output as a BN case: gamma 1, beta 0, identity.  mean,
    # invstd and the running stats only: with beta = 0 and mean ~ 0, B_z
    # vanishes at x = mean (see _Case)
    case = types.SimpleNamespace(
        x=out, skip=None, a=None, act="none", dtype=out.dtype, C=K,
        P=v.shape[0], gamma=torch.ones(K), beta=torch.zeros(K),
        rm0=torch.zeros(K), rv0=torch.ones(K), nominal_r=torch.zeros(K))
    rm, rv = case.rm0.cuda(), case.rv0.cuda()
    res = nat.bn_act_fwd_train(out, None, case.gamma.cuda(),
                               case.beta.cuda(), None, rm, rv, MOMENTUM,
                               BN_EPS, 0, s1, s2, False)
    ref = _Ref(case, "cpu")
    tag = f"conv-stats->bn {shape}"
    _check_stats(case, ref, res[2], res[3], tag, key="conv->bn var const")
    _check_fwd(case, ref, dict(run_mean=rm, run_var=rv), tag)


# --------------------------------------------------------- PReLU alone

# small shapes as above, and per C one capped-grid shape with
# n_pix ~ 1.5 pstep (the second grid-stride iteration), ~6.3 M elements
PRELU_SHAPES = [(1, 8, 3), (2, 64, 33), (3, 1024, 5),
                (3, 8, 511), (1, 64, 313), (1, 1024, 79)]


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", PRELU_SHAPES,
                         ids=[f"{n}x{c}x{h}" for n, c, h in PRELU_SHAPES])
def test_prelu_against_fp64(shape, dtype):
    N, C, HW = shape
    P = N * HW * HW
    rows = 256 // (C // 8)
    if P > 4096:
        assert (P + rows - 1) // rows > 2048
        assert 2048 * rows < P < 2 * 2048 * rows and P % rows != 0
    gen = torch.Generator().manual_seed(60 + PRELU_SHAPES.index(shape))
    xr = (torch.randn(P, C, generator=gen) * 2).to(dtype)
    gr = torch.randn(P, C, generator=gen).to(dtype)
    a = torch.rand(C, generator=gen) - 0.4
    # x of +0 and -0 under a nonzero gradient: the x > 0 / x <= 0 split
    xr[0, :] = 0.0
    xr[P - 1, :] = -0.0
    xr[P // 2, ::3] = 0.0
    gr[0, :] = 1.5
    gr[P - 1, :] = -2.0
    gr[P // 2, :] = 0.75
    x, g = _nchw(xr, N, C, HW).cuda(), _nchw(gr, N, C, HW).cuda()
    nat = _nat()
    y = nat.prelu_fwd(x, a.cuda())
    dx, da = nat.prelu_bwd(g, x, a.cuda())
    assert y.dtype == dtype and dx.dtype == dtype and da.dtype == FP32

    dev = "cuda" if P > 4096 else "cpu"
    X, G, A = _rows(x).to(dev).double(), _rows(g).to(dev).double(), \
        a.to(dev).double()
    y_ref = torch.where(X > 0, X, A * X)
    dx_ref = torch.where(X > 0, G, A * G)
    da_ref = ((X <= 0).double() * X * G).sum(0)
    yk, dxk = _rows(y).to(dev).double(), _rows(dx).to(dev).double()
    if dtype == FP32:
        # one fp32 product, exact in fp64: the rounded reference is it
        assert torch.equal(yk.float(), y_ref.float())
        assert torch.equal(dxk.float(), dx_ref.float())
    else:
        assert ((yk - y_ref).abs() <= BF16_RND * y_ref.abs()).all()
        assert ((dxk - dx_ref).abs() <= BF16_RND * dx_ref.abs()).all()
    # the planted zeros take the x <= 0 branch: dx = a g, not g
    zero_rows = torch.tensor([0, P - 1], device=dev)
    want = (A * G[zero_rows]).to(dtype).double()
    assert torch.equal(dxk[zero_rows], want)
    e = (da.to(dev).double() - da_ref).abs()
    B = C_BOUND * EPS24 * (X * G).abs().sum(0)
    q = _ratio(e, B)
    _note("err/bound prelu da", q)
    print(f"[prelu {shape} {dtype}] da err/bound {q:.3g}")
    assert (e <= B).all(), q


# ---------------------------------------------------------------- guards

def _bad_inputs():
    """(why, x) that no vec8 kernel can index: C = 4, C = 48, fp16"""
    return [("C=4", torch.randn(2, 4, 6, 6, device="cuda")),
            ("C=48", torch.randn(2, 48, 6, 6, device="cuda")),
            ("fp16", torch.randn(2, 16, 6, 6, device="cuda",
                                 dtype=torch.float16))]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["C4", "C48", "fp16"])
def test_vec8_bindings_reject(which):
    """The five vec8 bindings raise before any launch."""
    nat = _nat()
    why, x = _bad_inputs()[which]
    x = _cl(x)
    C = x.shape[1]
    vec = lambda: torch.ones(C, device="cuda")
    with pytest.raises(RuntimeError):
        nat.prelu_fwd(x, vec())
    with pytest.raises(RuntimeError):
        nat.prelu_bwd(x, x, vec())
    with pytest.raises(RuntimeError):
        nat.bn_act_fwd_train(x, None, vec(), vec(), None, vec(), vec(), 0.1,
                             BN_EPS, 0, None, None, False)
    with pytest.raises(RuntimeError):
        nat.bn_act_bwd(x, x, x, vec(), vec(), vec(), None, 0, False)
    with pytest.raises(RuntimeError):
        nat.bn_act_eval(x, None, vec(), vec(), None, vec(), vec(), BN_EPS, 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64],
                         ids=["fp16", "fp64"])
def test_dtype_only_bindings_reject(dtype):
    """maxpool and the five pack entry points take fp32 / bf16 only."""
    nat = _nat()
    x = _cl(torch.randn(2, 32, 6, 6, device="cuda").to(dtype))
    ok = _cl(torch.randn(2, 32, 6, 6, device="cuda"))
    idx = torch.zeros(2, 3, 3, 32, device="cuda", dtype=torch.uint8)
    mp = torch.zeros(2, 6, 6, 1, device="cuda", dtype=torch.int32)
    calls = [
        lambda: nat.maxpool_fwd(x, 3, 2, 1),
        lambda: nat.maxpool_bwd(x[:, :, :3, :3], idx, 6, 6, 3, 2, 1),
        lambda: nat.sign_pack_nhwc(x),
        lambda: nat.sign_mask_pack_nhwc(x),
        lambda: nat.binsign_decode(x, False),
        lambda: nat.ste_mask_mul(x, ok, 0, 0.0, 0.0),
        lambda: nat.ste_mask_mul(ok, x, 0, 0.0, 0.0),
        lambda: nat.mask_mul_packed(x, mp, 32, False),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"call {i} accepted {dtype}")
    # the numel % 8 rule of the two flat kernels stays
    odd = torch.randn(7, device="cuda")
    with pytest.raises(RuntimeError):
        nat.binsign_decode(odd, False)
    with pytest.raises(RuntimeError):
        nat.ste_mask_mul(odd, odd, 0, 0.0, 0.0)


def test_multi_tensor_lists_must_pair_with_the_leading_list():
    """fused_sgd / fused_adam / weight_kd_fwd index every list by the
    leading list's tensor number and element count: a short list, a
    non-fp32 entry or a short tensor raises before any launch, and a
    correct call afterwards still matches torch.optim.SGD."""
    from bdbnn_amd.ops.optim import FusedSGD
    nat = _nat()
    torch.manual_seed(80)
    new = lambda n=1000: torch.randn(n, device="cuda")
    p, g, buf = ([new() for _ in range(3)] for _ in range(3))
    before = [t.clone() for t in p]
    with pytest.raises(RuntimeError):                 # two grads for three
        nat.fused_sgd(p, g[:2], buf, 0.1, 0.9, 1e-4)
    with pytest.raises(RuntimeError):                 # one grad bf16
        nat.fused_sgd(p, [g[0], g[1].bfloat16(), g[2]], buf, 0.1, 0.9, 1e-4)
    with pytest.raises(RuntimeError):                 # one buffer short
        nat.fused_sgd(p, g, [buf[0], new(999), buf[2]], 0.1, 0.9, 1e-4)
    with pytest.raises(RuntimeError):                 # short m2 list
        nat.fused_adam(p, g, buf, [new(), new()], 1e-3, 0.9, 0.999, 1e-8,
                       0.0, 0.1, 0.001)
    with pytest.raises(RuntimeError):                 # two teachers for three
        nat.weight_kd_fwd(p, g[:2])
    torch.cuda.synchronize()
    for t, b in zip(p, before):
        assert torch.equal(t, b), "a rejected call wrote its parameters"

    ps = [t.clone().requires_grad_(True) for t in p]
    ref = [t.detach().clone().requires_grad_(True) for t in ps]
    for t, r, gi in zip(ps, ref, g):
        t.grad = gi.clone()
        r.grad = gi.clone()
    opt = FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4)
    topt = torch.optim.SGD(ref, lr=0.1, momentum=0.9, weight_decay=1e-4)
    for _ in range(3):
        opt.step()
        topt.step()
        for t in ps + ref:
            t.grad = t.grad * 0.9 + 0.01  # evolve grads deterministically
    for t, r in zip(ps, ref):
        assert torch.allclose(t, r, atol=1e-5, rtol=1e-5)


def test_bn_act_fwd_train_rejects_mistyped_statistics():
    """The running stats are written through float pointers and the
    pre-accumulated sums read through them: fp64 running_mean, one running
    stat without the other, pre_s1 without pre_s2 raise; the valid call
    on the same (2, 8, 4, 4) bf16 input stays within the oracle's bounds."""
    nat = _nat()
    case = _Case((2, 8, 4), BF16, "relu", False, seed=81)
    x = case.x.cuda()
    assert x.shape == (2, 8, 4, 4)
    assert x.is_contiguous(memory_format=torch.channels_last)
    gamma, beta = case.gamma.cuda(), case.beta.cuda()
    rm, rv = case.rm0.cuda(), case.rv0.cuda()
    call = lambda rm, rv, s1=None, s2=None: nat.bn_act_fwd_train(
        x, None, gamma, beta, None, rm, rv, MOMENTUM, BN_EPS, ACTS["relu"],
        s1, s2, False)
    with pytest.raises(RuntimeError):
        call(rm.double(), rv)
    with pytest.raises(RuntimeError):
        call(rm, None)
    with pytest.raises(RuntimeError):
        call(None, rv)
    with pytest.raises(RuntimeError):
        call(rm, rv, torch.zeros(32, 8, device="cuda"), None)
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu(), case.rm0) and torch.equal(rv.cpu(), case.rv0)
    _run_native(case, False, "cpu", "guards-2x8x4-bf16-relu")


@pytest.mark.parametrize("which", [0, 2], ids=["C4", "fp16"])
def test_unsupported_inputs_take_the_torch_composition(which):
    """fused_bn_act and ChannelPReLU on a 4-channel and on an fp16 CUDA
    tensor: the torch composition, the same code, so equal."""
    why, x0 = _bad_inputs()[which]
    C, dtype = x0.shape[1], x0.dtype
    torch.manual_seed(70)
    # PReLU
    m = ChannelPReLU(C).cuda()
    with torch.no_grad():
        m.weight.uniform_(-0.4, 0.6)
    x = _cl(x0).clone().requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    w2 = m.weight.detach().clone().requires_grad_(True)
    y = m(x)
    y2 = F.prelu(x2, w2.to(dtype))
    assert torch.equal(y, y2)
    g = torch.randn_like(y)
    y.backward(g)
    y2.backward(g)
    assert torch.equal(x.grad, x2.grad)
    # da: the same sum in another order
    assert torch.allclose(m.weight.grad, w2.grad, rtol=1e-2, atol=1e-2)
    # BN (+skip) + act, training and eval
    for act in (None, "relu", m):
        bn, bn2 = (torch.nn.BatchNorm2d(C).cuda() for _ in range(2))
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
        bn2.load_state_dict(bn.state_dict())
        skip = _cl(torch.randn_like(x0))
        for train in (True, False):
            bn.train(train)
            bn2.train(train)
            xa = _cl(x0).clone().requires_grad_(True)
            xb = _cl(x0).clone().requires_grad_(True)
            out = fused_bn_act(xa, bn, act, skip=skip)
            z = bn2(xb) + skip
            want = (z if act is None else torch.relu(z) if act == "relu"
                    else F.prelu(z, m.weight.to(dtype)))
            assert torch.equal(out, want), (why, act, train)
            out.backward(g)
            want.backward(g)
            assert torch.equal(xa.grad, xb.grad), (why, act, train)
            assert torch.equal(bn.weight.grad, bn2.weight.grad)
            assert torch.equal(bn.running_var, bn2.running_var)
            bn.zero_grad()
            bn2.zero_grad()
            m.zero_grad()
