"""The small kernels that decide the loss and every parameter update of a
training step -- the four multi-tensor kernels (csrc/kurtosis.hip,
csrc/kd.hip, csrc/optim.hip) and the two row-wise losses (csrc/loss.hip)
-- against fp64 formulas written out here, from the same rounded inputs
the kernels get, at the sizes where they go wrong: tensors that end inside,
at and just past a 32768-element chunk and a 256-thread block, more than
64 parameters, mixed NCHW / channels_last lists, C from 1 to 1001 and a
backward whose grid-stride loop runs more than once.

Bounds.  eps = 2^-24 (fp32 unit roundoff).  Every bound is c eps S with S a
sum of the magnitudes of the terms the kernel adds up, so a cancelling
result is not asked to be relatively exact.  A bf16 store adds 2^-8 |ref|
per rounding (the convention of test_gpu_bn_act_oracle.py); the inputs are
the rounded ones on both sides, so there is no input-rounding term.

  kurtosis   raw moments are summed in fp64, so what is left is the fp32
             store:  |kurt - ref| <= c eps |kurt|,  loss: c eps sum_l loss_l
  kurtosis backward reads (mu, sigma, kurt, z3m) back as fp32 and works in
             fp32.  With K = 8 gs / (n sigma), D = kurt - target,
             P = z^3 - z3m - z knn, dz = |z| + |mu| / sigma (mu is rounded):
               |g - ref| <= c eps |K| ( (|kurt| + |target|) |P|
                   + |D| (|z|^3 + |z3m| + |z| knn + dz (3 z^2 + knn)) )
             D is formed from the fp32 kurt, so its error is relative to
             |kurt| + |target| and not to the difference: within 1e-3 of the
             target the gradient keeps ~4 digits, which this bound allows.
  weight KD  loss: c eps sum_pairs sum_e |exp(t) (t - s)| / n
             grad: c eps |ref|
  SGD        with B = |g| + wd |p| + mom |buf|:
               buf: c eps B        p: c eps (|p| + lr B)
  Adam       with G = |g| + wd |p|, M = b1 |m| + (1 - b1) G,
             V = b2 v + (1 - b2) G^2, u = (m' / bc1) / (sqrt(v' / bc2) + e):
               m: c eps M      v: c eps V
               p: c eps (|p| + lr (M / (bc1 denom) + |u| (1 + V / v')))
  optimiser classes, three steps: the per-step scales above are summed
             over the steps, and a step's M, V, B include those of the
             steps before it (the state carries their error on, with a
             factor <= 1).
  logit KD   row: sum_c p_t (1 + |s - m_s| + |lz_s|) (1 + |t - m_t| + |lz_t|)
             loss: c eps mean over rows of that
             ds:  c eps gs (p_s (1 + |s| + |lse_s|) + p_t (1 + |t| + |lse_t|))
             (the row statistic lse = m + log z is stored in fp32, so a row
             shifted by 200 loses 200 eps in the exponent; the forward works
             with s - m and does not)
  CE         loss: c eps mean over rows of (1 + |m| + |lz| + |s_y|)
             ds:  c eps gs (p (1 + |s| + |lse|) + |p - onehot|)
  bf16 ds    is stored rounded by the kernel and rounded again after the
             fp32 product with the upstream gradient: 2 * 2^-8 |ref|.  (A
             bf16 ds times the 0-dim fp32 gradient in torch rounds the
             gradient to bf16 first, a third rounding; this file found it
             as 29x the bound and ops/losses.py now forms the product in
             fp32.)

The constants c.  Each kernel's arithmetic was modelled by the same fp32
operations in torch on the CPU (the _model_* functions below; run
_model_figures() to repeat it), the largest err / (eps S) over the cases of
this file taken, and c set 16x above it.
See the table at C_BOUND for the model figures and for what an MI355X gave.

Hyper-parameters.  The binding hands lr, betas, ... to the kernels as fp32.
The single-step references use those rounded values.  torch.optim in fp64
cannot be told to, so the tests through the optimiser classes use values
that fp32 holds exactly (lr = 2^-7, betas = (0.875, 1 - 2^-10), ...).  With
the defaults the kernel's 1.f - beta2 is 0.00100005 against 0.001: 4.7e-5
relative in the weight of g^2, 2.3e-5 in the first update.  That is the
format of the argument, not an error of the arithmetic, and is left alone.

Measured on an MI355X (MEASURED_MI355X below; every test prints its own
err / bound before it asserts, and the module prints the largest): every
quantity is within 0.11 of its bound, most at 0.05-0.07, which is the 1/16
the constants were set at: the GPU's errors are those of the CPU models
(sgd a little below, the kernel's a*b+c being fused; weight-KD gradient and
logit-KD a little above or below through expf / logf).  The largest is the
cross-entropy loss at 600 x 1000 in bf16, 0.105: 600 rows added with
atomicAdd in fp32.  No case needed a change to a kernel's arithmetic, the
near-target kurtosis gradient (0.026) included.

What the file found on the parent of the commit that added it, on an
MI355X: the weight-KD loss of a channels_last student 449x its bound
(1640x through WeightKDLoss), gradients right; the cross-entropy gradient
with a strided target 4e6x to 1e10x; a parameter whose loaded state kept
NCHW strides 5e5x (SGD) and 8e4x (Adam) after two more steps; the Adam
parameter that skipped a step 6e4x; fp64 logits read as fp32; and the
bf16 loss gradients 29x through the rounded upstream gradient.
"""

import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops.kd import DistributionLoss, WeightKDLoss, _FusedWeightKD
from bdbnn_amd.ops.kurtosis import kurtosis_loss_fused
from bdbnn_amd.ops.losses import FusedCrossEntropy, fused_logit_kd
from bdbnn_amd.ops.optim import FusedAdam, FusedSGD

EPS24 = 2.0 ** -24
BF16_RND = 2.0 ** -8
FP32, BF16 = torch.float32, torch.bfloat16
CL = torch.channels_last
CHUNK = 32768          # BDBNN_CHUNK_ELEMS: what one block covers
MAX_TENSORS = 64       # BDBNN_MAX_TENSORS: tensors per fused call
UP = 1.7               # the non-unit upstream gradient

# MODEL_FIGURE: the largest err / (eps S) of the CPU model of each kernel
# (_model_figures(), rounded up); c = 16 x that.  MEASURED_MI355X: the
# largest err / (eps S) this file gave on the GPU, and the margin c /
# measured that is left.
MODEL_FIGURE = {
    "kurt": 0.67, "kurt loss": 1.08, "kurt grad": 0.80,
    "wkd loss": 0.67, "wkd grad": 2.07,
    "sgd": 2.67, "adam": 3.75, "sgd steps": 1.14, "adam steps": 0.94,
    "kd loss": 3.04, "kd grad": 1.68, "ce loss": 4.94, "ce grad": 1.80,
}
C_BOUND = {k: 16.0 * v for k, v in MODEL_FIGURE.items()}
MEASURED_MI355X = {            # err / (eps S)      err / bound   margin
    "kurt": 0.67,              # the fp32 store     0.062         16x
    "kurt loss": 1.08,         #                    0.062         16x
    "kurt grad": 0.79,         # far 0.055 of the bound, near-target 0.026
    "wkd loss": 0.67,          #                    0.062         16x
    "wkd grad": 2.40,          #                    0.072         14x
    "sgd": 2.06,               #                    0.048         21x
    "adam": 3.75,              #                    0.062         16x
    "sgd steps": 1.14,         #                    0.062         16x
    "adam steps": 0.94,        #                    0.062         16x
    "kd loss": 2.83,           # bf16 2.14          0.058         17x
    "kd grad": 1.76,           # bf16 0.49          0.065         15x
    "ce loss": 8.31,           # fp32 4.94, bf16 8.31 (600 x 1000)  0.105  9.5x
    "ce grad": 1.80,           # bf16 0: inside the two roundings  0.062  16x
}

_MEASURED = {}


def _nat():
    return _C.native_required()


def _note(key, value):
    value = float(value)
    if not (value <= _MEASURED.get(key, -1.0)):
        _MEASURED[key] = value


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _MEASURED:
        print("\n[scalar kernels oracle] largest err / (eps S), its c, "
              "err / bound")
        for k in sorted(_MEASURED):
            c = C_BOUND[k.split(" bf16")[0]]
            print(f"  {k:18s} {_MEASURED[k]:9.4g}  c={c:g}  "
                  f"{_MEASURED[k] / c:.3g}")


def _fig(got, ref, scale, extra=None):
    """max (|got - ref| - extra) / (eps scale); nan-safe.  `extra` is the
    bf16 rounding allowance, taken off the error before the fp32 bound."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    if extra is not None:
        err = (err - extra).clamp_min(0)
    q = err / (EPS24 * scale)
    q = torch.where(err == 0, torch.zeros_like(q), q)
    q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
    return q.max().item() if q.numel() else 0.0


def _check(tag, figs):
    """figs: {quantity: (key into C_BOUND, figure)}; prints, then asserts"""
    line = []
    for name, (key, v) in figs.items():
        _note(key, v)
        line.append(f"{name}:{v / C_BOUND[key.split(' bf16')[0]]:.3g}")
    print(f"[{tag}] err/bound " + " ".join(line))
    for name, (key, v) in figs.items():
        assert v <= C_BOUND[key.split(" bf16")[0]], (tag, name, v)


def _f32(x):
    """a python float as the binding's (float) cast leaves it"""
    return torch.tensor(x, dtype=FP32).item()


# ------------------------------------------------------- multi-tensor lists

def _specs(first=1):
    """(shape, channels_last) of the size list every multi-tensor test uses"""
    return [((first,), False), ((255,), False), ((256,), False),
            ((257,), False), ((CHUNK - 1,), False), ((CHUNK,), False),
            ((CHUNK + 1,), False), ((2 * CHUNK + 5,), False),
            ((16, 8, 3, 3), True), ((8, 16, 1, 1), False),
            ((16, 8, 3, 3), False)]


def _rand_list(specs, seed, scales, means, positive=False):
    """CPU fp32 tensors, tensor i = scales[i % k] * randn + means[i % k]: a
    block that reads the wrong tensor or the wrong offset cannot pass"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (shape, _) in enumerate(specs):
        t = torch.randn(shape, generator=g)
        t = t * scales[i % len(scales)] + means[i % len(means)]
        out.append(t.square() + 1e-3 if positive else t)
    return out


def _place(ts, specs, dev, cl=None):
    """to the device, 4-D tensors channels_last where the spec (or the
    override `cl`) says so"""
    out = []
    for t, (_, want) in zip(ts, specs):
        t = t.to(dev)
        if t.dim() == 4 and (want if cl is None else cl):
            t = t.contiguous(memory_format=CL)
        out.append(t)
    return out


# ----------------------------------------------------------------- kurtosis

KURT_SCALES, KURT_MEANS = (0.05, 2.0, 0.5, 1.0), (0.3, -1.0, 0.0, 0.7, -0.2)


def _kurt_inputs():
    specs = _specs(first=2)
    ws = _rand_list(specs, 101, KURT_SCALES, KURT_MEANS)
    # targets: far from the tensor's kurtosis, and within 1e-3 of it
    kurts = [_kurt_ref(w.double(), 0.0, 1.0)["kurt"].item() for w in ws]
    tg = [1.8 if i % 2 == 0 else k + (5e-4 if i % 4 == 1 else -5e-4)
          for i, k in enumerate(kurts)]
    return specs, ws, tg


def _kurt_ref(w, tgt, gs):
    """fp64 formulas of ops/kurtosis.py's docstring; tgt, gs python floats"""
    n = w.numel()
    mu = w.mean()
    d = w - mu
    sigma = (d.square().sum() / (n - 1)).sqrt()          # unbiased
    z = d / sigma
    kurt = z.pow(4).mean()
    z3m = z.pow(3).mean()
    knn = kurt * n / (n - 1)
    D = kurt - tgt
    K = 8.0 * gs / (n * sigma)
    P = z.pow(3) - z3m - z * knn
    dz = z.abs() + mu.abs() / sigma
    S = K.abs() * ((kurt.abs() + abs(tgt)) * P.abs()
                   + D.abs() * (z.abs().pow(3) + z3m.abs() + z.abs() * knn
                                + dz * (3 * z.square() + knn)))
    return dict(kurt=kurt, loss=D * D, grad=K * D * P, S_grad=S,
                stats=(mu, sigma, kurt, z3m))


def _model_kurt(w, tgt, gs):
    """the kernel's arithmetic: fp64 moments, fp32 stores, fp32 backward"""
    r = _kurt_ref(w.double(), tgt, gs)
    mu, sigma, kurt, z3m = (s.float() for s in r["stats"])
    n = w.numel()
    tgt32, gs32 = torch.tensor(tgt, dtype=FP32), torch.tensor(gs, dtype=FP32)
    coef = gs32 * 2.0 * (kurt - tgt32) * 4.0 / (float(n) * sigma)
    knn = kurt * float(n) / float(n - 1)
    z = (w - mu) / sigma
    grad = coef * (z * z * z - z3m - z * knn)
    return r["kurt"].float(), r["loss"].float(), grad


@pytest.mark.parametrize("mode", ["sum", "avg"])
def test_kurtosis_against_fp64(mode):
    specs, ws_cpu, tg = _kurt_inputs()
    ws = [w.requires_grad_(True) for w in _place(ws_cpu, specs, "cuda")]
    loss, kurts = kurtosis_loss_fused(ws, tg, mode)
    loss.backward(torch.tensor(UP, device="cuda"))
    L = len(ws)
    gs = _f32(UP) / (L if mode == "avg" else 1)
    refs = [_kurt_ref(w.detach().double(), _f32(t), gs)
            for w, t in zip(ws, tg)]
    near = [abs(r["kurt"].item() - _f32(t)) for r, t in zip(refs, tg)]
    assert max(near[1::2]) <= 1e-3 and min(near[0::2]) > 0.1
    k_ref = torch.stack([r["kurt"] for r in refs])
    l_ref = torch.stack([r["loss"] for r in refs])
    div = L if mode == "avg" else 1
    figs = {"kurt": ("kurt", _fig(kurts, k_ref, k_ref.abs())),
            "loss": ("kurt loss", _fig(loss, l_ref.sum() / div,
                                       l_ref.sum() / div))}
    g_far = max(_fig(w.grad, r["grad"], r["S_grad"])
                for w, r in zip(ws[0::2], refs[0::2]))
    g_near = max(_fig(w.grad, r["grad"], r["S_grad"])
                 for w, r in zip(ws[1::2], refs[1::2]))
    figs["grad far"] = ("kurt grad", g_far)
    figs["grad near"] = ("kurt grad", g_near)
    for w in ws:
        assert w.grad.stride() == w.stride()
    _check(f"kurtosis {mode}", figs)


def test_kurtosis_refuses_65_tensors():
    """one more than BDBNN_MAX_TENSORS raises before anything is launched
    or allocated: make_meta is the first thing kurtosis_fwd does"""
    ws = [torch.randn(8, device="cuda", requires_grad=True)
          for _ in range(MAX_TENSORS + 1)]
    with pytest.raises(RuntimeError, match="too many tensors"):
        kurtosis_loss_fused(ws, [1.8] * len(ws), "sum")
    with pytest.raises(RuntimeError, match="too many tensors"):
        _nat().kurtosis_fwd([w.detach() for w in ws],
                            torch.full((len(ws),), 1.8))
    assert all(w.grad is None for w in ws)
    loss, _ = kurtosis_loss_fused(ws[:MAX_TENSORS], [1.8] * MAX_TENSORS, "sum")
    assert torch.isfinite(loss)


# ---------------------------------------------------------------- weight KD

WKD_SCALES, WKD_MEANS = (0.5, 0.1, 1.0, 0.25), (0.2, -0.5, 0.0, 1.0, -1.0)
WKD_LAYOUTS = {"nchw-nchw": (False, False), "cl-cl": (True, True),
               "cl-nchw": (True, False), "nchw-cl": (False, True)}


def _wkd_inputs():
    specs = _specs()
    ws = _rand_list(specs, 201, WKD_SCALES, WKD_MEANS)
    wt = _rand_list(specs, 202, WKD_SCALES[1:] + WKD_SCALES[:1],
                    WKD_MEANS[2:] + WKD_MEANS[:2])
    return specs, ws, wt


def _wkd_ref(ws, wt, gs):
    """fp64: sum over pairs of mean(exp(t) (t - s)); d/ds = -gs exp(t) / n"""
    loss, S, grads = 0.0, 0.0, []
    for s, t in zip(ws, wt):
        s, t = s.double(), t.double()
        term = t.exp() * (t - s)
        loss = loss + term.mean()
        S = S + term.abs().mean()
        grads.append(-gs * t.exp() / t.numel())
    return loss, S, grads


def _model_wkd(ws, wt, gs):
    loss = torch.zeros((), dtype=torch.float64)
    grads = []
    for s, t in zip(ws, wt):
        loss += (torch.exp(t) * (t - s)).double().sum() / t.numel()
        coef = -torch.tensor(gs, dtype=FP32) / float(t.numel())
        grads.append(coef * torch.exp(t))
    return loss.float(), grads


@pytest.mark.parametrize("layout", list(WKD_LAYOUTS))
def test_weight_kd_against_fp64(layout):
    """student / teacher 4-D tensors in every mix of the two dense layouts:
    the kernel pairs elements over physical memory, so the teacher has to
    reach it in the student's layout (a channels_last student against a
    teacher put back into NCHW sums exp(t) s over mismatched pairs)."""
    s_cl, t_cl = WKD_LAYOUTS[layout]
    specs, ws_cpu, wt_cpu = _wkd_inputs()
    ws = [w.requires_grad_(True)
          for w in _place(ws_cpu, specs, "cuda", cl=s_cl)]
    wt = _place(wt_cpu, specs, "cuda", cl=t_cl)
    loss = _FusedWeightKD.apply(len(ws), *ws, *wt)
    loss.backward(torch.tensor(UP, device="cuda"))
    l_ref, S, g_ref = _wkd_ref([w.detach() for w in ws], wt, _f32(UP))
    figs = {"loss": ("wkd loss", _fig(loss, l_ref, S)),
            "grad": ("wkd grad", max(_fig(w.grad, g, g.abs())
                                     for w, g in zip(ws, g_ref)))}
    _check(f"weight KD {layout}", figs)


class _TwoConvs(nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.conv1 = nn.Conv2d(3, 8, 3, bias=False)      # excluded by name
        self.a = nn.Conv2d(8, 16, 3, bias=False)
        self.b = nn.Conv2d(16, 8, 1, bias=False)
        self.c = nn.Conv2d(8, 8, 3, bias=False)


@pytest.mark.parametrize("teacher_cl", [True, False])
def test_weight_kd_loss_module_channels_last_student(teacher_cl):
    """WeightKDLoss as the trainer builds it: the student converted to
    channels_last, the teacher converted or not"""
    stud = _TwoConvs(301).cuda().to(memory_format=CL)
    teach = _TwoConvs(302).cuda()
    if teacher_cl:
        teach = teach.to(memory_format=CL)
    kd = WeightKDLoss(stud, teach)
    assert len(kd.pairs) == 3
    loss = kd()
    loss.backward(torch.tensor(UP, device="cuda"))
    ws = [p[0] for p in kd.pairs]
    l_ref, S, g_ref = _wkd_ref([w.detach() for w in ws],
                               [p[1].detach() for p in kd.pairs], _f32(UP))
    figs = {"loss": ("wkd loss", _fig(loss, l_ref, S)),
            "grad": ("wkd grad", max(_fig(w.grad, g, g.abs())
                                     for w, g in zip(ws, g_ref)))}
    _check(f"WeightKDLoss teacher_cl={teacher_cl}", figs)


def test_fused_lists_must_share_each_tensors_layout():
    """a further list whose tensor is dense in the other memory format is
    an error, not a silent permutation; nothing is written"""
    nat = _nat()
    torch.manual_seed(303)
    p = [torch.randn(16, 8, 3, 3, device="cuda").contiguous(memory_format=CL)]
    g = [torch.randn(16, 8, 3, 3, device="cuda").contiguous(memory_format=CL)]
    nchw = [torch.randn(16, 8, 3, 3, device="cuda")]
    before = p[0].clone()
    msg = "pair elements over physical memory"
    with pytest.raises(RuntimeError, match=msg):
        nat.fused_sgd(p, g, nchw, 0.1, 0.9, 0.0)
    with pytest.raises(RuntimeError, match=msg):
        nat.fused_sgd(p, nchw, g, 0.1, 0.9, 0.0)
    with pytest.raises(RuntimeError, match=msg):
        nat.fused_adam(p, g, g, nchw, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001)
    with pytest.raises(RuntimeError, match=msg):
        nat.weight_kd_fwd(p, nchw)
    torch.cuda.synchronize()
    assert torch.equal(p[0], before)
    # size-1 dimensions: dense in both formats, whatever the strides say
    a = [torch.randn(8, 16, 1, 1, device="cuda")]
    b = [torch.randn(8, 16, 1, 1, device="cuda").as_strided(
        (8, 16, 1, 1), (16, 1, 16, 16))]
    assert a[0].stride() != b[0].stride()
    nat.weight_kd_fwd(a, b)
    nat.fused_sgd(a, b, [torch.zeros_like(a[0])], 0.1, 0.9, 0.0)


# -------------------------------------------------- SGD / Adam, single step

OPT_SCALES, OPT_MEANS = (0.5, 0.1, 1.0, 0.25), (0.2, -0.5, 0.0, 1.0, -1.0)


def _opt_inputs(n_lists, zero_grad_elems=False):
    """p, g and state lists (random, non-zero), rolled against each other"""
    specs = _specs()
    lists = []
    for k in range(n_lists):
        lists.append(_rand_list(specs, 400 + k,
                                OPT_SCALES[k % 4:] + OPT_SCALES[:k % 4],
                                OPT_MEANS[k % 5:] + OPT_MEANS[:k % 5],
                                positive=(k == 3)))
    if zero_grad_elems:                 # every third element: g = m = v = 0
        for l in lists[1:]:
            for t in l:
                t.view(-1)[::3] = 0
    return specs, lists


def _sgd_ref(p, g, b, lr, mom, wd):
    p, g, b = p.double(), g.double(), b.double()
    B = g.abs() + wd * p.abs() + mom * b.abs()
    b2 = b * mom + (g + wd * p)
    return dict(p=p - lr * b2, buf=b2, S_p=p.abs() + lr * B, S_buf=B)


def _model_sgd(p, g, b, lr, mom, wd):
    gi = g + wd * p
    bi = b * mom + gi
    return p - lr * bi, bi


def _adam_ref(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2):
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    G = g.abs() + wd * p.abs()
    gi = g + wd * p
    M = b1 * m.abs() + (1 - b1) * G
    V = b2 * v + (1 - b2) * G * G
    m2 = m * b1 + (1 - b1) * gi
    v2 = v * b2 + (1 - b2) * gi * gi
    denom = (v2 / bc2).sqrt() + eps
    u = (m2 / bc1) / denom
    rel_v = torch.where(v2 > 0, V / v2, torch.zeros_like(V))
    S_p = p.abs() + lr * (M / (bc1 * denom) + u.abs() * (1 + rel_v))
    return dict(p=p - lr * u, m=m2, v=v2, S_p=S_p, S_m=M, S_v=V)


def _model_adam(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2):
    inv1, inv2 = 1.0 / torch.tensor(bc1, dtype=FP32), \
        1.0 / torch.tensor(bc2, dtype=FP32)
    gi = g + wd * p
    mi = m * b1 + (1.0 - torch.tensor(b1, dtype=FP32)) * gi
    vi = v * b2 + (1.0 - torch.tensor(b2, dtype=FP32)) * gi * gi
    denom = torch.sqrt(vi * inv2) + eps
    return p - lr * (mi * inv1) / denom, mi, vi


SGD_CASES = [(0.1, 0.9, 1e-4), (0.1, 0.0, 0.0), (0.05, 0.9, 0.0),
             (0.1, 0.0, 5e-4)]


@pytest.mark.parametrize("lr,mom,wd", SGD_CASES)
def test_fused_sgd_single_step_against_fp64(lr, mom, wd):
    specs, (p0, g0, b0) = _opt_inputs(3, zero_grad_elems=True)
    p, g, b = (_place(l, specs, "cuda") for l in (p0, g0, b0))
    keep = [t.clone() for t in p]
    _nat().fused_sgd(p, g, b, lr, mom, wd)
    figs = {"p": 0.0, "buf": 0.0}
    for pk, p_in, gi, b_in, bk in zip(p, keep, g, _place(b0, specs, "cuda"),
                                      b):
        r = _sgd_ref(p_in, gi, b_in, _f32(lr), _f32(mom), _f32(wd))
        figs["p"] = max(figs["p"], _fig(pk, r["p"], r["S_p"]))
        figs["buf"] = max(figs["buf"], _fig(bk, r["buf"], r["S_buf"]))
    _check(f"sgd lr={lr} mom={mom} wd={wd}",
           {k: ("sgd", v) for k, v in figs.items()})


ADAM_CASES = [(1, 0.0), (1, 1e-4), (1000, 0.0), (1000, 1e-4)]


@pytest.mark.parametrize("step,wd", ADAM_CASES)
def test_fused_adam_single_step_against_fp64(step, wd):
    """step 1: bc2 = 0.001; step 1000: bc2 = 0.63.  Every third element has
    g = m = v = 0: with wd = 0 its denominator is eps alone."""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    specs, (p0, g0, m0, v0) = _opt_inputs(4, zero_grad_elems=True)
    p, g, m, v = (_place(l, specs, "cuda") for l in (p0, g0, m0, v0))
    ins = [[t.clone() for t in l] for l in (p, g, m, v)]
    _nat().fused_adam(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2)
    hp = [_f32(x) for x in (lr, b1, b2, eps, wd, bc1, bc2)]
    figs = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i in range(len(p)):
        r = _adam_ref(*(l[i] for l in ins), *hp)
        figs["p"] = max(figs["p"], _fig(p[i], r["p"], r["S_p"]))
        figs["m"] = max(figs["m"], _fig(m[i], r["m"], r["S_m"]))
        figs["v"] = max(figs["v"], _fig(v[i], r["v"], r["S_v"]))
    _check(f"adam step={step} wd={wd}",
           {k: ("adam", v) for k, v in figs.items()})


# ------------------------------------- SGD / Adam through the optimiser classes

N_PARAMS = 130         # 64 + 64 + 2 tensors per fused launch
SKIP_FIRST = 5         # this parameter has no .grad on the first step
RELAID = 8             # channels_last parameter whose state is saved NCHW
BF16_GRADS = (1, 4, 8, 19)
# held exactly by fp32, so torch.optim in fp64 gets what the kernels get
SGD_KW = dict(lr=2.0 ** -4, momentum=0.875, weight_decay=2.0 ** -13)
ADAM_KW = dict(lr=2.0 ** -7, betas=(0.875, 1 - 2.0 ** -10), eps=2.0 ** -27,
               weight_decay=2.0 ** -13)


def _class_specs():
    specs = _specs() + _specs()
    specs += [((3 + i % 7,), False) for i in range(N_PARAMS - len(specs))]
    assert len(specs) == N_PARAMS and specs[RELAID] == ((16, 8, 3, 3), True)
    return specs


def _class_grads(specs, step):
    gs = _rand_list(specs, 500 + step, OPT_SCALES, OPT_MEANS[1:])
    return [g.to(BF16).float() if i in BF16_GRADS else g
            for i, g in enumerate(gs)]


def _run_class(kind, dev, dtype, fused):
    """three steps of FusedSGD / FusedAdam (or torch.optim in `dtype`) on
    the 130 parameters; returns parameters, state and the bound scales.
    After the first step the optimiser is rebuilt around a channels_last
    copy of parameter RELAID and the state moved over with state_dict() /
    load_state_dict(), which keeps the NCHW strides of the saved buffers."""
    specs = _class_specs()
    init = _rand_list(specs, 499, OPT_SCALES, OPT_MEANS)
    first = list(specs)
    first[RELAID] = (specs[RELAID][0], False)              # NCHW at first
    ps = [t.to(dtype).requires_grad_(True)
          for t in _place(init, first if fused else specs, dev)]
    kw = SGD_KW if kind == "sgd" else ADAM_KW
    if fused:
        make = FusedSGD if kind == "sgd" else FusedAdam
    else:
        make = torch.optim.SGD if kind == "sgd" else torch.optim.Adam
    opt = make(ps, **kw)
    hist = []
    for step in range(3):
        grads = _place(_class_grads(specs, step),
                       first if (fused and step == 0) else specs, dev)
        for i, (p, g) in enumerate(zip(ps, grads)):
            if step == 0 and i == SKIP_FIRST:
                p.grad = None
            elif fused and i in BF16_GRADS:
                p.grad = g.to(dtype)                       # step() up-casts
                p.grad.data = p.grad.data.to(BF16)
            else:
                p.grad = g.to(dtype)
        if not fused:
            hist.append([(p.detach().clone(),
                          None if p.grad is None else p.grad.clone(),
                          {k: v.clone() for k, v in opt.state[p].items()
                           if torch.is_tensor(v)}) for p in ps])
        opt.step()
        if fused and step == 0:
            saved = opt.state_dict()
            new = ps[RELAID].detach().clone(memory_format=CL)
            assert new.stride() != ps[RELAID].stride()
            ps[RELAID] = new.requires_grad_(True)
            opt = make(ps, **kw)
            opt.load_state_dict(saved)
            st = [v for v in opt.state[ps[RELAID]].values()
                  if torch.is_tensor(v) and v.dim() == 4]
            assert st and all(v.stride() != new.stride() for v in st), \
                "the round trip no longer produces the mismatched layout"
    return ps, opt, hist


def _class_scales(kind, hist, final):
    """the per-step scales of the module docstring, summed over the steps;
    a step's B (M, V) includes those of the steps before it"""
    kw = SGD_KW if kind == "sgd" else ADAM_KW
    lr, wd = kw["lr"], kw["weight_decay"]
    out = []
    for i in range(len(final)):
        S = torch.zeros_like(final[i])
        accB = torch.zeros_like(S)
        accV = torch.zeros_like(S)
        t = 0
        for step in range(3):
            p, g, st = hist[step][i]
            if g is None:
                continue
            t += 1
            if kind == "sgd":
                buf = st.get("momentum_buffer", torch.zeros_like(p))
                accB = accB + g.abs() + wd * p.abs() \
                    + kw["momentum"] * buf.abs()
                S = S + p.abs() + lr * accB
            else:
                b1, b2 = kw["betas"]
                m = st.get("exp_avg", torch.zeros_like(p))
                v = st.get("exp_avg_sq", torch.zeros_like(p))
                r = _adam_ref(p, g, m, v, lr, b1, b2, kw["eps"], wd,
                              1 - b1 ** t, 1 - b2 ** t)
                accB = accB + r["S_m"]
                accV = accV + r["S_v"]
                bc1 = 1 - b1 ** t
                denom = (r["v"] / (1 - b2 ** t)).sqrt() + kw["eps"]
                u = (r["m"] / bc1) / denom
                S = S + p.abs() + lr * (accB / (bc1 * denom)
                                        + u.abs() * (1 + accV / r["v"]))
        out.append(S)
    return out


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optimiser_classes_three_steps_against_torch_optim_fp64(kind):
    ps, opt, _ = _run_class(kind, "cuda", FP32, fused=True)
    ref, topt, hist = _run_class(kind, "cuda", torch.float64, fused=False)
    scales = _class_scales(kind, hist, [r.detach() for r in ref])
    key = f"{kind} steps"
    per = [_fig(p.detach(), r.detach(), S)
           for p, r, S in zip(ps, ref, scales)]
    special = (SKIP_FIRST, RELAID)
    figs = {"re-laid state": (key, per[RELAID]),
            "skipped a step": (key, per[SKIP_FIRST]),
            "its group": (key, max(v for i, v in enumerate(per)
                                   if i not in special))}
    _check(f"{kind} classes", figs)
    names = ("momentum_buffer",) if kind == "sgd" else ("exp_avg",
                                                        "exp_avg_sq")
    for p in ps:
        for n in names:
            assert same_layout(opt.state[p][n], p), (n, p.shape)
    if kind == "adam":
        steps = [int(opt.state[p]["step"]) for p in ps]
        assert steps[SKIP_FIRST] == 2 and set(
            steps[:SKIP_FIRST] + steps[SKIP_FIRST + 1:]) == {3}


def same_layout(a, b):
    """equal strides, or dense in the same memory format (size-1
    dimensions leave the strides ambiguous), as the binding checks it"""
    return (a.stride() == b.stride()
            or (a.is_contiguous() and b.is_contiguous())
            or (a.is_contiguous(memory_format=CL)
                and b.is_contiguous(memory_format=CL)))


# --------------------------------------------------- logit KD, cross-entropy

LOGIT_SHAPES = [(1, 1), (1, 10), (3, 10), (7, 255), (5, 256), (4, 257),
                (2, 1000), (3, 1001), (600, 1000)]


def _logits(B, C, dtype, seed):
    """3 randn, row 0 shifted by +200 and the last row by -200 (B = 1: one
    shift, its sign from the seed); rounded to dtype"""
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(B, C, generator=g)
    if B == 1:
        x[0] += 200.0 if seed % 2 else -200.0
    else:
        x[0] += 200.0
        x[-1] -= 200.0
    return x.to(dtype)


def _noncontig(t):
    """the same values as a column slice of a wider tensor"""
    wide = torch.zeros(t.shape[0], t.shape[1] + 7, dtype=t.dtype,
                       device=t.device)
    wide[:, 3:3 + t.shape[1]] = t
    v = wide[:, 3:3 + t.shape[1]]
    assert not v.is_contiguous() or t.shape[0] == 1
    return v


def _fin(x):
    """|x| with -inf logits taken as 0: their probability is exactly 0"""
    return torch.where(torch.isinf(x), torch.zeros_like(x), x.abs())


def _row_stats(x):
    m = x.max(1, keepdim=True).values
    lz = (x - m).exp().sum(1, keepdim=True).log()
    return m, lz, m + lz


def _kd_ref(s, t, gs):
    """fp64 from the rounded logits; gs = upstream / B"""
    s, t = s.double(), t.double()
    ms, lzs, lse_s = _row_stats(s)
    mt, lzt, lse_t = _row_stats(t)
    ps, pt = (s - lse_s).exp(), (t - lse_t).exp()
    rows = -(pt * (s - lse_s)).sum(1)
    S_rows = (pt * (1 + (s - ms).abs() + lzs.abs())
              * (1 + (t - mt).abs() + lzt.abs())).sum(1)
    S_ds = gs * (ps * (1 + s.abs() + lse_s.abs())
                 + pt * (1 + t.abs() + lse_t.abs()))
    return dict(loss=rows.mean(), S_loss=S_rows.mean(),
                ds=gs * (ps - pt), S_ds=S_ds)


def _ce_ref(s, y, gs):
    s = s.double()
    m, lz, lse = _row_stats(s)
    p = (s - lse).exp()
    sy = s.gather(1, y[:, None])
    onehot = torch.zeros_like(s).scatter_(1, y[:, None], 1.0)
    S_rows = 1 + m.abs() + lz.abs() + sy.abs()
    S_ds = gs * (p * (1 + _fin(s) + lse.abs()) + (p - onehot).abs())
    return dict(loss=(lse - sy).mean(), S_loss=S_rows.mean(),
                ds=gs * (p - onehot), S_ds=S_ds)


def _model_rows(x):
    """fp32 row statistics as the forward kernels form them"""
    m = x.max(1, keepdim=True).values
    z = torch.exp(x - m).sum(1, keepdim=True)
    return m, torch.log(z)


def _model_seq_mean(rows):
    """the atomicAdd of row / B, one row after the other, in fp32"""
    acc = torch.zeros((), dtype=FP32)
    B = float(rows.numel())
    for r in rows.flatten():
        acc = acc + r / B
    return acc


def _model_kd(s, t, up):
    dt = s.dtype
    s32, t32 = s.float(), t.float()
    ms, lzs = _model_rows(s32)
    mt, lzt = _model_rows(t32)
    pt = torch.exp(t32 - mt - lzt)
    rows = -(pt * (s32 - ms - lzs)).sum(1)
    lse_s, lse_t = ms + lzs, mt + lzt
    gscale = torch.tensor(1.0 / s.shape[0], dtype=FP32)
    ds = gscale * (torch.exp(s32 - lse_s) - torch.exp(t32 - lse_t))
    return _model_seq_mean(rows), ds.to(dt) * torch.tensor(up, dtype=FP32)


def _model_ce(s, y, up):
    dt = s.dtype
    s32 = s.float()
    m, lz = _model_rows(s32)
    lse = m + lz
    rows = lse - s32.gather(1, y[:, None])
    onehot = torch.zeros_like(s32).scatter_(1, y[:, None], 1.0)
    gscale = torch.tensor(1.0 / s.shape[0], dtype=FP32)
    ds = gscale * (torch.exp(s32 - lse) - onehot)
    return _model_seq_mean(rows), ds.to(dt) * torch.tensor(up, dtype=FP32)


def _ce_inputs(B, C, dtype):
    s = _logits(B, C, dtype, 700 + B + C)
    g = torch.Generator().manual_seed(800 + B + C)
    y = torch.randint(0, C, (B,), generator=g)
    y[0] = 0                                    # class 0 and class C - 1
    y[-1] = C - 1 if B > 1 or C == 1 else y[-1]
    if B == 1 and C > 1:
        y[0] = C - 1 if (B + C) % 2 else 0
    if B > 2 and C > 1:                         # -inf at a non-target class
        s[1, (int(y[1]) + 1) % C] = -math.inf
    other = torch.randint(0, C, (B,), generator=g)
    return s, y, other


def _loss_figs(kind, dtype, loss, grad, ref):
    bf = dtype == BF16
    sfx = " bf16" if bf else ""
    extra = 2 * BF16_RND * ref["ds"].abs() if bf else None
    return {"loss": (f"{kind} loss{sfx}",
                     _fig(loss, ref["loss"], ref["S_loss"])),
            "ds": (f"{kind} grad{sfx}",
                   _fig(grad, ref["ds"], ref["S_ds"], extra))}


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", LOGIT_SHAPES)
def test_logit_kd_against_fp64(B, C, dtype):
    """contiguous and column-slice students; the teacher once in the
    student's dtype and once in fp32 (the binding rounds it to bf16)"""
    s_cpu = _logits(B, C, dtype, 600 + B + C)
    t32 = _logits(B, C, FP32, 650 + B + C).flip(0)   # shifts on other rows
    for variant in ("contiguous", "sliced s, fp32 teacher"):
        s = s_cpu.cuda()
        t = t32.cuda().to(dtype)
        if variant != "contiguous":
            s = _noncontig(s)
            t = _noncontig(t32.cuda())
        s = s.detach().requires_grad_(True)
        loss = fused_logit_kd(s, t)
        loss.backward(torch.tensor(UP, device="cuda"))
        assert loss.dtype == FP32 and s.grad.dtype == dtype
        ref = _kd_ref(s.detach(), t.to(dtype), _f32(UP) / B)
        _check(f"logit KD {B}x{C} {variant}",
               _loss_figs("kd", dtype, loss, s.grad, ref))


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", LOGIT_SHAPES)
def test_cross_entropy_against_fp64(B, C, dtype):
    """contiguous inputs, then a column-slice s with a strided y: ce_bwd
    has to read the target through its strides as ce_fwd does"""
    s_cpu, y_cpu, other = _ce_inputs(B, C, dtype)
    for variant in ("contiguous", "sliced s, strided y"):
        s, y = s_cpu.cuda(), y_cpu.cuda()
        if variant != "contiguous":
            s = _noncontig(s)
            y = torch.stack([y, other.cuda()], 1)[:, 0]
            assert y.stride() == (2,)
        s = s.detach().requires_grad_(True)
        loss = FusedCrossEntropy()(s, y)
        loss.backward(torch.tensor(UP, device="cuda"))
        assert loss.dtype == FP32 and s.grad.dtype == dtype
        ref = _ce_ref(s.detach(), y, _f32(UP) / B)
        _check(f"CE {B}x{C} {variant}",
               _loss_figs("ce", dtype, loss, s.grad, ref))


def test_other_logit_dtypes_take_the_torch_formulas():
    """fp64 logits are routed to torch (the kernels would read them as
    fp32): the result is F.cross_entropy's own, in fp64"""
    g = torch.Generator().manual_seed(900)
    s = (3 * torch.randn(5, 10, generator=g, dtype=torch.float64)).cuda()
    t = (3 * torch.randn(5, 10, generator=g, dtype=torch.float64)).cuda()
    y = torch.randint(0, 10, (5,), generator=g).cuda()
    s1 = s.clone().requires_grad_(True)
    s2 = s.clone().requires_grad_(True)
    loss = FusedCrossEntropy()(s1, y)
    ref = F.cross_entropy(s2, y)
    assert loss.dtype == torch.float64 and torch.equal(loss, ref)
    loss.backward()
    ref.backward()
    assert torch.equal(s1.grad, s2.grad)
    kd = DistributionLoss()(s, t)
    kd_ref = -(F.softmax(t, 1) * F.log_softmax(s, 1)).sum(1).mean()
    assert kd.dtype == torch.float64 and torch.equal(kd, kd_ref)


def test_loss_bindings_refuse_fp64_logits():
    """the four entry points raise before any launch"""
    nat = _nat()
    s = torch.randn(4, 10, device="cuda", dtype=torch.float64)
    y = torch.zeros(4, dtype=torch.long, device="cuda")
    st1 = torch.zeros(4, device="cuda")
    st4 = torch.zeros(4, 4, device="cuda")
    msg = "fp32 or bf16"
    with pytest.raises(RuntimeError, match=msg):
        nat.ce_fwd(s, y)
    with pytest.raises(RuntimeError, match=msg):
        nat.ce_bwd(s, y, st1, 1.0)
    with pytest.raises(RuntimeError, match=msg):
        nat.kd_logit_fwd(s, s)
    with pytest.raises(RuntimeError, match=msg):
        nat.kd_logit_bwd(s, s, st4, 1.0)


# ------------------------------------------------------------ the CPU models

def _model_figures():
    """err / (eps S) of the fp32 CPU models against the fp64 references,
    over the cases of this file; C_BOUND is 16x these.  Needs no GPU."""
    out = {}

    def note(k, v):
        out[k] = max(out.get(k, 0.0), v)

    specs, ws, tg = _kurt_inputs()
    for mode_div in (1, len(ws)):
        gs = _f32(UP) / mode_div
        tot_m, tot_r = torch.zeros((), dtype=FP32), 0.0
        for i, (w, t) in enumerate(zip(ws, tg)):
            r = _kurt_ref(w.double(), _f32(t), gs)
            k, l, g = _model_kurt(w, _f32(t), gs)
            note("kurt", _fig(k, r["kurt"], r["kurt"].abs()))
            note("kurt grad", _fig(g, r["grad"], r["S_grad"]))
            tot_m, tot_r = tot_m + l, tot_r + r["loss"]
        note("kurt loss", _fig(tot_m / mode_div, tot_r / mode_div,
                               tot_r / mode_div))
    specs, ws, wt = _wkd_inputs()
    l_ref, S, g_ref = _wkd_ref(ws, wt, _f32(UP))
    l_m, g_m = _model_wkd(ws, wt, _f32(UP))
    note("wkd loss", _fig(l_m, l_ref, S))
    note("wkd grad", max(_fig(a, b, b.abs()) for a, b in zip(g_m, g_ref)))
    specs, (p, g, b) = _opt_inputs(3, zero_grad_elems=True)
    for lr, mom, wd in SGD_CASES:
        hp = [_f32(x) for x in (lr, mom, wd)]
        for pi, gi, bi in zip(p, g, b):
            r = _sgd_ref(pi, gi, bi, *hp)
            pm, bm = _model_sgd(pi, gi, bi, *hp)
            note("sgd", _fig(pm, r["p"], r["S_p"]))
            note("sgd", _fig(bm, r["buf"], r["S_buf"]))
    specs, (p, g, m, v) = _opt_inputs(4, zero_grad_elems=True)
    for step, wd in ADAM_CASES:
        hp = [_f32(x) for x in (1e-3, 0.9, 0.999, 1e-8, wd,
                                1 - 0.9 ** step, 1 - 0.999 ** step)]
        for i in range(len(p)):
            r = _adam_ref(p[i], g[i], m[i], v[i], *hp)
            pm, mm, vm = _model_adam(p[i], g[i], m[i], v[i], *hp)
            note("adam", _fig(pm, r["p"], r["S_p"]))
            note("adam", _fig(mm, r["m"], r["S_m"]))
            note("adam", _fig(vm, r["v"], r["S_v"]))
    for kind in ("sgd", "adam"):
        ps, _, _ = _run_class(kind, "cpu", FP32, fused=True)
        ref, _, hist = _run_class(kind, "cpu", torch.float64, fused=False)
        scales = _class_scales(kind, hist, [r.detach() for r in ref])
        note(f"{kind} steps", max(_fig(a.detach(), b.detach(), S)
                                  for a, b, S in zip(ps, ref, scales)))
    for B, C in LOGIT_SHAPES:
        for dtype in (FP32, BF16):
            bf = dtype == BF16
            s = _logits(B, C, dtype, 600 + B + C)
            t = _logits(B, C, FP32, 650 + B + C).flip(0).to(dtype)
            ref = _kd_ref(s, t, _f32(UP) / B)
            l, ds = _model_kd(s, t, _f32(UP))
            extra = 2 * BF16_RND * ref["ds"].abs() if bf else None
            note("kd loss", _fig(l, ref["loss"], ref["S_loss"]))
            note("kd grad", _fig(ds, ref["ds"], ref["S_ds"], extra))
            s, y, _ = _ce_inputs(B, C, dtype)
            ref = _ce_ref(s, y, _f32(UP) / B)
            l, ds = _model_ce(s, y, _f32(UP))
            extra = 2 * BF16_RND * ref["ds"].abs() if bf else None
            note("ce loss", _fig(l, ref["loss"], ref["S_loss"]))
            note("ce grad", _fig(ds, ref["ds"], ref["S_ds"], extra))
    return out
