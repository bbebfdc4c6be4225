"""FusedSGD / FusedAdam semantics that need no GPU: the pure-torch branch
against torch.optim run in fp64 (a parameter that skips a step included),
the layout of optimiser state after a state_dict round trip, and the dtype
predicate that decides which logits reach the loss.hip kernels."""

import pytest
import torch

from bdbnn_amd.ops.optim import FusedAdam, FusedSGD

SHAPES = [(1,), (257,), (16, 8, 3, 3), (8, 16, 1, 1), (5, 7)]
CASES = [
    ("sgd", dict(lr=0.1, momentum=0.9, weight_decay=1e-4)),
    ("sgd", dict(lr=0.1, momentum=0.0, weight_decay=0.0)),
    ("adam", dict(lr=1e-2, weight_decay=1e-4)),
    ("adam", dict(lr=1e-2, weight_decay=0.0)),
]


def _make(kind, params, kw, fused):
    if kind == "sgd":
        return (FusedSGD if fused else torch.optim.SGD)(params, **kw)
    return (FusedAdam if fused else torch.optim.Adam)(params, **kw)


@pytest.mark.parametrize("kind,kw", CASES)
def test_cpu_branch_matches_torch_optim_fp64_with_a_skipped_step(kind, kw):
    """Three steps in fp64 on both sides, so the only difference left is the
    order of a few fp64 operations: 1e-12 relative.  Parameter 1 has no
    .grad on the first step; its bias correction then lags one step behind
    the others', which a step count shared by the group gets wrong (4.5e-3
    after three steps at lr = 1e-2)."""
    g = torch.Generator().manual_seed(11)
    init = [torch.randn(s, generator=g, dtype=torch.float64) for s in SHAPES]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64)
              for s in SHAPES] for _ in range(3)]
    ours = [t.clone().requires_grad_(True) for t in init]
    ref = [t.clone().requires_grad_(True) for t in init]
    opt, topt = _make(kind, ours, kw, True), _make(kind, ref, kw, False)
    for step in range(3):
        for i, (p, r) in enumerate(zip(ours, ref)):
            skip = step == 0 and i == 1
            p.grad = None if skip else grads[step][i].clone()
            r.grad = None if skip else grads[step][i].clone()
        opt.step()
        topt.step()
    for i, (p, r) in enumerate(zip(ours, ref)):
        err = (p - r).abs().max().item()
        assert err <= 1e-12 * (1 + r.abs().max().item()), (i, err)
    if kind == "adam":
        assert [opt.state[p]["step"] for p in ours] == [3, 2, 3, 3, 3]


@pytest.mark.parametrize("kind,kw", CASES[::2])
def test_loaded_state_takes_its_parameters_layout(kind, kw):
    """A state dict saved from an NCHW run and loaded for channels_last
    parameters keeps the saved strides; the fused kernels pair state and
    parameter over physical memory, so step() must bring the state into
    the parameter's layout (and keep it in self.state)."""
    g = torch.Generator().manual_seed(12)
    w = torch.randn(16, 3, 3, 3, generator=g)
    grad = torch.randn(16, 3, 3, 3, generator=g)
    src = w.clone().requires_grad_(True)
    src.grad = grad.clone()
    saved = _make(kind, [src], kw, True)
    saved.step()

    cl = torch.channels_last
    dst = src.detach().clone(memory_format=cl).requires_grad_(True)
    assert dst.stride() == (27, 1, 9, 3)
    opt = _make(kind, [dst], kw, True)
    opt.load_state_dict(saved.state_dict())
    ref = w.double().requires_grad_(True)      # torch.optim, both steps
    topt = _make(kind, [ref], kw, False)
    ref.grad = grad.double()
    topt.step()

    dst.grad = grad.contiguous(memory_format=cl)
    ref.grad = grad.double()
    opt.step()
    topt.step()
    state = [v for v in opt.state[dst].values() if torch.is_tensor(v)
             and v.dim() == 4]
    assert len(state) == (1 if kind == "sgd" else 2)
    for t in state:
        assert t.stride() == dst.stride(), t.stride()
    # fp32 step against fp64: a few fp32 roundings of values of order 1
    assert (dst.double() - ref).abs().max().item() <= 1e-5


@pytest.mark.parametrize("dtype,expect", [
    (torch.float32, True), (torch.bfloat16, True),
    (torch.float16, False), (torch.float64, False)])
def test_native_logits_predicate_is_dtype_exact(dtype, expect, monkeypatch):
    """Only fp32 and bf16 (B, C) device logits reach the kernels.  The
    device and the extension are faked here so the dtype decides alone."""
    from bdbnn_amd import _C
    from bdbnn_amd.ops.losses import native_logits

    class _Logits:
        is_cuda = True

        def __init__(self, dtype, dim=2):
            self.dtype, self._dim = dtype, dim

        def dim(self):
            return self._dim

    monkeypatch.setattr(_C, "has_native", lambda: True)
    assert native_logits(_Logits(dtype)) is expect
    assert native_logits(_Logits(dtype, dim=3)) is False
    assert native_logits(torch.zeros(2, 3, dtype=dtype)) is False   # on CPU


def test_oracle_constants_are_16x_their_cpu_models():
    """tests/test_gpu_scalar_kernels_oracle.py bounds each kernel by
    c eps S with c = 16 x the figure of an fp32 CPU model of the kernel:
    the recorded figures must be what the models give."""
    import test_gpu_scalar_kernels_oracle as oracle
    figs = oracle._model_figures()
    assert set(figs) == set(oracle.MODEL_FIGURE) == set(oracle.C_BOUND)
    for k, v in figs.items():
        rec = oracle.MODEL_FIGURE[k]
        assert 0.9 * rec <= v <= rec, (k, v, rec)
        assert oracle.C_BOUND[k] == 16.0 * rec
