"""Which weight-gradient kernels one bf16 step of ResNet-18 at 64x64 runs:
with BDBNN_WGRAD3 on, every stride-1 3x3 binary conv that wgrad3_supported
admits takes conv_wgrad3 and needs no repack_cplane (all 13: every class
is routed); with the knob off all 13 run repack_cplane + conv_wgrad2.  The
stride-2 convs keep their kernels on either setting."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.ops import binary_conv as bc

NAMES = ("conv_wgrad3", "conv_wgrad2", "repack_cplane", "conv_wgrad2_s2",
         "repack_cplane_s2")


def _step(monkeypatch, knob):
    from bdbnn_amd.models import imagenet as im
    nat = _C.native_required()
    monkeypatch.setattr(bc, "_WGRAD3", knob)
    calls = {n: [] for n in NAMES}
    for name in NAMES:
        def counted(*a, _r=getattr(nat, name), _c=calls[name], **kw):
            _c.append(1)
            return _r(*a, **kw)
        monkeypatch.setattr(nat, name, counted)
    admitted = []
    real_ok = nat.wgrad3_supported

    def ok(*a):
        admitted.append(bool(real_ok(*a)))
        return admitted[-1]
    monkeypatch.setattr(nat, "wgrad3_supported", ok)

    torch.manual_seed(93)
    m = im.resnet18(False, num_classes=10).cuda().to(
        memory_format=torch.channels_last)
    x = torch.randn(8, 3, 64, 64, device="cuda").contiguous(
        memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(m(x).float(), y)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    counts = {n: len(c) for n, c in calls.items()}
    print(f"knob {'on' if knob else 'off'}: {counts}, predicate {admitted}")
    return counts, admitted


def test_resnet18_knob_on_runs_wgrad3_without_repack(monkeypatch):
    counts, admitted = _step(monkeypatch, True)
    assert len(admitted) == 13          # asked once per stride-1 3x3 conv
    n3 = sum(admitted)
    assert n3 == 13                     # every class is routed
    assert counts["conv_wgrad3"] == n3
    assert counts["conv_wgrad2"] == 13 - n3
    assert counts["repack_cplane"] == 13 - n3
    # stride 2: the 4 convs test_gpu_bwd_s2_routing.py has on record
    assert counts["conv_wgrad2_s2"] == 4 and counts["repack_cplane_s2"] == 4


def test_resnet18_knob_off_runs_repack_and_wgrad2(monkeypatch):
    counts, admitted = _step(monkeypatch, False)
    assert admitted == []               # the knob is checked first
    assert counts["conv_wgrad3"] == 0
    assert counts["conv_wgrad2"] == 13 and counts["repack_cplane"] == 13
    assert counts["conv_wgrad2_s2"] == 4 and counts["repack_cplane_s2"] == 4
