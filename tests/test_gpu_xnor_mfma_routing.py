"""Routing of the binary conv forward between the i8 MFMA kernel
(csrc/xnor_conv_mfma.hip) and the XNOR+popcount kernel: the routing table
behind nat.xnor_conv_fwd, the BDBNN_XNOR_MFMA knob, want_stats."""

import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _resnet18_forward_route_calls():
    """(MFMA, VALU) forward conv calls of one bf16-autocast training
    forward of imagenet.resnet18 at 2x3x64x64."""
    from bdbnn_amd.models import imagenet as im
    nat = _nat()
    torch.manual_seed(81)
    m = im.resnet18(False, num_classes=10).cuda().to(
        memory_format=torch.channels_last)
    m.train()
    x = _cl(torch.randn(2, 3, 64, 64, device="cuda"))
    before = nat.xnor_route_calls()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(x)
    torch.cuda.synchronize()
    after = nat.xnor_route_calls()
    assert torch.isfinite(out.float()).all()
    return after[0] - before[0], after[1] - before[1]


def test_resnet18_forward_takes_mfma_for_its_3x3_convs():
    """16 3x3 binary convs on the MFMA kernel; the three 1x1/s2
    downsample convs stay on the VALU kernel."""
    mfma, valu = _resnet18_forward_route_calls()
    print(f"route calls: mfma={mfma} valu={valu}")
    assert mfma == 16
    assert valu == 3


_CHILD = """
import json, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from test_gpu_xnor_mfma_routing import _resnet18_forward_route_calls
print("ROUTE " + json.dumps(_resnet18_forward_route_calls()))
"""


def test_knob_off_takes_mfma_for_none():
    """BDBNN_XNOR_MFMA is read once per process, so the knob-off forward
    runs in a fresh child process."""
    env = dict(os.environ, BDBNN_XNOR_MFMA="0")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROUTE ")]
    assert line, p.stdout[-2000:]
    mfma, valu = json.loads(line[-1][len("ROUTE "):])
    print(f"knob off: mfma={mfma} valu={valu}")
    assert mfma == 0
    assert valu == 19


def test_want_stats_takes_the_valu_kernel():
    """A supported shape with want_stats=True stays on the VALU kernel,
    and its epilogue sums still match the stored output (tolerances of
    test_conv_epilogue_stats_match_output_sums)."""
    torch.manual_seed(82)
    nat = _nat()
    x = torch.randn(3, 64, 14, 14, device="cuda")
    w = torch.randn(64, 64, 3, 3, device="cuda")
    assert nat.xnor_mfma_supported(64, 64, 3, 3, 1, 1)
    xp = nat.sign_pack_nhwc(_cl(x))
    wp, alpha, stab = nat.weight_pack(w)
    before = nat.xnor_route_calls()
    out, s1, s2 = nat.xnor_conv_fwd(xp, wp, alpha, stab, 64, 1, 1, False,
                                    True)
    after = nat.xnor_route_calls()
    assert after[0] == before[0] and after[1] == before[1] + 1
    v = out.double()
    ref1 = v.sum(dim=(0, 2, 3))
    ref2 = (v * v).sum(dim=(0, 2, 3))
    tol = 64.0 * 2.0 ** -24
    assert ((s1.sum(0).double() - ref1).abs()
            <= tol * v.abs().sum(dim=(0, 2, 3))).all()
    assert ((s2.sum(0).double() - ref2).abs() <= tol * ref2).all()
    assert torch.allclose(s1.sum(0), ref1.float(), rtol=1e-4, atol=1e-2)
    assert torch.allclose(s2.sum(0), ref2.float(), rtol=1e-4, atol=1e-1)
    # and without stats the same call is the MFMA kernel's, bit for bit
    out2 = nat.xnor_conv_fwd(xp, wp, alpha, stab, 64, 1, 1, False, False)[0]
    assert nat.xnor_route_calls()[0] == after[0] + 1
    assert torch.equal(out2, out)
