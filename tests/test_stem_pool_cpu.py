"""fused_bn_relu_maxpool off the GPU: the exact composition."""

import torch
import torch.nn.functional as F

from bdbnn_amd.ops.bn_act import fused_bn_relu_maxpool
from bdbnn_amd.ops.pool import FusedMaxPool2d


def _pair(C):
    torch.manual_seed(5)
    bn = torch.nn.BatchNorm2d(C)
    bn2 = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.normal_(); bn.bias.normal_()
        bn2.load_state_dict(bn.state_dict())
    return bn, bn2


def test_cpu_training_matches_composition_exactly():
    bn, bn2 = _pair(16)
    x = torch.randn(2, 16, 9, 11, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    out = fused_bn_relu_maxpool(x, bn, FusedMaxPool2d(3, 2, 1))
    ref = F.max_pool2d(F.relu(bn2(x2)), 3, 2, 1)
    assert torch.equal(out, ref)
    g = torch.randn_like(ref)
    out.backward(g)
    ref.backward(g)
    assert torch.equal(x.grad, x2.grad)
    assert torch.equal(bn.weight.grad, bn2.weight.grad)
    assert torch.equal(bn.bias.grad, bn2.bias.grad)
    assert torch.equal(bn.running_mean, bn2.running_mean)
    assert torch.equal(bn.running_var, bn2.running_var)
    assert bn.num_batches_tracked.item() == bn2.num_batches_tracked.item()


def test_cpu_eval_and_pack_request():
    bn, bn2 = _pair(32)
    bn.eval(); bn2.eval()
    x = torch.randn(1, 32, 8, 8)
    out, pk = fused_bn_relu_maxpool(x, bn, FusedMaxPool2d(2, 2, 0),
                                    pack=True)
    assert pk is None
    assert torch.equal(out, F.max_pool2d(F.relu(bn2(x)), 2, 2, 0))


def test_cpu_model_forward_unchanged_by_the_knob(monkeypatch):
    from bdbnn_amd.models import imagenet as im
    from bdbnn_amd.models import resnet_common as rc
    torch.manual_seed(6)
    m = im.resnet18(False, num_classes=10)
    m.eval()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        a = m(x)
        monkeypatch.setattr(rc, "_FUSE_STEM_POOL", False)
        b = m(x)
    assert torch.equal(a, b)
