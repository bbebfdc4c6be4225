"""Routing of the ImageNet stem tail (bn1 -> ReLU -> maxpool) in
ResNet.forward onto the fused op of csrc/bn_pool.hip, the hand-off of its
epilogue pack to layer1.0.conv1, and the BDBNN_FUSE_STEM_POOL knob."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from bdbnn_amd import _C
from bdbnn_amd.models import imagenet as im
from bdbnn_amd.models import resnet_common as rc


def _nat():
    return _C.native_required()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _count(monkeypatch, name):
    nat = _nat()
    real = getattr(nat, name)
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(nat, name, counted)
    return calls


def _model(ctor=im.resnet18, seed=90):
    torch.manual_seed(seed)
    return ctor(False, num_classes=10).cuda().to(
        memory_format=torch.channels_last)


def _batch(seed=91):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = _cl(torch.randn(2, 3, 64, 64, device="cuda", generator=g))
    y = torch.randint(0, 10, (2,), device="cuda", generator=g)
    return x, y


def _step(m, backward=True):
    x, y = _batch()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(x)
        loss = torch.nn.functional.cross_entropy(out.float(), y)
    if backward:
        loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    return loss.detach()


def _spy_prepack(monkeypatch, conv):
    seen = []
    real = conv.forward_with_stats

    def spy(x, prepack=None, skip_cell=None):
        seen.append(prepack)
        return real(x, prepack=prepack, skip_cell=skip_cell)
    monkeypatch.setattr(conv, "forward_with_stats", spy)
    return seen


def test_training_runs_fused_op_once_and_hands_over_the_pack(monkeypatch):
    assert rc._FUSE_STEM_POOL     # the default
    m = _model()
    m.train()
    fused = _count(monkeypatch, "bn_relu_maxpool_fwd_train")
    fused_bwd = _count(monkeypatch, "bn_relu_maxpool_bwd")
    pool = _count(monkeypatch, "maxpool_fwd")
    packs = _count(monkeypatch, "sign_mask_pack_nhwc")
    seen = _spy_prepack(monkeypatch, m.layer1[0].conv1)
    _step(m)
    assert len(fused) == 1 and len(fused_bwd) == 1 and len(pool) == 0
    assert len(seen) == 1 and seen[0] is not None
    xp, mp = seen[0]
    assert xp.shape == (2, 16, 16, 2) and mp.shape == xp.shape
    n_on = len(packs)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n

    # knob off: one more pack pass — layer1.0.conv1 packs its own input
    monkeypatch.setattr(rc, "_FUSE_STEM_POOL", False)
    del packs[:], seen[:], fused[:]
    m.zero_grad(set_to_none=True)
    _step(m)
    assert len(fused) == 0 and len(pool) == 1
    assert seen == [None]
    print(f"sign_mask_pack_nhwc calls: {n_on} fused, {len(packs)} unfused")
    assert len(packs) == n_on + 1


@pytest.mark.parametrize("why", ["knob_off", "eval", "no_grad"])
def test_old_composition_cases(monkeypatch, why):
    m = _model()
    m.train()
    if why == "knob_off":
        monkeypatch.setattr(rc, "_FUSE_STEM_POOL", False)
    elif why == "eval":
        _step(m)              # populate the running statistics
        m.eval()
    fused = _count(monkeypatch, "bn_relu_maxpool_fwd_train")
    pool = _count(monkeypatch, "maxpool_fwd")
    if why == "no_grad":
        with torch.no_grad():
            _step(m, backward=False)
    else:
        _step(m, backward=(why != "eval"))
    assert len(fused) == 0 and len(pool) == 1


def test_real_valued_model_gets_a_plain_tensor(monkeypatch):
    m = _model(im.resnet18_real)
    m.train()
    fused = _count(monkeypatch, "bn_relu_maxpool_fwd_train")
    _step(m)
    assert len(fused) == 1


def test_state_dict_keys_unchanged(monkeypatch):
    m = _model()
    keys = list(m.state_dict().keys())
    m.train()
    _step(m)
    assert list(m.state_dict().keys()) == keys
    assert m.bn1.num_batches_tracked.item() == 1
    monkeypatch.setattr(rc, "_FUSE_STEM_POOL", False)
    m2 = _model()
    assert list(m2.state_dict().keys()) == keys
    m2.load_state_dict(m.state_dict())


def test_one_step_loss_fused_vs_knob_off(monkeypatch):
    """Same seed, one training step each way: the losses agree to the bf16
    tolerance of test_fused_bn_act_train_bf16, and so do the running
    statistics of bn1."""
    m_on, m_off = _model(seed=92), _model(seed=92)
    m_on.train(); m_off.train()
    loss_on = _step(m_on)
    monkeypatch.setattr(rc, "_FUSE_STEM_POOL", False)
    loss_off = _step(m_off)
    print(f"loss fused {loss_on.item():.6f} unfused {loss_off.item():.6f}")
    assert torch.allclose(loss_on, loss_off, atol=5e-2, rtol=5e-2)
    assert torch.allclose(m_on.bn1.running_mean, m_off.bn1.running_mean,
                          atol=1e-4)
    assert torch.allclose(m_on.bn1.running_var, m_off.bn1.running_var,
                          atol=1e-4)
    g_on, g_off = m_on.bn1.weight.grad, m_off.bn1.weight.grad
    assert torch.isfinite(g_on).all() and torch.isfinite(g_off).all()
