"""The fused stem tail's entry points (csrc/bn_pool.hip) must be part of
the built extension — checked on a CPU-only machine too, where a source
file missing from setup.py would otherwise only show up as an undefined
symbol on the GPU box."""

import pytest


EXPECTED_STEM_POOL = ["bn_relu_maxpool_fwd_train", "bn_relu_maxpool_bwd"]

# the unfused pair stays exported: benchmarks and tests call it directly
# and it is the A/B baseline
KEPT = ["bn_act_fwd_train", "bn_act_bwd", "maxpool_fwd", "maxpool_bwd"]


def test_native_extension_exposes_stem_pool():
    _native = pytest.importorskip("bdbnn_amd._native")
    missing = [n for n in EXPECTED_STEM_POOL + KEPT
               if not hasattr(_native, n)]
    assert not missing, missing
