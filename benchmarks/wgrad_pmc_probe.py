#!/usr/bin/env python3
"""Minimal probe for rocprofv3 --pmc runs (counters only, one run per
counter group): repeats the stride-1 weight gradient on the four ResNet-18
layer shapes at batch 2048, 10 calls each of repack_cplane + conv_wgrad2
and of conv_wgrad3."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bdbnn_amd import _C

nat = _C.native_required()
cl = lambda t: t.contiguous(memory_format=torch.channels_last)
for (C, H, K) in [(64, 56, 64), (128, 28, 128), (256, 14, 256),
                  (512, 7, 512)]:
    x = cl(torch.randn(2048, C, H, H, device="cuda", dtype=torch.bfloat16))
    g = cl(torch.randn(2048, K, H, H, device="cuda", dtype=torch.bfloat16))
    xp = nat.sign_pack_nhwc(x)
    del x
    for _ in range(10):
        old = nat.conv_wgrad2(g, nat.repack_cplane(xp, C, H), C)
    for _ in range(10):
        new = nat.conv_wgrad3(g, xp, C)
    torch.cuda.synchronize()
    del g, xp, old, new
print("probe done")
