#!/usr/bin/env python3
"""Per-layer dgrad cost of the value-mask activation modes (ReAct
polynomial = mode 1, EDE = mode 2) on the four ResNet-18 stride-1 layer
shapes: the owned MFMA kernel vs the fallback pipeline it replaces, with
the clip-STE (mode 0) kernel as the floor.

  python benchmarks/backward_modes_bench.py [batch] [repeats]

Columns (ms per call; median over the repeats, [min-max] spread):
  (a) dgrad_weight_decode + conv_dgrad2_x
  (b) binsign_decode + aten dgrad (MIOpen) + ste_mask_mul
  (c) dgrad_weight_decode + conv_dgrad2 (mode 0)
Host clock around 20 launches ending in a synchronise: launch overhead
is part of every figure and a large part at the smallest shape (512x7x7),
so read the columns as per-call pipeline cost, not kernel time.
The three variants are timed alternately inside every repeat so drift of
a shared machine hits them alike.
"""

import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bdbnn_amd import _C
from bdbnn_amd.ops.binarize import binsign, weight_scale


def timeit(fn, iters=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def fmt(samples):
    return (f"{statistics.median(samples):.3f} "
            f"[{min(samples):.3f}-{max(samples):.3f}]")


def main():
    nat = _C.native_required()
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    # EDE (t, k) mid-schedule; the kernel's cost does not depend on them
    T, K_EDE = 1.0, 1.0
    print(f"batch {N}; ms per call, median [min-max] of {reps} repeats "
          f"x 20 calls\n")
    print("| layer | mode | (a) wdec + conv_dgrad2_x | (b) fallback: "
          "binsign_decode + MIOpen dgrad + ste_mask_mul | (c) mode-0 wdec + "
          "conv_dgrad2 | (a)/(b) | (a)/(c) |")
    print("|---|---|---|---|---|---|---|")
    for (C, H, K) in [(64, 56, 64), (128, 28, 128), (256, 14, 256),
                      (512, 7, 512)]:
        torch.manual_seed(0)
        x = cl(torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16))
        w = torch.randn(K, C, 3, 3, device="cuda")
        g = cl(torch.randn(N, K, H, H, device="cuda", dtype=torch.bfloat16))
        _, mp = nat.sign_mask_pack_nhwc(x)
        wp, alpha, _ = nat.weight_pack(w)
        for mode, t, k in [(1, 0.0, 0.0), (2, T, K_EDE)]:

            def owned():
                wd = nat.dgrad_weight_decode(wp, alpha, C)
                return nat.conv_dgrad2_x(g, wd, x, C, mode, t, k)

            def fallback():
                # what BinaryConvFunction.backward runs for dx when the
                # owned path is off (dgrad only; wgrad is common to both)
                xb = nat.binsign_decode(x, 1)
                wb = (weight_scale(w) * binsign(w)).to(torch.bfloat16)
                dxb = torch.ops.aten.convolution_backward(
                    g, xb, wb, None, [1, 1], [1, 1], [1, 1], False, [0, 0],
                    1, [True, False, False])[0]
                return nat.ste_mask_mul(dxb, x, mode, t, k)

            def floor():
                wd = nat.dgrad_weight_decode(wp, alpha, C)
                return nat.conv_dgrad2(g, wd, mp, C)

            fns = (owned, fallback, floor)
            for fn in fns:          # warm-up: code objects, MIOpen find
                for _ in range(3):
                    fn()
            samples = [[], [], []]
            for _ in range(reps):
                for s, fn in zip(samples, fns):
                    s.append(timeit(fn))
            a, b, c = (statistics.median(s) for s in samples)
            print(f"| {C}x{H}x{H}->{K} | {mode} | {fmt(samples[0])} "
                  f"| {fmt(samples[1])} | {fmt(samples[2])} "
                  f"| {a / b:.2f} | {a / c:.2f} |", flush=True)


if __name__ == "__main__":
    main()
