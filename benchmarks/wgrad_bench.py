#!/usr/bin/env python3
"""Stride-1 3x3 weight gradient per layer: conv_wgrad3
(csrc/conv_wgrad3.hip, reads the NHWC sign plane) against repack_cplane +
conv_wgrad2 (csrc/conv_bwd.hip), both through their own bindings from this
one build, at the four stride-1 shapes of ImageNet ResNet-18.

  python benchmarks/wgrad_bench.py [batch ...] [--repeats R]

Default batches 256 and 2048.  ms per call, median [min-max] over the
repeats; the two paths are timed alternately inside every repeat so drift
of a shared machine hits them alike.  Host clock around 20 calls ending in
a synchronise: launch overhead is part of every figure.  Useful T MAC/s =
N*H*W*K*9*C / time (dummy columns not counted); peak % is against the
1.25 P MAC/s bf16 MFMA peak.  `close` compares the slab sums of the two
paths (fp32 summation order differs).  This table decides
wgrad3_class_routed in conv_wgrad3.hip: a class ships on wgrad3 when its
whole range at batch 2048 lies below the old path's.
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bdbnn_amd import _C

# (C, H, K)
SHAPES = [(64, 56, 64), (128, 28, 128), (256, 14, 256), (512, 7, 512)]
PEAK_MACS = 1.25e15


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
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", type=int, nargs="*", default=[256, 2048])
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    nat = _C.native_required()
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    for N in args.batch:
        print(f"\nbatch {N}; median [min-max] of {args.repeats} repeats x 20 "
              f"calls\n")
        print("| C | HxW | K | path | ms per call | T MAC/s | peak % "
              "| close |")
        print("|---|---|---|---|---|---|---|---|")
        for C, H, K in SHAPES:
            torch.manual_seed(0)
            x = cl(torch.randn(N, C, H, H, device="cuda",
                               dtype=torch.bfloat16))
            g = cl(torch.randn(N, K, H, H, device="cuda",
                               dtype=torch.bfloat16))
            xp = nat.sign_pack_nhwc(x)
            del x
            macs = N * H * H * K * 9 * C

            def new():
                return nat.conv_wgrad3(g, xp, C)

            def old():
                return nat.conv_wgrad2(g, nat.repack_cplane(xp, C, H), C)

            a, b = new().sum(0), old().sum(0)
            close = torch.allclose(a, b, rtol=1e-3,
                                   atol=1e-3 * b.abs().max().item())
            fns = [("wgrad3", new), ("repack+wgrad2", old)]
            for _, fn in fns:
                for _ in range(3):
                    fn()
            samples = [[] for _ in fns]
            for _ in range(args.repeats):
                for s, (_, fn) in zip(samples, fns):
                    s.append(timeit(fn))
            for (name, _), s in zip(fns, samples):
                m = statistics.median(s) * 1e-3
                print(f"| {C} | {H}x{H} | {K} | {name} | {fmt(s)} "
                      f"| {macs / m / 1e12:.0f} "
                      f"| {100 * macs / m / PEAK_MACS:.1f} | {close} |",
                      flush=True)
            del xp, g


if __name__ == "__main__":
    main()
