#!/usr/bin/env python3
"""Binary conv forward per layer: the i8 MFMA kernel
(csrc/xnor_conv_mfma.hip) against the XNOR+popcount kernel
(csrc/xnor_conv.hip), both forced through their own bindings from this one
build, bf16 output, at the seven 3x3 shapes of ImageNet ResNet-18/34.

  python benchmarks/xnor_mfma_bench.py [batch ...] [--repeats R]

Default batches 256 and 2048.  ms per call, median [min-max] over the
repeats; the two kernels are timed alternately inside every repeat so
drift of a shared machine hits them alike.  Host clock around 20 calls
ending in a synchronise: launch overhead is part of every figure.
T MAC/s = N*Ho*Wo*K*9*C / time; GB/s out = output bytes / time.  This
table decides the routing table in xnor_conv_mfma.hip: a class ships on
the MFMA kernel when its whole range lies below the VALU kernel's.
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bdbnn_amd import _C

# (C, H, K, stride): 3x3/s1 C=K stages, then the 3x3/s2 downsampling convs
SHAPES = [(64, 56, 64, 1), (128, 28, 128, 1), (256, 14, 256, 1),
          (512, 7, 512, 1), (64, 56, 128, 2), (128, 28, 256, 2),
          (256, 14, 512, 2)]


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
        print(f"\nbatch {N}, bf16 out; median [min-max] of {args.repeats} "
              f"repeats x 20 calls\n")
        print("| C | HxW | K | stride | kernel | ms per call | T MAC/s "
              "| out GB | out GB/s | equal |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for C, H, K, stride in SHAPES:
            torch.manual_seed(0)
            x = cl(torch.randn(N, C, H, H, device="cuda",
                               dtype=torch.bfloat16))
            w = torch.randn(K, C, 3, 3, device="cuda")
            xp = nat.sign_pack_nhwc(x)
            wp, alpha, stab = nat.weight_pack(w)
            del x
            Ho = (H + 2 - 3) // stride + 1
            macs = N * Ho * Ho * K * 9 * C
            obytes = N * Ho * Ho * K * 2

            def mfma():
                return nat.xnor_conv_mfma_fwd(xp, wp, alpha, C, stride, 1,
                                              True)

            def valu():
                return nat.xnor_conv_valu_fwd(xp, wp, alpha, stab, C, stride,
                                              1, True, False)[0]

            same = torch.equal(mfma(), valu())
            fns = [("mfma", mfma), ("valu", valu)]
            for _, fn in fns:
                for _ in range(3):
                    fn()
            samples = [[] for _ in fns]
            for _ in range(args.repeats):
                for s, (_, fn) in zip(samples, fns):
                    s.append(timeit(fn))
            for (name, _), s in zip(fns, samples):
                m = statistics.median(s) * 1e-3
                print(f"| {C} | {H}x{H} | {K} | {stride} | {name} | {fmt(s)} "
                      f"| {macs / m / 1e12:.0f} | {obytes / 1e9:.3f} "
                      f"| {obytes / m / 1e9:.0f} | {same} |", flush=True)
            del xp


if __name__ == "__main__":
    main()
