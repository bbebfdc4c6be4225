#!/usr/bin/env python3
"""Per-conv backward cost of the stride-2 binary convs (3x3/s2/p1 conv1 and
1x1/s2/p0 downsample.0 of layer{2,3,4}.0) on the ImageNet ResNet-18
shapes: the owned parity kernels (csrc/conv_bwd_s2.hip) vs the same build
with BDBNN_MFMA_BWD_S2=0, which runs exactly the previous backward
(decode_packed / binsign_decode + weight decode + MIOpen dgrad and wrw +
a separate mask pass).

  python benchmarks/backward_s2_bench.py [batch] [repeats]

One row per (shape, kernel size, mask).  Columns are ms per backward call
of BinaryConvFunction (dx AND dw), median [min-max] over the repeats:
  owned    knob on
  off      knob off
  off'     knob off again — a second, independent sample set of the same
           code, so the table carries the run-to-run spread of the
           knob-off path itself
  spread   max - min over all knob-off samples (off and off')
  verdict  "ok" when median(owned) <= median(off) + spread
Host clock around 20 backward calls ending in a synchronise: launch
overhead is part of every figure.  The three variants are timed alternately
inside every repeat so drift of a shared machine hits them alike.
"""

import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bdbnn_amd import _C
from bdbnn_amd.ops import binary_conv as bc
from bdbnn_amd.ops.binary_conv import BinaryConvFunction

SHAPES = [(64, 56, 128), (128, 28, 256), (256, 14, 512)]   # C, H=W, K
MASKS = [("ste", "ste", None, None), ("approx", "approx", None, None),
         ("ede", "ste", 1.0, 1.0)]


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
    assert bc._MFMA_BWD, "run with BDBNN_MFMA_BWD unset"
    print(f"batch {N}; ms per backward call (dx + dw), median [min-max] of "
          f"{reps} repeats x 20 calls\n")
    print("| conv | mask | owned | off | off' | spread | owned/off "
          "| verdict |")
    print("|---|---|---|---|---|---|---|---|")
    losers = []
    for (C, H, K) in SHAPES:
        for ks, pad in ((3, 1), (1, 0)):
            # shapes the predicate keeps on the fallback (measured
            # slower) run the same code on both sides of the knob
            routed = nat.dgrad2_s2_supported(H, H, C, K, ks)
            for name, act, t, k in MASKS:
                torch.manual_seed(0)
                x = cl(torch.randn(N, C, H, H, device="cuda",
                                   dtype=torch.bfloat16)).requires_grad_(True)
                w = torch.randn(K, C, ks, ks,
                                device="cuda").requires_grad_(True)
                out, _, _ = BinaryConvFunction.apply(x, w, 2, pad, act, t, k,
                                                     False)
                gout = cl(torch.randn_like(out))

                def backward(flag):
                    def run():
                        bc._MFMA_BWD_S2 = flag
                        return torch.autograd.grad(out, (x, w), gout,
                                                   retain_graph=True)
                    return run

                fns = (backward(True), backward(False), backward(False))
                for fn in fns:      # warm-up: code objects, MIOpen find
                    for _ in range(3):
                        fn()
                samples = [[], [], []]
                for _ in range(reps):
                    for s, fn in zip(samples, fns):
                        s.append(timeit(fn))
                bc._MFMA_BWD_S2 = True
                a, b = (statistics.median(s) for s in samples[:2])
                off_all = samples[1] + samples[2]
                spread = max(off_all) - min(off_all)
                ok = a <= b + spread
                tag = (f"{C}x{H}x{H}->{K} {ks}x{ks}"
                       + ("" if routed else " (not routed)"))
                if not ok:
                    losers.append(f"{tag} {name}")
                print(f"| {tag} | {name} | {fmt(samples[0])} "
                      f"| {fmt(samples[1])} | {fmt(samples[2])} "
                      f"| {spread:.3f} | {a / b:.2f} "
                      f"| {'ok' if ok else 'SLOWER'} |", flush=True)
                del out, gout, x, w
    print("\nslower than knob-off beyond its spread: "
          + (", ".join(losers) if losers else "none"))


if __name__ == "__main__":
    main()
