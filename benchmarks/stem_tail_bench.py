#!/usr/bin/env python3
"""Stem tail bn1 -> ReLU -> maxpool(3,2,1) at the ImageNet ResNet shape
(112x112x64, bf16): the fused op of csrc/bn_pool.hip against the unfused
composition it replaces (bn_act + maxpool + layer1.0.conv1's
sign_mask_pack), both from this one build.

  python benchmarks/stem_tail_bench.py [batch ...] [--repeats R]

Default batches 256 and 2048.  Per batch, ms per call of the forward
alone and of forward + backward, median [min-max] over the repeats; the
two variants are timed alternately inside every repeat so drift of a
shared machine hits them alike.  Host clock around 20 calls ending in a
synchronise: launch overhead is part of every figure.  Both variants
include the bn_stats pass over x (one read of S), which the fusion does
not touch.

Also prints the memory each variant must move, from the shape alone
(S = conv output, P = S/4 pooled, idx = u8 argmax plane), and the
achieved TB/s = those bytes / measured time.
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bdbnn_amd import _C

EPS, MOM = 1e-5, 0.1
KS, STRIDE, PAD = 3, 2, 1


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


def byte_counts(N, C=64, H=112, W=112, esize=2):
    """Bytes each pass must move, from the shape alone."""
    S = N * H * W * C * esize
    Ho, Wo = (H + 2 * PAD - KS) // STRIDE + 1, (W + 2 * PAD - KS) // STRIDE + 1
    P = N * Ho * Wo * C * esize
    idx = N * Ho * Wo * C
    stats = S                                    # bn_stats, both variants
    unf_fwd = (2 * S) + (S + P + idx) + P        # bn_act, maxpool, pack
    unf_bwd = (P + idx + S) + 3 * S + (3 * S + S)  # pool bwd, reduce, apply
    fus_fwd = S + P + idx
    fus_bwd = (S + P + idx) + (2 * S + P + idx)
    return dict(S=S, P=P, idx=idx, stats=stats, unf_fwd=unf_fwd,
                unf_bwd=unf_bwd, fus_fwd=fus_fwd, fus_bwd=fus_bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", type=int, nargs="*", default=[256, 2048])
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    nat = _C.native_required()
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    C, H = 64, 112
    for N in args.batch:
        torch.manual_seed(0)
        x = cl((torch.randn(N, C, H, H, device="cuda") * 2)
               .to(torch.bfloat16))
        gamma = torch.rand(C, device="cuda") + 0.5
        beta = torch.randn(C, device="cuda") * 0.3
        rm = torch.zeros(C, device="cuda")
        rv = torch.ones(C, device="cuda")

        def unfused_fwd():
            act, _, mean, invstd = nat.bn_act_fwd_train(
                x, None, gamma, beta, None, rm, rv, MOM, EPS, 2, None, None,
                False)
            out, idx = nat.maxpool_fwd(act, KS, STRIDE, PAD)
            xp, mp = nat.sign_mask_pack_nhwc(out)
            return act, out, idx, mean, invstd

        def fused_fwd():
            return nat.bn_relu_maxpool_fwd_train(
                x, gamma, beta, rm, rv, MOM, EPS, KS, STRIDE, PAD, None,
                None, True)

        act, out, idx, mean, invstd = unfused_fwd()
        dy = cl(torch.randn_like(out))

        def unfused_bwd():
            dact = nat.maxpool_bwd(dy, idx, H, H, KS, STRIDE, PAD)
            return nat.bn_act_bwd(dact, act, x, mean, invstd, gamma, None,
                                  2, False)

        def fused_bwd():
            return nat.bn_relu_maxpool_bwd(dy, idx, x, mean, invstd, gamma,
                                           beta, KS, STRIDE, PAD)

        def both(f, b):
            def run():
                f()
                b()
            return run

        fns = [unfused_fwd, fused_fwd, both(unfused_fwd, unfused_bwd),
               both(fused_fwd, fused_bwd)]
        for fn in fns:
            for _ in range(3):
                fn()
        samples = [[] for _ in fns]
        for _ in range(args.repeats):
            for s, fn in zip(samples, fns):
                s.append(timeit(fn))
        b = byte_counts(N)
        med = [statistics.median(s) for s in samples]
        gb = lambda v: v / 1e9
        rows = [
            ("forward", "unfused", samples[0], b["stats"] + b["unf_fwd"]),
            ("forward", "fused", samples[1], b["stats"] + b["fus_fwd"]),
            ("forward+backward", "unfused", samples[2],
             b["stats"] + b["unf_fwd"] + b["unf_bwd"]),
            ("forward+backward", "fused", samples[3],
             b["stats"] + b["fus_fwd"] + b["fus_bwd"]),
        ]
        print(f"\nbatch {N}, {H}x{H}x{C} bf16: S = {gb(b['S']):.3f} GB, "
              f"P = {gb(b['P']):.3f} GB, idx = {gb(b['idx']):.3f} GB; "
              f"median [min-max] of {args.repeats} repeats x 20 calls\n")
        print("| pass | variant | ms per call | GB moved (shape) | TB/s |")
        print("|---|---|---|---|---|")
        for (what, var, s, nbytes), m in zip(rows, med):
            print(f"| {what} | {var} | {fmt(s)} | {gb(nbytes):.2f} "
                  f"| {nbytes / (m * 1e-3) / 1e12:.2f} |")
        print(f"\nwithout the shared bn_stats read ({gb(b['stats']):.2f} "
              f"GB): unfused {gb(b['unf_fwd'] + b['unf_bwd']):.1f} GB, "
              f"fused {gb(b['fus_fwd'] + b['fus_bwd']):.1f} GB; "
              f"fused/unfused time: forward {med[1] / med[0]:.2f}, "
              f"forward+backward {med[3] / med[2]:.2f}", flush=True)
        del x, act, out, idx, dy


if __name__ == "__main__":
    main()
