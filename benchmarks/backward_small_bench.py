#!/usr/bin/env python3
"""Backward cost of the 16/32-channel stride-1 binary convs of CIFAR
ResNet-20 (C = K = 16 at 32x32, C = K = 32 at 16x16): the owned kernels of
csrc/conv_bwd_small.hip vs the same build with BDBNN_MFMA_BWD_SMALL=0, which
runs exactly the previous backward (decode_packed / binsign_decode + weight
decode + MIOpen dgrad and wrw + separate mask passes).

  python benchmarks/backward_small_bench.py layers [batch] [repeats]
  python benchmarks/backward_small_bench.py e2e [runs] [steps] [warmup]
  python benchmarks/backward_small_bench.py step [steps] [warmup]

layers: one row per (class, mask).  ms per backward call of
BinaryConvFunction (dx AND dw), median [min-max] over the repeats; host
clock around 20 calls ending in a synchronise, so launch overhead is part
of every figure; both paths alternate inside every repeat of one process.
The ship rule of the project: a class is routed to the owned kernels only
if owned's WHOLE range lies below the fallback's whole range in both mask
modes.  Below the table the two new kernels alone, with bytes moved / time
(g + saved x or mask plane + dx for dgrad; g + sign plane + slabs for
wgrad): at a few MB per call launch overhead is a large share, so these
are informative only.

step: one process, a ResNet-20 training step (batch 256, 32x32, bf16
autocast, kurtosis on, EDE injected, pre-staged device batches); prints
one JSON line with images/s.  e2e: runs `step` in fresh processes with the
knob on and off alternately and prints each run, medians and ranges.
"""

import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = [(16, 32, 16), (32, 16, 32)]                  # C, H = W, K
MASKS = [("ste", "ste", None, None), ("ede", "ste", 1.0, 1.0)]


def timeit(fn, iters=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def fmt(samples, digits=3):
    return (f"{statistics.median(samples):.{digits}f} "
            f"[{min(samples):.{digits}f}-{max(samples):.{digits}f}]")


def layers(N, reps):
    from bdbnn_amd import _C
    from bdbnn_amd.ops import binary_conv as bc
    from bdbnn_amd.ops.binary_conv import BinaryConvFunction
    nat = _C.native_required()
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    assert bc._MFMA_BWD, "run with BDBNN_MFMA_BWD unset"
    print(f"batch {N}; ms per backward call (dx + dw), median [min-max] of "
          f"{reps} repeats x 20 calls\n")
    print("| conv | mask | owned | fallback | owned/fallback | ranges |")
    print("|---|---|---|---|---|---|")
    verdict = {}
    for (C, H, K) in CLASSES:
        for name, act, t, k in MASKS:
            torch.manual_seed(0)
            x = cl(torch.randn(N, C, H, H, device="cuda",
                               dtype=torch.bfloat16)).requires_grad_(True)
            w = torch.randn(K, C, 3, 3, device="cuda").requires_grad_(True)
            out, _, _ = BinaryConvFunction.apply(x, w, 1, 1, act, t, k, False)
            gout = cl(torch.randn_like(out))

            def backward(flag):
                def run():
                    bc._MFMA_BWD_SMALL = flag
                    return torch.autograd.grad(out, (x, w), gout,
                                               retain_graph=True)
                return run

            fns = (backward(True), backward(False))
            for fn in fns:          # warm-up: code objects, MIOpen find
                for _ in range(3):
                    fn()
            samples = [[], []]
            for _ in range(reps):
                for s, fn in zip(samples, fns):
                    s.append(timeit(fn))
            below = max(samples[0]) < min(samples[1])
            verdict[(C, K)] = verdict.get((C, K), True) and below
            a, b = (statistics.median(s) for s in samples)
            print(f"| {C}x{H}x{H}->{K} | {name} | {fmt(samples[0])} "
                  f"| {fmt(samples[1])} | {a / b:.2f} "
                  f"| {'owned below' if below else 'TOUCH'} |", flush=True)
            del out, gout, x, w
    for (C, K), ok in verdict.items():
        print(f"\nclass C={C} K={K}: "
              + ("ship (owned below the fallback in both modes)" if ok
                 else "keep on the fallback (ranges touch)"))

    print(f"\nkernels alone, us per call, median [min-max] of {reps} x 20; "
          "GB/s = bytes moved / median\n")
    print("| conv | kernel | us | MB | GB/s |")
    print("|---|---|---|---|---|")
    for (C, H, K) in CLASSES:
        torch.manual_seed(0)
        x = cl(torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16))
        g = cl(torch.randn(N, K, H, H, device="cuda", dtype=torch.bfloat16))
        w = torch.randn(K, C, 3, 3, device="cuda")
        xp, mp = nat.sign_mask_pack_nhwc(x)
        wp, alpha, _ = nat.weight_pack(w)
        wd = nat.dgrad_weight_decode(wp, alpha, C)
        px = N * H * H
        nslab = nat.conv_wgrad_small(g, xp, C, fold=False).shape[0]
        rows = [
            ("dgrad mode 0",
             lambda: nat.conv_dgrad_small(g, wd, C, 0, mp, None, 0.0, 0.0),
             px * (2 * K + 4 + 2 * C)),
            ("dgrad mode 2",
             lambda: nat.conv_dgrad_small(g, wd, C, 2, None, x, 1.0, 1.0),
             px * (2 * K + 4 * C)),
            (f"wgrad ({nslab} slabs)",
             lambda: nat.conv_wgrad_small(g, xp, C, fold=False),
             px * (2 * K + 4) + nslab * 36 * C * K),
            ("wgrad + slab fold",
             lambda: nat.conv_wgrad_small(g, xp, C),
             px * (2 * K + 4) + (2 * nslab + 1) * 36 * C * K),
        ]
        for label, fn, nbytes in rows:
            for _ in range(3):
                fn()
            s = [timeit(fn) * 1e3 for _ in range(reps)]
            med = statistics.median(s)
            print(f"| {C}x{H}x{H}->{K} | {label} | {fmt(s, 1)} "
                  f"| {nbytes / 1e6:.2f} | {nbytes / med / 1e3:.0f} |",
                  flush=True)


def step(steps, warmup, batch=256):
    """one process: a ResNet-20 recipe step, images/s as one JSON line"""
    from bdbnn_amd.engine import Trainer
    from bdbnn_amd.engine.trainer import ede_inject
    from bdbnn_amd.models import cifar10
    from bdbnn_amd.ops import binary_conv as bc

    class TArgs:    # scripts/train_cifar10_bdbnn.sh: -a resnet20 --ede --amp
        arch = "resnet20"
        dataset = "cifar10"
        lr = 1e-3
        momentum = 0.9
        weight_decay = 1e-4
        epochs = 200
        w_kurtosis = True
        weight_name = ["all"]
        remove_weight_name = None
        w_kurtosis_target = 1.8
        w_lambda_kurtosis = 1.0
        kurtosis_mode = "avg"
        diffkurt = False
        kurtepoch = 0
        react = False
        alpha = 0.9
        beta = 200.0
        w_lambda_ce = 1.0
        amp = True
        print_freq = 10 ** 9
        ede = True
        start_epoch = 0

    torch.manual_seed(1234)
    device = torch.device("cuda:0")
    trainer = Trainer(cifar10.resnet20(), TArgs, device=device)
    ede_inject(trainer.model, 10, TArgs.epochs)
    batches = []
    for _ in range(4):
        x = torch.randn(batch, 3, 32, 32, device=device).contiguous(
            memory_format=torch.channels_last)
        batches.append((x, torch.randint(0, 10, (batch,), device=device)))
    trainer.model.train()

    def one(i):
        x, y = batches[i % 4]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            total, _, _, _ = trainer._step_losses(x, y, 0)
        trainer.optimizer.zero_grad(set_to_none=True)
        total.backward()
        trainer.model.finish_gradient_sync()
        trainer.optimizer.step()

    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(i)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    print(json.dumps({"metric": "resnet20_train_images_per_sec",
                      "value": round(batch * steps / el, 1),
                      "ms_per_step": round(el / steps * 1e3, 3),
                      "bwd_small": bool(bc._MFMA_BWD_SMALL),
                      "batch": batch, "steps": steps, "warmup": warmup}))


def e2e(runs, steps, warmup):
    vals = {"1": [], "0": []}
    for r in range(runs):
        for knob in ("1", "0"):
            env = dict(os.environ, BDBNN_MFMA_BWD_SMALL=knob)
            out = subprocess.run(
                [sys.executable, os.path.abspath(__file__), "step",
                 str(steps), str(warmup)],
                env=env, check=True, capture_output=True, text=True,
                timeout=300).stdout.strip().splitlines()[-1]
            vals[knob].append(json.loads(out)["value"])
            print(f"run {r} knob {knob}: {out}", flush=True)
    on, off = vals["1"], vals["0"]
    print(f"\nResNet-20 step, images/s, median [min-max] of {runs} runs x "
          f"{steps} steps")
    print(f"knob on : {fmt(on, 0)}")
    print(f"knob off: {fmt(off, 0)}")
    print("ranges " + ("do not touch" if min(on) > max(off) or
                       min(off) > max(on) else "touch")
          + f"; on/off medians {statistics.median(on) / statistics.median(off):.3f}")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "layers"
    a = [int(v) for v in sys.argv[2:]]
    if what == "layers":
        layers(*(a + [256, 7][len(a):]))
    elif what == "step":
        step(*(a + [50, 15][len(a):]))
    elif what == "e2e":
        e2e(*(a + [6, 50, 15][len(a):]))
    else:
        sys.exit(__doc__)
