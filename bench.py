#!/usr/bin/env python3
"""Flagship benchmark: BD-BNN ResNet-18 training step on ImageNet-shaped
synthetic data (BASELINE.json metric: train images/sec, node aggregate).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]
    # N>1: launched by the driver as torch.distributed.run, one rank/GPU
    # over RCCL; reads RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the env.

The timed step is the full training step of the BD-BNN method on the
named config: binary-conv forward (XNOR kernel), CE + kurtosis losses,
backward (dense MFMA convs + fused mask/kurtosis kernels), bucketed
gradient all-reduce, fused optimizer step.  --ts adds the fp32-teacher
KD path (BASELINE config 3).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the result
line; nothing else is measured.  --dump-outputs DIR additionally writes
results of the run as it happened as DIR/<name>.npy (float32): for
training the last timed step's losses and whole-model aggregates (see
_train_step_summary), for --infer the logits.
The seed fixes weights and inputs, so two runs or two builds get the
same inputs and can be compared output for output.
--full is reserved for secondary measurements; the benchmark has none
today, so it changes nothing.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch-size", type=int, default=2048,
                   help="per-GPU batch size")
    p.add_argument("--arch", default="resnet18")
    p.add_argument("--ts", action="store_true",
                   help="teacher-student KD path (BASELINE config 3)")
    p.add_argument("--infer", action="store_true",
                   help="binary inference path: packed weights + hipGraph "
                        "(BASELINE config 5, throughput-only)")
    p.add_argument("--no-kurt", action="store_true")
    p.add_argument("--diffkurt", action="store_true",
                   help="per-layer kurtosis target lists (BASELINE config 4)")
    p.add_argument("--image", type=int, default=224)
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last step's "
                        "outputs to DIR/<name>.npy (float32)")
    p.add_argument("--full", action="store_true",
                   help="also run secondary measurements (none today: the "
                        "plain run already does only the headline figure)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")
    return args


# --dump-outputs budget: 64 MB in all, 16 MB (4M float32) per array
_DUMP_MAX_ELEMS = 4 * 1024 * 1024
_DUMP_MAX_BYTES = 64 * 1024 * 1024


def _dump_outputs(out_dir, arrays):
    """Write {name: tensor} as out_dir/name.npy in float32.  An array over
    the per-array cap is replaced by a fixed sample of its flattened
    elements: evenly spaced indices, the same on every run and build."""
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        shape = tuple(t.shape)
        if flat.numel() > _DUMP_MAX_ELEMS:
            idx = torch.linspace(0, flat.numel() - 1, _DUMP_MAX_ELEMS,
                                 dtype=torch.float64).round().long()
            flat = flat[idx.to(flat.device)]
            shape = (_DUMP_MAX_ELEMS,)
        a = flat.float().cpu().numpy().reshape(shape)
        total += a.nbytes
        if total > _DUMP_MAX_BYTES:
            raise ValueError(f"--dump-outputs: more than "
                             f"{_DUMP_MAX_BYTES >> 20} MB of outputs")
        np.save(os.path.join(out_dir, name + ".npy"), a)


def _train_step_summary(last, params, seeded):
    """What --dump-outputs writes for the training path.  Everything is
    taken from the run as it happened; no state is rewound.

    The kernels sum BN statistics and weight gradients with fp32 atomics,
    and every sign() layer multiplies that last-bit noise.  After W+N
    steps single logits differ by ~0.5 between two runs of one build, and
    even per-tensor gradient or update norms by up to 35 % (measured,
    docs/TUNING.md), so neither can tell two builds apart.  Whole-batch
    and whole-model aggregates repeat to within 2e-3 (bf16 eps is 7.8e-3)
    and still depend on every kernel of the step:

      loss, ce     last timed step's losses: forward of weights that W+N-1
                   steps of backward, all-reduce and optimizer produced
      kurt         its kurtosis loss, a function of those weights alone
                   (1.43 at the seeded weights, 0.46 after 25 steps)
      logits_std   std of the last step's logits
      update_norm  L2 norm of (all weights now - seeded weights)
    """
    total, ce, kurt, out = last
    with torch.no_grad():
        arrays = {
            "loss": total, "ce": ce,
            "logits_std": out.float().std(),
            "update_norm": torch.stack(
                [(p.detach().float() - s.float()).norm()
                 for p, s in zip(params, seeded)]).norm(),
        }
        if kurt is not None:
            arrays["kurt"] = kurt.detach()
    return arrays


def _seed_miopen_find_db(want=None):
    """Merge the recorded MIOpen find results for the flagship shapes
    (benchmarks/miopen_find_db/*.ufdb.txt) into the user find-db.

    The few convolutions still on MIOpen (stride-2 binary-conv backward,
    1x1 downsample backward, stem weight gradient) otherwise trigger a
    find on the first backward of a fresh account: every applicable solver
    is compiled and timed, ~150 s at b2048, for the same choices that are
    recorded here.  Entries the user already has win; other MIOpen
    versions use another file name and ignore this one, so a warning
    says when no recorded file name starts with ``want``, the prefix MIOpen
    uses on this device: <arch><CUs in hex>.HIP.<major>_<minor>_<patch>_"""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "benchmarks", "miopen_find_db")
    dst = os.path.expanduser(os.environ.get(
        "MIOPEN_USER_DB_PATH", os.path.join("~", ".config", "miopen")))
    try:
        names = [n for n in os.listdir(src) if n.endswith(".ufdb.txt")]
        if want and not any(n.startswith(want) for n in names):
            print(f"bench: no recorded MIOpen find-db for {want}* under "
                  f"{src}; the first backward will run MIOpen's find "
                  "(minutes on an empty find-db) - re-record it, see "
                  "docs/TUNING.md", file=sys.stderr)
        os.makedirs(dst, exist_ok=True)
        for name in names:
            with open(os.path.join(src, name)) as f:
                recorded = [l for l in f.read().splitlines() if "=" in l]
            path = os.path.join(dst, name)
            old = ""
            if os.path.exists(path):
                with open(path) as f:
                    old = f.read()
            have = {l.split("=", 1)[0] for l in old.splitlines() if "=" in l}
            new = [l for l in recorded if l.split("=", 1)[0] not in have]
            if new:
                with open(path, "a") as f:
                    if old and not old.endswith("\n"):
                        f.write("\n")
                    f.write("".join(l + "\n" for l in new))
    except OSError:
        pass  # read-only home: MIOpen falls back to finding by itself


def main():
    args = parse_args()
    import bdbnn_amd  # noqa: F401
    from bdbnn_amd.engine import Trainer
    from bdbnn_amd.models import imagenet as im
    from bdbnn_amd.parallel import init_distributed

    rank, local_rank, world_size = init_distributed()
    shared_db = world_size > 1 and "MIOPEN_USER_DB_PATH" in os.environ
    if world_size > 1:
        # per-rank MIOpen find db: concurrent ranks otherwise serialize on
        # the shared user-db file lock during warmup
        os.environ.setdefault("MIOPEN_USER_DB_PATH",
                              f"/tmp/miopen-rank{local_rank}")
    use_cuda = torch.cuda.is_available()
    device = torch.device(f"cuda:{local_rank}") if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)
        # one writer per find-db directory: with a directory the user
        # shares between ranks, only local rank 0 merges
        if not shared_db or local_rank == 0:
            pr = torch.cuda.get_device_properties(device)
            v = torch.backends.cudnn.version() or 0  # MIOpen's, on ROCm
            _seed_miopen_find_db(
                f"{pr.gcnArchName.split(':')[0]}"
                f"{pr.multi_processor_count:x}.HIP."
                f"{v // 1000000}_{v // 1000 % 1000}_{v % 1000}_")

    torch.manual_seed(1234 + rank)

    if not use_cuda and args.batch_size >= 512:
        # CPU-only machine (no-flag contract: must finish in minutes)
        args.batch_size = 16
        args.image = min(args.image, 64)

    class TArgs:  # minimal trainer config (mirrors train.py flags)
        arch = args.arch
        dataset = "imagenet"
        lr = 1e-3
        momentum = 0.9
        weight_decay = 1e-4
        epochs = 90
        w_kurtosis = not args.no_kurt
        weight_name = ["all"]
        remove_weight_name = None
        w_kurtosis_target = 1.8
        w_lambda_kurtosis = 1.0
        kurtosis_mode = "avg"
        diffkurt = args.diffkurt
        kurtepoch = 0
        react = False
        alpha = 0.9
        beta = 200.0
        w_lambda_ce = 1.0
        amp = use_cuda
        print_freq = 10**9
        ede = False
        start_epoch = 0

    model = im.__dict__[args.arch](False)

    if args.infer:
        from bdbnn_amd.engine import PackedInference
        assert use_cuda, "--infer needs a GPU"
        eng = PackedInference(model).capture(
            (args.batch_size, 3, args.image, args.image))
        x = torch.randn(args.batch_size, 3, args.image, args.image,
                        device=device)
        for _ in range(args.warmup):
            eng(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y = eng(x)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if args.dump_outputs:
            _dump_outputs(args.dump_outputs, {"logits": y})
        print(json.dumps({
            "metric": "infer_images_per_sec",
            "value": round(args.batch_size * args.steps / elapsed, 2),
            "unit": "images/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000.0, 3),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"model": f"{args.arch}_bdbnn_infer",
                       "global_batch": args.batch_size,
                       "image": f"3x{args.image}x{args.image}",
                       "parallelism": "dp1", "hipgraph": True}}))
        return

    teacher = im.__dict__[args.arch + "_real"](False) if args.ts else None
    trainer = Trainer(model, TArgs, teacher=teacher, device=device,
                      world_size=world_size, rank=rank)

    # synthetic ImageNet-shaped data, random-init weights (no datasets in
    # this offline image); a few fixed batches resident on device
    n_batches = 4
    batches = []
    for i in range(n_batches):
        x = torch.randn(args.batch_size, 3, args.image, args.image,
                        device=device)
        if use_cuda:
            x = x.contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 1000, (args.batch_size,), device=device)
        batches.append((x, y))

    trainer.model.train()

    # --dump-outputs: the seeded weights, kept to measure after the timing
    # how far warm-up and timed steps moved them
    params = list(trainer.model.parameters())
    seeded = ([p.detach().clone() for p in params]
              if args.dump_outputs else None)

    def step(i, keep=False):
        x, y = batches[i % n_batches]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=TArgs.amp):
            total, ce, kurt, out = (
                trainer._step_losses_ts(x, y, 0) if args.ts
                else trainer._step_losses(x, y, 0))
        trainer.optimizer.zero_grad(set_to_none=True)
        total.backward()
        trainer.model.finish_gradient_sync()
        trainer.optimizer.step()
        if keep:
            # what a caller of the step receives, detached from the graph
            return total.detach(), ce.detach(), kurt, out.detach()
        return total

    for i in range(args.warmup):
        step(i)

    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = step(i, keep=(args.dump_outputs is not None
                             and i == args.steps - 1))
    if use_cuda:
        torch.cuda.synchronize()
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if dist.is_available() and dist.is_initialized():
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if use_cuda else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    n = world_size if world_size > 1 else args.gpus
    images_per_sec = args.batch_size * n * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0 and args.dump_outputs:
        _dump_outputs(args.dump_outputs,
                      _train_step_summary(last, params, seeded))

    if rank == 0:
        result = {
            "metric": "train_images_per_sec",
            "value": round(images_per_sec, 2),
            "unit": "images/s",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if use_cuda else "fp32",
            "data": "synthetic",
            "config": {
                "model": f"{args.arch}_bdbnn" + ("_ts" if args.ts else ""),
                "global_batch": args.batch_size * n,
                "image": f"3x{args.image}x{args.image}",
                "kurtosis": not args.no_kurt,
                "parallelism": f"dp{n}",
            },
        }
        print(json.dumps(result))


if __name__ == "__main__":
    main()
