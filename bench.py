#!/usr/bin/env python3
"""Flagship benchmark: Qwen2.5-7B serving throughput (output tokens/sec)
with p50 TTFT, sharded PP=N across N MI355X GPUs (BASELINE.json metric).

Single GPU:      python bench.py --steps 3 --warmup 1
Compare builds:  python bench.py --steps 3 --warmup 1 --dump-outputs DIR
Multi GPU (driver): python -m torch.distributed.run --nnodes=1 \
    --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

A "step" is one full serving round: prefill a synthetic batch of prompts
(random token ids, random-init weights — no network for checkpoints) and
decode a fixed number of new tokens per sequence. Weak scaling: the per-GPU
batch is fixed, so the global batch grows with N. Rank 0 prints ONE JSON
line with the aggregate output tokens/sec over the whole job.

A plain run only sets up, warms up, times the steps and prints that line.
--dump-outputs DIR also writes what the last timed step returned to its
caller as DIR/<name>.npy; weights, prompts and greedy decoding are seeded,
so two builds run with the same arguments can be compared array for array.
--full is where any measurement beyond the headline figure belongs (none
today: the TTFT in the result line falls out of the timed steps).
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tensorlink_amd.models.configs import get_config  # noqa: E402
from tensorlink_amd.models.loader import skip_default_init  # noqa: E402
from tensorlink_amd.parallel.comm import init_distributed  # noqa: E402
from tensorlink_amd.parallel.planner import plan_for_world  # noqa: E402
from tensorlink_amd.parallel.pipeline import (  # noqa: E402
    PipelineRunner, SamplingParams)


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--model", default="Qwen/Qwen2.5-7B-Instruct")
    p.add_argument("--batch-per-gpu", type=int, default=256,
                   help="sequences per GPU (weak scaling)")
    p.add_argument("--prompt-len", type=int, default=512)
    p.add_argument("--new-tokens", type=int, default=128)
    p.add_argument("--micro-batches", type=int, default=0,
                   help="decode micro-batches in flight (0 => world size)")
    p.add_argument("--mode", choices=["serve", "train"], default="serve")
    p.add_argument("--dp", type=int, default=1,
                   help="data-parallel replicas (train mode; world=dp*pp)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs as "
                        "DIR/<name>.npy (float64)")
    p.add_argument("--full", action="store_true",
                   help="also run every measurement beyond the headline "
                        "figure (none today)")
    return p.parse_args()


DUMP_LIMIT_BYTES = 60_000_000       # array data; headers stay under 64 MB


def dump_outputs(out_dir, arrays):
    """Write {name: array-like} as out_dir/<name>.npy in float64, at most
    DUMP_LIMIT_BYTES in all: a larger array is cut down to a fixed, seeded
    sample of its flattened elements (same indices every run)."""
    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_LIMIT_BYTES // 8 // max(1, len(arrays))
    for name, a in arrays.items():
        if isinstance(a, torch.Tensor):
            a = a.detach().to("cpu", torch.float64).numpy()
        a = np.asarray(a, dtype=np.float64)
        if a.size > budget:
            idx = np.random.default_rng(0).choice(a.size, budget,
                                                  replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def run_train(args, rank, world, device, use_gpu, config):
    """Training benchmark (BASELINE config #3 shape): 1F1B (+DP) steps,
    metric = training tokens/s."""
    from tensorlink_amd.parallel.dp import HybridTrainer
    B = args.batch_per_gpu * world
    S = args.prompt_len
    trainer = HybridTrainer(config.name if config.name != "custom" else
                            config, rank, world, dp=args.dp, device=device,
                            lr=1e-4)
    torch.manual_seed(17)
    ids = torch.randint(0, config.vocab_size, (B, S)) if rank == 0 else None
    n_micro = max(1, trainer.pp)

    def sync():
        if world > 1:
            torch.distributed.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        trainer.train_step(ids, ids, n_micro=n_micro)
    sync()
    t0 = time.perf_counter()
    losses = [trainer.train_step(ids, ids, n_micro=n_micro)
              for _ in range(args.steps)]
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        e = torch.tensor([elapsed], dtype=torch.float64)
        torch.distributed.all_reduce(e, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(e.item())
    if rank == 0 and args.dump_outputs:
        # train_step hands its caller the step's loss and nothing else
        dump_outputs(args.dump_outputs, {"loss": [losses[-1]]})
    if rank == 0:
        print(json.dumps({
            "metric": "training tokens/sec (1F1B pipeline + fused AdamW)",
            "value": B * S * args.steps / elapsed,
            "unit": "tokens/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if use_gpu else "fp32", "data": "synthetic",
            "loss_first": losses[0], "loss_last": losses[-1],
            "config": {"model": args.model, "global_batch": B,
                       "seq_len": S,
                       "parallelism": f"dp{args.dp}xpp{world // args.dp}"},
        }))


def main():
    args = parse_args()
    rank, world = init_distributed()
    if world != args.gpus and "WORLD_SIZE" in os.environ:
        args.gpus = world
    assert world == args.gpus or world == 1, \
        f"launched world={world} but --gpus={args.gpus}"
    world = max(world, 1)

    use_gpu = torch.cuda.is_available()
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", rank))) \
        if use_gpu else torch.device("cpu")
    if use_gpu:
        torch.cuda.set_device(device)

    from tensorlink_amd.utils.tunable import setup_tunableop
    setup_tunableop(tune=bool(os.environ.get("TL_TUNE")))

    config = get_config(args.model)
    if args.mode == "train":
        run_train(args, rank, world, device, use_gpu, config)
        return

    B = args.batch_per_gpu * world          # weak scaling: global batch
    S, T = args.prompt_len, args.new_tokens
    plan = plan_for_world(config, world, batch_size=B, seq_len=S + T)
    # the seeded random init below overwrites every weight, and the host
    # RNG is re-seeded before the prompts are drawn: skip torch's default
    # init, which costs most of a minute of host time on the 7B model
    with skip_default_init():
        runner = PipelineRunner(plan, rank, world, device=device,
                                init="random", seed=1234)

    torch.manual_seed(17)
    input_ids = torch.randint(0, config.vocab_size, (B, S)) \
        if rank == 0 else None
    sp = SamplingParams(temperature=0.0, max_new_tokens=T)
    # serving default: 4 prefill micro-batches — requests in chunk m see
    # their first token after m+1 chunks: TTFT p50 drops 1.37s -> 0.88s
    # for ~1.4% throughput (measured; 8 chunks cost ~7% in host-side
    # dispatch for only marginal TTFT gain)
    n_mb = args.micro_batches or (4 if world == 1 else world)

    def sync():
        if world > 1:
            torch.distributed.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        runner.generate(input_ids, sp, micro_batches=n_mb)

    ttfts = []
    out = None
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out, stats = runner.generate(input_ids, sp, micro_batches=n_mb,
                                     return_stats=True)
        if rank == 0:
            print(f"[step] {stats}", file=sys.stderr)
        tt = stats.get("ttft_p50_s", stats.get("ttft_s"))
        if tt is not None:
            ttfts.append(tt)
    sync()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    # MAX over ranks (ranks are barrier-synced; take max to be safe)
    if world > 1:
        e = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if use_gpu else "cpu")
        torch.distributed.all_reduce(e, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(e.item())

    total_tokens = B * T * args.steps
    tps = total_tokens / elapsed
    ms_per_step = elapsed / args.steps * 1000.0
    ttft_p50 = statistics.median(ttfts) if ttfts else None

    if os.environ.get("TL_TUNE") and rank == 0:
        from tensorlink_amd.utils.tunable import save_tunableop
        save_tunableop()

    if os.environ.get("TL_TRACE"):          # per-rank Chrome trace export
        from tensorlink_amd.utils.tracing import export_from_env
        export_from_env(runner.tracer)

    if rank == 0 and args.dump_outputs:
        # generate() returns the new token ids [B, T] on rank 0
        dump_outputs(args.dump_outputs, {"tokens": out})

    if rank == 0:
        print(json.dumps({
            "metric": "output tokens/sec (Qwen2.5-7B serving, PP sharded)",
            "value": tps,
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if use_gpu else "fp32",
            "data": "synthetic",
            "ttft_p50_s": ttft_p50,
            "config": {
                "model": args.model,
                "global_batch": B,
                "seq_len": S,
                "new_tokens": T,
                "parallelism": f"pp{world}",
                "micro_batches": n_mb,
            },
        }))


if __name__ == "__main__":
    main()
