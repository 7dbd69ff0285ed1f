"""Driver benchmark contract (see BASELINE.json / BASELINE.md).

Headline config: ResNet-18 / CIFAR-10-shaped synthetic data, repetition code r=3 with
s=1 rev_grad adversary, colocated topology on N GPUs (weak scaling: each GPU computes
r=3 group batches of 128 images per step; N groups total, so the DISTINCT trained
images per step = N*128 — redundant compute is the cost of the code and is not
counted in the throughput metric).

Launched by the driver as
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W
(single process, no torchrun, for N=1).  Rank 0 prints ONE JSON line.

A plain run does only what the headline figure needs: set up, warm up, time exactly
K steps, print the line.  `--full` adds the measurements that take runs of their
own: the plain-DP reference arm (`vs_baseline`, `baseline_images_per_sec`) and one
post-bracket step with loss readback (`final_loss`); without it those keys are null.
`--dump-outputs DIR` writes what the last timed step computed (the updated flat
parameters) as DIR/params.npy for build-to-build comparison; that step then starts
from the seeded start state, so that its inputs are the same in every run (see
StartState, dump_outputs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# Cross-rank kernel determinism: repetition-vote group members live on DIFFERENT
# ranks, so every rank must run the SAME conv/compiled kernels or replica gradients
# diverge systematically (beyond fp-reorder noise).  FAST find picks MIOpen algos
# from the heuristic (deterministic across ranks; measured perf-neutral vs full
# find), and a shared inductor cache makes all ranks reuse identical compiled
# kernels.  Must be set before torch/MIOpen initialise.
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
os.environ.setdefault("TORCHINDUCTOR_CACHE_DIR", "/tmp/draco_inductor_cache")

import torch

DUMP_BUDGET_BYTES = 60 * 2**20  # stays under the 64 MB cap incl. .npy headers


def _optimizer_state(tr):
    return {name: getattr(tr.opt, name)
            for name in ("buf", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")
            if isinstance(getattr(tr.opt, name, None), torch.Tensor)}


class StartState:
    """Seeded start state (flat parameters + optimizer state) for --dump-outputs.

    Training is chaotic and GPU conv backward is not bitwise reproducible (see
    VoteAggregator): measured on ResNet-18, a 1e-6 relative parameter perturbation
    moves the NEXT step's gradient by ~5%, so after a few steps two runs of one
    build hold unrelated gradients and nothing could be compared output for output.
    With --dump-outputs the LAST timed step therefore starts from this snapshot
    (two in-place device copies inside the bracket, once per run, ~0.1 ms): its
    inputs — state, batch and adversary of step warmup+steps-1 — are then identical
    from run to run, and its outputs differ only by that one step's fp-reorder
    noise.  restore() puts the trained state back (minus the rewound step's update)
    so post-bracket telemetry still sees a trained model."""

    def __init__(self, tr):
        self.live = [tr.space.flat_param, *_optimizer_state(tr).values()]
        self.start = [t.clone() for t in self.live]
        self.trained = None

    def _load(self, src):
        with torch.no_grad():
            for dst, s in zip(self.live, src):
                dst.copy_(s)

    def rewind(self):
        self.trained = [t.clone() for t in self.live]
        self._load(self.start)

    def restore(self):
        if self.trained is not None:
            self._load(self.trained)


def dump_outputs(tr, out_dir):
    """Write what a caller of the last train_step() holds afterwards — the updated
    flat parameters — as float32 DIR/params.npy.  The step started from StartState
    (zero optimizer buffers), so params = start - lr * update(decoded gradient):
    the decoded gradient is in the dump at lr/|param| resolution (float32 keeps
    ~5 of its digits at lr=0.01), while one bf16 step's own run-to-run noise
    (MIOpen fwd+bwd: 0.6-1% of the gradient norm on identical inputs, 0.1% in
    fp32) lands at ~5e-6 of the parameter norm.  The gradient and the optimizer
    buffer themselves are NOT dumped: after the rewound step both are that same
    gradient again, carrying that noise at full size.  An array over the byte
    budget is written as a fixed seeded sample (sorted indices of randperm(d),
    seed 0), so two builds run with the same arguments dump the same elements."""
    import numpy as np

    d = tr.space.d  # drop the shard-alignment padding
    arrays = {"params": tr.space.flat_param}
    share = DUMP_BUDGET_BYTES // 4 // len(arrays)
    idx = None
    if d > share:
        g = torch.Generator().manual_seed(0)
        idx = torch.randperm(d, generator=g)[:share].sort().values
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = a.detach()[:d]
        if idx is not None:
            a = a[idx.to(a.device)]  # gather on device: only the sample crosses
        a = a.to(device="cpu", dtype=torch.float32)
        np.save(os.path.join(out_dir, f"{name}.npy"), a.contiguous().numpy())


def main():
    # The driver parses EXACTLY ONE JSON line from stdout.  Native libraries chat on
    # fd 1 (e.g. LAPACK XERBLA "** On entry to ZLASCL ..."), so redirect fd 1 to
    # stderr for the whole run and restore it only for the final JSON print.
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    sys.stdout = os.fdopen(os.dup(2), "w")

    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch-size", type=int, default=128)
    p.add_argument("--network", type=str, default="ResNet18")
    p.add_argument("--dataset", type=str, default="Cifar10")
    p.add_argument("--approach", type=str, default="maj_vote")
    p.add_argument("--mode", type=str, default="maj_vote")
    p.add_argument("--group-size", type=int, default=3)
    p.add_argument("--worker-fail", type=int, default=1)
    p.add_argument("--err-mode", type=str, default="rev_grad")
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--vote-granularity", type=str, default="row")
    p.add_argument("--dtype", type=str, default="bf16")
    p.add_argument("--device", type=str, default="auto")
    p.add_argument("--channels-last", type=lambda v: v.lower() in ("1","true"), default=True)
    p.add_argument("--hip-graphs", type=lambda v: v.lower() in ("1","true"), default=True)
    # OFF by default: torch.compile's GPU codegen (inductor) is Triton-backed, and
    # this build's ground rule is hand-written HIP/CDNA4 + PyTorch-ROCm kernels only
    # (BASELINE.json north star: "no Triton").  The flag documents the measured +27%
    # for anyone who wants it.
    p.add_argument("--compile", type=lambda v: v.lower() in ("1","true"), default=False)
    p.add_argument("--full", action="store_true",
                   help="also run the plain-DP reference arm (vs_baseline) and the "
                        "post-bracket loss-readback step (final_loss)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps write the last step's updated parameters "
                        "as DIR/params.npy (float32, <= 64 MB)")
    args = p.parse_args()

    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")

    cfg = Config(
        network=args.network,
        dataset=args.dataset,
        batch_size=args.batch_size,
        approach=args.approach,
        mode=args.mode,
        group_size=args.group_size,
        worker_fail=args.worker_fail,
        err_mode=args.err_mode,
        lr=args.lr,
        vote_granularity=args.vote_granularity,
        dtype=args.dtype,
        device=args.device,
        max_steps=args.steps + args.warmup + 10,
        eval_freq=0,
        log_dir="",
        train_dir="output/bench_ckpt",
        topology="colocated",
        channels_last=args.channels_last,
        hip_graphs=args.hip_graphs,
        compile=args.compile,
    )
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    t.logger.close()
    on_gpu = t.device.type == "cuda"

    def timed_region(tr, steps, warmup, start_state=None):
        """warmup untimed, then EXACTLY `steps` steps bracketed by barrier+sync on
        both sides; returns MAX elapsed over ranks (slowest rank defines the job).
        With a start_state the last step runs from it (see StartState)."""
        for _ in range(warmup):
            tr.train_step()
        # inside the timed region: no per-step host sync, no per-step loss readback
        # (the bracket barriers + synchronizes; every step's work still runs fully)
        tr.step_sync = False
        tr.collect_loss = False
        tr.comm.barrier()
        if on_gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            if start_state is not None and i == steps - 1:
                start_state.rewind()
            tr.train_step()
        if on_gpu:
            torch.cuda.synchronize()
        tr.comm.barrier()
        if on_gpu:
            torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        tr.step_sync = True
        tr.collect_loss = True
        el = torch.tensor([elapsed], dtype=torch.float64)
        if tr.comm.distributed:
            el_dev = el.to(tr.device) if tr.comm.backend == "nccl" else el
            tr.comm.all_reduce(el_dev, op="max")
            elapsed = float(el_dev[0])
        return elapsed

    start_state = StartState(t) if args.dump_outputs else None
    elapsed = timed_region(t, args.steps, args.warmup, start_state)
    if start_state is not None:
        if rank == 0:
            dump_outputs(t, args.dump_outputs)
        start_state.restore()

    # post-bracket honesty telemetry (--full): one more step with loss readback
    final_loss = t.train_step()["loss"] if args.full else None
    ms_per_step = elapsed / args.steps * 1000.0

    # DISTINCT images per step (redundant compute is the price of the code and is
    # not counted): maj_vote -> G*B (G=world groups); cyclic -> n*B global batch;
    # baseline -> world*B
    if args.approach == "cyclic":
        distinct_per_step = t.n * args.batch_size
        # actually computed per step: each rank computes its DISTINCT local
        # sub-batches once (band overlap between same-rank logical workers deduped)
        processed = world * len(t._local_subs) * args.batch_size
    elif args.approach == "maj_vote":
        distinct_per_step = world * args.batch_size
        processed = world * args.group_size * args.batch_size
    else:
        distinct_per_step = world * args.batch_size
        processed = distinct_per_step

    # ---- plain-DP reference arm (--full only): same model/world, approach=baseline
    # mode=normal, NO adversary, processing the SAME distinct images per step as the
    # coded arm (cyclic trains an n*B global batch, so the fair plain-DP rank batch is
    # distinct/world) — vs_baseline = coded ÷ plain throughput at equal work.
    # (The reference repo publishes no numbers, BASELINE.md, so the plain arm is
    # the denominator.)
    vs_baseline = None
    baseline_ips = None
    if args.full and args.approach != "baseline":
        import dataclasses

        bcfg = dataclasses.replace(
            cfg, approach="baseline", mode="normal", worker_fail=0, err_mode="none",
            batch_size=max(distinct_per_step // world, 1),
            train_dir="output/bench_ckpt_base")
        tb = Trainer(bcfg)
        tb.logger.stdout_every = 0
        tb.logger.close()
        bsteps = max(min(args.steps, 10), 1)
        belapsed = timed_region(tb, bsteps, min(args.warmup, 3))
        baseline_ips = distinct_per_step * bsteps / belapsed
        tb.close()
    images_per_sec = distinct_per_step * args.steps / elapsed
    if baseline_ips is not None:
        vs_baseline = round(images_per_sec / baseline_ips, 4)

    # restore the real stdout for the contract line
    sys.stdout.flush()
    os.dup2(real_stdout, 1)
    sys.stdout = os.fdopen(real_stdout, "w")
    if rank == 0:
        result = {
            "metric": (f"images/sec (effective), {args.network} {args.dataset}, "
                       f"{args.approach} r={args.group_size if args.approach == 'maj_vote' else 2 * args.worker_fail + 1}, "
                       f"s={args.worker_fail} adversary"),
            "value": round(images_per_sec, 2),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            # coded throughput ÷ plain-DP (baseline normal, no adversary) on the
            # same box — the reference publishes no absolute numbers
            "vs_baseline": vs_baseline,
            "baseline_images_per_sec": round(baseline_ips, 2) if baseline_ips else None,
            "final_loss": (round(final_loss, 4)
                           if final_loss is not None and final_loss == final_loss else None),
            "skipped_updates": t.skipped_updates,
            "vote_degenerate_steps": getattr(t.agg, "degenerate_steps", None),
            "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 3) if on_gpu else None,
            "dtype": args.dtype if on_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.network,
                "global_batch": distinct_per_step,
                "images_processed_per_step": processed,
                "seq_len": None,
                "input": "3x32x32" if args.dataset == "Cifar10" else args.dataset,
                "parallelism": (
                    f"coded-dp{world}("
                    + (f"repetition r={args.group_size}" if args.approach == "maj_vote"
                       else f"cyclic r={2 * args.worker_fail + 1}" if args.approach == "cyclic"
                       else f"baseline {args.mode}")
                    + f", s={args.worker_fail}, {args.err_mode})"
                ),
                "topology": "colocated",
                "optimizer": "fused SGD momentum=0.5",
            },
        }
        print(json.dumps(result), flush=True)
    t.close()
    if t.comm.distributed:
        t.comm.shutdown()


if __name__ == "__main__":
    main()
