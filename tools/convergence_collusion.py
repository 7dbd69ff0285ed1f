"""Every baseline rule against the per-worker rev_grad adversary and the colluding
ALIE / inner-product adversaries, on CPU through the trainer: LeNet on synthetic MNIST,
P=7 logical workers in one process, f=1, 40 steps; the cell is the mean of the last five
training losses.  Prints the markdown table of profiles/convergence_collusion.md and,
since the centered_clip column (auto radius, 3 iterations) was added, of
profiles/convergence_centered_clip.md.

  python tools/convergence_collusion.py > profiles/convergence_centered_clip.md

With --worker-momentum BETA every worker sends its momentum instead of its gradient
(Config.worker_momentum, with the server's --momentum set to 0 as that flag requires):
the table of profiles/convergence_worker_momentum.md.
"""
import argparse
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from draco_amd.config import Config
from draco_amd.parallel import Trainer

MODES = ("normal", "median", "trimmed_mean", "meamed", "phocas", "krum", "multi_krum",
         "bulyan", "geometric_median", "centered_clip")
ATTACKS = (("rev_grad", "rev_grad", float("nan")), ("IPM eps=0.1", "ipm", 0.1),
           ("IPM eps=12", "ipm", 12.0), ("ALIE z=1.0", "alie", 1.0), ("ALIE z=1.5", "alie", 1.5))


def run(args, tmp, mode, err_mode, param, fail):
    cfg = Config(network="LeNet", dataset="MNIST", batch_size=args.batch_size, device="cpu",
                 lr=args.lr, dtype="fp32", max_steps=args.steps + 10, eval_freq=0, log_dir="",
                 train_dir=tmp, approach="baseline", mode=mode, worker_fail=fail,
                 err_mode=err_mode, attack_param=param, workers_per_rank=args.workers)
    if args.worker_momentum != 0.0:
        cfg.worker_momentum = args.worker_momentum
        cfg.momentum = 0.0
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    losses = [t.train_step()["loss"] for _ in range(args.steps)]
    t.close()
    return losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=7)
    ap.add_argument("--fail", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--worker-momentum", type=float, default=0.0)
    args = ap.parse_args()
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True, check=True,
                                cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except Exception:
        commit = "unknown"
    with tempfile.TemporaryDirectory() as tmp:
        clean = run(args, tmp, "normal", "rev_grad", float("nan"), 0)
        print("# Baseline rules under colluding adversaries (CPU, through the trainer)\n")
        print(f"LeNet on synthetic MNIST, P={args.workers} logical workers in one process "
              f"(`--workers-per-rank {args.workers}`), f={args.fail}, lr {args.lr}, batch "
              f"{args.batch_size} per worker, {args.steps} steps, fp32.  Each cell is the mean "
              "of the last five training losses (nan: the loss diverged).  A record of one "
              "run, not a test.\n")
        if args.worker_momentum != 0.0:
            print(f"Command: `python tools/convergence_collusion.py --worker-momentum "
                  f"{args.worker_momentum} --steps {args.steps}` on the change that adds worker "
                  f"momentum (parent commit {commit}): every worker sends m = beta*m + "
                  f"(1-beta)*g with beta = {args.worker_momentum} (m = g on the first step), "
                  "and the server's SGD momentum is 0 (it is 0.5 without the flag); "
                  "centered_clip runs with its defaults (auto radius, 3 iterations).\n")
        else:
            print(f"Command: `python tools/convergence_collusion.py` on the change that adds "
                  f"centered clipping (parent commit {commit}); centered_clip runs with its "
                  "defaults (auto radius, 3 iterations, no worker momentum).\n")
        print(f"First-step loss {clean[0]:.2f}; clean training (normal, no adversary) "
              f"reaches {np.mean(clean[-5:]):.2f}.\n")
        print("| attack | " + " | ".join(MODES) + " |")
        print("|---|" + "---|" * len(MODES))
        for label, err_mode, param in ATTACKS:
            cells = []
            for mode in MODES:
                losses = run(args, tmp, mode, err_mode, param, args.fail)
                cells.append(f"{np.mean(losses[-5:]):.2f}")
            print(f"| {label} | " + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    main()
