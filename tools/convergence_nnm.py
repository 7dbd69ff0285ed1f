"""Nearest-neighbour mixing (--pre-aggregation nnm) in front of five baseline rules under
the colluding ALIE / inner-product adversaries, on CPU through the trainer: LeNet on
synthetic MNIST, P=7 logical workers in one process, f=1, 200 steps, one run per cell;
the cell is the mean of the last five training losses, without -> with mixing.  Prints
the markdown table of profiles/convergence_nnm.md.

  python tools/convergence_nnm.py > profiles/convergence_nnm.md
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from draco_amd.config import Config
from draco_amd.parallel import Trainer

MODES = ("median", "trimmed_mean", "krum", "multi_krum", "centered_clip")
ATTACKS = (("ALIE z=1.0", "alie", 1.0), ("IPM eps=0.1", "ipm", 0.1))


def run(args, tmp, mode, err_mode, param, fail, pre):
    cfg = Config(network="LeNet", dataset="MNIST", batch_size=args.batch_size, device="cpu",
                 lr=args.lr, dtype="fp32", max_steps=args.steps + 10, eval_freq=0, log_dir="",
                 train_dir=tmp, approach="baseline", mode=mode, worker_fail=fail,
                 err_mode=err_mode, attack_param=param, workers_per_rank=args.workers,
                 pre_aggregation=pre)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    losses = [t.train_step()["loss"] for _ in range(args.steps)]
    t.close()
    return float(np.mean(losses[-5:])), losses[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=7)
    ap.add_argument("--fail", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--batch-size", type=int, default=32)
    args = ap.parse_args()
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    with tempfile.TemporaryDirectory() as tmp:
        clean, first = run(args, tmp, "normal", "rev_grad", float("nan"), 0, "none")
        print("# Nearest-neighbour mixing in front of the baseline rules (CPU, through the "
              "trainer)\n")
        print(f"LeNet on synthetic MNIST, P={args.workers} logical workers in one process "
              f"(`--workers-per-rank {args.workers}`), f={args.fail}, lr {args.lr}, batch "
              f"{args.batch_size} per worker, {args.steps} steps, fp32, one run per cell.  Each "
              "cell is the mean of the last five training losses (nan: the loss diverged), "
              "`--pre-aggregation none` -> `--pre-aggregation nnm`.  A record of one run, "
              "not a test; cells where mixing does not help are reported as they came out.\n")
        print("Command: `python tools/convergence_nnm.py`.\n")
        print(f"First-step loss {first:.2f}; clean training (normal, no adversary, no mixing) "
              f"reaches {clean:.2f}.\n")
        print("| attack | " + " | ".join(MODES) + " |")
        print("|---|" + "---|" * len(MODES))
        for label, err_mode, param in ATTACKS:
            cells = []
            for mode in MODES:
                off, _ = run(args, tmp, mode, err_mode, param, args.fail, "none")
                on, _ = run(args, tmp, mode, err_mode, param, args.fail, "nnm")
                cells.append(f"{off:.2f} -> {on:.2f}")
            print(f"| {label} | " + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    main()
