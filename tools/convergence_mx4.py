"""The MXFP4 wire (--compress-grad mx4) with both roundings beside the fp32 wire for four
baseline rules and the mean, clean and under rev_grad and the colluding ALIE adversary, on
CPU through the trainer: LeNet on synthetic MNIST, P=7 logical workers in one process, f=1,
200 steps, one run per cell; the cell is the mean of the last five training losses, none ->
mx4 nearest -> mx4 stochastic.  Prints the markdown table of profiles/convergence_mx4.md.

  python tools/convergence_mx4.py > profiles/convergence_mx4.md
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

MODES = ("median", "trimmed_mean", "multi_krum", "centered_clip", "normal")
ATTACKS = (("clean", "none", float("nan")), ("rev_grad", "rev_grad", float("nan")),
           ("ALIE z=1.0", "alie", 1.0))
WIRES = (("none", "stochastic"), ("mx4", "nearest"), ("mx4", "stochastic"))


def run(args, tmp, mode, err_mode, param, wire, rounding):
    cfg = Config(network="LeNet", dataset="MNIST", batch_size=args.batch_size, device="cpu",
                 lr=args.lr, dtype="fp32", max_steps=args.steps + 10, eval_freq=0, log_dir="",
                 train_dir=tmp, approach="baseline", mode=mode, worker_fail=args.fail,
                 err_mode=err_mode, attack_param=param, workers_per_rank=args.workers,
                 compress_grad=wire, mx_rounding=rounding)
    cfg.sanity()
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    losses = [t.train_step()["loss"] for _ in range(args.steps)]
    t.close()
    return float(np.mean(losses[-5:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=7)
    ap.add_argument("--fail", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--batch-size", type=int, default=32)
    args = ap.parse_args()
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    print("# The MXFP4 wire, nearest and stochastic rounding, beside the fp32 wire (CPU, "
          "through the trainer)\n")
    print(f"LeNet on synthetic MNIST, P={args.workers} logical workers in one process "
          f"(`--workers-per-rank {args.workers}`), f={args.fail}, lr {args.lr}, batch "
          f"{args.batch_size} per worker, {args.steps} steps, fp32, one run per cell.  Each cell "
          "is the mean of the last five training losses (nan: the loss diverged), "
          "`--compress-grad none` -> `--compress-grad mx4 --mx-rounding nearest` -> "
          "`--compress-grad mx4 --mx-rounding stochastic`.  The first-step loss is 2.30.  "
          "Column `normal` is the mean (on mx4 and under ALIE the trim=0 mean over the exchange "
          "path); the clean row has no adversary (`--err-mode none`) with the rules still set "
          f"for f={args.fail}.  A record of one run, not a test; cells are reported as they "
          "came out.\n")
    print("Command: `python tools/convergence_mx4.py`.\n")
    print("| attack | " + " | ".join(MODES) + " |")
    print("|---|" + "---|" * len(MODES), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for label, err_mode, param in ATTACKS:
            cells = [" -> ".join(f"{run(args, tmp, mode, err_mode, param, w, r):.2f}"
                                 for w, r in WIRES) for mode in MODES]
            print(f"| {label} | " + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    main()
