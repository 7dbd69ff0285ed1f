"""signSGD with majority vote (--compress-grad sign) next to the plain mean, on CPU through
the trainer: LeNet on synthetic MNIST, P=7 logical workers in one process, f=1; clean,
rev_grad and constant; with and without --worker-momentum 0.9 (Signum).  The server's
SGD momentum is 0 in every run, so that the two halves differ in the worker momentum
alone.  Prints the markdown of profiles/convergence_sign_majority.md.

  python tools/convergence_sign.py > profiles/convergence_sign_majority.md
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

ATTACKS = (("clean", "rev_grad", 0), ("rev_grad", "rev_grad", 1), ("constant", "constant", 1))


def run(args, tmp, compress, lr, err_mode, fail, beta):
    cfg = Config(network="LeNet", dataset="MNIST", batch_size=args.batch_size, device="cpu",
                 lr=lr, momentum=0.0, dtype="fp32", max_steps=args.steps + 10, eval_freq=0,
                 log_dir="", train_dir=tmp, approach="baseline", mode="normal",
                 worker_fail=fail, err_mode=err_mode, workers_per_rank=args.workers,
                 compress_grad=compress, worker_momentum=beta)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    losses = [t.train_step()["loss"] for _ in range(args.steps)]
    t.close()
    return losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lr", type=float, default=0.05, help="the plain mean's lr")
    ap.add_argument("--sign-lr", type=float, default=0.001, help="lr under the sign wire")
    ap.add_argument("--batch-size", type=int, default=32)
    args = ap.parse_args()
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    print("# signSGD with majority vote next to the plain mean (CPU, through the trainer)\n")
    print(f"LeNet on synthetic MNIST, P={args.workers} logical workers in one process "
          f"(`--workers-per-rank {args.workers}`), f=1 (f=0 in the clean row), batch "
          f"{args.batch_size} per worker, {args.steps} steps, fp32, `--momentum 0` everywhere.  "
          f"`sign` is `--compress-grad sign` at lr {args.sign_lr} (the step per coordinate); "
          f"`mean` is the same command without it at lr {args.lr}.  Each cell is first-step "
          "loss -> mean of the last five training losses (nan: the loss diverged).  One run "
          "per cell, one seed: a record, not a test.\n")
    print(f"Command: `python tools/convergence_sign.py --steps {args.steps} --lr {args.lr} "
          f"--sign-lr {args.sign_lr}`\n")
    print("| attack | sign | sign, worker momentum 0.9 | mean | mean, worker momentum 0.9 |")
    print("|---|---|---|---|---|")
    with tempfile.TemporaryDirectory() as tmp:
        for label, err_mode, fail in ATTACKS:
            cells = []
            for compress, lr in (("sign", args.sign_lr), ("none", args.lr)):
                for beta in (0.0, 0.9):
                    losses = run(args, tmp, compress, lr, err_mode, fail, beta)
                    cells.append(f"{losses[0]:.2f} -> {np.mean(losses[-5:]):.2f}")
            print(f"| {label} | " + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    main()
