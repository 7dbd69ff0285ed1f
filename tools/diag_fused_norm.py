"""Whole-network gradient of ResNet-18 at the seeded start state that bench.py's
--dump-outputs step uses (batch 128): the fused-norm bf16 path and the torch bf16 path
(fused_norm off) against the torch fp32 gradient of the same batch, and against each
other, with each arm's own repeat noise.  Tells a wrong fused gradient (far from fp32)
from a merely differently rounded one (as far from fp32 as the torch bf16 path is).

  python tools/diag_fused_norm.py        (needs the GPU)
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from draco_amd.config import Config
from draco_amd.parallel.trainer import Trainer

def grads(fused, dtype, reps=3):
    cfg = Config(network="ResNet18", dataset="Cifar10", batch_size=128, device="cuda", dtype=dtype,
                 approach="maj_vote", mode="maj_vote", group_size=3, worker_fail=0, lr=0.01,
                 fused_norm=fused, hip_graphs=False, eval_freq=0, log_dir="",
                 train_dir=tempfile.mkdtemp())
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    x, y = t.data.batch_for(0, 24)
    out = []
    for _ in range(reps + 1):
        g = t.space.alloc_payload(1)[0]
        t._forward_backward(x, y, g)
        torch.cuda.synchronize()
        out.append(g[: t.space.d].double().clone())
    pn = float(t.space.flat_param[: t.space.d].double().norm())
    t.close()
    return out[1:], pn

def rel(a, b):
    return float((a - b).norm() / b.norm())


ref, pn = grads(False, "fp32")
par, _ = grads(False, "bf16")
new, _ = grads(True, "bf16")
print(f"|param|={pn:.4f} |grad fp32|={float(ref[0].norm()):.4f}  lr*|grad|/|param|={0.01*float(ref[0].norm())/pn:.3e}")
print("repeat noise fp32   ", [f"{rel(ref[i], ref[0]):.3e}" for i in (1, 2)])
print("repeat noise parent ", [f"{rel(par[i], par[0]):.3e}" for i in (1, 2)])
print("repeat noise fused  ", [f"{rel(new[i], new[0]):.3e}" for i in (1, 2)])
print("parent bf16 vs fp32 ", [f"{rel(p, ref[0]):.3e}" for p in par])
print("fused  bf16 vs fp32 ", [f"{rel(n, ref[0]):.3e}" for n in new])
print("fused vs parent     ", [f"{rel(n, p):.3e}" for n, p in zip(new, par)])

