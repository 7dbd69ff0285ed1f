"""Typed run configuration + CLI with the reference's user-facing flag names
(/root/reference/src/distributed_nn.py:23-77, README.md:104-121) plus MI355X-native
extensions (topology, dtype, workers-per-rank, vote-atol).
"""
from __future__ import annotations

import argparse
from dataclasses import dataclass, fields


@dataclass
class Config:
    # reference-parity flags
    batch_size: int = 128
    test_batch_size: int = 100
    max_steps: int = 10000
    epochs: int = 100
    lr: float = 0.01
    momentum: float = 0.5
    seed: int = 1
    network: str = "LeNet"            # LeNet|FC|ResNet18|ResNet34|ResNet50|ResNet101|ResNet152|VGG11|VGG13|VGG16|VGG19
    mode: str = "normal"              # normal|geometric_median|krum|median|trimmed_mean|meamed|phocas|
                                      # multi_krum|bulyan|centered_clip|maj_vote|cyclic (aggregation rule;
                                      # trimmed_mean drops worker_fail per end; meamed/phocas keep
                                      # the P-worker_fail values nearest the median / the
                                      # worker_fail-trimmed mean; multi_krum/bulyan take
                                      # f = worker_fail and need P >= 2f+3 / 4f+3 workers;
                                      # centered_clip takes clip_tau / clip_iters, not worker_fail)
    dataset: str = "MNIST"            # MNIST|Cifar10|ImageNetSynthetic
    comm_type: str = "Bcast"          # accepted for parity; collectives are always fused (README.md:111)
    err_mode: str = "rev_grad"        # rev_grad|constant|random|gauss|none, computed by one worker
                                      # from its own gradient, or the colluding alie|ipm
                                      # (coding/collusion.py: baseline approach, colocated
                                      # topology only; their strength is attack_param)
    approach: str = "maj_vote"        # baseline|maj_vote|cyclic
    num_aggregate: int = 5            # parity flag (unused, as in reference)
    eval_freq: int = 50
    train_dir: str = "output/models/"
    adversarial: int = 1              # parity flag (err magnitude switch; reference hardcodes -100)
    worker_fail: int = 2
    group_size: int = 5
    compress_grad: str = "none"       # none|bf16 wire dtype for gradient exchange (replaces the
                                      # reference's blosc/snappy CPU compression)
    checkpoint_step: int = 0
    optimizer: str = "sgd"            # sgd|adam (fused flat kernels, optim/flat_sgd.py)

    # MI355X-native extensions
    topology: str = "colocated"       # colocated (all ranks compute) | ps (rank0 = parameter server)
    workers_per_rank: int = 0         # 0 = derive from approach (r for maj_vote, 1 for baseline);
                                      # baseline and cyclic host this many logical workers per rank
    vote_atol: float = 0.0            # absolute vote tolerance (0.0 = reference bitwise semantics)
    vote_rtol: float = -1.0           # relative vote tolerance; -1 = auto (0 on CPU, 1e-3 on GPU --
                                      # MIOpen conv backward is not bitwise-reproducible; see
                                      # parallel/aggregators.VoteAggregator)
    vote_granularity: str = "row"     # row | segment: tolerance ball over the whole
                                      # gradient vs per parameter tensor (segment is
                                      # ~10-1000x tighter against within-tolerance
                                      # adversaries; see VoteAggregator)
    dtype: str = "bf16"               # bf16|fp32 compute dtype (grads/aggregation always fp32)
    device: str = "auto"              # auto|cuda|cpu
    deterministic: bool = False
    channels_last: bool = True    # NHWC conv layout in the flat space (wins ~3% with hipGraphs)
    hip_graphs: bool = True       # capture fwd+bwd in hipGraphs (launch-bound models; GPU only)
    straggler_timeout: float = 0.0  # ps topology: seconds after first gradient before
                                    # missing workers become erasures (0 = wait forever)
    bucket_mb: float = 25.0       # per-layer overlap: backward hooks ship the payload
                                  # row in ~bucket_mb chunks while backward continues
                                  # (eager path, baseline/maj_vote; 0 = whole-row)
    health_timeout: float = 0.0   # colocated topology: heartbeat staleness (seconds)
                                  # after which a rank is declared dead and its
                                  # logical workers become erasures (0 = disabled)
    nan_guard: bool = True        # failure detection: skip updates on non-finite decode
    gpu_timing: bool = False      # device-accurate phase spans via HIP events (metrics)
    compile: bool = False         # torch.compile the model before hipGraph capture
    fused_norm: bool = True       # ResNet BatchNorm+add+ReLU through the fused NHWC HIP
                                  # kernels (GPU, not under compile; ops/fused_bn.py)
    data_root: str = ""           # directory with real MNIST/CIFAR files (IDX/pickle);
                                  # empty or missing files -> deterministic synthetic data
    synthetic_task: str = "means" # means | teacher (see data/synthetic.py: teacher is
                                  # the non-saturating convergence-evidence task)
    log_dir: str = "output/logs/"
    attack_param: float = float("nan")  # colluding err modes: z of alie (mu - z*sigma), eps of
                                        # ipm (-eps*mu); nan = the default (alie: the paper's
                                        # z_max, which is 0 at many small P; ipm: 0.1)
    clip_tau: float = 0.0         # mode centered_clip: clipping radius; <= 0 or nan = auto (the
                                  # lower median of the step's distances to the previous
                                  # aggregate; see parallel/aggregators.CenteredClipAggregator)
    clip_iters: int = 3           # mode centered_clip: clipping iterations per step (>= 1)
    worker_momentum: float = 0.0  # beta of the worker-side momentum (arXiv:2012.10333): every
                                  # logical worker sends m = beta*m + (1-beta)*g instead of g
                                  # (0 = off; baseline approach, colocated topology, with
                                  # --momentum 0 under sgd; see ops.worker_momentum_)

    def sanity(self):
        from .coding.collusion import COLLUDING_MODES

        if self.worker_momentum != 0.0:
            what = f"worker-momentum {self.worker_momentum!r}: "
            if not 0.0 <= self.worker_momentum < 1.0:  # also catches nan
                raise ValueError(what + "--worker-momentum must be in [0, 1)")
            if self.approach != "baseline":
                raise ValueError(
                    what + "worker momentum needs --approach baseline (the coded approaches "
                    "compare or decode the workers' gradients of one step), got "
                    f"{self.approach!r}")
            if self.topology == "ps":
                raise ValueError(
                    what + "worker momentum needs the colocated topology, not --topology ps")
            if self.health_timeout > 0:
                raise ValueError(
                    what + "worker momentum cannot be combined with --health-timeout (the "
                    "momentum state of a survivor world is not built)")
            if self.optimizer == "sgd" and self.momentum != 0.0:
                raise ValueError(
                    what + f"worker momentum with --optimizer sgd --momentum {self.momentum!r} "
                    "would stack two momenta (the server step is x <- x - lr*agg(m)); "
                    "pass --momentum 0")

        if self.err_mode in COLLUDING_MODES:
            what = (f"err-mode {self.err_mode!r} is a colluding mode "
                    f"({'/'.join(COLLUDING_MODES)}): ")
            if self.approach != "baseline":
                raise ValueError(
                    what + "colluding modes need --approach baseline (the coded approaches' "
                    f"threat model is per-worker corruption), got {self.approach!r}")
            if self.topology == "ps":
                raise ValueError(
                    what + "colluding modes need the colocated topology, not --topology ps")
            if self.health_timeout > 0:
                raise ValueError(
                    what + "colluding modes cannot be combined with --health-timeout (the "
                    "row-to-worker mapping of a survivor world is not built)")
            if self.worker_fail < 1:
                raise ValueError(what + "colluding modes need --worker-fail >= 1")
        if self.approach == "maj_vote" and self.group_size < 1:
            raise ValueError("group-size must be >= 1 for maj_vote")
        if self.approach == "cyclic" and self.worker_fail < 1:
            raise ValueError("cyclic approach needs worker-fail >= 1")


def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    for f in fields(Config):
        flag = "--" + f.name.replace("_", "-")
        if f.type == "bool" or isinstance(f.default, bool):
            parser.add_argument(flag, type=lambda s: s.lower() in ("1", "true", "yes"),
                                default=f.default)
        else:
            parser.add_argument(flag, type=type(f.default), default=f.default)
    # accepted-for-parity flags with no framework meaning
    parser.add_argument("--hostfile", type=str, default="", help="accepted for CLI parity; ranks come from torchrun env")
    parser.add_argument("--no-cuda", action="store_true", default=False)
    parser.add_argument("--log-interval", type=int, default=10)
    return parser


def from_args(args: argparse.Namespace) -> Config:
    cfg = Config(**{f.name: getattr(args, f.name) for f in fields(Config)})
    if getattr(args, "no_cuda", False):
        cfg.device = "cpu"
    cfg.sanity()
    return cfg


def parse_cli(argv=None) -> Config:
    p = argparse.ArgumentParser(description="draco_amd distributed training")
    add_args(p)
    return from_args(p.parse_args(argv))
