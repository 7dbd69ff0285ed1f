"""The two places every aggregation rule and the cyclic adversary are built from:
build_baseline_aggregator (Trainer and the PS master) and inject_encoded_ (trainer
whole-row path, trainer bucket path, PS worker)."""
import pytest
import torch

from draco_amd.config import Config
from draco_amd.models import build_model
from draco_amd.ops import fallback as fb
from draco_amd.parallel import Communicator, FlatSpace
from draco_amd.parallel import aggregators as A

CPU = torch.device("cpu")
P = 7  # Bulyan's floor at f = 1 (4f + 3)
RULE_PARAMS = ("trim", "b", "center", "f", "s", "tau", "iters")
MODES = ("normal/geometric_median/krum/median/trimmed_mean/meamed/phocas/"
         "multi_krum/bulyan/centered_clip")

# (mode, err_mode) -> class, name, rule parameters at worker_fail=1, clip_tau=2.5,
# clip_iters=5: what the trainer's and the PS master's own mode ladders built before the
# two were merged into the builder
EXPECTED = [
    ("normal", "rev_grad", A.MeanAggregator, "mean", {}),
    ("geometric_median", "rev_grad", A.GeoMedianAggregator, "geo_median", {}),
    ("krum", "rev_grad", A.KrumAggregator, "krum", {"s": 1}),
    ("median", "rev_grad", A.TrimmedMeanAggregator, "median", {"trim": None}),
    ("trimmed_mean", "rev_grad", A.TrimmedMeanAggregator, "trimmed_mean", {"trim": 1}),
    ("meamed", "rev_grad", A.MeanAroundAggregator, "meamed", {"b": 1, "center": "median"}),
    ("phocas", "rev_grad", A.MeanAroundAggregator, "phocas",
     {"b": 1, "center": "trimmed_mean"}),
    ("multi_krum", "rev_grad", A.MultiKrumAggregator, "multi_krum", {"f": 1}),
    ("bulyan", "rev_grad", A.BulyanAggregator, "bulyan", {"f": 1}),
    ("centered_clip", "rev_grad", A.CenteredClipAggregator, "centered_clip",
     {"tau": 2.5, "iters": 5}),
    # the plain mean under a colluding adversary goes over the exchange path
    ("normal", "alie", A.TrimmedMeanAggregator, "mean", {"trim": 0}),
]


@pytest.fixture(scope="module")
def space():
    torch.manual_seed(0)
    return FlatSpace(build_model("FC", "MNIST"), 1, CPU)


@pytest.mark.parametrize("mode,err_mode,cls,name,params", EXPECTED,
                         ids=[f"{e[0]}-{e[1]}" for e in EXPECTED])
def test_build_baseline_aggregator(space, mode, err_mode, cls, name, params):
    assert A.BASELINE_MODES == MODES
    assert [e[0] for e in EXPECTED[:10]] == MODES.split("/")
    cfg = Config(network="FC", dataset="MNIST", device="cpu", approach="baseline", mode=mode,
                 worker_fail=1, err_mode=err_mode, clip_tau=2.5, clip_iters=5)
    agg = A.build_baseline_aggregator(cfg, Communicator(0, 1, CPU), space, P)
    assert type(agg) is cls and agg.name == name
    assert agg.num_workers == P
    got = {k: getattr(agg, k) for k in RULE_PARAMS if hasattr(agg, k)}
    assert got == params


def test_inject_encoded_slices_compose():
    base = torch.randn(2, 16, generator=torch.Generator().manual_seed(5))
    for mode in ("rev_grad", "constant", "random", "none"):
        whole, halves = base.clone(), base.clone()
        A.inject_encoded_(whole, mode)
        A.inject_encoded_(halves[:, :8], mode)
        A.inject_encoded_(halves[:, 8:], mode)
        assert torch.equal(whole.view(torch.int32), halves.view(torch.int32)), mode
    assert torch.equal(whole, base)  # "none" touches nothing
    rev = base.clone()
    A.inject_encoded_(rev, "rev_grad")
    assert torch.allclose(rev, base + base * fb.ADVERSARY_)  # additive, both planes
    noisy = base.clone()
    A.inject_encoded_(noisy, "gauss")  # scales by the mean over its slice: no composition
    assert not torch.equal(noisy, base) and bool(torch.isfinite(noisy).all())
    with pytest.raises(ValueError):
        A.inject_encoded_(base.clone(), "no_such_mode")
