"""Coordinate-wise median / trimmed mean (arXiv:1803.01498): the CPU definition of
ops.column_trimmed_mean against numpy, its non-finite rule and breakdown guarantee,
the TrimmedMeanAggregator at world=1 and sharded over gloo, the baseline modes in
both topologies, and training under attack.

Error bound used against the float64 oracle (the file-header bound of
tests/test_kernels_gpu_edges.py): a sequential fp32 sum of k terms followed by one
division carries at most (k+1) roundings of relative size 2^-24 each, so
|got - ref| <= (k+1) * 2^-24 * sum|kept terms|.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.parallel.aggregators import TrimmedMeanAggregator
from draco_amd.parallel.comm import Communicator
from draco_amd.parallel.flat import FlatSpace
from tests.dist_util import run_dist

EPS = 2.0 ** -24
NONFINITE = [float("nan"), float("inf"), float("-inf")]


def _median_bounds(P):
    return (P - 1) // 2, P // 2 + 1


def _run(x, lo, hi):
    x = torch.as_tensor(x, dtype=torch.float32).contiguous()
    out = torch.empty(x.shape[1], dtype=torch.float32)
    ops.column_trimmed_mean(x, lo, hi, out)
    return out.numpy()


def _definition_fp32(x, lo, hi):
    """The op's definition, step by step in numpy fp32."""
    a = np.where(np.isnan(x), np.float32(np.inf), x.astype(np.float32))
    s = np.sort(a, axis=0)
    acc = s[lo].copy()
    with np.errstate(invalid="ignore"):
        for k in range(lo + 1, hi):
            acc = (acc + s[k]).astype(np.float32)
        return (acc / np.float32(hi - lo)).astype(np.float32)


def _same(a, b):
    """== wherever finite or infinite, NaN exactly where the other is NaN."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        a[~np.isnan(a)], b[~np.isnan(b)])


def _cases(P):
    cases = {_median_bounds(P), (0, P), (0, 1), (P - 1, P)}
    if P >= 3:
        cases.add((1, P - 1))
    if P >= 5:
        cases.add((2, P - 2))
        cases.add((1, 4))
    return sorted(cases)


# --------------------------------------------------------------- 1. vs float64 numpy
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 8])
def test_fallback_matches_float64_numpy(P):
    rng = np.random.default_rng(100 + P)
    d = 96
    x = rng.normal(size=(P, d)).astype(np.float32)
    x[:, :32] = rng.integers(-8, 8, size=(P, 32)) / 4.0  # exact ties
    x64 = x.astype(np.float64)
    srt = np.sort(x64, axis=0)
    for lo, hi in _cases(P):
        got = _run(x, lo, hi)
        k = hi - lo
        ref = srt[lo:hi].mean(0)
        bound = (k + 1) * EPS * np.abs(srt[lo:hi]).sum(0)
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (P, lo, hi)
        assert np.array_equal(got, _definition_fp32(x, lo, hi)), (P, lo, hi)
    lo, hi = _median_bounds(P)
    got = _run(x, lo, hi)
    med = np.median(x64, axis=0)  # numpy convention: even P averages the middle two
    if P % 2 == 1:
        assert np.array_equal(got.astype(np.float64), med)
    else:
        assert (np.abs(got.astype(np.float64) - med) <= 3 * EPS * np.abs(srt[lo:hi]).sum(0)).all()


def test_rejects_bad_rank_range():
    x = torch.zeros(3, 8)
    out = torch.zeros(8)
    for lo, hi in [(1, 1), (2, 1), (0, 4), (-1, 2)]:
        with pytest.raises(ValueError):
            ops.column_trimmed_mean(x, lo, hi, out)


# --------------------------------------------------------------- 2. non-finite rule
@pytest.mark.parametrize("P,b", [(3, 1), (5, 1), (5, 2), (8, 2), (8, 3)])
def test_nonfinite_rule(P, b):
    rng = np.random.default_rng(7 * P + b)
    d = 64
    clean = rng.normal(size=(P, d)).astype(np.float32)
    cols = [0, 5, 17, 63]
    for bad in NONFINITE:
        for nbad in range(1, b + 1):
            x = clean.copy()
            rows = rng.choice(P, size=nbad, replace=False)
            for r in rows:
                x[r, cols] = bad
            honest = np.delete(clean, rows, axis=0)
            for lo, hi in [(b, P - b), _median_bounds(P)]:
                got = _run(x, lo, hi)
                assert _same(got, _definition_fp32(x, lo, hi))
                # at most b corrupted rows and at least b trimmed per end (the median
                # trims (P-1)//2 >= b): finite and inside the clean rows' envelope
                assert lo >= b and P - hi >= b
                assert np.isfinite(got[cols]).all(), (bad, nbad, lo, hi)
                assert (got[cols] >= honest[:, cols].min(0)).all()
                assert (got[cols] <= honest[:, cols].max(0)).all()


def test_mixed_nonfinite_rows_trimmed():
    """One row of each kind with b=2 (P=7): NaN and +inf go to the top, -inf to the
    bottom, all three are trimmed."""
    rng = np.random.default_rng(11)
    x = rng.normal(size=(7, 32)).astype(np.float32)
    x[1] = np.nan
    x[3] = np.inf
    x[6] = -np.inf
    got = _run(x, 2, 5)
    assert np.isfinite(got).all()
    assert _same(got, _definition_fp32(x, 2, 5))


def test_both_infinities_kept_gives_nan():
    x = np.zeros((3, 4), dtype=np.float32)
    x[0] = np.inf
    x[2] = -np.inf
    got = _run(x, 0, 3)
    assert np.isnan(got).all()


# --------------------------------------------------------------- 3. row permutation
@pytest.mark.parametrize("P", [2, 5, 8])
def test_row_permutation_invariance(P):
    rng = np.random.default_rng(P)
    x = rng.normal(size=(P, 128)).astype(np.float32)
    x[:, :40] = rng.integers(-3, 3, size=(P, 40))
    x[0, 7] = np.nan
    x[P - 1, 9] = np.inf
    for lo, hi in _cases(P):
        base = _run(x, lo, hi)
        for _ in range(4):
            perm = rng.permutation(P)
            assert _same(_run(x[perm], lo, hi), base)


# --------------------------------------------------------------- 4. aggregator, world=1
def _setup(d_in=30, d_out=7):
    torch.manual_seed(3)
    comm = Communicator(0, 1, torch.device("cpu"))
    model = nn.Sequential(nn.Linear(d_in, d_out), nn.Linear(d_out, 4))
    space = FlatSpace(model, 1, torch.device("cpu"))
    return comm, space


@pytest.mark.parametrize("P", [5, 6])
@pytest.mark.parametrize("trim", [None, 1])
def test_aggregator_matches_numpy_oracle(P, trim):
    comm, space = _setup()
    assert space.d_pad > space.d
    agg = TrimmedMeanAggregator(comm, space, num_workers=P, trim=trim)
    assert agg.name == ("median" if trim is None else "trimmed_mean")
    rng = np.random.default_rng(20 + P)
    payload = torch.tensor(rng.normal(size=(P, space.d_pad)), dtype=torch.float32)
    payload[:, space.d:] = 0.0
    out = agg.aggregate(payload, 0).numpy()
    X = payload[:, : space.d].double().numpy()
    srt = np.sort(X, axis=0)
    if trim is None:
        lo, hi = _median_bounds(P)
        ref = np.median(X, axis=0)
    else:
        lo, hi = trim, P - trim
        ref = srt[lo:hi].mean(0)
    bound = (hi - lo + 1) * EPS * np.abs(srt[lo:hi]).sum(0)
    assert (np.abs(out[: space.d] - ref) <= bound).all()
    assert (out[space.d:] == 0.0).all()  # padding tail stays exactly zero


# --------------------------------------------------------------- 5. envelope
@pytest.mark.parametrize("attack", ["finite", "nonfinite"])
def test_envelope_property(attack):
    """Breakdown guarantee: P=7, b=2 corrupted rows, b trimmed per end -> every output
    coordinate lies within the five honest rows' [min, max]."""
    comm, space = _setup()
    P, b = 7, 2
    rng = np.random.default_rng(5)
    g = rng.normal(size=space.d_pad).astype(np.float32)
    rows = np.stack([g + 0.1 * rng.normal(size=space.d_pad).astype(np.float32)
                     for _ in range(P)])
    rows[:, space.d:] = 0.0
    bad = [1, 4]
    variants = []
    if attack == "finite":
        v = rows.copy()
        v[1] = -100.0 * g
        v[4] = -100.0
        variants.append(v)
    else:
        for a, c in [(np.nan, np.nan), (np.inf, np.inf), (-np.inf, -np.inf),
                     (np.nan, -np.inf), (np.inf, -np.inf)]:
            v = rows.copy()
            v[1] = a
            v[4] = c
            variants.append(v)
    honest = np.delete(rows, bad, axis=0)[:, : space.d]
    hmin, hmax = honest.min(0), honest.max(0)
    for v in variants:
        for trim in (b, None):
            agg = TrimmedMeanAggregator(comm, space, num_workers=P, trim=trim)
            out = agg.aggregate(torch.tensor(v), 0).numpy()[: space.d]
            assert np.isfinite(out).all()
            assert (out >= hmin).all() and (out <= hmax).all()


# --------------------------------------------------------------- 6. constructor / modes
def test_constructor_errors():
    comm, space = _setup()
    with pytest.raises(ValueError):
        TrimmedMeanAggregator(comm, space, num_workers=65)
    with pytest.raises(ValueError):
        TrimmedMeanAggregator(comm, space, num_workers=4, trim=2)
    with pytest.raises(ValueError):
        TrimmedMeanAggregator(comm, space, num_workers=5, trim=3)
    TrimmedMeanAggregator(comm, space, num_workers=64)
    TrimmedMeanAggregator(comm, space, num_workers=5, trim=2)
    # the received row count rules at call time (survivor world after a failure)
    agg = TrimmedMeanAggregator(comm, space, num_workers=5, trim=2)
    with pytest.raises(ValueError):
        agg.aggregate(torch.zeros(4, space.d_pad), 0)


def _cfg(tmp_path, **kw):
    base = dict(
        network="FC", dataset="MNIST", batch_size=8, device="cpu", lr=0.05,
        max_steps=100, eval_freq=0, log_dir="", train_dir=str(tmp_path / "ckpt"),
    )
    base.update(kw)
    return Config(**base)


def test_trainer_builds_aggregator_for_modes(tmp_path):
    from draco_amd.parallel import Trainer

    t = Trainer(_cfg(tmp_path, approach="baseline", mode="median", worker_fail=0))
    assert isinstance(t.agg, TrimmedMeanAggregator) and t.agg.name == "median"
    assert t.agg.trim is None
    t.close()
    t = Trainer(_cfg(tmp_path, approach="baseline", mode="trimmed_mean", worker_fail=1,
                     workers_per_rank=3))
    assert isinstance(t.agg, TrimmedMeanAggregator) and t.agg.name == "trimmed_mean"
    assert t.agg.trim == 1 and t.agg.num_workers == 3
    t.close()
    with pytest.raises(ValueError):  # one worker cannot lose one per end
        Trainer(_cfg(tmp_path, approach="baseline", mode="trimmed_mean", worker_fail=1))
    with pytest.raises(ValueError, match="median/trimmed_mean"):
        Trainer(_cfg(tmp_path, approach="baseline", mode="bulyan", worker_fail=0))


# --------------------------------------------------------------- 7. training under attack
def test_median_and_trimmed_mean_survive_attack(tmp_path):
    """Pattern, model, step count and margin of
    tests/test_trainer.py::test_coded_beats_baseline_under_attack, with P=8 logical
    workers in one process (the worker count of one 8-GPU node) and one rev_grad
    adversary per step; "clean" is plain averaging over the same 8 workers.

    Why P=8 and not the smallest legal P: unlike the coded decodes, these rules do not
    reproduce the clean gradient — a one-sided adversary shifts the selected order
    statistic, a bias that scales with b/P (arXiv:1803.01498 Thm 1), so at step 25,
    where the loss is still falling fast, they lag clean training by a P-dependent
    amount.  Measured final losses (clean / median / trimmed mean / bound 2*clean+0.1):
    P=4 0.053/0.235/0.235/0.206, P=5 0.052/0.224/0.165/0.205 (median misses the
    margin at both), P=6 0.057/0.178/0.140/0.213, P=8 0.056/0.185/0.117/0.212."""
    from draco_amd.parallel import Trainer

    def run(mode, fail, steps=25):
        t = Trainer(_cfg(tmp_path, approach="baseline", mode=mode, worker_fail=fail,
                         err_mode="rev_grad", workers_per_rank=8))
        t.logger.stdout_every = 0
        assert t.P == 8
        losses = [t.train_step()["loss"] for _ in range(steps)]
        skipped = t.skipped_updates
        t.close()
        return losses, skipped

    clean, _ = run("normal", 0)
    attacked_mean, _ = run("normal", 1)
    median, med_skipped = run("median", 1)
    trimmed, tm_skipped = run("trimmed_mean", 1)

    assert clean[-1] < 1.0
    assert np.isnan(attacked_mean[-1]) or attacked_mean[-1] > 5 * clean[-1]
    assert median[-1] < 2.0 * clean[-1] + 0.1
    assert trimmed[-1] < 2.0 * clean[-1] + 0.1
    assert med_skipped == 0 and tm_skipped == 0


# --------------------------------------------------------------- 8. sharding invariance
def _worker_grad(w, d):
    gen = torch.Generator().manual_seed(4000 + w)
    g = torch.randn(d, generator=gen)
    g[::5] = torch.randint(-2, 3, (len(g[::5]),), generator=gen).float()  # ties
    if w == 2:
        g = g * -100.0
    if w == 3:
        g[10:20] = float("nan")
    return g


def _decode(comm, world, rank, L):
    torch.manual_seed(7)
    model = nn.Linear(50, 10)
    space = FlatSpace(model, world, torch.device("cpu"))
    payload = space.alloc_payload(L)
    for l in range(L):
        payload[l, : space.d] = _worker_grad(l * world + rank, space.d)
    outs = []
    for trim in (None, 1, 2):
        agg = TrimmedMeanAggregator(comm, space, num_workers=L * world, trim=trim)
        outs.append(agg.aggregate(payload, step=0)[: space.d].clone())
    return torch.stack(outs)


def _shard_worker(rank, world, L):
    comm = Communicator(rank, world, torch.device("cpu"), backend="gloo")
    out = _decode(comm, world, rank, L)
    comm.shutdown()
    return out.numpy()


def test_sharded_decode_bit_equals_world1():
    """Coordinate-wise rules commute with sharding exactly: P=6 logical workers as
    2 ranks x 3 decode to the same bits as 1 rank x 6."""
    res = run_dist(_shard_worker, 2, 3)
    # world=1 hosts worker w in slot l=w; world=2 hosts w = l*2 + rank
    local = _decode(Communicator(0, 1, torch.device("cpu")), 1, 0, 6).numpy()
    for r in range(2):
        assert _same(res[r], local), r
    assert np.isfinite(local[2]).all()  # trim=2 removes both the outlier and the NaN


# --------------------------------------------------------------- 9. PS topology
def _ps_worker(rank, world, steps):
    from draco_amd.parallel.ps import Master, Worker

    out = {}
    for mode in ("median", "trimmed_mean"):
        cfg = Config(network="FC", dataset="MNIST", batch_size=4, device="cpu", lr=0.05,
                     topology="ps", approach="baseline", mode=mode, worker_fail=1,
                     err_mode="rev_grad", max_steps=50, eval_freq=0, log_dir="",
                     train_dir="/tmp/draco_ps_tm")
        role = Master(cfg) if rank == 0 else Worker(cfg)
        role.run(max_steps=steps)
        if rank == 0:
            out[mode] = (type(role.agg).__name__, role.agg.name, role.agg.trim,
                         float(role.space.flat_param.double().sum()))
    return out if rank == 0 else None


def test_ps_master_builds_and_steps():
    res = run_dist(_ps_worker, 4, 2)[0]  # 1 PS + 3 workers, one adversary
    assert res["median"][:3] == ("TrimmedMeanAggregator", "median", None)
    assert res["trimmed_mean"][:3] == ("TrimmedMeanAggregator", "trimmed_mean", 1)
    assert np.isfinite(res["median"][3]) and np.isfinite(res["trimmed_mean"][3])
