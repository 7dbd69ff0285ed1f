"""Mean around median ("MeaMed", arXiv:1802.10116) and Phocas (arXiv:1805.09682): the
CPU definition of ops.column_mean_around against numpy, its window rule, non-finite
rule and radius guarantee, the MeanAroundAggregator at world=1 and sharded over gloo,
the baseline modes in both topologies, and training under attack.

Error bound used against the float64 oracle (as in tests/test_trimmed_mean.py): a
sequential fp32 sum of k terms followed by one division carries at most (k+1)
roundings of relative size 2^-24 each, so |got - ref| <= (k+1) * 2^-24 * sum|kept|.
It applies where the fp32 and the float64 window start agree; where they differ the
column is a rounding tie of step 3 (two candidates at distances from the centre that
differ by less than the rounding of the centre) and is left out, under a cap.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.ops import fallback as fb
from draco_amd.parallel.aggregators import MeanAroundAggregator
from draco_amd.parallel.comm import Communicator
from draco_amd.parallel.flat import FlatSpace
from tests.dist_util import run_dist
from tests.mean_around_util import (
    bounds,
    data,
    definition_fp32,
    definition_fp64,
    legal_bs,
    plant,
    same,
)

EPS = 2.0 ** -24
CENTERS = ["median", "trimmed_mean"]


def _run(x, keep, clo, chi):
    x = torch.as_tensor(x, dtype=torch.float32).contiguous()
    out = torch.empty(x.shape[1], dtype=torch.float32)
    ops.column_mean_around(x, keep, clo, chi, out)
    return out.numpy()


def _ctm(x, lo, hi):
    x = torch.as_tensor(x, dtype=torch.float32).contiguous()
    out = torch.empty(x.shape[1], dtype=torch.float32)
    ops.column_trimmed_mean(x, lo, hi, out)
    return out.numpy()


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


# --------------------------------------------------------------- 1. vs float64 numpy
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 33, 64])
def test_fallback_matches_float64_numpy(P):
    d = 384
    x = data(P, d, seed=300 + P).numpy()
    grid_col = np.zeros(d, dtype=bool)
    grid_col[::3] = True
    for b in legal_bs(P):
        for center in CENTERS:
            keep, clo, chi = bounds(P, b, center)
            got = _run(x, keep, clo, chi)
            ref32, w32 = definition_fp32(x, keep, clo, chi)
            assert np.array_equal(_bits(got), _bits(ref32)), (P, b, center)
            ref, w64, kept_abs = definition_fp64(x, keep, clo, chi)
            agree = w32 == w64
            assert (~agree).sum() <= 0.01 * d, (P, b, center, int((~agree).sum()))
            assert agree[grid_col].all(), (P, b, center)
            err = np.abs(got.astype(np.float64) - ref)
            assert (err[agree] <= ((keep + 1) * EPS * kept_abs)[agree]).all(), (P, b, center)


def test_rejects_bad_arguments():
    x = torch.zeros(3, 8)
    out = torch.zeros(8)
    for keep, clo, chi in [(0, 1, 2), (4, 1, 2), (-1, 1, 2), (2, 1, 1), (2, 2, 1), (2, 0, 4),
                           (2, -1, 2)]:
        with pytest.raises(ValueError):
            ops.column_mean_around(x, keep, clo, chi, out)
    with pytest.raises(ValueError):
        ops.column_mean_around(x, 2, 1, 2, torch.zeros(12))
    ops.column_mean_around(torch.zeros(3, 0), 2, 1, 2, torch.zeros(0))  # d = 0: no-op


def test_tie_keeps_the_nearest_set():
    """The farther end goes, and a tie drops the top.  Around c = 2 the column
    {1, 1, 2, 2, 3} with keep = 3 keeps {1, 2, 2}: the definition is NOT "the window
    whose farthest member is nearest", which would keep {1, 1, 2}."""
    x = np.array([[1.0], [1.0], [2.0], [2.0], [2.0]], dtype=np.float32).repeat(4, axis=1)
    # median centre: c = 2; b = 2 drops both 1s -> mean 2
    assert (_run(x, 3, 2, 3) == 2.0).all()
    x = np.array([[1.0], [1.0], [2.0], [2.0], [3.0]], dtype=np.float32).repeat(4, axis=1)
    # c = 2, b = 1: |1-2| == |3-2| is a tie, the top goes -> mean(1,1,2,2) = 1.5
    assert (_run(x, 4, 2, 3) == 1.5).all()
    # b = 2: then the bottom 1 against the top 2 -> 1 is farther -> mean(1,2,2)
    got = _run(x, 3, 2, 3)
    assert np.array_equal(_bits(got), _bits(_ctm(x, 1, 4)))


# --------------------------------------------------------------- 2. window coverage
@pytest.mark.parametrize("center", CENTERS)
@pytest.mark.parametrize("b", [1, 2, 3])
def test_window_coverage_and_cross_checks(b, center):
    P, d = 9, 192
    x = data(P, d, seed=40 + b)
    groups = plant(x, b, col0=16)
    keep, clo, chi = bounds(P, b, center)
    xn = x.numpy()
    got = _run(xn, keep, clo, chi)
    _, w = definition_fp32(xn, keep, clo, chi)
    _, _, w_fb = fb.mean_around_window(x, keep, clo, chi)
    assert np.array_equal(w, w_fb.numpy())
    for m, cols in groups.items():
        assert (w[cols] == m).all(), (m, w[cols])
        # the window [m, m+keep) summed ascending is column_trimmed_mean's arithmetic
        assert np.array_equal(_bits(got[cols]), _bits(_ctm(xn, m, m + keep)[cols])), m
    # all b outliers high -> ranks [0, P-b); all low -> ranks [b, P)
    assert np.array_equal(_bits(got[groups[0]]), _bits(_ctm(xn, 0, P - b)[groups[0]]))
    assert np.array_equal(_bits(got[groups[b]]), _bits(_ctm(xn, b, P)[groups[b]]))
    # every column, planted or not: the bits of the trimmed mean over its own window
    for m in range(b + 1):
        sel = w == m
        assert np.array_equal(_bits(got[sel]), _bits(_ctm(xn, m, m + keep)[sel]))
    # keep = P: nothing dropped, whatever the centre
    assert np.array_equal(_bits(_run(xn, P, clo, chi)), _bits(_ctm(xn, 0, P)))


# --------------------------------------------------------------- 3. non-finite rule
NAN, INF = float("nan"), float("inf")
BIG = {"nan": 1e30, "inf": 1e30, "-inf": -1e30}
VAL = {"nan": NAN, "inf": INF, "-inf": -INF}


def _nonfinite_patterns(b):
    pats = [[k] * n for k in VAL for n in range(1, b + 1)]
    pats += [["nan", "-inf"], ["inf", "-inf"]]
    if b >= 3:
        pats += [["nan", "inf", "-inf"], ["-inf", "-inf", "nan"]]
    return pats


@pytest.mark.parametrize("P,b", [(5, 2), (7, 3)])
def test_nonfinite_rule(P, b):
    rng = np.random.default_rng(9 * P + b)
    d = 64
    clean = data(P, d, seed=70 + P).numpy()
    cols = [0, 5, 17, 18, 63]
    for pat in _nonfinite_patterns(b):
        rows = rng.choice(P, size=len(pat), replace=False)
        x, y = clean.copy(), clean.copy()
        for r, kind in zip(rows, pat):
            x[r, cols] = VAL[kind]
            y[r, cols] = BIG[kind]
        for center in CENTERS:
            keep, clo, chi = bounds(P, b, center)
            got = _run(x, keep, clo, chi)
            assert np.isfinite(got).all(), (pat, center)
            assert np.array_equal(_bits(got), _bits(_run(y, keep, clo, chi))), (pat, center)
            assert np.array_equal(_bits(got), _bits(definition_fp32(x, keep, clo, chi)[0]))


@pytest.mark.parametrize("P,b", [(5, 2), (7, 3)])
def test_more_than_b_nonfinite_rows(P, b):
    """Beyond the rule's tolerance the result may be inf or NaN; the op and the
    step-by-step numpy definition agree on where the NaNs are (and on the rest)."""
    rng = np.random.default_rng(P)
    clean = data(P, 64, seed=80 + P).numpy()
    for pat in [["nan"] * (b + 1), ["inf"] * (b + 1), ["-inf"] * (b + 1),
                ["inf"] * b + ["-inf"], ["-inf"] * b + ["nan"], ["nan"] * P]:
        rows = rng.choice(P, size=len(pat), replace=False)
        x = clean.copy()
        for r, kind in zip(rows, pat):
            x[r, ::2] = VAL[kind]
        for center in CENTERS:
            keep, clo, chi = bounds(P, b, center)
            got = _run(x, keep, clo, chi)
            ref, _ = definition_fp32(x, keep, clo, chi)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (pat, center)
            assert same(got, ref), (pat, center)
            assert np.isfinite(got[1::2]).all()


# --------------------------------------------------------------- 4. radius property
def _setup(d_in=30, d_out=7):
    torch.manual_seed(3)
    comm = Communicator(0, 1, torch.device("cpu"))
    model = nn.Sequential(nn.Linear(d_in, d_out), nn.Linear(d_out, 4))
    space = FlatSpace(model, 1, torch.device("cpu"))
    return comm, space


@pytest.mark.parametrize("center", CENTERS)
@pytest.mark.parametrize("attack", ["finite", "nonfinite"])
def test_radius_property(attack, center):
    """P=7, b=2 corrupted rows: the rule's centre c lies inside the honest [min, max]
    and |out - c| <= R = max over honest h of |h - c|.  The output itself may leave the
    honest [min, max] (a corrupted value just outside it can be nearer to c than a far
    honest one), so no envelope is asserted.  Slack: c and the output are fp32 results
    of at most keep+1 roundings each on values of magnitude <= |c| + R."""
    comm, space = _setup()
    P, b = 7, 2
    keep, clo, chi = bounds(P, b, center)
    rng = np.random.default_rng(5)
    g = rng.normal(size=space.d_pad).astype(np.float32)
    rows = np.stack([g + 0.1 * rng.normal(size=space.d_pad).astype(np.float32)
                     for _ in range(P)])
    rows[:, space.d:] = 0.0
    bad = [1, 4]
    honest = np.delete(rows, bad, axis=0)
    hmin, hmax = honest.min(0), honest.max(0)
    variants = []
    if attack == "finite":
        v = rows.copy()
        v[1] = -100.0 * g
        v[4] = -100.0
        variants.append(v)
        for lo_off, hi_off in [(1e-3, 1e-3), (0.05, 0.0), (0.0, 0.05)]:
            v = rows.copy()
            v[1] = hmax + np.float32(hi_off)  # just outside (or on) the honest range
            v[4] = hmin - np.float32(lo_off)
            variants.append(v)
            v = rows.copy()
            v[1] = hmax + np.float32(hi_off)  # both on one side
            v[4] = hmax + np.float32(2 * hi_off)
            variants.append(v)
    else:
        for a, c in [(np.nan, np.nan), (np.inf, np.inf), (-np.inf, -np.inf),
                     (np.nan, -np.inf), (np.inf, -np.inf)]:
            v = rows.copy()
            v[1] = a
            v[4] = c
            variants.append(v)
    d = space.d
    h64 = honest[:, :d].astype(np.float64)
    for v in variants:
        agg = MeanAroundAggregator(comm, space, num_workers=P, b=b, center=center)
        out = agg.aggregate(torch.tensor(v), 0).numpy()[:d].astype(np.float64)
        assert np.isfinite(out).all()
        s = np.sort(np.where(np.isnan(v[:, :d]), np.inf, v[:, :d].astype(np.float64)), axis=0)
        c = s[clo:chi].mean(0)  # the rule's own centre, over all P rows
        assert np.isfinite(c).all()
        assert (c >= h64.min(0)).all() and (c <= h64.max(0)).all()
        R = np.abs(h64 - c).max(0)
        slack = 8 * (keep + 1) * EPS * (np.abs(c) + R)
        assert (np.abs(out - c) <= R + slack).all()


# --------------------------------------------------------------- 5. row permutation
@pytest.mark.parametrize("P", [3, 5, 8])
def test_row_permutation_invariance(P):
    rng = np.random.default_rng(P)
    x = data(P, 129, seed=P).numpy()
    x[0, 7] = np.nan
    x[P - 1, 9] = np.inf
    x[1, 9] = -np.inf
    for b in legal_bs(P):
        for center in CENTERS:
            keep, clo, chi = bounds(P, b, center)
            base = _run(x, keep, clo, chi)
            for _ in range(4):
                perm = rng.permutation(P)
                got = _run(x[perm], keep, clo, chi)
                assert same(got, base)
                ok = ~np.isnan(base)
                assert np.array_equal(_bits(got[ok]), _bits(base[ok]))


# --------------------------------------------------------------- 6. aggregator, world=1
@pytest.mark.parametrize("P", [5, 6])
@pytest.mark.parametrize("center", CENTERS)
@pytest.mark.parametrize("b", [1, 2])
def test_aggregator_matches_numpy_definition(P, center, b):
    comm, space = _setup()
    assert space.d_pad > space.d
    agg = MeanAroundAggregator(comm, space, num_workers=P, b=b, center=center)
    assert agg.name == ("meamed" if center == "median" else "phocas")
    rng = np.random.default_rng(20 + P)
    payload = torch.tensor(rng.normal(size=(P, space.d_pad)), dtype=torch.float32)
    payload[:, space.d:] = 0.0
    out = agg.aggregate(payload, 0).numpy()
    X = payload[:, : space.d].numpy()
    keep, clo, chi = bounds(P, b, center)
    ref, w64, kept_abs = definition_fp64(X, keep, clo, chi)
    _, w32 = definition_fp32(X, keep, clo, chi)
    agree = w32 == w64
    assert (~agree).sum() <= 0.01 * space.d
    err = np.abs(out[: space.d].astype(np.float64) - ref)
    assert (err[agree] <= ((keep + 1) * EPS * kept_abs)[agree]).all()
    assert (out[space.d:] == 0.0).all()  # padding tail stays exactly zero


# --------------------------------------------------------------- 7. constructor / call errors
def test_constructor_and_call_errors():
    comm, space = _setup()
    for center in CENTERS:
        with pytest.raises(ValueError):
            MeanAroundAggregator(comm, space, num_workers=65, b=1, center=center)
        with pytest.raises(ValueError):
            MeanAroundAggregator(comm, space, num_workers=5, b=-1, center=center)
        with pytest.raises(ValueError):
            MeanAroundAggregator(comm, space, num_workers=4, b=2, center=center)
        with pytest.raises(ValueError):
            MeanAroundAggregator(comm, space, num_workers=5, b=3, center=center)
        MeanAroundAggregator(comm, space, num_workers=64, b=31, center=center)
        MeanAroundAggregator(comm, space, num_workers=1, b=0, center=center)
        # the received row count rules at call time (survivor world after a failure)
        agg = MeanAroundAggregator(comm, space, num_workers=5, b=2, center=center)
        with pytest.raises(ValueError):
            agg.aggregate(torch.zeros(4, space.d_pad), 0)
        agg.b = -1
        with pytest.raises(ValueError):
            agg.aggregate(torch.zeros(5, space.d_pad), 0)
    with pytest.raises(ValueError):
        MeanAroundAggregator(comm, space, num_workers=5, b=1, center="mean")


# --------------------------------------------------------------- 8. trainer construction
def _cfg(tmp_path, **kw):
    base = dict(
        network="FC", dataset="MNIST", batch_size=8, device="cpu", lr=0.05,
        max_steps=100, eval_freq=0, log_dir="", train_dir=str(tmp_path / "ckpt"),
    )
    base.update(kw)
    return Config(**base)


def test_trainer_builds_aggregator_for_modes(tmp_path):
    from draco_amd.parallel import MeanAroundAggregator as exported
    from draco_amd.parallel import Trainer

    assert exported is MeanAroundAggregator
    for mode, center in [("meamed", "median"), ("phocas", "trimmed_mean")]:
        t = Trainer(_cfg(tmp_path, approach="baseline", mode=mode, worker_fail=1,
                         workers_per_rank=3))
        assert isinstance(t.agg, MeanAroundAggregator) and t.agg.name == mode
        assert t.agg.b == 1 and t.agg.center == center and t.agg.num_workers == 3
        t.close()
    with pytest.raises(ValueError):  # one worker cannot lose one
        Trainer(_cfg(tmp_path, approach="baseline", mode="meamed", worker_fail=1))
    with pytest.raises(ValueError, match="median/trimmed_mean/meamed/phocas"):
        Trainer(_cfg(tmp_path, approach="baseline", mode="bulyan", worker_fail=0))


# --------------------------------------------------------------- 9. training under attack
def test_meamed_and_phocas_track_clean_training_at_P4(tmp_path):
    """The harness of tests/test_trimmed_mean.py::test_median_and_trimmed_mean_survive_attack
    (FC / synthetic MNIST, batch 8, lr 0.05, 25 steps, one rev_grad adversary per step,
    "clean" = plain averaging over the same workers) at P=4, the smallest P the existing
    rules miss the inherited 2*clean+0.1 margin at.  Both new rules drop only the b
    values farthest from the centre, so a one-sided adversary costs no honest value.

    Final losses from a torch prototype of the definition (skipped updates 0 in every arm):

    | P | clean | bound 2*clean+0.1 | median | trimmed_mean | meamed | phocas |
    |---|-------|-------------------|--------|--------------|--------|--------|
    | 4 | 0.053 | 0.206             | 0.235  | 0.235        | 0.056  | 0.056  |
    | 5 | 0.052 | 0.204             | 0.224  | 0.165        | 0.056  | 0.056  |
    | 6 | 0.057 | 0.213             | 0.178  | 0.140        | 0.059  | 0.059  |
    | 8 | 0.056 | 0.212             | 0.185  | 0.117        | 0.058  | 0.058  |
    """
    from draco_amd.parallel import Trainer

    def run(mode, fail, steps=25):
        t = Trainer(_cfg(tmp_path, approach="baseline", mode=mode, worker_fail=fail,
                         err_mode="rev_grad", workers_per_rank=4))
        t.logger.stdout_every = 0
        assert t.P == 4
        losses = [t.train_step()["loss"] for _ in range(steps)]
        skipped = t.skipped_updates
        t.close()
        return losses, skipped

    clean, _ = run("normal", 0)
    attacked_mean, _ = run("normal", 1)
    trimmed, tm_skipped = run("trimmed_mean", 1)
    meamed, mm_skipped = run("meamed", 1)
    phocas, ph_skipped = run("phocas", 1)
    print(f"final losses: clean {clean[-1]:.4f} attacked mean {attacked_mean[-1]:.4f} "
          f"trimmed_mean {trimmed[-1]:.4f} meamed {meamed[-1]:.4f} phocas {phocas[-1]:.4f}")

    assert clean[-1] < 1.0
    assert np.isnan(attacked_mean[-1]) or attacked_mean[-1] > 5 * clean[-1]
    assert meamed[-1] < 2.0 * clean[-1] + 0.1
    assert phocas[-1] < 2.0 * clean[-1] + 0.1
    assert meamed[-1] < trimmed[-1]
    assert phocas[-1] < trimmed[-1]
    assert tm_skipped == 0 and mm_skipped == 0 and ph_skipped == 0


# --------------------------------------------------------------- 10. sharding invariance
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
    for center in CENTERS:
        for b in (1, 2):
            agg = MeanAroundAggregator(comm, space, num_workers=L * world, b=b, center=center)
            outs.append(agg.aggregate(payload, step=0)[: space.d].clone())
    return torch.stack(outs)


def _shard_worker(rank, world, L):
    comm = Communicator(rank, world, torch.device("cpu"), backend="gloo")
    out = _decode(comm, world, rank, L)
    comm.shutdown()
    return out.numpy()


def test_sharded_decode_bit_equals_world1():
    """Per-coordinate rules commute with sharding exactly: P=6 logical workers as
    2 ranks x 3 decode to the same bits as 1 rank x 6."""
    res = run_dist(_shard_worker, 2, 3)
    # world=1 hosts worker w in slot l=w; world=2 hosts w = l*2 + rank
    local = _decode(Communicator(0, 1, torch.device("cpu")), 1, 0, 6).numpy()
    for r in range(2):
        assert same(res[r], local), r
        ok = ~np.isnan(local)
        assert np.array_equal(_bits(res[r][ok]), _bits(local[ok])), r
    assert np.isfinite(local[1]).all() and np.isfinite(local[3]).all()  # b=2 drops both


# --------------------------------------------------------------- 11. PS topology
def _ps_worker(rank, world, mode, steps):
    from draco_amd.parallel.ps import Master, Worker

    cfg = Config(network="FC", dataset="MNIST", batch_size=4, device="cpu", lr=0.05,
                 topology="ps", approach="baseline", mode=mode, worker_fail=1,
                 err_mode="rev_grad", max_steps=50, eval_freq=0, log_dir="",
                 train_dir="/tmp/draco_ps_ma")
    role = Master(cfg) if rank == 0 else Worker(cfg)
    role.run(max_steps=steps)
    if rank == 0:
        return (type(role.agg).__name__, role.agg.name, role.agg.b, role.agg.center,
                bool(torch.isfinite(role.space.flat_param).all()))
    return None


# one mode per launch: a second Master in the same processes re-arms the store's abort
# flag while the first round's worker pollers may still be waiting to read it
@pytest.mark.parametrize("mode,center", [("meamed", "median"), ("phocas", "trimmed_mean")])
def test_ps_master_builds_and_steps(mode, center):
    res = run_dist(_ps_worker, 4, mode, 2)[0]  # 1 PS + 3 workers, one adversary
    assert res == ("MeanAroundAggregator", mode, 1, center, True)
