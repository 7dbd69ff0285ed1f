"""Multi-Krum (arXiv:1703.02757 §4) and Bulyan (arXiv:1802.07927) on the CPU: the
definition of ops.segment_mean_around against independent numpy statements, the two
Krum selections against brute-force fp64 loop oracles, MultiKrumAggregator and
BulyanAggregator at world=1 end to end and sharded over gloo, their configuration
errors, the baseline wiring in both topologies, and training under attack.

Error bound against the float64 definition: that of tests/test_mean_around.py — a
sequential fp32 sum of k terms and one division carry at most (k+1) roundings of
relative size 2^-24, so |got - ref| <= (k+1) * 2^-24 * sum|kept| where the fp32 and the
float64 window start agree (where they differ the column is a rounding tie of the
window rule and is left out, under a cap).
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.ops import fallback as fb
from draco_amd.parallel.aggregators import (
    BulyanAggregator,
    MultiKrumAggregator,
    select_bulyan,
    select_multi_krum,
)
from draco_amd.parallel.comm import Communicator
from draco_amd.parallel.flat import FlatSpace
from tests.bulyan_util import (
    EPS,
    gram_error_bound,
    oracle_bulyan,
    oracle_distances,
    oracle_multi_krum,
    random_sel,
    seg_definition_fp32,
    separated_rows,
)
from tests.dist_util import run_dist
from tests.mean_around_util import data, definition_fp64, legal_bs, median_bounds, plant, same

# an empty segment, odd bounds, seg[0] > 0 and seg[L] < d
D_OP = 96
SEG_OP = [3, 3, 10, 25, 64, 65, 90]


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def _run(x, sel, seg, keep, clo, chi):
    x = torch.as_tensor(x, dtype=torch.float32).contiguous()
    out = torch.full((x.shape[1],), -7.0, dtype=torch.float32)  # the op writes every element
    ops.segment_mean_around(x, torch.as_tensor(sel), torch.as_tensor(seg), keep, clo, chi, out)
    return out.numpy()


def _cases(T):
    """(keep, clo, chi): the legal b of T with the median and the trimmed-mean centre,
    and the plain mean."""
    out = {(T, 0, T)}
    for b in legal_bs(T):
        out.add((T - b,) + median_bounds(T))
        out.add((T - b, b, T - b))
    return sorted(out)


# --------------------------------------------------------------- 1. the op's definition
@pytest.mark.parametrize("P,T", [(1, 1), (4, 1), (5, 2), (7, 5), (9, 9), (12, 7), (36, 33),
                                 (64, 64)])
def test_fallback_matches_independent_definitions(P, T):
    x = data(P, D_OP, seed=900 + P)
    if T > 2:
        plant(x, min((T - 1) // 2, 3), col0=30)  # far outliers, in whichever rows are selected
    xn = x.numpy()
    L = len(SEG_OP) - 1
    sel = random_sel(L, P, T, seed=P * 100 + T).numpy()
    covered = np.zeros(D_OP, dtype=bool)
    covered[SEG_OP[0]:SEG_OP[-1]] = True
    for keep, clo, chi in _cases(T):
        got = _run(xn, sel, SEG_OP, keep, clo, chi)
        assert np.array_equal(_bits(got), _bits(seg_definition_fp32(xn, sel, SEG_OP, keep,
                                                                    clo, chi)))
        # outside [seg[0], seg[L]): +0.0, sign included
        assert (got[~covered] == 0.0).all() and not np.signbit(got[~covered]).any()
        # the order of sel[l] cannot matter
        assert np.array_equal(_bits(got), _bits(_run(xn, sel[:, ::-1].copy(), SEG_OP, keep,
                                                     clo, chi)))
        for l in range(L):
            lo, hi = SEG_OP[l], SEG_OP[l + 1]
            if hi == lo:
                continue
            ref, w64, kept_abs = definition_fp64(xn[sel[l]][:, lo:hi], keep, clo, chi)
            _, _, w32 = fb.mean_around_window(x[sel[l]][:, lo:hi], keep, clo, chi)
            agree = w32.numpy() == w64
            assert (~agree).sum() <= max(1, 0.02 * (hi - lo)), (l, keep, clo, chi)
            err = np.abs(got[lo:hi].astype(np.float64) - ref)
            assert (err[agree] <= ((keep + 1) * EPS * kept_abs)[agree]).all(), (l, keep, clo, chi)


def test_unselected_rows_are_never_read_and_sel_is_clamped():
    P, T = 7, 4
    x = data(P, D_OP, seed=11)
    L = len(SEG_OP) - 1
    sel = random_sel(L, P, T, seed=12)
    clean = _run(x, sel, SEG_OP, 3, 1, 3)
    assert np.isfinite(clean).all()
    for bad in (float("nan"), float("inf"), -float("inf")):
        y = x.clone()
        for l in range(L):  # poison, per segment, every row that lost the selection
            lose = sorted(set(range(P)) - set(sel[l].tolist()))
            y[lose, SEG_OP[l]:SEG_OP[l + 1]] = bad
        y[:, : SEG_OP[0]] = bad
        y[:, SEG_OP[-1]:] = bad
        assert np.array_equal(_bits(_run(y, sel, SEG_OP, 3, 1, 3)), _bits(clean))
    # out-of-range indices are clamped into [0, P) (checked on the CPU only)
    wild = sel.clone()
    wild[0, 0], wild[2, 1], wild[4, 3] = -3, P + 5, 2 ** 40
    got = _run(x, wild, SEG_OP, 3, 1, 3)
    assert np.array_equal(_bits(got), _bits(_run(x, wild.clamp(0, P - 1), SEG_OP, 3, 1, 3)))


def test_rejects_bad_arguments():
    x = torch.zeros(5, 8)
    seg = torch.tensor([0, 4, 8])
    sel = torch.tensor([[0, 1, 2], [2, 3, 4]])
    out = torch.zeros(8)
    ops.segment_mean_around(x, sel, seg, 2, 1, 2, out)
    for keep, clo, chi in [(0, 1, 2), (4, 1, 2), (-1, 1, 2), (2, 1, 1), (2, 2, 1), (2, 0, 4),
                           (2, -1, 2)]:
        with pytest.raises(ValueError):
            ops.segment_mean_around(x, sel, seg, keep, clo, chi, out)
    with pytest.raises(ValueError):
        ops.segment_mean_around(x, sel, seg, 2, 1, 2, torch.zeros(12))
    with pytest.raises(ValueError):  # sel rows != L
        ops.segment_mean_around(x, sel[:1], seg, 2, 1, 2, out)
    with pytest.raises(ValueError):  # T > P
        ops.segment_mean_around(x[:2], sel, seg, 2, 1, 2, out)
    with pytest.raises(ValueError):  # T = 0
        ops.segment_mean_around(x, sel[:, :0], seg, 1, 0, 1, out)
    ops.segment_mean_around(torch.zeros(5, 0), sel, torch.tensor([0, 0, 0]), 2, 1, 2,
                            torch.zeros(0))  # d = 0: no-op


# --------------------------------------------------------------- 2. the two selections
def _layers():
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(30, 7), nn.Linear(7, 4))
    return FlatSpace(model, 1, torch.device("cpu"))


def _gram(rows, seg):
    return fb.segment_gram(torch.tensor(rows), torch.as_tensor(seg))


def _assert_gaps_dwarf_gram_rounding(Xl, honest, bad, f, m, theta):
    """The test data's own margin: with exact distances D and an fp32-Gram error of at
    most e per honest pair, (1) every honest-adversary distance stays above every honest
    pair's, so an honest row's kept distances are honest ones whichever arithmetic sorts
    them (keep <= remaining honest - 2) and its score moves by at most keep*e; (2) at
    every decision the winning score and the next different one lie at least 10 such
    errors apart.  An exact tie is only the structural one of keep = 1 — two rows that
    are each other's nearest neighbour share one (symmetric) distance — which every
    arithmetic breaks by the lower index."""
    D = oracle_distances(Xl)
    e = gram_error_bound(Xl, honest)
    hmax = max(D[i, j] for i in honest for j in honest if i != j)
    for a in bad:
        e_bad = gram_error_bound(Xl, honest + [a])
        assert min(D[i, a] for i in honest) - e_bad > hmax + e
    keep = max(Xl.shape[0] - f - 2, 1)
    _, scores = oracle_multi_krum(D, f, m)
    hs = sorted(scores[i] for i in honest)
    assert min(b - a for a, b in zip(hs, hs[1:])) > 10 * keep * e
    _, history = oracle_bulyan(D, f, theta)
    for t, cand in enumerate(history):
        hs = sorted(s for i, s in cand.items() if i in honest and np.isfinite(s))
        keep_t = max(Xl.shape[0] - t - f - 2, 1)
        later = [s for s in hs if s != hs[0]]
        assert len(hs) - len(later) == 1 or keep_t == 1, t
        if later:
            assert later[0] - hs[0] > 10 * keep_t * e, t


@pytest.mark.parametrize("P,f,attack", [(7, 1, "rev"), (11, 2, "rev"), (7, 0, None),
                                        (11, 2, "nan"), (7, 1, "inf")])
def test_selection_matches_bruteforce_oracle(P, f, attack):
    space = _layers()
    seg = space.seg_bounds.numpy()
    bad = [1, 5][:f]
    rows = separated_rows(P, space.d, bad, seed=50 + P + f, attack=attack or "rev")
    honest = [p for p in range(P) if p not in bad]
    gram = _gram(rows, seg)
    theta, m = P - 2 * f, P - f
    got_mk = select_multi_krum(gram, f, m)
    got_bu = select_bulyan(gram, f, theta)
    assert got_mk.dtype == torch.int64 and got_bu.dtype == torch.int64
    assert tuple(got_mk.shape) == (len(seg) - 1, m) and tuple(got_bu.shape) == (len(seg) - 1, theta)
    for l in range(len(seg) - 1):
        Xl = rows[:, seg[l]:seg[l + 1]]
        if attack in (None, "rev"):
            _assert_gaps_dwarf_gram_rounding(Xl, honest, bad, f, m, theta)
        D = oracle_distances(Xl)
        assert got_mk[l].tolist() == oracle_multi_krum(D, f, m)[0], l
        assert got_bu[l].tolist() == oracle_bulyan(D, f, theta)[0], l
        assert not set(bad) & set(got_mk[l].tolist()) and not set(bad) & set(got_bu[l].tolist())
        # a smaller m is a prefix of the same order
        assert select_multi_krum(gram, f, 2)[l].tolist() == oracle_multi_krum(D, f, 2)[0]


@pytest.mark.parametrize("P,f", [(7, 1), (11, 2), (5, 0)])
def test_selection_on_all_tied_rows(P, f):
    """Identical rows: every score ties.  The iterative form must still return theta
    DISTINCT rows (a removed row is never chosen again), and on an exactly tied Gram
    both forms take the lowest indices."""
    space = _layers()
    row = np.random.default_rng(1).normal(size=space.d).astype(np.float32)
    rows = np.stack([row] * P)
    theta, m = P - 2 * f, P - f
    gram = _gram(rows, space.seg_bounds)
    for sel, T in ((select_bulyan(gram, f, theta), theta), (select_multi_krum(gram, f, m), m)):
        for l in range(sel.shape[0]):
            assert len(set(sel[l].tolist())) == T and set(sel[l].tolist()) <= set(range(P))
    exact = torch.full((3, P, P), 2.5)
    assert select_bulyan(exact, f, theta).tolist() == [list(range(theta))] * 3
    assert select_multi_krum(exact, f, m).tolist() == [list(range(m))] * 3
    # every distance non-finite: still theta distinct rows, lowest index first
    poisoned = torch.full((2, P, P), float("nan"))
    assert select_bulyan(poisoned, f, theta).tolist() == [list(range(theta))] * 2


# --------------------------------------------------------------- 3. aggregators, world=1
def _setup():
    space = _layers()
    assert space.d_pad > space.d
    return Communicator(0, 1, torch.device("cpu")), space


@pytest.mark.parametrize("attack", ["plus100", "collude", "nan", "inf", "-inf"])
@pytest.mark.parametrize("P,f", [(7, 1), (11, 2)])
def test_aggregators_match_oracle_end_to_end(P, f, attack):
    """f adversarial rows: the output is finite, equals the numpy definition over the
    oracle's selection, and no adversarial row is selected — with one exception that
    is the algorithm's, not the code's: f = 2 COLLUDING rows (identical, distance 0 to
    each other) win Bulyan's late picks, where max(n'-f-2, 1) = 1 and a row's score is
    the distance to its nearest remaining neighbour.  At most f of the theta selected
    rows are then corrupted and the second stage bounds them: the radius guarantee
    below is asserted in every case, over the selected honest rows."""
    comm, space = _setup()
    d, seg = space.d, space.seg_bounds.numpy()
    bad = [2, 6][:f]
    honest = [p for p in range(P) if p not in bad]
    rows = separated_rows(P, d, bad, seed=7 * P + f, attack=attack)
    payload = torch.zeros(P, space.d_pad)
    payload[:, :d] = torch.tensor(rows)
    theta, beta, m = P - 2 * f, P - 4 * f, P - f
    plans = [
        (BulyanAggregator(comm, space, num_workers=P, f=f), "bulyan", oracle_bulyan, theta,
         (beta, (theta - 1) // 2, theta // 2 + 1)),
        (MultiKrumAggregator(comm, space, num_workers=P, f=f), "multi_krum",
         lambda D, f_, T: oracle_multi_krum(D, f_, T), m, (m, 0, m)),
    ]
    for agg, name, oracle, T, (keep, clo, chi) in plans:
        assert agg.name == name
        out = agg.aggregate(payload, 0).numpy()
        sel = agg.last_sel.numpy()
        assert sel.shape == (len(seg) - 1, T)
        assert np.isfinite(out).all(), name
        if name == "bulyan" and attack == "collude" and f > 1:
            assert (np.isin(sel, bad).sum(axis=1) <= f).all()
            assert np.isin(sel, bad).any()  # the exception is real, not hypothetical
        else:
            assert not np.isin(sel, bad).any(), name  # no adversarial row in any selection
        for l in range(len(seg) - 1):
            D = oracle_distances(rows[:, seg[l]:seg[l + 1]])
            assert sel[l].tolist() == oracle(D, f, T)[0], (name, l)
        assert np.array_equal(_bits(out[:d]),
                              _bits(seg_definition_fp32(rows, sel, seg, keep, clo, chi)))
        assert (out[d:] == 0.0).all()  # padding tail stays exactly zero
        if name == "bulyan":
            # radius guarantee of column_mean_around over the selected rows: c = their
            # median, R = max over selected honest h of |h - c|; slack as in
            # tests/test_mean_around.py::test_radius_property
            for l in range(len(seg) - 1):
                lo, hi = seg[l], seg[l + 1]
                S = rows[sel[l]][:, lo:hi].astype(np.float64)
                H = rows[[p for p in sel[l] if p in honest]][:, lo:hi].astype(np.float64)
                c = np.sort(S, axis=0)[clo:chi].mean(0)
                assert (c >= H.min(0)).all() and (c <= H.max(0)).all()
                R = np.abs(H - c).max(0)
                slack = 8 * (keep + 1) * EPS * (np.abs(c) + R)
                assert (np.abs(out[lo:hi] - c) <= R + slack).all(), l


def test_bulyan_radius_with_a_selected_adversary():
    """What Bulyan adds to Krum, at the op level: of theta=5 selected rows one is
    corrupted (it got through the selection), keep = theta - 2f = 3 — the median of
    the selected values stays inside the selected honest [min, max] and the output
    within the honest radius of it, on every coordinate."""
    P, theta, f = 7, 5, 1
    x = data(P, D_OP, seed=21)
    sel = random_sel(len(SEG_OP) - 1, P, theta, seed=22)
    y = x.clone()
    for l in range(sel.shape[0]):
        y[sel[l, 0], SEG_OP[l]:SEG_OP[l + 1]] += 50.0  # the corrupted selected row
    keep, clo, chi = theta - 2 * f, (theta - 1) // 2, theta // 2 + 1
    out = _run(y, sel, SEG_OP, keep, clo, chi)
    for l in range(sel.shape[0]):
        lo, hi = SEG_OP[l], SEG_OP[l + 1]
        if hi == lo:
            continue
        S = y[sel[l]][:, lo:hi].double().numpy()
        H = S[1:]
        c = np.sort(S, axis=0)[clo:chi].mean(0)
        R = np.abs(H - c).max(0)
        assert (c >= H.min(0)).all() and (c <= H.max(0)).all()
        assert (np.abs(out[lo:hi] - c) <= R + 8 * (keep + 1) * EPS * (np.abs(c) + R)).all()


# --------------------------------------------------------------- 4. configuration errors
def test_constructor_and_survivor_world_errors():
    comm, space = _setup()
    for f in (1, 2):
        with pytest.raises(ValueError):
            BulyanAggregator(comm, space, num_workers=4 * f + 2, f=f)
        BulyanAggregator(comm, space, num_workers=4 * f + 3, f=f)
        with pytest.raises(ValueError):
            MultiKrumAggregator(comm, space, num_workers=2 * f + 2, f=f)
        MultiKrumAggregator(comm, space, num_workers=2 * f + 3, f=f)
    for cls in (BulyanAggregator, MultiKrumAggregator):
        with pytest.raises(ValueError):
            cls(comm, space, num_workers=33, f=1)
        cls(comm, space, num_workers=32, f=1)
        with pytest.raises(ValueError):
            cls(comm, space, num_workers=9, f=-1)
        # the received row count rules at call time (survivor world after a failure)
        agg = cls(comm, space, num_workers=7, f=1)
        need = 7 if cls is BulyanAggregator else 5
        with pytest.raises(ValueError):
            agg.aggregate(torch.zeros(need - 1, space.d_pad), 0)
        agg.aggregate(torch.zeros(need, space.d_pad), 0)
        with pytest.raises(ValueError):
            agg.aggregate(torch.zeros(33, space.d_pad), 0)
    for m in (0, 7, -1):  # m outside 1..P-f
        with pytest.raises(ValueError):
            MultiKrumAggregator(comm, space, num_workers=7, f=1, m=m)
    agg = MultiKrumAggregator(comm, space, num_workers=7, f=1, m=6)
    with pytest.raises(ValueError):  # m = 6 > P - f = 5 once a worker is gone
        agg.aggregate(torch.zeros(6, space.d_pad), 0)
    assert MultiKrumAggregator(comm, space, num_workers=7, f=1, m=2).aggregate(
        torch.zeros(7, space.d_pad), 0).shape == (space.d_pad,)


# --------------------------------------------------------------- 5. wiring
def _cfg(tmp_path, **kw):
    base = dict(
        network="FC", dataset="MNIST", batch_size=8, device="cpu", lr=0.05,
        max_steps=100, eval_freq=0, log_dir="", train_dir=str(tmp_path / "ckpt"),
    )
    base.update(kw)
    return Config(**base)


def test_trainer_builds_aggregator_for_modes(tmp_path):
    import draco_amd.parallel as par
    from draco_amd.parallel import Trainer

    assert par.BulyanAggregator is BulyanAggregator
    assert par.MultiKrumAggregator is MultiKrumAggregator
    assert "BulyanAggregator" in par.__all__ and "MultiKrumAggregator" in par.__all__
    for mode, cls in [("multi_krum", MultiKrumAggregator), ("bulyan", BulyanAggregator)]:
        t = Trainer(_cfg(tmp_path, approach="baseline", mode=mode, worker_fail=1,
                         workers_per_rank=7))
        assert isinstance(t.agg, cls) and t.agg.name == mode
        assert t.agg.f == 1 and t.agg.num_workers == 7
        t.close()
        with pytest.raises(ValueError):  # one worker is below both floors
            Trainer(_cfg(tmp_path, approach="baseline", mode=mode, worker_fail=1))
    with pytest.raises(ValueError):  # 6 < 4f + 3
        Trainer(_cfg(tmp_path, approach="baseline", mode="bulyan", worker_fail=1,
                     workers_per_rank=6))
    with pytest.raises(ValueError, match="median/trimmed_mean/meamed/phocas/multi_krum/bulyan"):
        Trainer(_cfg(tmp_path, approach="baseline", mode="nonesuch", worker_fail=0))


def _ps_worker(rank, world, mode, steps):
    from draco_amd.parallel.ps import Master, Worker

    cfg = Config(network="FC", dataset="MNIST", batch_size=4, device="cpu", lr=0.05,
                 topology="ps", approach="baseline", mode=mode, worker_fail=0,
                 err_mode="rev_grad", max_steps=50, eval_freq=0, log_dir="",
                 train_dir="/tmp/draco_ps_bulyan")
    role = Master(cfg) if rank == 0 else Worker(cfg)
    role.run(max_steps=steps)
    if rank == 0:
        return (type(role.agg).__name__, role.agg.name, role.agg.f, role.agg.num_workers,
                bool(torch.isfinite(role.space.flat_param).all()))
    return None


# one mode per launch, as in tests/test_mean_around.py
@pytest.mark.parametrize("mode,cls", [("multi_krum", "MultiKrumAggregator"),
                                      ("bulyan", "BulyanAggregator")])
def test_ps_master_builds_and_steps(mode, cls):
    res = run_dist(_ps_worker, 4, mode, 2)[0]  # 1 PS + 3 workers: the floor of both at f = 0
    assert res == (cls, mode, 0, 3, True)


# --------------------------------------------------------------- 6. sharding invariance
def _decode(comm, world, rank, L):
    torch.manual_seed(7)
    model = nn.Sequential(nn.Linear(50, 10), nn.Linear(10, 3))
    space = FlatSpace(model, world, torch.device("cpu"))
    P = L * world
    outs, sels = [], []
    for attack in ("rev", "nan"):
        rows = separated_rows(P, space.d, [3], seed=4000, attack=attack)
        payload = space.alloc_payload(L)
        for l in range(L):
            payload[l, : space.d] = torch.tensor(rows[l * world + rank])
        for agg in (BulyanAggregator(comm, space, num_workers=P, f=1),
                    MultiKrumAggregator(comm, space, num_workers=P, f=1),
                    MultiKrumAggregator(comm, space, num_workers=P, f=1, m=3)):
            outs.append(agg.aggregate(payload, step=0)[: space.d].clone())
            sels.append(agg.last_sel.clone().numpy())
    return torch.stack(outs).numpy(), sels


def _shard_worker(rank, world, L):
    comm = Communicator(rank, world, torch.device("cpu"), backend="gloo")
    out = _decode(comm, world, rank, L)
    comm.shutdown()
    return out


def test_sharded_decode_bit_equals_world1():
    """2 ranks x 4 workers decode to the same bits as 1 rank x 8 in both modes (the
    smallest even P at which Bulyan runs with f = 1; P = 7 cannot be split over two
    equal ranks).  Every rank holds the identical allreduced Gram, hence the identical
    selection; across world sizes the Gram differs in its last bits (partial sums per
    shard), which the well separated rows absorb; the rest is per coordinate."""
    res = run_dist(_shard_worker, 2, 4)
    local, local_sel = _decode(Communicator(0, 1, torch.device("cpu")), 1, 0, 8)
    assert np.isfinite(local).all()
    for r in range(2):
        out, sels = res[r]
        for a, b in zip(sels, local_sel):
            assert np.array_equal(a, b), r
            assert not np.isin(a, [3]).any()  # the adversary, finite or not
        assert same(out, local), r
        assert np.array_equal(_bits(out), _bits(local)), r


# --------------------------------------------------------------- 7. training under attack
def test_multi_krum_and_bulyan_track_clean_training(tmp_path):
    """LeNet / synthetic MNIST, batch 8, lr 0.05, P=7 workers in one process, one
    rev_grad adversary per step; "clean" is plain averaging over the same 7 workers
    without the adversary, for the same number of steps.  The bound is that of
    tests/test_mean_around.py (final < 2*clean + 0.1).

    Length: 100 steps.  LeNet sits on the ln(10) plateau for the first ~30 steps (clean
    loss 2.11 at step 25, where the bound would hold for any rule that does not
    diverge), then falls 10x in 20 steps; a bound on the FINAL loss says something about
    the rule only once the clean run is past that cliff, where a lag of a few steps is
    no longer a factor of several in the loss.  Measured on the CPU (skipped updates 0
    in every arm; attacked plain mean: NaN):

    | step | clean | bound 2*clean+0.1 | multi_krum | bulyan | meamed | median |
    |------|-------|-------------------|------------|--------|--------|--------|
    |  25  | 2.109 | 4.318             | 2.088      | 2.139  | 2.094  | 2.170  |
    |  40  | 1.467 | 3.034             | 1.500      | 1.879  | 1.542  | 1.968  |
    |  60  | 0.215 | 0.531             | 0.284      | 1.255* | 0.309  | 1.288* |
    |  80  | 0.116 | 0.332             | 0.108      | 0.284  | 0.113  | 0.294  |
    | 100  | 0.046 | 0.192             | 0.050      | 0.107  | 0.050  | 0.096  |
    | 120  | 0.024 | 0.148             | 0.032      | 0.044  | 0.032  | 0.044  |

    * misses the bound: on the cliff Bulyan runs ~15 steps behind clean training, as
    the coordinate-wise median does and as Bulyan does WITHOUT an adversary (0.763 at
    step 60): at P=7, f=1 it averages beta=3 of 7 values around the median, so its
    gradient is about as noisy as the median's at batch 8.  Multi-Krum averages 6 of 7
    and tracks the clean curve throughout.
    """
    from draco_amd.parallel import Trainer

    def run(mode, fail, steps=100):
        t = Trainer(_cfg(tmp_path, network="LeNet", approach="baseline", mode=mode,
                         worker_fail=fail, err_mode="rev_grad", workers_per_rank=7))
        t.logger.stdout_every = 0
        assert t.P == 7
        losses = [t.train_step()["loss"] for _ in range(steps)]
        skipped = t.skipped_updates
        t.close()
        return losses, skipped

    clean, _ = run("normal", 0)
    attacked_mean, _ = run("normal", 1)
    multi_krum, mk_skipped = run("multi_krum", 1)
    bulyan, bu_skipped = run("bulyan", 1)
    print(f"final losses: clean {clean[-1]:.4f} attacked mean {attacked_mean[-1]:.4f} "
          f"multi_krum {multi_krum[-1]:.4f} bulyan {bulyan[-1]:.4f}")

    assert clean[-1] < 0.1 * clean[0]  # past the cliff
    assert np.isnan(attacked_mean[-1]) or attacked_mean[-1] > 5 * clean[-1]
    assert multi_krum[-1] < 2.0 * clean[-1] + 0.1
    assert bulyan[-1] < 2.0 * clean[-1] + 0.1
    assert mk_skipped == 0 and bu_skipped == 0
