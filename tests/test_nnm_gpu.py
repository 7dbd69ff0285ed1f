"""ops.mix_rows_ on the MI355X: the MFMA kernel (k_mix_rows) against the fp64 loop of
tests/nnm_util.py within its derived bound, and nnm + multi_krum end to end.  A wave owns
128 consecutive columns, 16 bytes per lane per row: n runs over one float4, one float4
below / at / above that width and two widths plus 4 (a second wave); W is zero-padded to
one 32x32 tile: P runs over 1, 2, 3 and the tile's edge 31, 32.
"""
import pytest
import torch
import torch.nn as nn

from tests.bulyan_util import separated_rows
from tests.nnm_util import EPS, check_mix, mix_case, mix_ref, skip_sets

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops.native import available

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"
SENTINEL = -12345.0


@pytest.mark.parametrize("kind", ["none", "first", "last", "all_but_one"])
@pytest.mark.parametrize("n", [4, 124, 128, 132, 260])
@pytest.mark.parametrize("P", [1, 2, 3, 31, 32])
def test_kernel_within_bound_of_fp64_loop(P, n, kind):
    skip = skip_sets(P)[kind]
    x, w = mix_case(P, n, skip, seed=1000 * P + n)
    before = torch.full((64,), SENTINEL, device=DEV)  # an unrelated earlier allocation
    runs = []
    for _ in range(2):
        buf = torch.full((P * n + 64,), SENTINEL, device=DEV)  # 64 guard floats behind
        y = buf[: P * n].view(P, n)
        y.copy_(x)
        ops.mix_rows_(y, w.to(DEV), skip)
        torch.cuda.synchronize()
        assert bool((buf[P * n:] == SENTINEL).all()) and bool((before == SENTINEL).all())
        runs.append(y.cpu())
    check_mix(runs[0], x, w, skip, (P, n, kind))
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))


def test_host_rejections():
    def call(P, n, skip=(), x=None, w=None):
        x = torch.zeros(P, n, device=DEV) if x is None else x
        ops.mix_rows_(x, torch.zeros(P, P, device=DEV) if w is None else w, skip)
    for bad in (dict(P=33, n=8), dict(P=4, n=6), dict(P=4, n=8, skip=[4]),
                dict(P=4, n=8, x=torch.zeros(8, 4, device=DEV).t()),
                dict(P=4, n=8, w=torch.zeros(4, 5, device=DEV)),
                dict(P=4, n=8, w=torch.zeros(4, 4))):
        with pytest.raises(RuntimeError):
            call(**bad)
    call(4, 0)  # n = 0 and P = 0: no launch
    call(0, 8)
    torch.cuda.synchronize()


def test_gpu_nnm_multi_krum_matches_cpu():
    """P = 9, f = 1, row 4 non-finite: both devices exclude row 4 and Multi-Krum (m = 8)
    averages the 8 finite mixed rows, whatever their score order.  A mixed value is within
    b = mix_ref's bound of exact on either device, so the devices differ by at most 2b per
    row; the mean averages that and adds its own 2*(8+4)*2^-24 * mean|y| per device."""
    from draco_amd.config import Config
    from draco_amd.parallel import Communicator, FlatSpace
    from draco_amd.parallel.aggregators import build_baseline_aggregator
    P, bad = 9, 4
    cfg = Config(approach="baseline", mode="multi_krum", worker_fail=1, pre_aggregation="nnm")
    outs = {}
    for dev in ("cpu", DEV):
        device = torch.device(dev)
        torch.manual_seed(5)
        model = nn.Sequential(nn.Linear(300, 40), nn.Linear(40, 9)).to(device)
        space = FlatSpace(model, 1, device)
        rows = torch.zeros(P, space.d_pad)  # the pad tail is always zero in production
        rows[:, : space.d] = torch.from_numpy(separated_rows(P, space.d, [bad], 3, "nan"))
        agg = build_baseline_aggregator(cfg, Communicator(0, 1, device), space, P)
        payload = space.alloc_payload(P)
        payload.copy_(rows.to(device))
        outs[dev] = agg.aggregate(payload, step=0).cpu()
        assert bool(torch.isnan(payload[bad]).all())
    good = [p for p in range(P) if p != bad]
    W = torch.nan_to_num(agg.mixing.last_weights.cpu(), nan=0.0)
    y, b = mix_ref(rows, W, [bad])
    bound = 2 * b[good].mean(dim=0) + 2 * 2 * (8 + 4) * EPS * y[good].abs().mean(dim=0)
    diff = (outs[DEV].double() - outs["cpu"].double()).abs()
    assert bool(torch.isfinite(outs[DEV]).all()) and bool((diff <= bound).all())
    assert bool((outs[DEV][space.d:] == 0).all())
