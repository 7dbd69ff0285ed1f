"""ops.mx8_segment_gram / ops.mx8_segment_mean_around on the CPU: the fallbacks against
decode-then-op, their checks, and the gate in the Multi-Krum / Bulyan aggregators."""
import pytest
import torch

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.parallel import Communicator
from draco_amd.parallel import aggregators as A
from tests import mx8_util as U
from tests.bulyan_util import random_sel
from tests.test_mx8 import BASE, CPU, _space_and_rows

SEG = torch.tensor([3, 3, 70, 129, 321, 570])  # chunk 576: the GPU tests' table
PLANS = {"multi_krum": (6, 6, 0, 6), "bulyan": (5, 3, 2, 3)}  # P = 7, f = 1: (T, keep, clo, chi)


def test_fallbacks_equal_decode_then_op():
    g = torch.Generator().manual_seed(1)
    packed = torch.randint(0, 256, (7, U.chunk_bytes(576)), generator=g, dtype=torch.uint8)
    x = torch.from_numpy(U.decode(packed.numpy(), 576))
    assert U.same_values(ops.mx8_segment_gram(packed, SEG), ops.segment_gram(x, SEG))
    for T, keep, clo, chi in PLANS.values():
        sel, got, ref = random_sel(5, 7, T, seed=T), torch.empty(576), torch.empty(576)
        ops.segment_mean_around(x, sel, SEG, keep, clo, chi, ref)
        ops.mx8_segment_mean_around(packed, sel, SEG, keep, clo, chi, got)
        assert U.same_values(got, ref)


def test_fallback_rejections():
    u8, out, sel = torch.zeros(33 * 80, dtype=torch.uint8), torch.zeros(64), torch.zeros(1, 2).long()
    seg, p2 = torch.tensor([0, 64]), u8[:160].view(2, 80)
    for packed in (u8.view(33, 80), u8[:192].view(2, 96), p2.int(), u8[:160]):  # P, length, dtype
        with pytest.raises(ValueError):
            ops.mx8_segment_gram(packed, seg)
        with pytest.raises(ValueError):
            ops.mx8_segment_mean_around(packed, sel, seg, 1, 0, 1, out)
    for s, o, keep in ((torch.zeros(1, 3).long(), out, 1), (sel, out.double(), 1), (sel, out, 3)):
        with pytest.raises(ValueError):  # T > P, out dtype, keep > T
            ops.mx8_segment_mean_around(p2, s, seg, keep, 0, 1, o)
    assert ops.mx8_segment_gram(u8[:0].view(2, 0), torch.tensor([0, 0])).shape == (1, 2, 2)


@pytest.mark.parametrize("mode", list(PLANS))
@pytest.mark.parametrize("kw", [{}, {"pre_aggregation": "nnm"}])
def test_aggregator_gate(mode, kw):
    """No fp32 block on the packed path, one behind nnm; the rule on the decoded rows either way."""
    space, rows = _space_and_rows(1, 7)
    agg = A.build_baseline_aggregator(Config(**{**BASE, "mode": mode, **kw}),
                                      Communicator(0, 1, CPU), space, 7)
    out = agg.aggregate(rows.clone(), step=0).clone()
    assert (agg._recv32 is None) == (not kw)
    x = U.roundtrip(rows, space.shard)
    if agg.mixing is not None:
        agg.mixing(x)
    ref = type(agg)(Communicator(0, 1, CPU), space, num_workers=7, f=1)
    assert U.same_values(out, ref.aggregate(x, step=0)) and torch.equal(agg.last_sel, ref.last_sel)
