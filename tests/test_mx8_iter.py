"""ops.mx8_clip_step_ / ops.mx8_weiszfeld_step on the CPU: fallbacks, checks, aggregator gate."""
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.parallel import Communicator, FlatSpace
from draco_amd.parallel import aggregators as A
from tests import mx8_util as U
from tests.test_mx8 import BASE, CPU

SEG, P, CHUNK = [3, 3, 70, 129, 321, 570], 7, 576  # an empty segment, gaps at both ends


def test_fallbacks_equal_decode_then_op():
    g = torch.Generator().manual_seed(1)
    packed = torch.randint(0, 256, (P, U.chunk_bytes(CHUNK)), generator=g, dtype=torch.uint8)
    x, seg = torch.from_numpy(U.decode(packed.numpy(), CHUNK)), torch.tensor(SEG)
    w = torch.rand(P, generator=g) / P
    w[2] = 0.0
    v = torch.randn(CHUNK, generator=g)
    v_ref = v.clone()
    d2, d2_ref = ops.mx8_clip_step_(packed, v, w), ops.clip_step_(x, v_ref, w)
    assert U.same_values(v, v_ref) and U.same_values(d2, d2_ref)
    ws = torch.rand(P, len(SEG) - 1, generator=g)
    z, z_ref = torch.full((CHUNK,), -5.0), torch.full((CHUNK,), -5.0)
    part = ops.mx8_weiszfeld_step(packed, ws, seg, z)
    ops.segment_weighted_mean(x, ws, seg, z_ref)
    assert U.same_values(z, z_ref) and U.same_values(part, ops.segment_sqdist(x, z_ref, seg))
    assert bool((z[:3] == -5.0).all() and (z[570:] == -5.0).all())


def test_fallback_rejections():
    u8, f = torch.zeros(65 * 80, dtype=torch.uint8), torch.zeros(128)
    p2, seg = u8[:160].view(2, 80), torch.tensor([0, 64])
    cases = [(u8.view(65, 80), f[:64], torch.zeros(65), torch.zeros(65, 1)),    # P = 65
             (u8[:192].view(2, 96), f[:64], torch.zeros(2), torch.zeros(2, 1)),  # record length
             (p2.int(), f[:64], torch.zeros(2), torch.zeros(2, 1)),              # dtype
             (p2, f[:64], torch.zeros(3), torch.zeros(2, 2)),                    # w shape
             (p2, f, torch.zeros(2), torch.zeros(2, 1))]                         # v / z length
    for packed, vz, w, ws in cases:
        with pytest.raises(ValueError):
            ops.mx8_clip_step_(packed, vz, w)
        with pytest.raises(ValueError):
            ops.mx8_weiszfeld_step(packed, ws, seg, vz)
    assert ops.mx8_clip_step_(u8[:0].view(2, 0), f[:0], torch.zeros(2)).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("mode", ["geometric_median", "centered_clip"])
@pytest.mark.parametrize("kw", [{}, {"pre_aggregation": "nnm"}])
def test_aggregator_gate(mode, kw):
    """No fp32 block on the packed path, one behind nnm; the fp32 wire's output on decode(encode(.))."""
    torch.manual_seed(7)
    space = FlatSpace(nn.Linear(50, 10), 1, CPU)  # d = 510: the pad tail is not empty
    rows = torch.zeros(P, space.d_pad)
    rows[:, : space.d] = torch.randn(P, space.d) * 2.0 ** torch.randint(-8, 8, (P, 1)).float()

    def build(**wire):
        cfg = Config(**{**BASE, "mode": mode, **kw, **wire})
        return A.build_baseline_aggregator(cfg, Communicator(0, 1, CPU), space, P)
    agg, plain = build(), build(compress_grad="none")
    out = agg.aggregate(rows.clone(), step=0).clone()
    assert (agg._recv32 is None) == (not kw)
    ref = plain.aggregate(U.roundtrip(rows, space.shard), step=0)
    if mode == "centered_clip":
        assert U.same_values(out, ref)
    else:
        assert float((out - ref).abs().max()) <= 1e-3 * float(ref.abs().max())
