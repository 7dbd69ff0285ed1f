"""The fused mx8 rule ops on the CPU: the fallback, its checks, the aggregator's gate."""
import pytest
import torch

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.parallel import Communicator
from draco_amd.parallel import aggregators as A
from tests import mx8_util as U
from tests.test_mx8 import BASE, CPU, _space_and_rows

RULES = {"median": ("tm", 3, 4), "trimmed_mean": ("tm", 1, 6), "normal": ("tm", 0, 7),
         "meamed": ("ma", 6, 3, 4), "phocas": ("ma", 6, 1, 6)}  # P = 7, b = 1


def column_op(kind, x, args, out):  # the mx8_ op where x is packed bytes
    name = "column_trimmed_mean" if kind == "tm" else "column_mean_around"
    getattr(ops, ("mx8_" if x.dtype == torch.uint8 else "") + name)(x, *args, out)


def test_fallback_equals_decode_then_rule():
    g = torch.Generator().manual_seed(1)
    packed = torch.randint(0, 256, (7, U.chunk_bytes(320)), generator=g, dtype=torch.uint8)
    x = torch.from_numpy(U.decode(packed.numpy(), 320))
    for kind, *args in RULES.values():
        got, ref = torch.empty(320), torch.empty(320)
        column_op(kind, x, args, ref)
        column_op(kind, packed, args, got)
        assert U.same_values(got, ref)


def test_fallback_rejections():
    u8, out = torch.zeros(65 * 80, dtype=torch.uint8), torch.zeros(128)
    p2, o64 = u8[:160].view(2, 80), out[:64]
    for packed, o, lo in ((u8.view(65, 80), o64, 0), (u8[:192].view(2, 96), o64, 0),
                          (u8[:224].view(2, 112), out[:96], 0), (p2.int(), o64, 0),
                          (p2, o64.double(), 0), (p2, out[::2], 0), (p2, o64, 1)):
        with pytest.raises(ValueError):
            ops.mx8_column_trimmed_mean(packed, lo, 1, o)
        with pytest.raises(ValueError):
            ops.mx8_column_mean_around(packed, 1, lo, 1, o)
    ops.mx8_column_trimmed_mean(u8[:0].view(2, 0), 0, 1, out[:0])  # chunk = 0


@pytest.mark.parametrize("mode", list(RULES))
@pytest.mark.parametrize("kw", [{}, {"pre_aggregation": "nnm"},
                                {"err_mode": "alie", "attack_param": 1.0}])
def test_aggregator_gate(mode, kw):
    """No fp32 block on the packed path, one behind nnm or alie; the same output either way."""
    space, rows = _space_and_rows(1, 7)
    cfg = Config(**{**BASE, "mode": mode, **kw})
    agg = A.build_baseline_aggregator(cfg, Communicator(0, 1, CPU), space, 7)
    if "err_mode" in kw:  # the trainer attaches it
        from draco_amd.coding.collusion import Collusion
        agg.collusion = Collusion(1.0, -1.0)
    out = agg.aggregate(rows.clone(), step=0).clone()
    assert (agg._recv32 is None) == (not kw)
    x = U.roundtrip(rows, space.shard)
    if agg.mixing is not None:
        agg.mixing(x)  # alie with no rows set for the step changes nothing
    kind, *args = RULES[mode]
    ref = torch.empty(space.d_pad)
    column_op(kind, x, args, ref)
    assert U.same_values(out, ref)
