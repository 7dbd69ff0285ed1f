"""The fused mx4 rule ops on the CPU: the fallback, its checks, the aggregator's gate."""
import pytest
import torch

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.ops import fallback as fb
from draco_amd.parallel import Communicator
from draco_amd.parallel import aggregators as A
from tests import mx4_util as U
from tests.test_mx4 import BASE, CPU, _space_and_rows
from tests.test_mx8_fused import RULES  # P = 7, b = 1


def column_op(o, kind, x, args, out):  # the mx4_ op where x is packed bytes
    name = "column_trimmed_mean" if kind == "tm" else "column_mean_around"
    getattr(o, ("mx4_" if x.dtype == torch.uint8 else "") + name)(x, *args, out)


def reference(x, kind, args):
    """The fallback fp32 column op on decoded rows; at least a third of it is finite."""
    ref = torch.empty(x.shape[1])
    column_op(fb, kind, x, args, ref)
    assert int(torch.isfinite(ref).sum()) * 3 >= ref.numel()
    return ref


def test_fallback_equals_decode_then_rule():
    g = torch.Generator().manual_seed(1)
    packed = torch.randint(0, 256, (7, U.chunk_bytes(320)), generator=g, dtype=torch.uint8)
    x = torch.from_numpy(U.decode(packed.numpy(), 320))
    for kind, *args in RULES.values():
        got = torch.empty(320)
        column_op(ops, kind, packed, args, got)
        assert U.same_values(got, reference(x, kind, args))


def test_fallback_rejections():
    u8, out = torch.zeros(65 * 48, dtype=torch.uint8), torch.zeros(128)
    p2, o64 = u8[:96].view(2, 48), out[:64]
    # P = 65, record length, chunk 96, int32 records, fp64 out, strided out, lo >= hi
    for packed, o, lo in ((u8.view(65, 48), o64, 0), (u8[:128].view(2, 64), o64, 0),
                          (u8[:128].view(2, 64), out[:96], 0), (p2.int(), o64, 0),
                          (p2, o64.double(), 0), (p2, out[::2], 0), (p2, o64, 1)):
        with pytest.raises(ValueError):
            ops.mx4_column_trimmed_mean(packed, lo, 1, o)
        with pytest.raises(ValueError):
            ops.mx4_column_mean_around(packed, 1, lo, 1, o)
    for keep in (0, 3):
        with pytest.raises(ValueError):
            ops.mx4_column_mean_around(p2, keep, 0, 1, o64)
    ops.mx4_column_trimmed_mean(u8[:0].view(2, 0), 0, 1, out[:0])  # chunk = 0
    assert {"mx4_column_trimmed_mean", "mx4_column_mean_around"} <= set(ops.__all__)


@pytest.mark.parametrize("mode", list(RULES))
@pytest.mark.parametrize("kw", [{}, {"pre_aggregation": "nnm"},
                                {"err_mode": "alie", "attack_param": 1.0}])
def test_aggregator_gate(mode, kw):
    """No fp32 block on the packed path, one behind nnm or alie; the same output either way."""
    space, rows, _ = _space_and_rows(1, 7)
    if "pre_aggregation" in kw:
        rows[0, 3] = 1.0  # nnm mixes the NaN of row 0 into every row: nothing finite is left
    cfg = Config(**{**BASE, "mode": mode, **kw})
    agg = A.build_baseline_aggregator(cfg, Communicator(0, 1, CPU), space, 7)
    if "err_mode" in kw:  # the trainer attaches it
        from draco_amd.coding.collusion import Collusion
        agg.collusion = Collusion(1.0, -1.0)
    out = agg.aggregate(rows.clone(), step=0).clone()
    assert agg.wire == "mx4" and (agg._recv32 is None) == (not kw)
    x = U.roundtrip(rows, space.shard)
    if agg.mixing is not None:
        agg.mixing(x)  # alie with no rows set for the step changes nothing
    kind, *args = RULES[mode]
    assert U.same_values(out, reference(x, kind, args))


def test_multi_krum_still_decodes():
    space, rows, _ = _space_and_rows(1, 7)
    agg = A.build_baseline_aggregator(Config(**{**BASE, "mode": "multi_krum"}),
                                      Communicator(0, 1, CPU), space, 7)
    agg.aggregate(rows.clone(), step=0)
    assert agg.wire == "mx4" and agg._recv32 is not None
