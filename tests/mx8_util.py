"""Shared by tests/test_mx8.py and tests/test_mx8_gpu.py: the MXFP8 wire format stated in
plain numpy/fp64 (a 256-entry code table, a nearest-code search with ties to even, the
scale rule), and the inputs of the exact decode and encode tests."""
import numpy as np
import torch

_c = np.arange(256)
_e, _m = (_c >> 3) & 15, _c & 7
TABLE = np.where(_e > 0, (1 + _m / 8.0) * 2.0 ** (_e - 7.0), _m * 2.0 ** -9)  # fp64, exact
TABLE[(_c & 0x7F) == 0x7F] = np.nan
TABLE[128:] *= -1.0
POS = TABLE[:0x7F]  # the 127 non-negative finite code values, ascending


def chunk_bytes(chunk):
    return chunk + -(-(chunk // 32) // 16) * 16


def encode(x, chunk):
    """x: (n,) float32 numpy -> the packed uint8 row, by the definition."""
    x64 = x.astype(np.float64).reshape(-1, 32)
    fin = np.isfinite(x64)
    amax = np.where(fin, np.abs(x64), 0.0).max(axis=1)
    e = np.full(len(amax), -117)
    for b in np.nonzero(amax > 0)[0]:  # the smallest e with amax / 2^e <= 448
        k = int(np.ceil(np.log2(amax[b] / 448.0))) - 1
        while amax[b] / 2.0 ** k > 448.0:
            k += 1
        e[b] = max(k, -117)
    y = np.abs(np.where(fin, x64, 0.0)) / 2.0 ** e[:, None].astype(np.float64)  # exact in fp64
    hi = np.minimum(np.searchsorted(POS, y, side="left"), 126)  # POS[hi] >= y
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = y - POS[lo], POS[hi] - y
    code = np.where((dlo < dhi) | ((dlo == dhi) & (lo % 2 == 0)), lo, hi)
    code = np.where(fin, code, 0x7F) | (np.signbit(x64) * 0x80)
    rec = np.zeros((x.size // chunk, chunk_bytes(chunk)), dtype=np.uint8)
    rec[:, :chunk] = code.reshape(-1, chunk)
    rec[:, chunk: chunk + chunk // 32] = (e + 127).reshape(-1, chunk // 32)
    return rec.reshape(-1)


def decode(packed, chunk):
    """packed: (P, chunk_bytes) uint8 numpy -> (P, chunk) float32, by the definition."""
    s = packed[:, chunk: chunk + chunk // 32].astype(np.int64)
    scale = np.where(s == 255, np.nan, 2.0 ** (np.maximum(s, 10) - 127.0))
    with np.errstate(over="ignore", invalid="ignore"):
        return (TABLE[packed[:, :chunk]] * np.repeat(scale, 32, axis=1)).astype(np.float32)


def pack(o, x, chunk):
    """o.mx8_pack of x (o: draco_amd.ops or its fallback) into a fresh buffer."""
    out = torch.empty(x.numel() // chunk * chunk_bytes(chunk), dtype=torch.uint8, device=x.device)
    o.mx8_pack(x, out, chunk)
    return out


def roundtrip(x, chunk):
    """(P, n) fp32 tensor -> decode(encode(.)) per row, by the definition."""
    out = [decode(encode(r.numpy(), chunk).reshape(-1, chunk_bytes(chunk)), chunk).reshape(-1)
           for r in x]
    return torch.from_numpy(np.stack(out))


def same_values(a, b):
    """Bit for bit, with NaN compared as NaN-ness."""
    a, b = a.cpu(), b.cpu()
    an, bn = torch.isnan(a), torch.isnan(b)
    return torch.equal(an, bn) and torch.equal(a.view(torch.int32)[~an], b.view(torch.int32)[~bn])


DECODE_SCALES = (0, 9, 10, 127, 246, 247, 254, 255)


def decode_case():
    """(32, 80) uint8: all 256 codes x DECODE_SCALES as 64-element rows (chunk 64)."""
    rows = np.zeros((len(DECODE_SCALES) * 4, 80), dtype=np.uint8)
    for i, s in enumerate(DECODE_SCALES):
        rows[4 * i: 4 * i + 4, :64] = np.arange(256).reshape(4, 64)
        rows[4 * i: 4 * i + 4, 64:66] = s
    return rows


def _ulp(v, k):
    return (v.view(np.int32) + k).view(np.float32)


def encode_case():
    """(n,) float32, n % 64 == 0.  For block scales 2^-117, 2^0, 2^119: every positive code
    value, every midpoint of adjacent codes, one fp32 ulp either side of it, and the
    negatives, in blocks whose last element (448 * scale) fixes the scale; then the special
    blocks."""
    mids = (POS[:-1] + POS[1:]) / 2
    blocks = []
    for e in (-117, 0, 119):
        m = (mids * 2.0 ** e).astype(np.float32)  # exact: at most 5 significant bits
        v = np.concatenate([(POS * 2.0 ** e).astype(np.float32), m, _ulp(m, 1), _ulp(m, -1)])
        v = np.concatenate([v, -v])
        v = np.concatenate([v, np.zeros(-len(v) % 31, dtype=np.float32)]).reshape(-1, 31)
        top = np.full((len(v), 1), 448.0 * 2.0 ** e, dtype=np.float32)
        blocks.append(np.concatenate([v, top], axis=1))
    one = np.ones(32, dtype=np.float32)
    edge = np.stack([one * 0.3, one * 0.3])  # the e + 1 boundary: amax 1.75 and one ulp above
    edge[:, 5] = np.array([0x3FE00000, 0x3FE00001], dtype=np.int32).view(np.float32)
    assert edge.max(axis=1).view(np.int32).tolist() == [0x3FE00000, 0x3FE00001]
    special = np.stack([
        edge[0], edge[1],
        one * 0.0,
        np.where(np.arange(32) % 2 == 0, -0.0, 0.5).astype(np.float32),
        np.where(np.arange(32) == 3, np.inf, np.linspace(-3e-5, 7e-5, 32)).astype(np.float32),
        one * np.nan,
        np.linspace(-1e-39, 1e-39, 32).astype(np.float32),  # fp32 subnormals
        np.where(np.arange(32) % 3 == 0, -np.inf, np.where(np.arange(32) % 3 == 1, -np.nan, 2.5)
                 ).astype(np.float32),
    ])
    x = np.concatenate(blocks + [special]).reshape(-1)
    return np.concatenate([x, np.zeros(-len(x) % 64, dtype=np.float32)])


def random_case(n, seed, special=False):
    """Normal values times per-block powers of two in 2^-30 .. 2^30; with special, also
    NaN / +-Inf elements and zero blocks."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n // 32, 32, generator=g)
    x = x * 2.0 ** torch.randint(-30, 31, (n // 32, 1), generator=g).float()
    if special:
        x[torch.rand(x.shape, generator=g) < 0.05] = float("nan")
        x[torch.rand(x.shape, generator=g) < 0.03] = float("inf")
        x[torch.rand(x.shape, generator=g) < 0.03] = float("-inf")
        x[torch.rand(n // 32, generator=g) < 0.2] = 0.0
    return x.reshape(-1)
