"""Shared by tests/test_mx4.py and tests/test_mx4_gpu.py: the MXFP4 wire format stated in
plain numpy/fp64 (the grid, a search for the grid neighbours, the scale rule, the hash)."""
import numpy as np
import torch

from tests.mx8_util import same_values  # noqa: F401 - bit for bit, NaN as NaN-ness

GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])  # the magnitudes of codes 0..7
TABLE = np.concatenate([GRID, -GRID])


def chunk_bytes(chunk):
    return chunk // 2 + -(-(chunk // 32) // 16) * 16


def _h(a):
    a = a ^ (a >> np.uint32(16))
    a = a * np.uint32(0x7FEB352D)
    a = a ^ (a >> np.uint32(15))
    a = a * np.uint32(0x846CA68B)
    return a ^ (a >> np.uint32(16))


def encode(x, chunk, seed=None):
    """x: (n,) float32 numpy -> the packed uint8 row, by the definition."""
    x64 = x.astype(np.float64).reshape(-1, 32)
    fin = np.isfinite(x64)
    mag = np.abs(np.where(fin, x64, 0.0))
    amax = mag.max(axis=1)
    e = np.full(len(amax), -125)
    for b in np.nonzero(amax > 0)[0]:  # the smallest e with amax / 2^e <= 6
        k = int(np.ceil(np.log2(amax[b] / 6.0))) - 1
        while amax[b] / 2.0 ** k > 6.0:
            k += 1
        e[b] = max(k, -125)
    t = mag / 2.0 ** e[:, None].astype(np.float64)  # exact in fp64
    t = np.where(t < 2.0 ** -126, 0.0, t)
    lo = np.searchsorted(GRID, t, side="right") - 1  # GRID[lo] <= t
    hi = np.minimum(lo + 1, 7)
    p_up = (t - GRID[lo]) / np.where(hi > lo, GRID[hi] - GRID[lo], 1.0)  # exact in fp64
    if seed is None:
        up = (p_up > 0.5) | ((p_up == 0.5) & (lo % 2 == 1))
    else:
        with np.errstate(over="ignore"):
            key = _h(np.uint32(seed & 0xFFFFFFFF) ^ _h(np.uint32(((seed >> 32) + 0x9E3779B9) & 0xFFFFFFFF)))
            r = _h(np.arange(x.size, dtype=np.uint32) ^ key) >> np.uint32(8)
        up = r.reshape(-1, 32).astype(np.float64) < p_up * 2.0 ** 24
    code = (lo + up) | (np.signbit(x64) * 8)
    code = code.reshape(-1, chunk // 2, 2)
    rec = np.zeros((x.size // chunk, chunk_bytes(chunk)), dtype=np.uint8)
    rec[:, : chunk // 2] = code[:, :, 0] | (code[:, :, 1] << 4)
    s = np.where(fin.all(axis=1), e + 127, 255)
    rec[:, chunk // 2: chunk // 2 + chunk // 32] = s.reshape(-1, chunk // 32)
    return rec.reshape(-1)


def decode(packed, chunk):
    """packed: (P, chunk_bytes) uint8 numpy -> (P, chunk) float32, by the definition."""
    b = packed[:, : chunk // 2]
    codes = np.stack([b & 15, b >> 4], axis=2).reshape(len(packed), chunk)
    s = packed[:, chunk // 2: chunk // 2 + chunk // 32].astype(np.int64)
    scale = np.where(s == 255, np.nan, 2.0 ** (np.maximum(s, 2) - 127.0))
    with np.errstate(over="ignore", invalid="ignore"):
        return (TABLE[codes] * np.repeat(scale, 32, axis=1)).astype(np.float32)


def pack(o, x, chunk, seed=None):
    """o.mx4_pack of x (o: draco_amd.ops or its fallback) into a fresh buffer."""
    out = torch.empty(x.numel() // chunk * chunk_bytes(chunk), dtype=torch.uint8, device=x.device)
    o.mx4_pack(x, out, chunk, seed)
    return out


def roundtrip(x, chunk, seed=None):
    """(P, n) fp32 tensor -> decode(encode(.)) per row, by the definition."""
    out = [decode(encode(r.numpy(), chunk, seed).reshape(-1, chunk_bytes(chunk)), chunk).reshape(-1)
           for r in x]
    return torch.from_numpy(np.stack(out))


DECODE_SCALES = (0, 1, 2, 3, 127, 253, 254, 255)


def decode_case():
    """(8, 48) uint8, chunk 64: every code in either nibble, one row per DECODE_SCALES."""
    rows = np.zeros((len(DECODE_SCALES), chunk_bytes(64)), dtype=np.uint8)
    k = np.arange(32) % 16
    rows[:, :32] = k | ((15 - k) << 4)
    rows[:, 32:34] = np.array(DECODE_SCALES, dtype=np.uint8)[:, None]
    return rows


def _ulp(v, k):
    return (v.view(np.int32) + k).view(np.float32)


def encode_case():
    """(n,) float32, n % 64 == 0.  For block scales 2^-125 (s = 2), 2^0 and 2^126 (s = 253,
    where fp32 ends at t < 4): every grid value, every midpoint of neighbours, one fp32 ulp
    either side of each, and the negatives, as far as they fit under the block's last element
    (6 or 3.5 times the scale), which fixes the scale; then the special blocks."""
    mids = (GRID[:-1] + GRID[1:]) / 2
    blocks = []
    for e, top in ((-125, 6.0), (0, 6.0), (126, 3.5)):
        p = np.concatenate([GRID, mids])
        p = (p[p <= top] * 2.0 ** e).astype(np.float32)  # exact: at most 3 significant bits
        v = np.concatenate([p, _ulp(p[1:], 1), _ulp(p[1:], -1)])
        v = v[v <= np.float32(top * 2.0 ** e)]
        v = np.concatenate([v, -v])
        v = np.concatenate([v, np.zeros(-len(v) % 31, dtype=np.float32)]).reshape(-1, 31)
        top = np.full((len(v), 1), top * 2.0 ** e, dtype=np.float32)
        blocks.append(np.concatenate([v, top], axis=1))
    one = np.ones(32, dtype=np.float32)
    edge = np.stack([one * 0.3, one * 0.3])  # the e + 1 boundary: amax 1.5 and one ulp above
    edge[:, 5] = np.array([0x3FC00000, 0x3FC00001], dtype=np.int32).view(np.float32)
    idx = np.arange(32)
    special = np.stack([
        edge[0], edge[1],
        one * 0.0,
        np.where(idx % 2 == 0, -0.0, 0.5).astype(np.float32),
        np.where(idx == 3, 1.0, np.linspace(-0.04, 0.04, 32)).astype(np.float32),  # round to zero
        np.linspace(-1e-39, 1e-39, 32).astype(np.float32),  # fp32 subnormals, s = 2
        np.where(idx == 3, 1e-30, np.linspace(-1e-39, 1e-39, 32)).astype(np.float32),
        np.where(idx == 3, 3e38, np.linspace(-2e-38, 1e-39, 32)).astype(np.float32),  # t < 2^-126
        np.where(idx == 3, np.nan, np.linspace(-3e-5, 7e-5, 32)).astype(np.float32),
        np.where(idx == 7, np.inf, np.linspace(-3.0, 7.0, 32)).astype(np.float32),
        np.where(idx % 3 == 0, -np.inf, np.where(idx % 3 == 1, -np.nan, 2.5)).astype(np.float32),
    ])
    x = np.concatenate(blocks + [special]).reshape(-1)
    return np.concatenate([x, np.zeros(-len(x) % 64, dtype=np.float32)])


def random_case(n, seed, special=False, span=30):
    """Normal values times per-block powers of two in 2^-span .. 2^span; with special, also
    NaN / +-Inf elements and zero blocks."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n // 32, 32, generator=g)
    x = x * 2.0 ** torch.randint(-span, span + 1, (n // 32, 1), generator=g).float()
    if special:
        for p, v in ((0.01, "nan"), (0.005, "inf"), (0.005, "-inf")):
            x[torch.rand(x.shape, generator=g) < p] = float(v)
        x[torch.rand(n // 32, generator=g) < 0.2] = 0.0
    return x.reshape(-1)
