"""Numpy restatement of ``events @ Float8CSR`` (include/brainevent_amd.h, "FP8 weights for the event-driven CSR products") and the
matrices the GPU tests run: the only source of expected values.

    Q(c)   = decode(c) * 2^E                 E = 9 (e4m3) / 16 (e5m2); an exact integer for every finite code
    R_j    = sum over the active rows i, over the stored entries e of row i with indices[e] == j, of Q(codes[e])     (int64)
    out[j] = f32(f64(R_j) * ldexp(f64(f32(scale)), -E))

The decode table comes from torch's CPU FP8 -> f64 conversion; nothing here is compared with a device kernel of torch.
"""
import functools

import numpy as np
import torch

E = {'e4m3': 9, 'e5m2': 16}
DTYPE = {'e4m3': torch.float8_e4m3fn, 'e5m2': torch.float8_e5m2}
FMT_CODE = {'e4m3': 0, 'e5m2': 1}
NONFINITE_MASK = {'e4m3': 0x7f, 'e5m2': 0x7c}
Q_MAX = {'e4m3': 229376, 'e5m2': 3758096384}
# what the GPU cases are sized by (tests/test_csr_f8_cpu.py ties them to the source text)
MAX_ROW, MAX_SLICES, MAX_WIDTH = 16384, 1024, 20000
LANE_GROUP = 4                       # entries per lane-group
WAVE_PASS = 64 * LANE_GROUP          # entries of a block a wave decodes in one pass
LPB_VARIANTS = {8: 10, 16: 30, 0: 100}      # lanes per block -> a block_hint that selects it (thresholds 18 / 43)


def finite_codes(fmt: str) -> np.ndarray:
    c = np.arange(256, dtype=np.uint8)
    m = NONFINITE_MASK[fmt]
    return c[(c & m) != m]


@functools.lru_cache(maxsize=None)
def q_table(fmt: str) -> np.ndarray:
    """int64[256]: Q of every code (0 at the non-finite codes, which no case uses)."""
    dec = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(DTYPE[fmt]).to(torch.float64).numpy()
    q = np.zeros(256, dtype=np.int64)
    for c in finite_codes(fmt):
        v = dec[c] * 2.0 ** E[fmt]
        assert v == np.floor(v)
        q[c] = int(v)
    return q


def column_sums(codes, indices, indptr, active, k: int, fmt: str) -> np.ndarray:
    """int64[k]: R over the rows where ``active`` (bool [m]) is set."""
    q = q_table(fmt)
    R = np.zeros(k, dtype=np.int64)
    for i in np.flatnonzero(active):
        b, e = int(indptr[i]), int(indptr[i + 1])
        np.add.at(R, indices[b:e], q[codes[b:e]])
    return R


def finish(R: np.ndarray, scale, fmt: str) -> np.ndarray:
    inv = np.ldexp(np.float64(np.float32(scale)), -E[fmt])
    return (R.astype(np.float64) * inv).astype(np.float32)


def expected(codes, indices, indptr, active, k: int, fmt: str, scale=1.0) -> np.ndarray:
    """f32 [k] for one event vector, or [nb, k] for ``active`` of shape [nb, m]."""
    active = np.asarray(active, dtype=bool)
    if active.ndim == 2:
        return np.stack([expected(codes, indices, indptr, a, k, fmt, scale) for a in active])
    return finish(column_sums(codes, indices, indptr, active, k, fmt), scale, fmt)


def active_of(spikes: np.ndarray) -> np.ndarray:
    """The activity rule: float spikes > 0 (a negative or NaN value is inactive), everything else != 0."""
    return spikes > 0 if spikes.dtype.kind == 'f' else spikes != 0


def pack_bits(active: np.ndarray) -> np.ndarray:
    """uint32 words of a bool vector (bit i % 32 of word i // 32), or of every row of a matrix."""
    active = np.asarray(active, dtype=bool)
    if active.ndim == 2:
        return np.stack([pack_bits(a) for a in active])
    n = active.shape[0]
    pad = np.zeros((n + 31) // 32 * 32, dtype=bool)
    pad[:n] = active
    return np.packbits(pad.reshape(-1, 32)[:, ::-1], axis=1).view('>u4').astype(np.uint32).reshape(-1)


def from_rows(rows, k: int):
    """CSR arrays of a list of ``(columns, codes)`` pairs."""
    indptr = np.zeros(len(rows) + 1, dtype=np.int32)
    for i, (c, _) in enumerate(rows):
        indptr[i + 1] = indptr[i] + len(c)
    idx = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows]) if rows else np.zeros(0, np.int32)
    cod = np.concatenate([np.asarray(w, dtype=np.uint8) for _, w in rows]) if rows else np.zeros(0, np.uint8)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < k)
    return cod, idx.astype(np.int32), indptr


def random_matrix(m: int, k: int, fmt: str, seed: int, max_len: int = 40):
    """Rows of random length (some empty), columns unsorted and with duplicates, every entry a random finite code."""
    rng = np.random.default_rng(seed)
    fc = finite_codes(fmt)
    rows = []
    for i in range(m):
        n = 0 if rng.random() < 0.2 else int(rng.integers(1, max_len + 1))
        cols = rng.integers(0, k, n)
        if n >= 4:
            cols[1] = cols[0]                       # a duplicated column (delta 0 once sorted)
        rows.append((cols, rng.choice(fc, n)))
    return from_rows(rows, k)
