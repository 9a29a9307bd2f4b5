"""Numpy restatement of the FP8 gather direction (include/brainevent_amd.h, "Gather direction" of the FP8 CSR block) and the
constants the GPU cases are sized by.  For m stored rows over k ids and a bool vector s[k]:

    R_i    = sum over the stored entries e of row i with s[indices[e]] set, of Q(codes[e])      (int64)
    out[i] = f32(f64(R_i) * ldexp(f64(f32(scale)), -E))

``Q`` and the finish are ``csr_f8_cases.q_table`` / ``finish``: the same as the scatter direction's, which is why the two
directions — and every route of each — agree bit for bit.  Expected values come from here, never from a device kernel.
"""
import numpy as np

import csr_f8_cases as K

# what the GPU cases are sized by (tests/test_csr_f8_gather_cpu.py ties them to csrc/be_csr_f8_gather.hip and be_convert.hip)
LPR_MAX_ROW = {2: 8, 4: 20, 8: 45, 16: 100, 32: 200}      # lanes per row -> largest average row length nnz // m; 64 lanes above
LPRS = (2, 4, 8, 16, 32, 64)
QUADS = 2                                      # passes of a row a lane has in flight per trip of the walk
THREADS, GRID_CAP = 1024, 512                  # rows of one grid trip at LPR lanes per row: GRID_CAP * THREADS // LPR
LDS_BITMAP_BYTES = 150 * 1024                  # a packed bitmap larger than this is read from global memory
FILL_LPR_MAX_ROW = {1: 2, 4: 8, 16: 48}        # k_t_fill: lanes per row -> largest average row; 64 lanes above
FILL_THREADS, FILL_GRID_CAP = 256, 256 * 16


def lpr_of(avg: int) -> int:
    for lpr, top in LPR_MAX_ROW.items():
        if avg <= top:
            return lpr
    return 64


def pass_of(lpr: int) -> int:
    """Entries of a row that its lanes read per pass (4 consecutive entries per lane)."""
    return 4 * lpr


def trip_rows(lpr: int) -> int:
    return GRID_CAP * THREADS // lpr


def avg_for(lpr: int) -> int:
    """An average row length that selects ``lpr`` lanes per row (the top of its range; one past the last range for 64)."""
    return LPR_MAX_ROW.get(lpr, max(LPR_MAX_ROW.values()) + 1)


def fill_lpr_of(avg: int) -> int:
    for lpr, top in FILL_LPR_MAX_ROW.items():
        if avg <= top:
            return lpr
    return 64


def row_sums(codes, indices, indptr, active, fmt: str) -> np.ndarray:
    """int64[m]: R over the stored rows for the bool vector ``active`` [k]."""
    q = K.q_table(fmt)
    active = np.asarray(active, dtype=bool)
    indptr = np.asarray(indptr, dtype=np.int64)
    contrib = np.where(active[indices], q[codes], 0).astype(np.int64) if len(indices) else np.zeros(0, np.int64)
    csum = np.concatenate([[0], np.cumsum(contrib, dtype=np.int64)])
    return csum[indptr[1:]] - csum[indptr[:-1]]


def expected_gather(codes, indices, indptr, active, fmt: str, scale=1.0) -> np.ndarray:
    """f32 [m] for one bool vector [k], or [nb, m] for ``active`` of shape [nb, k]."""
    active = np.asarray(active, dtype=bool)
    if active.ndim == 2:
        return np.stack([expected_gather(codes, indices, indptr, a, fmt, scale) for a in active])
    return K.finish(row_sums(codes, indices, indptr, active, fmt), scale, fmt)


def transposed(codes, indices, indptr, k: int):
    """The CSR arrays of the transpose (k rows): entries ordered by column, stably."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int32), np.diff(indptr))
    order = np.argsort(indices, kind='stable')
    tptr = np.zeros(k + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=k), out=tptr[1:])
    return codes[order], rows[order].astype(np.int32), tptr.astype(np.int32)


def fixed_rows(m: int, k: int, row_len: int, fmt: str, seed: int):
    """``m`` rows of exactly ``row_len`` random entries (``indptr`` is the arithmetic one)."""
    rng = np.random.default_rng(seed)
    n = m * row_len
    codes = rng.choice(K.finite_codes(fmt), n).astype(np.uint8)
    indices = rng.integers(0, k, n).astype(np.int32)
    return codes, indices, (np.arange(m + 1, dtype=np.int64) * row_len)


def rows_of_lengths(lens, k: int, fmt: str, seed: int):
    """Rows of the given lengths, random unsorted columns (duplicates included), random finite codes."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    codes = rng.choice(K.finite_codes(fmt), n).astype(np.uint8)
    indices = rng.integers(0, k, n).astype(np.int32)
    indptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    return codes, indices, indptr
