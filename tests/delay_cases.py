"""Synaptic delays restated in numpy — shared by tests/test_delay_cpu.py (which holds the restatement to a brute-force dense
evaluation) and tests/test_delay_gpu.py.  numpy only: nothing here needs a device.

The semantics: ``(ring @ D)[j] = sum_{e : col(e) = j} w_e * s_{row(e)}(age = delays[e])``, age 0 = the vector
pushed last, history before the first push silent; the stacked matrix has row ``d * m + i`` = the entries of row ``i`` with delay
``d`` in their original order, i.e. a STABLE sort of the entries by ``(delay, row)``.

Exactness.  The generator draws weights ``k / 64`` with integer ``|k| <= 64``, so every partial sum of ``N < 2^17`` of them is a
multiple of ``1/64`` below ``2^17``: 23 bits, exact in f32 (and in the 64-bit fixed point of the planned and binned routes) whatever
the order of the additions.  For f16 the weights are integers ``|k| <= 4`` and rows hold at most 32 entries; the generator then
checks that ``sum |w|`` over every output column stays ``<= 2048``, below which every integer is an f16 number.  So every product
comparison of the GPU tests is an equality."""
import numpy as np

__all__ = ['TILES', 'SPLIT_TILE', 'RING_TILE_BITS', 'SPLIT_ROWS_PER_PASS', 'split_by_delay_np', 'pack_rows_np', 'unpack_words_np',
           'ring_np', 'delayed_currents_np', 'dense_delayed_np', 'exact_case', 'row_lengths_case', 'delay_pattern']

#: the tile constants of brainevent_amd/csrc/be_delay.hip that the GPU cases are sized by (tests/test_delay_cpu.py ties them to
#: the source text)
TILES = {'kMaxDepth': 256, 'kSplitThreads': 256, 'kSplitGridCap': 4096, 'kMaskGridCap': 64, 'kRingThreads': 256, 'kRingPer': 32}
#: entries one workgroup of the split takes per step (4 waves x 64 entries)
SPLIT_TILE = TILES['kSplitThreads']
#: rows one launch of the split (and of the row-mask kernel) covers before its grid-stride loop comes round
SPLIT_ROWS_PER_PASS = TILES['kSplitGridCap'] * (TILES['kSplitThreads'] // 64)
assert SPLIT_ROWS_PER_PASS == TILES['kMaskGridCap'] * 256
#: bits of one slot that one workgroup packs (push) or scans (compaction)
RING_TILE_BITS = TILES['kRingThreads'] * TILES['kRingPer']


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def pack_rows_np(mask):
    """bool ``[r, n]`` -> uint32 ``[r, ceil(n / 32)]``: bit ``i % 32`` of word ``i // 32``."""
    mask = np.atleast_2d(np.asarray(mask, dtype=bool))
    r, n = mask.shape
    nw = (n + 31) // 32
    padded = np.zeros((r, nw * 32), dtype=np.uint64)
    padded[:, :n] = mask
    return (padded.reshape(r, nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_words_np(words, n):
    """uint32 / int32 ``[ceil(n / 32)]`` -> bool ``[nw * 32]`` (ALL the bits of the words: the caller looks past ``n`` too)."""
    w = np.asarray(words).view(np.uint32).reshape(-1)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)


def split_by_delay_np(indptr, delays, m, depth):
    """``(indptr_s, perm, row_mask)`` of the stacked matrix: a stable sort of the entries by ``(delay, row)``."""
    indptr = np.asarray(indptr, dtype=np.int64)
    delays = np.asarray(delays, dtype=np.int64).reshape(-1)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(indptr))
    key = delays * m + rows
    perm = np.argsort(key, kind='stable')
    counts = np.bincount(key, minlength=depth * m)
    indptr_s = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return indptr_s, perm.astype(np.int64), pack_rows_np((counts > 0).reshape(depth, m))


class ring_np:
    """A list-based spike history: ``age(a)`` is the vector pushed ``a`` pushes ago, silent before the first push."""

    def __init__(self, n, depth):
        self.n, self.depth, self.history = int(n), int(depth), []

    def push(self, s):
        s = np.asarray(s)
        self.history.append((s > 0) if np.issubdtype(s.dtype, np.floating) else (s != 0))

    def age(self, a):
        assert 0 <= a < self.depth
        return self.history[-1 - a] if a < len(self.history) else np.zeros(self.n, dtype=bool)

    def ids(self, ages=None, row_mask=None):
        """sorted ``a * n + i`` over the set bits, gated by ``row_mask`` (uint32 ``[depth, ceil(n / 32)]``)."""
        ages = self.depth if ages is None else ages
        out = []
        for a in range(ages):
            s = self.age(a)
            if row_mask is not None:
                s = s & unpack_words_np(row_mask[a], self.n)[:self.n]
            out.append(a * self.n + np.nonzero(s)[0])
        return np.sort(np.concatenate(out)).astype(np.int64)


def delayed_currents_np(data, indices, indptr, delays, ring, n_post):
    """f64 loop over the entries: ``out[col(e)] += w_e * s_{row(e)}(age = delays[e])``."""
    data = np.asarray(data, dtype=np.float64).reshape(-1)
    indices, delays = np.asarray(indices).reshape(-1), np.asarray(delays).reshape(-1)
    out = np.zeros(n_post, dtype=np.float64)
    for i in range(len(indptr) - 1):
        for e in range(int(indptr[i]), int(indptr[i + 1])):
            if ring.age(int(delays[e]))[i]:
                out[indices[e]] += data[0] if data.size == 1 else data[e]
    return out


def dense_delayed_np(data, indices, indptr, delays, ring, n_post, depth):
    """Brute force: ``sum_d s(t - d) @ (W (.) [delay == d])`` with dense f64 matrices (duplicates summed)."""
    data = np.asarray(data, dtype=np.float64).reshape(-1)
    indices, delays = np.asarray(indices).reshape(-1), np.asarray(delays).reshape(-1)
    m = len(indptr) - 1
    rows = np.repeat(np.arange(m), np.diff(indptr))
    vals = np.broadcast_to(data, indices.shape) if data.size == 1 else data
    out = np.zeros(n_post, dtype=np.float64)
    for d in range(depth):
        W = np.zeros((m, n_post), dtype=np.float64)
        sel = delays == d
        np.add.at(W, (rows[sel], indices[sel]), vals[sel])
        out += ring.age(d).astype(np.float64) @ W
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------
def exact_case(seed, n_pre, n_post, depth, max_row, *, dtype=np.float32, fixed_len=None, parallel=False, homo=False):
    """``(data, indices, indptr, delays)`` whose delayed products are exact in ``dtype`` (module docstring).  ``fixed_len``: every
    row has that many entries; ``parallel``: every synapse is stored twice or more, with delays of its own (parallel synapses)."""
    rng = np.random.default_rng(seed)
    f16 = np.dtype(dtype) == np.float16
    if f16:
        assert max_row <= 32
    lens = np.full(n_pre, fixed_len) if fixed_len is not None else rng.integers(0, max_row + 1, n_pre)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(indptr[-1])
    indices = rng.integers(0, n_post, nnz).astype(np.int32)
    if parallel:                      # copy the first half of every row's targets into its second half
        for i in range(n_pre):
            b, e = indptr[i], indptr[i + 1]
            h = (e - b) // 2
            indices[b + h:b + 2 * h] = indices[b:b + h]
    delays = rng.integers(0, depth, nnz).astype(np.int32)
    if homo:
        data = np.array([0.75], dtype=dtype)
    elif f16:
        data = rng.integers(-4, 5, nnz).astype(dtype)
    else:
        data = (rng.integers(-64, 65, nnz) / 64.0).astype(dtype)
    col_abs = np.bincount(indices, weights=np.abs(np.broadcast_to(data.astype(np.float64), indices.shape)), minlength=n_post)
    assert nnz < 2 ** 17 and (not f16 or col_abs.max() <= 2048), "the case would not be exact"
    return data, indices, indptr, delays


def row_lengths_case(seed, tile=SPLIT_TILE):
    """The split's matrix: rows of 0, 1, 63, 64, 65, 257 and ``2 * tile + 3`` entries (shuffled, a few of each short kind)."""
    rng = np.random.default_rng(seed)
    lens = np.array([0, 1, 63, 64, 65, 257, 2 * tile + 3, 0, 1, 65, 64, 63])
    rng.shuffle(lens)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return lens, indptr


def delay_pattern(name, seed, indptr, depth):
    """One delay per entry: ``random``, ``equal``, ``ends`` (only 0 and depth - 1), ``sorted`` / ``reversed`` within the row (the
    last catches a fill that is not stable: equal delays sit next to each other in descending blocks)."""
    rng = np.random.default_rng(seed)
    nnz = int(indptr[-1])
    if name == 'equal':
        return np.full(nnz, depth // 2, dtype=np.int32)
    if name == 'ends':
        return (rng.integers(0, 2, nnz) * (depth - 1)).astype(np.int32)
    d = rng.integers(0, depth, nnz).astype(np.int32)
    if name == 'random':
        return d
    assert name in ('sorted', 'reversed')
    for i in range(len(indptr) - 1):
        seg = np.sort(d[indptr[i]:indptr[i + 1]])
        d[indptr[i]:indptr[i + 1]] = seg if name == 'sorted' else seg[::-1]
    return d
