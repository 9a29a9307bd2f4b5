"""The block layouts of the scatter plan restated on the host, from the layout comments of ``csrc/be_csr_plan.hip`` (not from its
kernels): what ``count -> scan -> fill`` must leave in ``seg`` and ``blob``, byte for byte.  Plain numpy, no loop over blocks.

``tests/test_plan_layout_cpu.py`` checks this module against itself, hand-written blocks and the constants in the source;
``tests/test_plan_build_exact_gpu.py`` checks the device against it.

Layout names: ``u16w`` (uint16 columns, per-entry weights), ``u16c`` (uint16 columns, counted entries: one shared weight), ``d8``,
``h8``, ``q8``.  A block is the part of row r in slice s.  Its *defined* bytes are the first ``nbytes`` ones, ``nbytes`` = 24 n4 /
16 n8 / 20 ng / 8 ng / 8 ng; the block occupies ``ceil(nbytes / 128)`` units of 128 bytes, and nothing writes the bytes behind the
defined ones.

GPU cases sized by ``THRESHOLDS`` (re-size them when a bound moves; ``test_plan_layout_cpu.py`` says so when one does):

  scan.chunk, scan.pass     test_scan_of_a_synthetic_table, test_scan_past_one_pass_end_to_end, test_block_index_of_32_bits
  grid.u16_cap              test_row_grid_second_trip (u16w, u16c), test_python_build_gives_the_same_plan,
                            test_plastic_rows_and_refresh_weights (u16), test_weight_statistics_of_the_fill
  grid.sorted_cap           the same tests (d8, h8, q8), test_q8_every_code, test_build_from_blocks
  kMaxSlices, kD8MaxSlices  test_scan_past_one_pass_end_to_end
  kD8MaxRow                 test_every_branch_of_the_row_sort, test_too_long_row_is_refused
  sort.*                    test_every_branch_of_the_row_sort, test_wide_buckets_take_64_bit_keys
  kD8MaxWidth, kH8MaxWidth  test_slice_arithmetic, test_escapes
"""
from typing import NamedTuple, Optional

import numpy as np

THRESHOLDS = {
    'scan.chunk': 2048,            # table entries per workgroup of k_scan_block_sums / k_scan_apply
    'scan.pass': 1024,             # chunk sums k_scan_sums scans per pass (one workgroup, a carry between passes)
    'grid.u16_cap': 4096,          # workgroups of k_plan_count / k_plan_fill / k_plan_refresh_rows (one row each, grid-stride)
    'grid.sorted_cap': 2048,       # ... of the d8 / h8 / q8 count, fill and row refresh
    'kMaxSlices': 4096,
    'kD8MaxRow': 16384,
    'kD8MaxSlices': 1024,
    'sort.bucket_target': 48,      # nb = ceil(len / 48) column ranges
    'sort.max_buckets': 1024,
    'sort.short_row': 256,         # rows up to this take the bitonic network
    'sort.bucket_one_per_lane': 64,
    'sort.bucket_limit': 256,      # a larger bucket sends the row to the bitonic network
    'sort.key32_bits': 18,         # buckets narrower than 2^18 columns sort 32-bit keys
    'kD8MaxWidth': 20000,
    'kH8MaxWidth': 40000,
}

LAYOUTS = ('u16w', 'u16c', 'd8', 'h8', 'q8')
GROUP = {'u16w': 4, 'u16c': 8, 'd8': 4, 'h8': 8, 'q8': 4}              # entries per lane-group
GROUP_BYTES = {'u16w': 24, 'u16c': 16, 'd8': 20, 'h8': 8, 'q8': 8}     # bytes per lane-group
SORTED = ('d8', 'h8', 'q8')


class Encoded(NamedTuple):
    layout: str
    m: int
    n_slices: int
    width: int
    slice_shift: int
    seg: np.ndarray          # (m, n_slices, 2) uint32
    units: int               # 128-byte units of the whole blob
    groups: np.ndarray       # per block, flat (r, s) order: n4 / n8 / ng
    nbytes: np.ndarray       # per block: defined bytes
    byte_off: np.ndarray     # per block: where its defined bytes start in `data`
    data: np.ndarray         # the defined bytes of all blocks, back to back (uint8)
    count: np.ndarray        # per block: stored entries (u16 layouts: the slots in front of the pads)

    def block(self, r: int, s: int) -> bytes:
        b = r * self.n_slices + s
        return self.data[self.byte_off[b]:self.byte_off[b] + self.nbytes[b]].tobytes()


# ------------------------------------------------------------------------------------------------------------ small helpers
def weight_bits(w) -> np.ndarray:
    """f32 bit patterns of f32 / f16 / bf16 weights, widened exactly (bf16: its 16 bits are the upper half of the f32)."""
    if type(w).__module__.startswith('torch'):
        import torch
        w = w.detach().cpu().reshape(-1)
        if w.dtype == torch.bfloat16:
            return w.view(torch.int16).numpy().astype(np.uint16).astype(np.uint32) << np.uint32(16)
        w = w.numpy()
    w = np.asarray(w).reshape(-1)
    assert w.dtype in (np.float32, np.float16), w.dtype
    return np.ascontiguousarray(w.astype(np.float32)).view(np.uint32)     # (f16 -> f32 is exact)


def _as_numpy(x):
    if type(x).__module__.startswith('torch'):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def row_pointers(indptr_or_row_len, m: int) -> np.ndarray:
    if np.ndim(indptr_or_row_len) == 0:
        return np.arange(m + 1, dtype=np.int64) * int(indptr_or_row_len)
    ptr = _as_numpy(indptr_or_row_len).astype(np.int64).reshape(-1)
    assert ptr.size == m + 1
    return ptr


def _excl(a: np.ndarray) -> np.ndarray:
    out = np.zeros(a.size, np.int64)
    np.cumsum(a[:-1], out=out[1:])
    return out


def _ragged_arange(counts: np.ndarray) -> np.ndarray:
    """0 .. counts[i] - 1 for every i, back to back."""
    total = int(counts.sum())
    return np.arange(total, dtype=np.int64) - np.repeat(_excl(counts), counts)


def _geometry(k, slice_shift, slice_width):
    W = int(slice_width) if slice_width else 1 << int(slice_shift)
    return W, -(-int(k) // W)


def _finish(layout, m, ns, W, slice_shift, groups, second, data, byte_off, nbytes, count) -> Encoded:
    units = (nbytes + 127) // 128
    seg = np.stack([_excl(units), second], axis=1).astype(np.uint32).reshape(m, ns, 2)
    total = int(units.sum())
    assert total < 1 << 32
    return Encoded(layout, m, ns, W, int(slice_shift), seg, total, groups, nbytes, byte_off, data, count)


# ------------------------------------------------------------------------------------------------------------ encode
def encode(layout, weights_or_codes, indices, indptr_or_row_len, m, k, slice_shift, slice_width) -> Encoded:
    assert layout in LAYOUTS
    W, ns = _geometry(k, slice_shift, slice_width)
    idx = _as_numpy(indices).astype(np.int64).reshape(-1)
    ptr = row_pointers(indptr_or_row_len, m)
    nnz = int(ptr[-1])
    assert idx.size == nnz and (nnz == 0 or (idx.min() >= 0 and idx.max() < k))
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    pos = np.arange(nnz, dtype=np.int64) - ptr[row]
    if layout in ('u16w', 'd8'):
        payload = weight_bits(weights_or_codes)
    elif layout == 'q8':
        payload = _as_numpy(weights_or_codes).reshape(-1).view(np.uint8)
    else:
        payload = np.zeros(nnz, np.uint32)
    assert payload.size == nnz
    nblk = m * ns
    G, GB = GROUP[layout], GROUP_BYTES[layout]

    if layout in ('u16w', 'u16c'):
        assert W <= 1 << slice_shift
        s = idx // W
        loc, blk = idx - s * W, row * ns + s
        count = np.bincount(blk, minlength=nblk).astype(np.int64)
        groups = -(-count // G)
        nbytes = groups * GB
        byte_off = _excl(nbytes)
        data = np.zeros(int(nbytes.sum()), np.uint8)
        # canonical order of a block's multiset: by (local column, weight bits); then the pads (weight 0, column 2^slice_shift)
        o = np.lexsort((payload, loc, blk))
        rank = np.arange(nnz, dtype=np.int64) - _excl(count)[blk[o]]
        sb = np.repeat(np.arange(nblk, dtype=np.int64), groups * G)
        j = _ragged_arange(groups * G)
        col_at = byte_off[sb] + (16 * groups[sb] if layout == 'u16w' else 0) + 2 * j
        cols = data.view(np.uint16)
        cols[col_at // 2] = 1 << slice_shift
        cols[(byte_off[blk[o]] + (16 * groups[blk[o]] if layout == 'u16w' else 0) + 2 * rank) // 2] = loc[o]
        if layout == 'u16w':
            data.view(np.uint32)[(byte_off[blk[o]] + 4 * rank) // 4] = payload[o]
        return _finish(layout, m, ns, W, slice_shift, groups, groups, data, byte_off, nbytes, count)

    # the sorted layouts: entries by (column, position in row); a block's first delta is 0
    o = np.lexsort((pos, idx, row))
    c, r, pay = idx[o], row[o], payload[o]
    s = c // W
    loc, blk = c - s * W, r * ns + s
    first = np.ones(nnz, bool)
    first[1:] = blk[1:] != blk[:-1]
    gap = np.zeros(nnz, np.int64)
    gap[1:] = c[1:] - c[:-1]
    gap[first] = 0
    esc = gap // 255 if layout == 'h8' else np.where(gap > 0, (gap - 1) // 255, 0)
    rem = gap - 255 * esc
    items = 1 + esc
    count = np.bincount(blk, minlength=nblk).astype(np.int64)
    tot = np.bincount(blk, weights=items, minlength=nblk).astype(np.int64)
    groups = -(-tot // G)
    base = np.zeros(nblk, np.int64)
    base[blk[first]] = loc[first]
    assert groups.max(initial=0) < 1 << 16 and base.max(initial=0) < 1 << 16
    nbytes = groups * GB
    byte_off = _excl(nbytes)
    cs = np.cumsum(items)
    before = np.zeros(nblk, np.int64)
    before[blk[first]] = (cs - items)[first]
    p = cs - before[blk] - 1                                   # the entry's item position in its block, its escapes in front of it
    data = np.full(int(nbytes.sum()), 255 if layout == 'h8' else 0, np.uint8)       # tail pads: 255 (h8), (0, 0) otherwise
    if layout == 'h8':
        data[byte_off[blk] + p] = rem
    else:
        dlt = byte_off + (16 if layout == 'd8' else 4) * groups                    # where a block's deltas start
        data[dlt[blk] + p] = rem
        ent = np.repeat(np.arange(nnz, dtype=np.int64), esc)
        data[dlt[blk[ent]] + p[ent] - esc[ent] + _ragged_arange(esc)] = 255            # escapes: (weight 0 / code 0, delta 255)
        if layout == 'd8':
            data.view(np.uint32)[(byte_off[blk] + 4 * p) // 4] = pay
        else:
            data[byte_off[blk] + p] = pay
    return _finish(layout, m, ns, W, slice_shift, groups, groups | (base << 16), data, byte_off, nbytes, count)


# ------------------------------------------------------------------------------------------------------------ read a blob
def defined_bytes(layout, seg, blob) -> np.ndarray:
    """The defined bytes of every block of a device blob, back to back in flat (r, s) order, by the table ``seg``."""
    seg = np.asarray(seg, np.uint32).reshape(-1, 2).astype(np.int64)
    groups = seg[:, 1] & (0xffff if layout in SORTED else 0xffffffff)
    nbytes = groups * GROUP_BYTES[layout]
    at = np.repeat(seg[:, 0] * 128 - _excl(nbytes), nbytes) + np.arange(int(nbytes.sum()), dtype=np.int64)
    blob = np.asarray(blob).reshape(-1).view(np.uint8)
    assert at.size == 0 or at.max() < blob.size, 'the table points past the blob'
    return blob[at]


def _u16_slots(layout, groups, byte_off, data):
    """(block, column, weight bits) of every slot of the u16 layouts, in stored order."""
    G = GROUP[layout]
    sb = np.repeat(np.arange(groups.size, dtype=np.int64), groups * G)
    j = _ragged_arange(groups * G)
    cols = data.view(np.uint16)[(byte_off[sb] + (16 * groups[sb] if layout == 'u16w' else 0) + 2 * j) // 2]
    bits = data.view(np.uint32)[(byte_off[sb] + 4 * j) // 4] if layout == 'u16w' else np.zeros(sb.size, np.uint32)
    return sb, j, cols.astype(np.int64), bits


def blocks_mismatch(enc: Encoded, blob) -> Optional[str]:
    """None when the defined bytes of ``blob`` (laid out by ``enc.seg``) are what the encoder states, else a description of the
    first block that differs.  u16 layouts: positions inside a block come from an LDS counter, so the entries are compared as a
    multiset; they must fill the first ``count`` slots, and every slot behind them must be a pad."""
    got = defined_bytes(enc.layout, enc.seg, blob)
    want = enc.data
    assert got.size == want.size
    if enc.layout in ('u16w', 'u16c'):
        got = np.ascontiguousarray(got)
        sb, j, cols, bits = _u16_slots(enc.layout, enc.groups, enc.byte_off, got)
        real = j < enc.count[sb]
        o = np.lexsort((bits[real], cols[real], sb[real]))
        canon = np.zeros(got.size, np.uint8)
        at_c = (enc.byte_off[sb] + (16 * enc.groups[sb] if enc.layout == 'u16w' else 0) + 2 * j) // 2
        cc, cb = cols.copy(), bits.copy()
        cc[real], cb[real] = cols[real][o], bits[real][o]            # (the sort is by block first: slots stay in their block)
        canon.view(np.uint16)[at_c] = cc
        if enc.layout == 'u16w':
            canon.view(np.uint32)[(enc.byte_off[sb] + 4 * j) // 4] = cb
        got = canon
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    b = int(np.searchsorted(enc.byte_off, bad[0], side='right') - 1)
    while enc.nbytes[b] == 0:
        b -= 1
    lo, hi = int(enc.byte_off[b]), int(enc.byte_off[b] + enc.nbytes[b])
    return (f'{enc.layout} block (row {b // enc.n_slices}, slice {b % enc.n_slices}), byte {int(bad[0]) - lo} of {hi - lo}: '
            f'got {got[lo:hi][:64].tolist()} want {want[lo:hi][:64].tolist()} ({bad.size} bytes differ in all)')


# ------------------------------------------------------------------------------------------------------------ decode
def decode(layout, seg, blob, k, slice_shift, slice_width):
    """(row, column, weight bits or code) of the stored entries, from the table and the blob alone.  Pads and escapes are left
    out.  d8 / q8: an escape or pad is an item of weight +0 / code 0 that adds nothing wherever it lands, and a stored entry of
    weight +0 / code 0 looks like one: such entries are left out too (what the step computes does not depend on them)."""
    W, ns = _geometry(k, slice_shift, slice_width)
    segf = np.asarray(seg, np.uint32).reshape(-1, 2).astype(np.int64)
    groups = segf[:, 1] & (0xffff if layout in SORTED else 0xffffffff)
    base = segf[:, 1] >> 16
    nbytes = groups * GROUP_BYTES[layout]
    byte_off = _excl(nbytes)
    data = np.ascontiguousarray(defined_bytes(layout, seg, blob))
    if layout in ('u16w', 'u16c'):
        sb, _, cols, bits = _u16_slots(layout, groups, byte_off, data)
        real = cols != 1 << slice_shift
        assert (bits[~real] == 0).all() and (cols[real] < W).all()
        return sb[real] // ns, (sb[real] % ns) * W + cols[real], bits[real]
    G = GROUP[layout]
    sb = np.repeat(np.arange(groups.size, dtype=np.int64), groups * G)
    j = _ragged_arange(groups * G)
    if layout == 'h8':
        step = data[byte_off[sb] + j].astype(np.int64)
        pay = np.zeros(sb.size, np.uint32)
        real = step != 255
    else:
        step = data[byte_off[sb] + (16 if layout == 'd8' else 4) * groups[sb] + j].astype(np.int64)
        pay = data.view(np.uint32)[(byte_off[sb] + 4 * j) // 4] if layout == 'd8' else data[byte_off[sb] + j]
        real = pay != 0
    run = np.cumsum(step)
    started = np.zeros(groups.size, np.int64)
    firsts = np.flatnonzero(j == 0)
    started[sb[firsts]] = (run - step)[firsts]
    loc = base[sb] + run - started[sb]
    assert (loc[real] < W).all()
    return sb[real] // ns, (sb[real] % ns) * W + loc[real], pay[real]


def triples(rows, cols, payload) -> np.ndarray:
    """A sorted (n, 3) int64 array: the multiset of (row, column, payload)."""
    t = np.stack([np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(payload).astype(np.int64)], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def csr_triples(layout, weights_or_codes, indices, indptr_or_row_len, m) -> np.ndarray:
    """What :func:`decode` must give back for a CSR (see there for the entries of weight +0 / code 0)."""
    ptr = row_pointers(indptr_or_row_len, m)
    idx = _as_numpy(indices).astype(np.int64).reshape(-1)
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    if layout in ('u16w', 'd8'):
        pay = weight_bits(weights_or_codes)
    elif layout == 'q8':
        pay = _as_numpy(weights_or_codes).reshape(-1).view(np.uint8)
    else:
        pay = np.zeros(idx.size, np.uint32)
    keep = pay != 0 if layout in ('d8', 'q8') else np.ones(idx.size, bool)
    return triples(row[keep], idx[keep], pay[keep])


# ------------------------------------------------------------------------------------------------------------ case builders
GAPS = (254, 255, 256, 510, 511)


def csr_of(rows):
    """(indices int32, indptr int32) of a list of rows of columns."""
    lens = np.array([len(r) for r in rows], np.int64)
    idx = np.concatenate([np.asarray(r, np.int64) for r in rows]) if rows else np.zeros(0, np.int64)
    return idx.astype(np.int32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def edge_rows(rng, k: int, W: int, n_random: int = 10):
    """Rows at the edges of the slice arithmetic and of the delta codes: columns at s*W - 1, s*W, s*W + 1 of the first, a middle
    and the last slice and column k - 1; a first entry at local column 0 and one at W - 1; chains and single gaps of 254, 255,
    256, 510, 511 and one gap of W - 1 inside a slice; repeated columns; empty rows; random rows."""
    ns = -(-k // W)
    slices = sorted({0, ns // 2, ns - 1})
    rows = [np.zeros(0, np.int64)]
    edge = [c for s in slices for c in (s * W - 1, s * W, s * W + 1)] + [k - 1]
    rows.append(np.array([c for c in edge if 0 <= c < k][::-1], np.int64))
    for s in slices:
        lo, hi = s * W, min(k, (s + 1) * W)
        rows.append(np.array([hi - 1, lo], np.int64))                          # local column 0 and the slice's last: one gap of W - 1
        chain, c = [lo], lo
        for g in GAPS:
            c += g
            if c < k:
                chain.append(c)
        chain = np.array(chain, np.int64)
        rng.shuffle(chain)
        rows.append(chain)
        for g in GAPS:
            if lo + 3 + g < hi:
                rows.append(np.array([lo + 3 + g, lo + 3], np.int64))
    rows.append(np.full(7, min(k - 1, W + 1), np.int64))
    rows.append(np.zeros(0, np.int64))
    for _ in range(n_random):
        rows.append(rng.integers(0, k, int(rng.integers(0, 40))))
    return rows


def escape_rows(layout: str, c0: int):
    """A block whose single escape pushes it over a lane-group boundary and over a 128-byte unit: ``n`` consecutive columns from
    ``c0`` and one more 256 further on (needs a slice of at least n + 256 columns from c0)."""
    n = {'d8': 23, 'h8': 127, 'q8': 63}[layout]          # n + 1 entries fill one unit exactly; the escape is the item too many
    return [np.concatenate([[c0 + n - 1 + 256], np.arange(c0, c0 + n)]).astype(np.int64)]


# ------------------------------------------------------------------------------------------------------------ the row sort
def expected_order(indices, indptr_or_row_len, m=None) -> np.ndarray:
    """Per row, ``lexsort((position, column))`` as uint16: the row-local position of the i-th smallest column."""
    if m is None:
        m = _as_numpy(indptr_or_row_len).size - 1
    ptr = row_pointers(indptr_or_row_len, m)
    idx = _as_numpy(indices).astype(np.int64).reshape(-1)
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    pos = np.arange(idx.size, dtype=np.int64) - ptr[row]
    return pos[np.lexsort((pos, idx, row))].astype(np.uint16)


class SortBranch(NamedTuple):
    branch: str              # 'short-ascending' | 'short-bitonic' | 'ascending' | 'counting' | 'fallback'
    largest: int             # keys of the largest bucket (0 outside the counting sort's reach)
    forms: frozenset         # rank sorts the buckets of a 'counting' row take: 'rank32', 'rank64', 'rank4'


def sort_branch(length: int, col_range: int, columns) -> SortBranch:
    """Which branch of the row sort a row of ``length`` entries takes when the plan covers ``col_range`` = slice_width * n_slices
    columns, and its largest bucket."""
    T = THRESHOLDS
    cols = np.asarray(columns, np.int64).reshape(-1)
    assert cols.size == length
    ascending = bool((cols[1:] >= cols[:-1]).all())
    if length <= T['sort.short_row']:
        return SortBranch('short-ascending' if ascending else 'short-bitonic', 0, frozenset())
    nb = min(-(-length // T['sort.bucket_target']), T['sort.max_buckets'])
    bw = -(-col_range // nb)
    sizes = np.bincount(np.minimum(cols // bw, nb - 1), minlength=nb)
    largest = int(sizes.max())
    if ascending:
        return SortBranch('ascending', largest, frozenset())
    if largest > T['sort.bucket_limit']:
        return SortBranch('fallback', largest, frozenset())
    forms = set()
    if (sizes > T['sort.bucket_one_per_lane']).any():
        forms.add('rank4')
    if ((sizes > 0) & (sizes <= T['sort.bucket_one_per_lane'])).any():
        forms.add('rank32' if bw < 1 << T['sort.key32_bits'] else 'rank64')
    return SortBranch('counting', largest, frozenset(forms))


def row_with_bucket(rng, length: int, largest: int, col_range: int, bucket: int = 1) -> np.ndarray:
    """A shuffled row of ``length`` columns whose bucket ``bucket`` holds exactly ``largest`` keys and no other bucket more."""
    nb = min(-(-length // THRESHOLDS['sort.bucket_target']), THRESHOLDS['sort.max_buckets'])
    bw = -(-col_range // nb)
    others = [b for b in range(nb) if b != bucket]
    rest = length - largest
    per = -(-rest // len(others))
    assert per < largest and (nb - 1) * bw < col_range
    parts = [rng.integers(bucket * bw, (bucket + 1) * bw, largest)]
    for i, b in enumerate(others):
        n = min(per, rest - i * per)
        if n > 0:
            parts.append(rng.integers(b * bw, min((b + 1) * bw, col_range), n))
    row = np.concatenate(parts)
    rng.shuffle(row)
    assert row.size == length
    return row
