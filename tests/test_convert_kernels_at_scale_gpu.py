"""The CSR -> CSC conversion kernels (csrc/be_convert.hip: k_t_count, k_scan64_totals, k_scan64_of_totals, k_scan64_apply,
k_t_cursor_init, k_t_fill, k_gather_by_perm) past their one-pass sizes: every grid-stride loop, tile carry, alignment branch,
lane choice and template instantiation of the file is crossed by a named case.

Assertion policy: these kernels move integers and bit patterns, so every comparison in this module is an equality; there is no
tolerance anywhere.  The reference is numpy on the host: `bincount` + `cumsum` for the offsets and a stable `argsort` of the
column ids for the slots.  The order inside a column is unspecified (slots are drawn from an atomic cursor), so `Ref.check`
canonicalises before it compares: with a permutation, the slots are sorted by (column of the slot, perm) and must then BE the
stable order — that proves perm is a permutation, that every slot lies in its own column and that nothing is lost or doubled —
and rows / weights must equal `row_of_entry[perm]` / `w[perm]` slot for slot; without one, the (column, row, weight bits) triples
are compared as sorted lists.  Weights are random bit patterns viewed as f16 / f32 / f64 with -0.0, a signalling NaN, the
smallest denormal and an infinity planted, compared as integers: a move that goes through an arithmetic type fails.
`test_checker_agrees_with_columns_as_sets` holds the checker to the per-column loop of tests/test_mirror_gpu.py where both run.

Every case is sized from the CONSTS table (tests/test_convert_kernels_thresholds_cpu.py compares it with the source) and asserts
on the host that it crosses the bound it is there for.

Which loop or branch is reached where:
  k_t_count vector loop, second trip (more than 4 * 256 * 4096 ids), few / many columns          test_count_past_one_trip
  k_t_count alignment head: nnz < head, nnz == head, head + quads + tail, 0/4/8/12 bytes off      test_count_at_every_alignment
  k_t_count range test in the head, the vector part of the second trip and the tail               test_out_of_range_ids_are_counted_not_dropped
  k_scan64_totals / k_scan64_apply tile carry at T-1, T, T+1, 2T+1 columns, checked exactly       test_scan_across_tiles
  k_scan64_of_totals strip loop (more than 1024 tiles, partial second strip);
    k_t_cursor_init second trip (more than 2048 * 256 block columns)                              test_scan_past_one_strip_of_totals
  64-bit carries of the three scan kernels; k_scan64_apply<int32_t>; BE_ERR_RANGE; n_cols = 0     test_scan_of_wide_counts_and_the_int32_output
  k_t_fill LPR 1 / 4 / 16 / 64 at the avg_row edges 2|3, 8|9, 48|49, fixed and ragged rows        test_fill_lane_choice_edges
  k_t_fill row loop, second trip, at every LPR                                                    test_fill_past_one_trip
  k_t_fill<.., WB 0 / 2 / 4 / 8>, with / without perm; k_t_fill<.., int64_t, WB> with a perm      test_fill_every_weight_width_and_perm_width
  column blocks: empty, one column, cuts off the multiples of 256; block_indptr / block_entries    test_column_blocks_at_scale
  column blocks that hold no entry (host path of CscBuilder.block: no launch)                     test_column_block_without_entries
  k_gather_by_perm second trip, 2 / 4 / 8-byte elements x int32 / int64 perm, out=, n = 0         test_gather_by_perm_past_one_trip
  the arrays a Mirror holds are this conversion; its refresh is the gather                        test_mirror_arrays_are_the_conversion,
                                                                                                  test_fixed_number_mirror_arrays_are_the_conversion

Not here: a perm past 2^31 entries (the int64 perm instantiations are driven directly at a small size instead, with the
destination preset to all ones so that a 32-bit store shows; a value truncated to 32 bits and widened again is the same number
below 2^32 entries).  A fill grid sized for another LPR, and a head of 0 ids in front of an unaligned id stream on hardware that
serves unaligned 16-byte loads, change no result: the row loop strides by the grid it is given, and the ids are the same ids.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# The loop bounds and dispatch thresholds of be_convert.hip as the cases below use them.
CONSTS = {
    'block': 256,                   # threads per workgroup of k_t_count, k_t_cursor_init, k_t_fill and k_gather_by_perm
    'count.ids_per_thread': 4,      # k_t_count: one 16-byte load of column ids per thread and trip
    'count.grid_cap': 256 * 16,     # grid_for((nnz + 3) / 4, 256, 256 * 16)
    'scan.tile': 1024 * 8,          # kScanTile: columns per workgroup of k_scan64_totals / k_scan64_apply
    'scan.strip': 1024,             # tile totals per trip of k_scan64_of_totals
    'cursor.grid_cap': 2048,        # k_t_cursor_init: grid_for(nb, 256, 2048)
    'fill.grid_cap': 256 * 16,      # k_t_fill<LPR>: grid_for(m, 256 / LPR, 256 * 16)
    'fill.avg_lpr1': 2,             # avg_row = nnz / m <= 2 -> LPR 1
    'fill.avg_lpr4': 8,             # <= 8 -> LPR 4
    'fill.avg_lpr16': 48,           # <= 48 -> LPR 16, above -> LPR 64
    'gather.grid_cap': 256 * 16,    # k_gather_by_perm: grid_for(n, 256, 256 * 16)
}
K = CONSTS
T = K['scan.tile']
BLOCK = K['block']
COUNT_SPAN = K['count.ids_per_thread'] * BLOCK * K['count.grid_cap']     # 4 194 304 ids per trip of k_t_count's vector loop
CURSOR_SPAN = BLOCK * K['cursor.grid_cap']                               # 524 288 block columns per trip of k_t_cursor_init
GATHER_SPAN = BLOCK * K['gather.grid_cap']                               # 1 048 576 elements per trip of k_gather_by_perm
STRIP_COLS = K['scan.strip'] * T                                         # 8 388 608 columns per trip of k_scan64_of_totals
COUNT_NNZ = COUNT_SPAN + K['count.ids_per_thread'] * BLOCK + 3           # one full trip, a second one of 256 quads, a tail of 3
LPRS = (1, 4, 16, 64)
# fixed row length that chooses each LPR in test_fill_past_one_trip: the upper edge of LPR 1 and one past the edge below the others
ROW_LEN_OF = {1: K['fill.avg_lpr1'], 4: K['fill.avg_lpr1'] + 1, 16: K['fill.avg_lpr4'] + 1, 64: K['fill.avg_lpr16'] + 1}

NP_INT = {2: np.int16, 4: np.int32, 8: np.int64}
T_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
T_FLOAT = {2: torch.float16, 4: torch.float32, 8: torch.float64}
# planted in every weight array: -0.0, a signalling NaN with a payload, the smallest denormal, +inf
SPECIALS = {2: [0x8000, 0x7d01, 0x0001, 0x7c00],
            4: [0x80000000, 0x7fa00001, 0x00000001, 0x7f800000],
            8: [0x8000000000000000, 0x7ff4000000000001, 0x0000000000000001, 0x7ff0000000000000]}


def lpr_of(avg_row):
    """fill_by_row_length restated: lanes per stored row from avg_row = nnz / m (integer division)."""
    if avg_row <= K['fill.avg_lpr1']:
        return 1
    if avg_row <= K['fill.avg_lpr4']:
        return 4
    if avg_row <= K['fill.avg_lpr16']:
        return 16
    return 64


def fill_span(lpr):
    """Stored rows per trip of k_t_fill<LPR>'s row loop."""
    return K['fill.grid_cap'] * (BLOCK // lpr)


def check_all_crossings():
    """The arithmetic behind the table in the module docstring (also run without a device by the thresholds module)."""
    assert COUNT_NNZ > COUNT_SPAN + K['count.ids_per_thread'] and COUNT_NNZ % K['count.ids_per_thread'] == 3
    assert 2 * T + 1 > 2 * T and (K['scan.strip'] + 1) * T + 5 > STRIP_COLS > CURSOR_SPAN
    assert [lpr_of(a) for a in (1, 2, 3, 8, 9, 48, 49)] == [1, 1, 4, 4, 16, 16, 64]
    for lpr in LPRS:
        assert lpr_of(ROW_LEN_OF[lpr]) == lpr and fill_span(lpr) + 7 > fill_span(lpr)
    assert [fill_span(lpr) for lpr in LPRS] == [1_048_576, 262_144, 65_536, 16_384]
    assert BLOCK * K['gather.grid_cap'] + 3 > GATHER_SPAN


# =================================================================================================================== helpers
def bit_weights(rng, n, wb):
    """`n` random bit patterns of `wb` bytes (host, as signed integers) with SPECIALS planted at random places."""
    bits = np.frombuffer(rng.bytes(n * wb), dtype=NP_INT[wb]).copy()
    if n >= 4:
        bits[rng.choice(n, 4, replace=False)] = np.array(SPECIALS[wb], dtype=np.uint64).astype(NP_INT[wb])
    return bits


def as_float(bits):
    """Host bit patterns -> device tensor of the float type of that width."""
    wb = bits.dtype.itemsize
    return torch.tensor(bits).cuda().view(T_FLOAT[wb])


def bits_of(t):
    """Device tensor -> its elements as host integers."""
    return None if t is None else t.view(T_INT[t.element_size()]).cpu().numpy()


def host(t):
    return None if t is None else t.cpu().numpy()


class Ref:
    """Stable host reference of one conversion, computed once: offsets by bincount + cumsum, slots by a stable argsort."""

    def __init__(self, idx, k, row_of_entry):
        self.idx, self.k, self.row_of_entry = idx, int(k), row_of_entry
        self.cptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=k))]).astype(np.int64)
        self.order = np.argsort(idx, kind='stable')
        for a in (self.cptr, self.order):
            a.flags.writeable = False

    def check(self, bptr, rows, perm=None, w=None, w_out=None, c0=0, c1=None):
        """The columns [c0, c1) as `bptr` (relative offsets), `rows`, `perm`, `w_out` (bit patterns) are those of the reference up
        to the order inside a column.  `w`: the source weights' bit patterns."""
        c1 = self.k if c1 is None else c1
        want_ptr = self.cptr[c0:c1 + 1] - self.cptr[c0]
        np.testing.assert_array_equal(bptr, want_ptr)
        n = int(want_ptr[-1])
        want = self.order[self.cptr[c0]:self.cptr[c1]]
        assert rows.shape == (n,) and rows.dtype == np.int32
        col_of_slot = np.repeat(np.arange(c1 - c0), np.diff(want_ptr))
        if perm is not None:
            assert perm.shape == (n,)
            np.testing.assert_array_equal(perm[np.lexsort((perm, col_of_slot))], want)
            np.testing.assert_array_equal(rows, self.row_of_entry[perm])
            if w is not None:
                assert w_out.shape == (n,) and w_out.dtype == w.dtype
                np.testing.assert_array_equal(w_out, w[perm])
            return
        keys = (rows,) if w is None else (w_out, rows)
        ref_keys = (self.row_of_entry[want],) if w is None else (w[want], self.row_of_entry[want])
        if w is not None:
            assert w_out.shape == (n,) and w_out.dtype == w.dtype
        got_order = np.lexsort(keys + (col_of_slot,))
        ref_order = np.lexsort(ref_keys + (self.idx[want] - c0,))
        np.testing.assert_array_equal(self.idx[want][ref_order] - c0, col_of_slot[got_order])
        for g, r in zip(keys, ref_keys):
            np.testing.assert_array_equal(g[got_order], r[ref_order])


def rows_of(ptr=None, m=None, row_len=None):
    if ptr is not None:
        return np.repeat(np.arange(len(ptr) - 1, dtype=np.int32), np.diff(ptr))
    return np.repeat(np.arange(m, dtype=np.int32), row_len)


def builder(idx, shape, ptr=None, row_len=-1):
    from brainevent_amd._convert import CscBuilder
    d_idx = idx if isinstance(idx, torch.Tensor) else torch.tensor(idx).cuda()
    d_ptr = None if ptr is None else torch.tensor(ptr).cuda()
    return CscBuilder(d_ptr, d_idx, shape=shape, row_len=row_len)


def convert_and_check(ref, b, w_bits=None, perm=True, c0=0, c1=None):
    """One block (default: all columns) through CscBuilder.block, checked; returns the host arrays."""
    c1 = b.k if c1 is None else c1
    data = None if w_bits is None else as_float(w_bits)
    rows, w_out, p = b.block(c0, c1, data=data, perm=perm)
    assert (p is not None) == bool(perm) and (w_out is not None) == (w_bits is not None)
    assert p is None or p.dtype == torch.int32
    assert w_out is None or w_out.dtype == data.dtype
    rows, w_out, p = host(rows), bits_of(w_out), host(p)
    ref.check(host(b.block_indptr(c0, c1)), rows, p, w_bits, w_out, c0, c1)
    return rows, w_out, p


def ragged_lengths(avg, rng):
    """Row lengths with nnz // m == avg exactly, from the set the issue names: 0, 1, LPR - 1, LPR, LPR + 1 around the lane count
    `avg` chooses, one row of 5000 entries and a run of 100 empty rows; filler rows bring the average to avg + 1/2."""
    lpr = lpr_of(avg)
    special = [5000] + [0] * 100 + [0, 1, lpr - 1, lpr, lpr + 1] * 40
    n0, s0 = len(special), sum(special)
    x = max(300, -(-(2 * s0 - (2 * avg + 1) * n0) // (2 * avg + 1)) + 1)
    m = n0 + x
    rest = avg * m + m // 2 - s0
    assert rest >= 0
    filler = np.full(x, rest // x, dtype=np.int64)
    filler[:rest % x] += 1
    lens = np.concatenate([np.asarray(special, dtype=np.int64), filler])
    head, tail = lens[:101], lens[101:]               # (the long row and the empty run stay where they are)
    lens = np.concatenate([head, rng.permutation(tail)])
    assert int(lens.sum()) // len(lens) == avg
    return lens


@functools.lru_cache(maxsize=None)
def fixed_case(lpr):
    """The matrix of test_fill_past_one_trip for one LPR: 7 stored rows more than one trip of k_t_fill<LPR> walks, fixed row
    length, 4099 columns.  Host arrays and the reference, shared by the cases that use the same matrix."""
    rng = np.random.default_rng(800 + lpr)
    m, k, row_len = fill_span(lpr) + 7, 4099, ROW_LEN_OF[lpr]
    idx = rng.integers(0, k, (m, row_len)).astype(np.int32)
    w = bit_weights(rng, m * row_len, 4)
    for a in (idx, w):
        a.flags.writeable = False
    return m, k, row_len, idx, w, Ref(idx.reshape(-1), k, rows_of(m=m, row_len=row_len))


@functools.lru_cache(maxsize=None)
def ragged_case(avg, ptr_dtype):
    rng = np.random.default_rng(700 + avg)
    lens = ragged_lengths(avg, rng)
    m, k = len(lens), 257
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(ptr_dtype)
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    w = bit_weights(rng, idx.size, 4)
    for a in (ptr, idx, w):
        a.flags.writeable = False
    return m, k, ptr, idx, w, Ref(idx, k, rows_of(ptr))


def finite_bit_weights(rng, n):
    """f32 bit patterns with a random sign and mantissa and an exponent in [2^-4, 2^4): every bit of the mantissa is in play,
    and the products and fixed-point plans that the containers build from them stay finite."""
    sign = rng.integers(0, 2, n, dtype=np.int64) << 31
    expo = rng.integers(123, 131, n, dtype=np.int64) << 23
    mant = rng.integers(0, 1 << 23, n, dtype=np.int64)
    return (sign | expo | mant).astype(np.uint32).view(np.int32)


# ===================================================================================================================== checker
def test_checker_agrees_with_columns_as_sets(be):
    """On the ragged 700 x 531 matrix of tests/test_mirror_gpu.py the vectorised checker and the per-column loop accept the same
    conversion, and both reject one with two slots of different columns exchanged."""
    from test_mirror_gpu import _columns_as_sets, rand_csr
    check_all_crossings()
    rng = np.random.default_rng(11)
    m, k = 700, 531
    _, idx, ptr = rand_csr(rng, m, k, rng.integers(0, 200, m))
    w = bit_weights(rng, idx.size, 4)
    ref = Ref(idx, k, rows_of(ptr))
    b = builder(idx, (m, k), ptr)
    rows, w_out, perm = convert_and_check(ref, b, w, perm=True)
    rows2, w_out2, _ = convert_and_check(ref, b, w, perm=False)
    convert_and_check(ref, b, None, perm=False)
    sptr, srows, sperm = be.csr_to_csc_index(ptr, idx, shape=(m, k), method='coo')
    np.testing.assert_array_equal(sptr, ref.cptr)
    np.testing.assert_array_equal(sperm, ref.order)                    # the stable route IS the reference
    assert _columns_as_sets(ref.cptr, rows, perm) == _columns_as_sets(sptr, srows, sperm)
    assert _columns_as_sets(ref.cptr, rows2) == _columns_as_sets(sptr, srows)
    # a synapse delivered to the wrong neuron: both checkers see it, with and without the permutation
    col_of_slot = np.repeat(np.arange(k), np.diff(ref.cptr))

    def exchange(first, *others):
        """Slot 0 against the last slot of another column that holds another row."""
        z = int(np.nonzero((col_of_slot != col_of_slot[0]) & (first != first[0]))[0][-1])
        for arr in (first,) + others:
            arr[[0, z]] = arr[[z, 0]]
        return z

    exchange(rows, perm, w_out)
    z = exchange(rows2, w_out2)
    assert _columns_as_sets(ref.cptr, rows, perm) != _columns_as_sets(sptr, srows, sperm)
    assert _columns_as_sets(ref.cptr, rows2) != _columns_as_sets(sptr, srows)
    with pytest.raises(AssertionError):
        ref.check(ref.cptr, rows, perm, w, w_out)
    with pytest.raises(AssertionError):
        ref.check(ref.cptr, rows2, None, w, w_out2)
    # a weight that lost one bit on the way, in its own column
    for arr in (rows2, w_out2):
        arr[[0, z]] = arr[[z, 0]]
    ref.check(ref.cptr, rows2, None, w, w_out2)
    w_out2[5] ^= 1
    with pytest.raises(AssertionError):
        ref.check(ref.cptr, rows2, None, w, w_out2)


# ======================================================================================================================= count
@pytest.mark.parametrize('k', [37, 100_003])
def test_count_past_one_trip(be, k):
    """Two trips of k_t_count's vector loop and a scalar tail of 3; 37 columns: every atomic contends with 1/37 of the others."""
    nnz = COUNT_NNZ
    assert (nnz >> 2) > BLOCK * K['count.grid_cap'] and nnz & 3 == 3
    rng = np.random.default_rng(100 + k)
    idx = rng.integers(0, k, nnz).astype(np.int32)
    b = builder(idx, (nnz, k), row_len=1)
    assert b.indices.data_ptr() % 16 == 0
    counts = np.bincount(idx, minlength=k)
    np.testing.assert_array_equal(host(b.counts), counts)
    np.testing.assert_array_equal(host(b.csc_indptr), np.concatenate([[0], np.cumsum(counts)]))
    assert b.max_col_count == int(counts.max())


def test_count_at_every_alignment(be):
    """The column ids start 0 / 4 / 8 / 12 bytes past a 16-byte boundary: head = 0 / 3 / 2 / 1 ids before the first aligned quad;
    nnz below, at and above the head, with and without quads and a tail."""
    rng = np.random.default_rng(2)
    k = 13
    buf = torch.zeros(1027 + 8, dtype=torch.int32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    for o in range(4):
        for nnz in (1, 2, 3, 4, 5, 7, 8, 1027):
            idx = rng.integers(0, k, nnz).astype(np.int32)
            buf.fill_(k - 1)                                  # (valid ids around the window: an over-read shows as a count)
            view = buf[o:o + nnz]
            view.copy_(torch.from_numpy(idx))
            b = builder(view, (nnz, k), row_len=1)
            assert b.indices.data_ptr() == buf.data_ptr() + 4 * o
            np.testing.assert_array_equal(host(b.counts), np.bincount(idx, minlength=k), err_msg=f'offset {o}, nnz {nnz}')
    # the whole conversion at each offset: ragged rows, perm and weights moved
    nnz, m, k = 1027, 90, 61
    lens = rng.multinomial(nnz, np.ones(m) / m)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, k, nnz).astype(np.int32)
    w = bit_weights(rng, nnz, 4)
    ref = Ref(idx, k, rows_of(ptr))
    for o in range(4):
        buf.fill_(k - 1)
        view = buf[o:o + nnz]
        view.copy_(torch.from_numpy(idx))
        b = builder(view, (m, k), ptr)
        assert b.indices.data_ptr() == buf.data_ptr() + 4 * o
        convert_and_check(ref, b, w, perm=True)


def test_out_of_range_ids_are_counted_not_dropped(be):
    """-1, k and 2^31 - 1 in the alignment head, in the vector part of the second trip and in the scalar tail: the error names
    exactly the planted number, and the same arguments with the ids repaired convert."""
    nnz, k, o = COUNT_NNZ, 100_003, 3
    head = 4 - o                                              # ids before the first 16-byte boundary
    n4 = (nnz - head) >> 2
    tail = nnz - head - 4 * n4
    second_trip = head + COUNT_SPAN                           # first id of the vector loop's second trip
    assert head == 1 and tail == 2 and n4 > BLOCK * K['count.grid_cap'] and second_trip + 8 <= head + 4 * n4
    rng = np.random.default_rng(3)
    idx = rng.integers(0, k, nnz).astype(np.int32)
    bad = {0: -1, second_trip + 4: k, second_trip + 5: -1, second_trip + 7: 2 ** 31 - 1, nnz - 2: 2 ** 31 - 1, nnz - 1: k}
    broken = idx.copy()
    for pos, v in bad.items():
        broken[pos] = v
    buf = torch.zeros(nnz + 4, dtype=torch.int32, device='cuda')
    view = buf[o:o + nnz]
    view.copy_(torch.from_numpy(broken))
    assert view.data_ptr() % 16 == 4 * o
    with pytest.raises(ValueError, match=rf'^csr_to_csc: {len(bad)} of {nnz} column ids lie outside \[0, {k}\)'):
        builder(view, (nnz, k), row_len=1)
    view.copy_(torch.from_numpy(idx))
    b = builder(view, (nnz, k), row_len=1)
    assert b.indices.data_ptr() == view.data_ptr()
    ref = Ref(idx, k, rows_of(m=nnz, row_len=1))
    convert_and_check(ref, b, None, perm=True)


# ======================================================================================================================== scan
@pytest.mark.parametrize('k', [1, T - 1, T, T + 1, 2 * T + 1])
def test_scan_across_tiles(be, k):
    rng = np.random.default_rng(400 + k)
    nnz = 3 * k
    idx = rng.integers(0, k, nnz).astype(np.int32)
    forced = [c for c in (0, T - 1, T, k - 1) if c < k]
    idx[:len(forced)] = forced
    b = builder(idx, (nnz, k), row_len=1)
    counts = np.bincount(idx, minlength=k)
    assert all(counts[c] > 0 for c in forced)
    off = b.offsets()
    assert off.dtype == torch.int32
    np.testing.assert_array_equal(host(off), np.concatenate([[0], np.cumsum(counts)]))


def test_scan_past_one_strip_of_totals(be):
    """1026 tiles: k_scan64_of_totals takes a second trip with 2 totals in it; one block of all columns puts k_t_cursor_init past
    its 524 288-column trip.  Entries in the first tile, on both sides of the strip edge, in the last (5-column) tile, at random."""
    k = (K['scan.strip'] + 1) * T + 5
    n_tiles = -(-k // T)
    assert n_tiles == K['scan.strip'] + 2 and k > STRIP_COLS and k > CURSOR_SPAN
    rng = np.random.default_rng(5)
    parts = [rng.integers(t * T, min((t + 1) * T, k), 1000) for t in (0, K['scan.strip'] - 1, K['scan.strip'], K['scan.strip'] + 1)]
    parts += [np.full(7, k - 1), rng.integers(0, k, 196_000)]
    idx = rng.permutation(np.concatenate(parts)).astype(np.int32)
    nnz = idx.size
    b = builder(idx, (nnz, k), row_len=1)
    ref = Ref(idx, k, rows_of(m=nnz, row_len=1))
    np.testing.assert_array_equal(host(b.csc_indptr), ref.cptr)
    convert_and_check(ref, b, bit_weights(rng, nnz, 4), perm=True)


def _scan(counts, n_cols, out_is_i64, scratch=None):
    """be_csr_to_csc_indptr on a device `counts` tensor: (indptr tensor, grand total read back, scratch)."""
    from brainevent_amd import _array as A
    from brainevent_amd._lib import call, fn
    out = torch.full((n_cols + 1,), -7, dtype=torch.int64 if out_is_i64 else torch.int32, device='cuda')
    if scratch is None:
        scratch = A.workspace(fn('be_csr_to_csc_scratch_bytes')(n_cols))
    total = ctypes.c_int64(-1)
    call('be_csr_to_csc_indptr', A.ptr(counts), n_cols, A.ptr(out), int(out_is_i64), ctypes.byref(total), A.ptr(scratch),
         scratch.numel(), A.stream_ptr())
    return out, int(total.value), scratch


def test_scan_of_wide_counts_and_the_int32_output(be):
    from brainevent_amd._error import KernelExecutionError
    rng = np.random.default_rng(6)
    n = 2 * T + 1
    # (a) counts near 2^40: every carry — wave, workgroup, tile, grand total — needs more than 32 bits
    wide = (1 << 40) - rng.integers(0, 1 << 20, n, dtype=np.int64)
    want = np.concatenate([np.zeros(1, np.uint64), np.cumsum(wide.astype(np.uint64))])
    assert want.dtype == np.uint64 and int(want[-1]) > 1 << 53 and int(want[-1]) < 1 << 63
    out, total, _ = _scan(torch.from_numpy(wide).cuda(), n, 1)
    np.testing.assert_array_equal(host(out).view(np.uint64), want)
    assert total == int(want[-1])
    # (b) the int32 output
    small = rng.integers(0, 100_000, n, dtype=np.int64)
    want = np.concatenate([[0], np.cumsum(small)])
    out, total, scratch = _scan(torch.from_numpy(small).cuda(), n, 0)
    assert out.dtype == torch.int32 and total == int(want[-1]) == int(out[n])
    np.testing.assert_array_equal(host(out), want)
    # (c) a total of exactly 2^31 - 1 is accepted
    assert int(small.sum()) < 2 ** 31 - 1
    edge = small.copy()
    edge[n // 2] += 2 ** 31 - 1 - int(small.sum())
    out, total, _ = _scan(torch.from_numpy(edge).cuda(), n, 0, scratch)
    assert total == 2 ** 31 - 1
    np.testing.assert_array_equal(host(out), np.concatenate([[0], np.cumsum(edge)]))
    # (d) one more is BE_ERR_RANGE (-4) ...
    over = edge.copy()
    over[0] += 1
    with pytest.raises(KernelExecutionError, match=r'status -4: .*does not fit an int32 indptr'):
        _scan(torch.from_numpy(over).cuda(), n, 0, scratch)
    out, total, _ = _scan(torch.from_numpy(over).cuda(), n, 1, scratch)            # the 64-bit output takes it
    assert total == 2 ** 31
    np.testing.assert_array_equal(host(out), np.concatenate([[0], np.cumsum(over)]))
    # ... and the same scratch buffer serves a good call afterwards
    out, total, _ = _scan(torch.from_numpy(small).cuda(), n, 0, scratch)
    np.testing.assert_array_equal(host(out), want)
    assert total == int(want[-1])
    # (e) no columns
    for i64 in (0, 1):
        out, total, _ = _scan(None, 0, i64)
        assert out.tolist() == [0] and total == 0


# ======================================================================================================================== fill
@pytest.mark.parametrize('row_len', [1, 2, 3, 8, 9, 48, 49])
def test_fill_lane_choice_edges(be, row_len):
    """avg_row on both sides of every LPR edge: fixed-length rows (avg_row is the row length itself), then ragged rows with the
    same avg_row whose lengths sit around the lane count, with int32 and int64 indptr."""
    rng = np.random.default_rng(70 + row_len)
    m, k = 300, 257
    idx = rng.integers(0, k, (m, row_len)).astype(np.int32)
    b = builder(idx, (m, k), row_len=row_len)
    assert b.nnz // b.m == row_len
    convert_and_check(Ref(idx.reshape(-1), k, rows_of(m=m, row_len=row_len)), b, bit_weights(rng, m * row_len, 4), perm=True)
    for ptr_dtype in (np.int32, np.int64):
        m, k, ptr, idx, w, ref = ragged_case(row_len, ptr_dtype)
        lens = np.diff(ptr)
        lpr = lpr_of(row_len)
        assert idx.size // m == row_len and lens.max() == 5000 and (lens[1:101] == 0).all()
        assert {0, 1, lpr - 1, lpr, lpr + 1} <= set(lens.tolist())
        b = builder(idx, (m, k), ptr)
        assert b.indptr.dtype == (torch.int32 if ptr_dtype == np.int32 else torch.int64)
        convert_and_check(ref, b, w, perm=True)


@pytest.mark.parametrize('lpr', LPRS)
def test_fill_past_one_trip(be, lpr):
    m, k, row_len, idx, w, ref = fixed_case(lpr)
    assert m > fill_span(lpr) and lpr_of((m * row_len) // m) == lpr and m * row_len <= 2_100_000
    b = builder(idx, (m, k), row_len=row_len)
    rows, _, _ = convert_and_check(ref, b, w, perm=True)
    per_row = np.bincount(rows, minlength=m)
    assert (per_row[fill_span(lpr):] == row_len).all() and len(per_row) == m         # the rows of the second trip are there


def test_fill_every_weight_width_and_perm_width(be):
    from brainevent_amd import _array as A
    from brainevent_amd._error import KernelExecutionError
    from brainevent_amd._lib import call
    rng = np.random.default_rng(9)
    m, k = 3000, 2000
    lens = rng.integers(0, 41, m)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(ptr[-1])
    assert lpr_of(nnz // m) == 16
    idx = rng.integers(0, k, nnz).astype(np.int32)
    ref = Ref(idx, k, rows_of(ptr))
    b = builder(idx, (m, k), ptr)
    weights = {wb: bit_weights(rng, nnz, wb) for wb in (2, 4, 8)}
    for wb in (0, 2, 4, 8):
        for perm in (True, False):
            convert_and_check(ref, b, weights.get(wb), perm=perm)

    def direct(wb, perm_is_i64=1):
        data = as_float(weights[wb]) if wb in weights else (torch.zeros(nnz, device='cuda') if wb else None)
        rows = torch.full((nnz,), -1, dtype=torch.int32, device='cuda')
        perm = torch.full((nnz,), -1, dtype=torch.int64, device='cuda')       # (all bits set: a 32-bit store would show)
        w_out = None if data is None else torch.zeros_like(data)
        cursor = torch.empty(k, dtype=torch.int64, device='cuda')
        call('be_csr_to_csc_fill_block', A.ptr(b.indices), A.ptr(b.indptr), 0, -1, m, nnz, 0, k, A.ptr(b.csc_indptr), A.ptr(cursor),
             A.ptr(rows), A.ptr(perm), perm_is_i64, A.ptr(data), wb, A.ptr(w_out), A.stream_ptr())
        return host(rows), bits_of(w_out), host(perm)

    for wb in (0, 2, 4, 8):                                                   # k_t_fill<16, int64_t, WB> with a perm
        rows, w_out, perm = direct(wb)
        assert perm.dtype == np.int64
        ref.check(ref.cptr, rows, perm, weights.get(wb), w_out)
    with pytest.raises(KernelExecutionError, match=r'status -1: .*weight element size must be 0, 2, 4 or 8'):
        direct(3)


def test_column_blocks_at_scale(be):
    """The LPR-16 matrix of test_fill_past_one_trip in column blocks: an empty one, one of a single column, cuts one short of and
    one past a multiple of the 256 columns a workgroup of k_t_cursor_init takes.  Every block is its slice of the whole
    conversion, and together they hold every entry once."""
    m, k, row_len, idx, w, ref = fixed_case(16)
    edges = [0, 1, 1, BLOCK - 1, BLOCK + 1, k // 2, k - 1, k]
    assert edges == sorted(edges) and (k // 2) % BLOCK != 0 and (k - 1) % BLOCK != 0
    b = builder(idx, (m, k), row_len=row_len)
    perms = []
    for c0, c1 in zip(edges[:-1], edges[1:]):
        assert b.block_entries(c0, c1) == int(ref.cptr[c1] - ref.cptr[c0])
        rows, w_out, perm = convert_and_check(ref, b, w, perm=True, c0=c0, c1=c1)
        convert_and_check(ref, b, w, perm=False, c0=c0, c1=c1)
        assert rows.size == b.block_entries(c0, c1)
        perms.append(perm)
    np.testing.assert_array_equal(np.sort(np.concatenate(perms)), np.arange(m * row_len))


@pytest.mark.parametrize('wb', [0, 4])
def test_column_block_without_entries(be, wb):
    """A block whose columns hold nothing — no columns at all, or a stretch of the matrix that no row reaches — is three empty
    arrays.  (CscBuilder.block used to hand the library the NULL pointers of its empty outputs: KernelExecutionError, with or
    without weights; found by the empty block of test_column_blocks_at_scale.)"""
    rng = np.random.default_rng(10)
    m, k, row_len = 50, 300, 9
    idx = rng.integers(0, 100, (m, row_len)).astype(np.int32)
    idx[idx >= 40] += 200                                                    # columns 40 ... 239 stay empty
    w = bit_weights(rng, idx.size, wb) if wb else None
    ref = Ref(idx.reshape(-1), k, rows_of(m=m, row_len=row_len))
    b = builder(idx, (m, k), row_len=row_len)
    for c0, c1 in ((40, 240), (100, 101), (7, 7), (0, 0), (k, k)):
        assert b.block_entries(c0, c1) == 0
        for perm in (True, False):
            rows, w_out, p = convert_and_check(ref, b, w, perm=perm, c0=c0, c1=c1)
            assert rows.size == 0 and (p is None or p.size == 0) and (w_out is None or w_out.size == 0)
    convert_and_check(ref, b, w, perm=True, c0=39, c1=241)                   # the empty stretch inside a block that holds entries
    convert_and_check(ref, b, w, perm=True)


# ====================================================================================================================== gather
@pytest.mark.parametrize('perm_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('wb', [2, 4, 8])
def test_gather_by_perm_past_one_trip(be, wb, perm_dtype):
    from brainevent_amd import _array as A
    from brainevent_amd._convert import gather_by_perm
    from brainevent_amd._lib import call
    n, n_src = BLOCK * K['gather.grid_cap'] + 3, 1000
    assert n > GATHER_SPAN
    rng = np.random.default_rng(110 + wb)
    src = bit_weights(rng, n_src, wb)
    perm = rng.integers(0, n_src, n)                                           # repeats: not a permutation
    d_src, d_perm = as_float(src), torch.from_numpy(perm).cuda().to(perm_dtype)
    out = gather_by_perm(d_src, d_perm)
    assert out.dtype == d_src.dtype and out.shape == (n,)
    np.testing.assert_array_equal(bits_of(out), src[perm])
    # into a given buffer: same pointer, nothing written past n
    guard = bit_weights(rng, n + 64, wb)
    buf = as_float(guard)
    got = gather_by_perm(d_src, d_perm, out=buf[:n])
    assert got.data_ptr() == buf.data_ptr()
    after = bits_of(buf)
    np.testing.assert_array_equal(after[:n], src[perm])
    np.testing.assert_array_equal(after[n:], guard[n:])
    # nothing to do: no launch (the entry point returns before it looks at its pointers)
    empty = gather_by_perm(d_src, d_perm[:0], out=buf[:0])
    assert empty.numel() == 0
    call('be_gather_by_perm', A.ptr(None), wb, A.ptr(None), int(perm_dtype == torch.int64), 0, A.ptr(None), A.stream_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits_of(buf), after)


# ====================================================================================================================== mirror
def _check_mirror(ref, mr, w, data):
    assert mr.indptr is not None and mr.indices is not None and mr.perm is not None and mr.data is not None
    ref.check(host(mr.indptr), host(mr.indices), host(mr.perm), w, bits_of(mr.data))
    np.testing.assert_array_equal(host(mr.counts), np.diff(ref.cptr))
    assert torch.equal(mr.data.view(torch.int32), data.reshape(-1)[mr.perm.long()].view(torch.int32))


def _check_refresh(be, container, mr, data, k, rng):
    buf = mr.data.data_ptr()
    data.mul_(-0.5)
    v = torch.from_numpy(rng.random(k) < 0.1).cuda()
    container @ be.BinaryArray(v)                                                   # one gather-side product
    assert container.buffers['mirror'] is mr and mr.data.data_ptr() == buf
    assert torch.equal(mr.data.view(torch.int32), data.reshape(-1)[mr.perm.long()].view(torch.int32))


@pytest.mark.parametrize('avg', [1, 2, 3, 8, 9, 48, 49])
def test_mirror_arrays_are_the_conversion(be, avg):
    """What `CSR.build_mirror(keep_raw=True)` holds for the ragged matrices of test_fill_lane_choice_edges passes the checker,
    and an in-place weight update reaches `mr.data` through `mr.perm` in the same buffer."""
    rng = np.random.default_rng(120 + avg)
    m, k, ptr, idx, _, ref = ragged_case(avg, np.int32)
    w = finite_bit_weights(rng, idx.size)
    data = as_float(w)
    csr = be.CSR((data, torch.tensor(idx).cuda(), torch.tensor(ptr).cuda()), shape=(m, k))
    mr = csr.build_mirror(keep_raw=True)
    _check_mirror(ref, mr, w, data)
    _check_refresh(be, csr, mr, data, k, rng)


def test_fixed_number_mirror_arrays_are_the_conversion(be):
    """The same for `FixedNumPerPre.prepare(mirror=True)` on the LPR-16 matrix of test_fill_past_one_trip."""
    rng = np.random.default_rng(12)
    m, k, row_len, idx, _, ref = fixed_case(16)
    w = finite_bit_weights(rng, idx.size)
    data = as_float(w).reshape(m, row_len)
    fcn = be.FixedNumPerPre((data, torch.tensor(idx).cuda()), shape=(m, k)).prepare(mirror=True)
    mr = fcn.buffers['mirror']
    _check_mirror(ref, mr, w, data)
    _check_refresh(be, fcn, mr, data, k, rng)
