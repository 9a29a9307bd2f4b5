"""The scatter plan's build — ``count -> scan -> fill`` of ``csrc/be_csr_plan.hip`` — against the host restatement of the layouts
(``tests/plan_layout_cases.py``).  Every comparison is equality: the segment table as a whole, the defined bytes of every block
(never the alignment padding behind them, which no kernel writes), ``blob_bytes == units << 7`` and the kept order of every row.
No tolerance anywhere in this file.

Each case is the smallest that crosses the bound it names; the bounds are ``plan_layout_cases.THRESHOLDS``, which
``tests/test_plan_layout_cpu.py`` holds against the source.  Blobs are allocated poisoned (0xA5), so a defined byte that no kernel
writes fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch

import plan_layout_cases as L
from brainevent_amd import _array as A
from brainevent_amd import _csr as C
from brainevent_amd._csr_f8 import Q8Plan
from brainevent_amd._error import KernelExecutionError
from brainevent_amd._lib import call, fn

pytestmark = pytest.mark.gpu

T = L.THRESHOLDS
U16_M = T['grid.u16_cap'] + 3            # rows with which the u16 row grids take a second trip
SORTED_M = T['grid.sorted_cap'] + 3      # ... and the d8 / h8 / q8 ones
LAYOUT_CODE = {'u16w': 0, 'u16c': 0, 'd8': 1, 'h8': 2}
PY_LAYOUT = {'u16w': 'u16', 'u16c': 'u16', 'd8': 'd8', 'h8': 'h8'}
HOMO = {'u16w': 0, 'u16c': 1, 'd8': 0, 'h8': 1}
TORCH_DTYPE = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}
FINITE = {'e4m3': [c for c in range(256) if c & 0x7f != 0x7f], 'e5m2': [c for c in range(256) if c & 0x7c != 0x7c]}


# ------------------------------------------------------------------------------------------------------------ helpers
def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def weights_for(layout, rng, n, dtype='f32'):
    """Multiples of 2^-8 in [-2, 2], rounded once to the dtype asked for (the encoder is given the rounded ones), zeros and a
    negative zero among them; codes for q8; the one shared weight of the counted layouts."""
    if layout in ('u16c', 'h8'):
        return torch.tensor([0.5])
    if layout == 'q8':
        return torch.from_numpy(rng.integers(0, 256, n).astype(np.uint8))
    w = (rng.integers(-512, 513, n) / 256.0).astype(np.float32)
    if n > 4:
        w[1], w[3] = -0.0, 0.0
    return torch.from_numpy(w).to(TORCH_DTYPE[dtype])


def ragged(rng, m, k, max_len=12):
    lens = rng.integers(0, max_len + 1, m)
    lens[::11] = 0
    lens[-1] = max_len
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rng.integers(0, k, int(ptr[-1])).astype(np.int32), ptr


class Built:
    pass


def build_raw(layout, pay, idx, ptr_or_len, m, k, shift, W, *, ptr_dtype=np.int32, with_order=True, fill_with_order=True):
    """count -> scan -> fill through the C entry points.  The blob is poisoned before the fill."""
    b = Built()
    st = A.stream_ptr()
    d_idx = dev(idx)
    fixed = np.ndim(ptr_or_len) == 0
    d_ptr = None if fixed else dev(np.asarray(ptr_or_len).astype(ptr_dtype))
    row_len = int(ptr_or_len) if fixed else -1
    is64 = int(d_ptr is not None and d_ptr.dtype == torch.int64)
    _, ns = L._geometry(k, shift, W)
    seg = torch.full((ns * m * 2,), -1, dtype=torch.int32, device='cuda')
    nnz = int(d_idx.numel())
    order = torch.full((max(nnz, 1),), -1, dtype=torch.int16, device='cuda') if with_order and layout in L.SORTED else None
    blob_bytes = ctypes.c_int64(-1)
    d_pay = dev(pay)
    if layout == 'q8':
        scratch = A.workspace(fn('be_scatter_plan_q8_scratch_bytes')(m, k, shift, W))
        call('be_scatter_plan_q8_count', A.ptr(d_idx), A.ptr(d_ptr), is64, row_len, m, k, shift, W, A.ptr(seg), A.ptr(scratch),
             scratch.numel(), ctypes.byref(blob_bytes), A.ptr(order), st)
    else:
        scratch = A.workspace(fn('be_scatter_plan_scratch_bytes')(m, k, shift, W))
        call('be_scatter_plan_count_ordered', A.ptr(d_idx), A.ptr(d_ptr), is64, row_len, m, k, shift, W, HOMO[layout],
             LAYOUT_CODE[layout], A.ptr(seg), A.ptr(scratch), scratch.numel(), ctypes.byref(blob_bytes), A.ptr(order), st)
    b.blob_bytes = int(blob_bytes.value)
    b.seg, b.order = seg, order
    b.d = (d_pay, d_idx, d_ptr, is64, row_len)
    b.geom = (m, k, shift, W)
    b.layout = layout
    fill_raw(b, fill_with_order)
    return b


def fill_raw(b, with_order=True):
    d_pay, d_idx, d_ptr, is64, row_len = b.d
    m, k, shift, W = b.geom
    st = A.stream_ptr()
    b.blob = torch.full((b.blob_bytes + 128,), 0xA5, dtype=torch.uint8, device='cuda')
    order = b.order if with_order else None
    b.maxabs = None
    if b.layout == 'q8':
        call('be_scatter_plan_q8_fill', A.ptr(d_pay), A.ptr(d_idx), A.ptr(d_ptr), is64, row_len, m, k, shift, W, A.ptr(b.seg),
             A.ptr(b.blob), A.ptr(order), st)
    else:
        maxabs = torch.full((2,), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
        call('be_scatter_plan_fill_ordered', A.ptr(d_pay), HOMO[b.layout], A.wcode(d_pay), A.ptr(d_idx), A.ptr(d_ptr), is64, row_len,
             m, k, shift, W, LAYOUT_CODE[b.layout], A.ptr(b.seg), A.ptr(b.blob), A.ptr(maxabs), A.ptr(order), st)
        b.maxabs = maxabs.cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()


def check_table(enc, seg, blob_bytes, tag=''):
    got = seg.cpu().numpy().view(np.uint32).reshape(enc.m, enc.n_slices, 2)
    if not np.array_equal(got, enc.seg):
        r, s, f = (int(v[0]) for v in np.nonzero(got != enc.seg))
        raise AssertionError(f'{tag}: seg[{r}][{s}].{"xy"[f]} is {got[r, s, f]:#x}, the layout says {enc.seg[r, s, f]:#x} '
                             f'({int((got != enc.seg).sum())} words differ)')
    assert blob_bytes == enc.units << 7, f'{tag}: blob_bytes {blob_bytes}, the layout says {enc.units << 7}'


def check_blocks(enc, blob, tag=''):
    assert blob.numel() >= enc.units << 7
    bad = L.blocks_mismatch(enc, blob.cpu().numpy())
    assert bad is None, f'{tag}: {bad}'


def check_table_and_blocks(enc, seg, blob, blob_bytes, tag=''):
    check_table(enc, seg, blob_bytes, tag)
    check_blocks(enc, blob, tag)


def check_stats(maxabs, pay, tag=''):
    """maxabs_bits after a fill: the largest |w| bit pattern and the smallest non-zero one (0 / 0xffffffff when there is none)."""
    ab = L.weight_bits(pay) & np.uint32(0x7fffffff)
    nz = ab[ab != 0]
    want = (int(ab.max(initial=0)), int(nz.min()) if nz.size else 0xffffffff)
    assert (int(maxabs[0]), int(maxabs[1])) == want, f'{tag}: maxabs_bits {maxabs.tolist()}, the weights say {want}'


def check_raw(b, pay, idx, ptr_or_len, tag=''):
    m, k, shift, W = b.geom
    enc = L.encode(b.layout, pay, idx, ptr_or_len, m, k, shift, W)
    check_table(enc, b.seg, b.blob_bytes, tag)
    if b.order is not None:
        got = b.order.cpu().numpy().view(np.uint16)[:idx.size]
        want = L.expected_order(idx, ptr_or_len, m)
        if not np.array_equal(got, want):
            ptr = L.row_pointers(ptr_or_len, m)
            r = int(np.searchsorted(ptr, np.flatnonzero(got != want)[0], side='right') - 1)
            raise AssertionError(f'{tag}: the kept order of row {r} ({ptr[r + 1] - ptr[r]} entries) is not the sorted one')
    check_blocks(enc, b.blob, tag)
    if b.maxabs is not None and not HOMO[b.layout]:
        check_stats(b.maxabs, pay, tag)
    return enc


# ------------------------------------------------------------------------------------------------------------ 1. row grids
GRID_CASES = [(lay, 'f32', p) for lay in L.LAYOUTS for p in ('i32', 'i64', 'fixed')] + \
             [(lay, dt, 'i32') for lay in ('u16w', 'd8') for dt in ('f16', 'bf16')]


@pytest.mark.parametrize('layout,dtype,rows', GRID_CASES)
def test_row_grid_second_trip(layout, dtype, rows):
    """More rows than the count and fill grids have workgroups: every grid-stride loop over rows takes a second trip.  Rows of 0-12
    entries over 3 slices (the last one partial); f32 / f16 / bf16 weights; int32 / int64 row pointers; fixed-length rows."""
    rng = np.random.default_rng(11)
    m = U16_M if layout.startswith('u16') else SORTED_M
    k, W, shift = 100, 40, 6
    if rows == 'fixed':
        ptr_or_len = 5
        idx = rng.integers(0, k, m * 5).astype(np.int32)
    else:
        idx, ptr_or_len = ragged(rng, m, k)
    pay = weights_for(layout, rng, idx.size, dtype)
    b = build_raw(layout, pay, idx, ptr_or_len, m, k, shift, W, ptr_dtype=np.int64 if rows == 'i64' else np.int32)
    check_raw(b, pay, idx, ptr_or_len, f'{layout}/{dtype}/{rows}')


@pytest.mark.parametrize('layout', ['u16w', 'u16c', 'd8', 'h8'])
def test_python_build_gives_the_same_plan(layout):
    """``ScatterPlan.build`` (what the products use) over the same row counts: table, blocks, size and the kept order."""
    rng = np.random.default_rng(12)
    m = U16_M if layout.startswith('u16') else SORTED_M
    k, W, shift = 100, 40, 6
    idx, ptr = ragged(rng, m, k)
    w = weights_for(layout, rng, idx.size)
    plan = C.ScatterPlan.build(dev(w), dev(idx), dev(ptr), shape=(m, k), slice_shift=shift, slice_width=W, layout=PY_LAYOUT[layout],
                               keep_order=True)
    assert plan.layout == LAYOUT_CODE[layout] and plan.n_slices == 3
    enc = L.encode(layout, w, idx, ptr, m, k, shift, W)
    check_table_and_blocks(enc, plan.seg, plan.blob, plan.blob.numel() - 128, layout)
    if layout == 'd8':
        np.testing.assert_array_equal(plan.order.cpu().numpy().view(np.uint16), L.expected_order(idx, ptr))


# ------------------------------------------------------------------------------------------------------------ 2. the scan
def scan_table(x):
    """be_scatter_plan_begin + be_scatter_plan_scan over a synthetic table whose .x fields are `x` (one slice of 16 columns per row)."""
    n = int(x.size)
    table = np.stack([x.astype(np.uint32), np.arange(n, dtype=np.uint32) * np.uint32(2654435761)], axis=1)
    seg = dev(table.view(np.int32))
    scratch = A.workspace(fn('be_scatter_plan_scratch_bytes')(n, 16, 4, 0))
    st = A.stream_ptr()
    out = ctypes.c_int64(-1)
    call('be_scatter_plan_begin', n, 16, 4, 0, A.ptr(scratch), scratch.numel(), st)
    call('be_scatter_plan_scan', n, 16, 4, 0, A.ptr(seg), A.ptr(scratch), scratch.numel(), ctypes.byref(out), st)
    torch.cuda.synchronize()
    return seg.cpu().numpy().view(np.uint32).reshape(n, 2), table, int(out.value)


def check_scan(x):
    got, table, blob_bytes = scan_table(x)
    want = np.concatenate([[0], np.cumsum(x.astype(np.uint64))[:-1]])
    bad = np.flatnonzero(got[:, 0] != want)
    assert bad.size == 0, (f'block start {bad[0]} (chunk {bad[0] // T["scan.chunk"]}) is {got[bad[0], 0]}, the running sum is '
                           f'{want[bad[0]]}; {bad.size} starts differ')
    np.testing.assert_array_equal(got[:, 1], table[:, 1])                 # the second words are not the scan's
    assert blob_bytes == int(x.astype(np.uint64).sum()) << 7


ONE_PASS = T['scan.chunk'] * T['scan.pass']


@pytest.mark.parametrize('n', [ONE_PASS - 1, ONE_PASS, ONE_PASS + 1, ONE_PASS + 3 * T['scan.chunk'] * 17 + 5, 1, T['scan.chunk'] + 1])
def test_scan_of_a_synthetic_table(n):
    """The three-kernel scan with its carry, around and past one pass of 1024 chunks of 2048: units in [0, 7] with runs of zeros
    (one longer than a chunk, one across the pass boundary); every block start is the running sum."""
    rng = np.random.default_rng(n % 1000)
    x = rng.integers(0, 8, n).astype(np.uint32)
    for lo in rng.integers(0, n, 40):
        x[lo:lo + int(rng.integers(1, 3000))] = 0
    x[max(0, ONE_PASS - 700):ONE_PASS + 900] = 0
    if n > 5000:
        x[ONE_PASS - 701 if n >= ONE_PASS else 100] = 7
    x[-1] = 5
    check_scan(x)


@pytest.mark.parametrize('layout', ['u16w', 'd8'])
def test_scan_past_one_pass_end_to_end(layout):
    """A whole build whose table is longer than one pass of the scan: u16 at slice_shift 4 (4096 slices of 16 columns: the
    per-slice loops of count and fill take 16 trips), d8 at 1024 slices of 64 columns."""
    rng = np.random.default_rng(21)
    if layout == 'u16w':
        k, W, shift, m = T['kMaxSlices'] * 16, 16, 4, 540
    else:
        k, W, shift, m = T['kD8MaxSlices'] * 64, 64, 6, 2100
    assert m * (k // W) > ONE_PASS + T['scan.chunk']
    idx, ptr = ragged(rng, m, k)
    idx[ptr[-2]:ptr[-1]] = np.arange(k - 12, k)[::-1]                     # the last row ends in the last slice
    pay = weights_for(layout, rng, idx.size)
    b = build_raw(layout, pay, idx, ptr, m, k, shift, W)
    check_raw(b, pay, idx, ptr, layout)


# ------------------------------------------------------------------------------------------------------------ 3. 32-bit block index
def test_block_index_of_32_bits():
    """Units summing to 2^32 - 1 pass (the last start is still a uint32) and report (2^32 - 1) << 7 bytes; 2^32 is refused with the
    range error, and a clean call follows.  No blob is allocated: only the table is scanned."""
    rng = np.random.default_rng(3)
    n = 2 * T['scan.chunk'] + 5
    x = rng.integers(0, 8, n).astype(np.uint32)
    x[7] = 0
    x[7] = (1 << 32) - 1 - int(x.astype(np.uint64).sum())
    check_scan(x)
    assert scan_table(x)[2] == ((1 << 32) - 1) << 7
    x[n - 2] += 1
    with pytest.raises(KernelExecutionError, match='32-bit block index'):
        scan_table(x)
    x[7] = 3
    check_scan(x)


# ------------------------------------------------------------------------------------------------------------ 4. the row sort
def sort_rows(rng, k):
    """(name, columns, branch the row must take, largest bucket or None) at col_range == k."""
    asc = np.sort(rng.integers(0, k, 5000))
    rows = [('len0', np.zeros(0, np.int64), 'short-ascending', None),
            ('len1', np.array([k - 1]), 'short-ascending', None),
            ('len2', np.array([77, 5]), 'short-bitonic', None),
            ('len255', rng.integers(0, k, 255), 'short-bitonic', None),
            ('len256', rng.integers(0, k, 256), 'short-bitonic', None),
            ('len257', rng.integers(0, k, 257), 'counting', None),
            ('short ascending', np.sort(rng.integers(0, k, 200)), 'short-ascending', None),
            ('ascending', asc, 'ascending', None),
            ('one inversion at the end', np.concatenate([asc, [asc[-1] - 1]]), 'counting', None),
            ('3000 copies', np.full(3000, 777), 'ascending', 3000),
            ('3000 copies and 2000 others', rng.permutation(np.concatenate([np.full(3000, 777), rng.integers(0, k, 2000)])),
             'fallback', None),
            ('clustered', rng.integers(40_000, 40_300, 6000), 'fallback', None),
            ('longest', rng.integers(0, k, T['kD8MaxRow']), 'counting', None)]
    for big, branch in ((64, 'counting'), (65, 'counting'), (256, 'counting'), (257, 'fallback')):
        rows.append((f'bucket of {big}', L.row_with_bucket(rng, 600, big, k, bucket=3), branch, big))
    return rows


@pytest.mark.parametrize('layout', ['d8', 'h8'])
def test_every_branch_of_the_row_sort(layout):
    """Each row lands in the branch of ``d8_sort_row`` it names (``sort_branch``), narrow buckets (k = 90 000: 32-bit keys): the
    kept order and the blocks are the sorted ones, when the fill reads the order back and when it sorts again."""
    rng = np.random.default_rng(41)
    k = 90_000
    W, shift = (18_000, 14) if layout == 'd8' else (30_000, 15)
    rows = sort_rows(rng, k)
    seen = set()
    for name, cols, branch, largest in rows:
        sb = L.sort_branch(len(cols), W * -(-k // W), cols)
        assert sb.branch == branch and (largest is None or sb.largest == largest), (name, sb)
        seen |= {branch} | set(sb.forms)
    assert seen == {'short-ascending', 'short-bitonic', 'ascending', 'counting', 'fallback', 'rank32', 'rank4'}
    assert L.sort_branch(600, k, rows[-4][1]).forms == {'rank32'} and 'rank4' in L.sort_branch(600, k, rows[-3][1]).forms
    idx, ptr = L.csr_of([r[1] for r in rows])
    m = len(rows)
    pay = weights_for(layout, rng, idx.size)
    b = build_raw(layout, pay, idx, ptr, m, k, shift, W)
    check_raw(b, pay, idx, ptr, f'{layout}, the fill reads the order')
    fill_raw(b, with_order=False)
    check_raw(b, pay, idx, ptr, f'{layout}, the fill sorts again')


@pytest.mark.parametrize('layout', ['d8', 'h8'])
def test_wide_buckets_take_64_bit_keys(layout):
    """k = 2 000 000 at the widest slices of the layout: rows of 257-300 entries have buckets of at least 2^18 columns, whose rank
    sort compares 64-bit keys."""
    rng = np.random.default_rng(42)
    k = 2_000_000
    W, shift = (T['kD8MaxWidth'], 14) if layout == 'd8' else (T['kH8MaxWidth'], 15)
    lens = [257, 300] + list(rng.integers(257, 301, 30))
    rows = [rng.integers(0, k, int(n)) for n in lens]
    rows[2][:40] = rows[2][40]                                  # one column many times
    for r in rows:
        sb = L.sort_branch(len(r), W * -(-k // W), r)
        assert sb.branch == 'counting' and 'rank64' in sb.forms and 'rank32' not in sb.forms, sb
    idx, ptr = L.csr_of(rows)
    pay = weights_for(layout, rng, idx.size)
    b = build_raw(layout, pay, idx, ptr, len(rows), k, shift, W)
    check_raw(b, pay, idx, ptr, f'{layout}, the fill reads the order')
    fill_raw(b, with_order=False)
    check_raw(b, pay, idx, ptr, f'{layout}, the fill sorts again')


@pytest.mark.parametrize('layout', ['d8', 'h8', 'q8'])
def test_too_long_row_is_refused(layout):
    """A row of 16385 entries is refused by name with the range error; a clean build follows."""
    rng = np.random.default_rng(43)
    k, W, shift = 50_000, 17_000, 15 if layout == 'h8' else 14
    rows = [rng.integers(0, k, 10), rng.integers(0, k, T['kD8MaxRow'] + 1), rng.integers(0, k, 3)]
    idx, ptr = L.csr_of(rows)
    pay = weights_for(layout, rng, idx.size)
    with pytest.raises(KernelExecutionError, match='16385|16384'):
        build_raw(layout, pay, idx, ptr, 3, k, shift, W)
    rows[1] = rows[1][:-1]
    idx, ptr = L.csr_of(rows)
    pay = weights_for(layout, rng, idx.size)
    check_raw(build_raw(layout, pay, idx, ptr, 3, k, shift, W), pay, idx, ptr, layout)


# ------------------------------------------------------------------------------------------------------------ 5. slices, 6. escapes
WIDTHS = [(lay, W) for lay in L.LAYOUTS for W in (3, 255, 257, 19999, 20000)] + [('h8', 39999), ('h8', 40000)]


@pytest.mark.parametrize('layout,W', WIDTHS)
def test_slice_arithmetic(layout, W):
    """Column -> (slice, local column) without a division: columns at s * W - 1, s * W, s * W + 1 of the first, a middle and the
    last slice, column k - 1, local columns 0 and W - 1, at widths next to the powers of two and at the layouts' caps."""
    rng = np.random.default_rng(50 + W)
    k = 7 * W + max(1, W // 2)
    rows = L.edge_rows(rng, k, W)
    idx, ptr = L.csr_of(rows)
    pay = weights_for(layout, rng, idx.size)
    shift = 15 if W > 16384 else max(4, int(np.ceil(np.log2(W))))
    b = build_raw(layout, pay, idx, ptr, len(rows), k, shift, W)
    check_raw(b, pay, idx, ptr, f'{layout}/{W}')


@pytest.mark.parametrize('layout', L.SORTED)
def test_escapes(layout):
    """Gaps of 254, 255, 256, 510, 511 and one of W - 1 inside a slice, alone and chained; a block whose one escape pushes it over
    a lane-group boundary and over a 128-byte unit."""
    rng = np.random.default_rng(60)
    W, k, shift = 1200, 3000, 11
    rows = L.edge_rows(rng, k, W) + L.escape_rows(layout, W + 7)
    long_block = len(rows) - 1
    idx, ptr = L.csr_of(rows)
    pay = weights_for(layout, rng, idx.size)
    if layout == 'q8':
        pay[::5] = 0                                             # the code 0x00 at every kind of gap
    b = build_raw(layout, pay, idx, ptr, len(rows), k, shift, W)
    enc = check_raw(b, pay, idx, ptr, layout)
    groups = int(enc.seg[long_block, 1, 1] & 0xffff)
    assert groups * L.GROUP_BYTES[layout] > 128 and (groups - 1) * L.GROUP_BYTES[layout] <= 128
    assert int((enc.data == 255).sum()) > 20


# ------------------------------------------------------------------------------------------------------------ 7. q8
@pytest.mark.parametrize('fmt', ['e4m3', 'e5m2'])
def test_q8_every_code(fmt):
    """``Q8Plan.build``: every finite code of the format is stored, the code 0x00 among the real entries (first of a block, behind
    a gap that needs escapes, at a remainder of 255: it must not be taken for an escape or a pad), rows past the grid cap."""
    rng = np.random.default_rng(70)
    m, k, W, shift = SORTED_M, 3000, 1200, 11
    idx, ptr = ragged(rng, m, k)
    codes = np.array(FINITE[fmt], np.uint8)[rng.integers(0, len(FINITE[fmt]), idx.size)]
    codes[:len(FINITE[fmt])] = FINITE[fmt]
    r = m - 1                                                  # the last row: 12 entries
    idx[ptr[r]:ptr[r] + 6] = [1200, 1200 + 255, 1200 + 255 + 600, 5, 5 + 255, 2999]
    codes[ptr[r]:ptr[r] + 6] = [0x00, 0x00, 0x00, 0x38, 0x00, 0x00]
    assert set(codes.tolist()) == set(FINITE[fmt])
    tcodes = torch.from_numpy(codes).view(torch.float8_e4m3fn if fmt == 'e4m3' else torch.float8_e5m2)
    plan = Q8Plan.build(tcodes.cuda(), dev(idx), dev(ptr), shape=(m, k), slice_shift=shift, slice_width=W)
    enc = L.encode('q8', codes, idx, ptr, m, k, shift, W)
    check_table_and_blocks(enc, plan.seg, plan.blob, plan.blob.numel() - 128, fmt)


# ------------------------------------------------------------------------------------------------------------ 8. build_from_blocks
@pytest.mark.parametrize('layout,rows', [('u16w', 'i32'), ('d8', 'i64'), ('h8', 'i32'), ('d8', 'fixed')])
def test_build_from_blocks(layout, rows):
    """Row blocks of 384 over 2048 + 3 rows: the table (one scan over per-block counts) and the bytes of the encoder."""
    rng = np.random.default_rng(80)
    m, k, W, shift = SORTED_M, 100, 40, 6
    if rows == 'fixed':
        idx, ptr = rng.integers(0, k, m * 5).astype(np.int32), (np.arange(m + 1) * 5).astype(np.int32)
    else:
        idx, ptr = ragged(rng, m, k)
    w = weights_for(layout, rng, idx.size)
    d_w, d_idx = dev(w), dev(idx)

    def get_block(r0, r1):
        lo, hi = int(ptr[r0]), int(ptr[r1])
        rel = None if rows == 'fixed' else dev((ptr[r0:r1 + 1] - ptr[r0]).astype(np.int64 if rows == 'i64' else np.int32))
        return (d_w if HOMO[layout] else d_w[lo:hi]), d_idx[lo:hi], rel

    plan = C.ScatterPlan.build_from_blocks(get_block, 384, shape=(m, k), nnz=idx.size, max_row_len=int(np.diff(ptr).max()),
                                           homo=bool(HOMO[layout]), slice_shift=shift, slice_width=W, layout=PY_LAYOUT[layout])
    assert plan.layout == LAYOUT_CODE[layout]
    enc = L.encode(layout, w, idx, ptr, m, k, shift, W)
    check_table_and_blocks(enc, plan.seg, plan.blob, plan.blob.numel() - 128, f'{layout}/{rows}')


# ------------------------------------------------------------------------------------------------------------ 9. refreshes
@pytest.mark.parametrize('route,keep_order', [('plan-d8', True), ('plan-d8', False), ('plan-u16', False)])
def test_plastic_rows_and_refresh_weights(route, keep_order):
    """After two ``update_on_pre`` steps on an armed container (the second with every row firing: more listed rows than the row
    refresh has workgroups) the table is unchanged and the blocks are the encoder's for the new weights; the same after a full
    ``refresh_weights``.  (The slot table is not looked at.)"""
    import brainevent_amd as be
    rng = np.random.default_rng(90)
    layout = 'd8' if route == 'plan-d8' else 'u16w'
    m = (SORTED_M if layout == 'd8' else U16_M) + 400
    k, W, shift = 6000, 2000, 11
    idx, ptr = ragged(rng, m, k)
    w = (rng.integers(0, 257, idx.size) / 256.0).astype(np.float32)
    M = be.CSR((dev(w), dev(idx), dev(ptr)), shape=(m, k))
    if layout == 'd8':
        plan = C.ScatterPlan.build(M.data, dev(idx), dev(ptr), shape=(m, k), slice_width=W, layout='d8', keep_order=keep_order)
        assert (plan.order is not None) == keep_order
    else:
        plan = C.ScatterPlan.build(M.data, dev(idx), dev(ptr), shape=(m, k), slice_shift=shift, slice_width=W, layout='u16')
    shift = plan.slice_shift
    M.buffers['scatter_plan'] = plan
    M.prepare(plastic=(0.0, 1.0))
    assert M.plastic_state['route'] == route and M.buffers['scatter_plan'] is plan
    check_table_and_blocks(L.encode(layout, w, idx, ptr, m, k, shift, W), plan.seg, plan.blob, plan.blob.numel() - 128, 'built')
    for step, fire in enumerate((0.3, 1.0)):
        spk = rng.random(m) < fire
        trace = (rng.integers(-256, 257, k) / 256.0).astype(np.float32)
        M.update_on_pre(dev(spk), dev(trace), 0.0, 1.0, inplace=True)
        w_new = M.data.reshape(-1).cpu().numpy()
        assert not np.array_equal(w_new, w)
        w = w_new
        assert M.buffers['scatter_plan'] is plan and not plan.is_stale(M.data)
        enc = L.encode(layout, w, idx, ptr, m, k, shift, W)
        check_table_and_blocks(enc, plan.seg, plan.blob, plan.blob.numel() - 128, f'{route}: row refresh {step}')
    w2 = (rng.integers(0, 257, idx.size) / 256.0).astype(np.float32)
    plan.blob.fill_(0xA5)
    plan.refresh_weights(dev(w2), dev(idx), dev(ptr))
    check_table_and_blocks(L.encode(layout, w2, idx, ptr, m, k, shift, W), plan.seg, plan.blob, plan.blob.numel() - 128,
                           f'{route}: refresh_weights')


# ------------------------------------------------------------------------------------------------------------ 10. statistics
@pytest.mark.parametrize('dtype', ['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('layout', ['u16w', 'd8'])
def test_weight_statistics_of_the_fill(layout, dtype):
    """``maxabs_bits`` after the fill: the bit pattern of the largest |w| (a negative one) and of the smallest non-zero |w| (zeros
    and a negative zero are present and must not count); with nothing but zeros they stay 0 and 0xffffffff."""
    rng = np.random.default_rng(100)
    m, k, W, shift = (U16_M if layout == 'u16w' else SORTED_M), 100, 40, 6
    idx, ptr = ragged(rng, m, k)
    w = weights_for(layout, rng, idx.size, 'f32').numpy().copy()
    w[w == 0] = 0.0
    w[2], w[-1], w[-2], w[5], w[6] = -0.0, -3.5, 2 ** -9, 0.0, 3.25        # the extremes sit in rows of different workgroups
    pay = torch.from_numpy(w).to(TORCH_DTYPE[dtype])
    b = build_raw(layout, pay, idx, ptr, m, k, shift, W)
    check_raw(b, pay, idx, ptr, f'{layout}/{dtype}')
    assert b.maxabs.tolist() == [np.float32(3.5).view(np.uint32), np.float32(2 ** -9).view(np.uint32)]
    zeros = torch.from_numpy(np.where(np.arange(idx.size) % 2, -0.0, 0.0).astype(np.float32)).to(TORCH_DTYPE[dtype])
    b = build_raw(layout, zeros, idx, ptr, m, k, shift, W)
    check_raw(b, zeros, idx, ptr, f'{layout}/{dtype} zeros')
    assert b.maxabs.tolist() == [0, 0xffffffff]
