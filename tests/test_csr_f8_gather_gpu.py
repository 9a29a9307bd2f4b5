"""The FP8 gather direction on the device, every comparison bit for bit against the numpy restatement
(tests/csr_f8_gather_cases.py): the streaming kernel by direct C call (be_binary_csrm*_nt_f8), the one-byte mirror fill
(be_csr_to_csc_fill_block_u8), and ``events @ W8.T`` / ``Float8CSC`` through Python on the streaming kernel, the planned mirror and
the raw mirror.  A row's sum is an exact integer whatever the order, so equality is the contract on every route."""
import ctypes

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _array as A
from brainevent_amd import _convert
from brainevent_amd import _csr as C
from brainevent_amd._lib import fn, last_error
import csr_f8_cases as K
import csr_f8_gather_cases as G

pytestmark = pytest.mark.gpu
FMTS = sorted(K.E)
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -5
SENTINEL = 0xA5


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Mat:
    """FP8 stored rows on the host (for the restatement) and on the device (for the calls).  ``row_len >= 0``: fixed-length rows,
    passed without an indptr.  ``shift``: the device arrays start ``shift`` bytes (codes) / elements (indices) into their buffers."""

    def __init__(self, codes, indices, indptr, m, k, fmt, i64=False, row_len=-1, shift=0):
        self.codes, self.indices, self.indptr, self.m, self.k, self.fmt = codes, indices, np.asarray(indptr, np.int64), m, k, fmt
        self._bufs = (dev(np.concatenate([np.zeros(shift, np.uint8), codes])), dev(np.concatenate([np.zeros(shift, np.int32), indices])))
        self.d_codes, self.d_indices = self._bufs[0][shift:], self._bufs[1][shift:]
        self.d_indptr = None if row_len >= 0 else dev(self.indptr.astype(np.int64 if i64 else np.int32))
        self.is64, self.row_len, self.nnz = int(i64), row_len, len(indices)
        assert self.indptr[-1] == self.nnz and len(self.indptr) == m + 1

    def expected(self, active, scale=1.0):
        return G.expected_gather(self.codes, self.indices, self.indptr, active, self.fmt, scale)


def spikes_of(kind, active):
    """(keep-alive tensor, spike dtype code) of a bool vector [k] or batch [nb, k] in the encoding ``kind``."""
    active = np.asarray(active, dtype=bool)
    if kind == 'bool':
        return dev(active.astype(np.uint8) * 3), A.BE_SPIKE_BOOL
    if kind == 'float':
        v = np.where(active, np.float32(0.5), np.float32(0.0)).astype(np.float32)
        off = np.flatnonzero(~active.reshape(-1))
        v.reshape(-1)[off[0::3]] = -2.0             # a negative value and a NaN are inactive
        v.reshape(-1)[off[1::3]] = np.nan
        assert np.array_equal(K.active_of(v), active)
        return dev(v), A.BE_SPIKE_FLOAT
    assert kind == 'bits'
    return dev(K.pack_bits(active).view(np.int32)), A.BE_SPIKE_BITS


def guarded(nbytes, fill):
    t = torch.full((nbytes + 256,), SENTINEL, dtype=torch.uint8, device='cuda')
    if nbytes:
        t[:nbytes] = fill
    return t


def tail_ok(t, nbytes):
    return bool((t[nbytes:] == SENTINEL).all())


def run(M, kind, active, scale=1.0, expect=OK, mv=False, sd=None, **over):
    """One call of be_binary_csrmm_nt_f8 (``mv``: be_binary_csrmv_nt_f8) into sentinel-guarded buffers; ``over`` replaces arguments."""
    active = np.asarray(active, dtype=bool)
    nb = 1 if active.ndim == 1 else active.shape[0]
    sp, code = spikes_of(kind, active)
    need = fn('be_binary_csrmm_nt_f8_workspace_bytes')(M.m, M.k, nb)
    assert need >= -(-M.k // 32) * 4 * nb and (not mv or need == fn('be_binary_csrmv_nt_f8_workspace_bytes')(M.m, M.k))
    ws, out = guarded(need, 0x5A), guarded(nb * M.m * 4, 0xFF)
    a = dict(codes=A.ptr(M.d_codes), fmt=K.FMT_CODE[M.fmt], scale=scale, indices=A.ptr(M.d_indices), indptr=A.ptr(M.d_indptr),
             is64=M.is64, row_len=M.row_len, nnz=M.nnz, spikes=A.ptr(sp), sd=code if sd is None else sd, out=A.ptr(out), m=M.m, k=M.k,
             nb=nb, ws=A.ptr(ws), ws_bytes=need)
    a.update(over)
    head = (a['codes'], a['fmt'], a['scale'], a['indices'], a['indptr'], a['is64'], a['row_len'], a['nnz'], a['spikes'], a['sd'],
            a['out'], a['m'], a['k'])
    if mv:
        assert nb == 1
        rc = fn('be_binary_csrmv_nt_f8')(*head, a['ws'], a['ws_bytes'], A.stream_ptr())
    else:
        rc = fn('be_binary_csrmm_nt_f8')(*head, a['nb'], a['ws'], a['ws_bytes'], A.stream_ptr())
    assert rc == expect, (rc, last_error())
    torch.cuda.synchronize()
    assert tail_ok(ws, need) and tail_ok(out, nb * M.m * 4), "wrote past the workspace / the output"
    if kind == 'bits':
        assert bool((ws[:need] == 0x5A).all()), "packed words are read in place: the workspace stays untouched"
    r = out[:nb * M.m * 4].view(torch.float32).cpu().numpy().reshape(nb, M.m)
    return r[0] if active.ndim == 1 else r


def check(M, active, scale=1.0, kinds=('bool',)):
    want = M.expected(active, scale)
    for kind in kinds:
        got = run(M, kind, active, scale)
        assert bits_equal(got, want), (kind, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    return want


# ------------------------------------------------------------------------------------------------- the kernel, by direct C call
@pytest.mark.parametrize('fmt', FMTS)
def test_small_shapes_all_and_none_active(fmt):
    rng = np.random.default_rng(1)
    for k in (1, 31, 32, 33, 1025):
        for m in (1, 3, 257):
            M = Mat(*K.random_matrix(m, k, fmt, seed=m * 7 + k), m, k, fmt, i64=(m + k) % 2 == 0)
            for active in (rng.random(k) < 0.4, np.ones(k, bool), np.zeros(k, bool)):
                check(M, active, 0.3, kinds=('bool', 'bits'))
            assert not run(M, 'bool', np.zeros(k, bool)).view(np.uint32).any()        # nothing active: +0.0 everywhere


@pytest.mark.parametrize('fmt', FMTS)
def test_a_bitmap_past_the_lds_limit_is_read_from_global_memory(fmt):
    k, m = G.LDS_BITMAP_BYTES * 8 + 1, 3
    assert -(-k // 32) * 4 > G.LDS_BITMAP_BYTES >= -(-(k - 1) // 32) * 4
    rng = np.random.default_rng(2)
    fc = K.finite_codes(fmt)
    rows = [(np.concatenate([[k - 1, 0, k - 1], rng.integers(0, k, n)]), rng.choice(fc, n + 3)) for n in (0, 70, 700)]
    M = Mat(*K.from_rows(rows, k), m, k, fmt)
    active = rng.random(k) < 0.5
    active[k - 1] = True
    check(M, active, 0.25, kinds=('bool', 'float', 'bits'))
    active[k - 1] = False
    check(M, active, kinds=('bool',))
    # one column fewer: the same rows (column k - 1 folded to k - 2) through the LDS bitmap
    M2 = Mat(M.codes, np.minimum(M.indices, k - 2), M.indptr, m, k - 1, fmt)
    check(M2, active[:k - 1], 0.25)


@pytest.mark.parametrize('lpr', G.LPRS)
@pytest.mark.parametrize('fmt', FMTS)
def test_row_lengths_around_a_pass_at_each_lanes_per_row_instance(fmt, lpr):
    """0, 1, one short of / exactly / one past a pass, two passes - 1 / + 0 / + 1 (a trip of the walk), four passes + 3, between
    odd-length filler rows that keep the average inside the instance's range and move the row starts over every residue mod 4."""
    P = G.pass_of(lpr)
    lens = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 4 * P + 3] + {2: [3] * 9, 4: [3] * 5, 8: [5] * 3, 16: [7], 32: [7], 64: [5] * 3}[lpr]
    lens = np.random.default_rng(lpr).permutation(lens)
    k = 1025
    for i64 in (False, True):
        codes, indices, indptr = G.rows_of_lengths(lens, k, fmt, seed=lpr)
        M = Mat(codes, indices, indptr, len(lens), k, fmt, i64=i64)
        assert G.lpr_of(M.nnz // M.m) == lpr and set(int(b) % 4 for b in indptr[:-1]) == {0, 1, 2, 3} and M.nnz % 4 != 0
        rng = np.random.default_rng(3)
        for p in (0.02, 0.5, 1.0):
            check(M, rng.random(k) < p, 0.3)


@pytest.mark.parametrize('fmt', FMTS)
def test_long_rows_among_short_ones_and_short_rows_among_long_ones(fmt):
    k = 3000
    rng = np.random.default_rng(4)
    for lens, lpr in (([3] * 300 + [5000] + [3] * 300, 4), ([700] * 20 + [1, 0, 3] + [700] * 20, 64)):
        codes, indices, indptr = G.rows_of_lengths(lens, k, fmt, seed=len(lens))
        M = Mat(codes, indices, indptr, len(lens), k, fmt)
        assert G.lpr_of(M.nnz // M.m) == lpr
        check(M, rng.random(k) < 0.3, 0.3)
        check(M, np.ones(k, bool))


@pytest.mark.parametrize('fmt', FMTS)
def test_rows_start_at_every_byte_and_dword_residue_and_end_at_the_array_end(fmt):
    """Consecutive odd-length rows: the row starts run through every residue mod 4 of ``codes`` (bytes) and ``indices`` (dwords); the
    entry count is no multiple of 4 and the last row ends where the arrays end.  Then the same matrix from arrays that themselves
    start 1, 2 and 3 bytes / elements into their allocations."""
    k = 97
    lens = [1, 3, 5, 7, 9, 1, 1, 3, 11, 33, 1, 5, 35, 3, 1]
    codes, indices, indptr = G.rows_of_lengths(lens, k, fmt, seed=8)
    assert set(int(b) % 4 for b in indptr[:-1]) == {0, 1, 2, 3} and len(codes) % 4 != 0 
    rng = np.random.default_rng(5)
    acts = [rng.random(k) < 0.5, np.ones(k, bool)]
    for shift in (0, 1, 2, 3):
        M = Mat(codes, indices, indptr, len(lens), k, fmt, shift=shift)
        assert M.d_codes.data_ptr() % 4 == shift
        for a in acts:
            check(M, a, 0.3)
    # the same with every tail length of the arrays: the last 1, 2 or 3 entries lie in a quad that is cut by the arrays' end
    for cut in (1, 2, 3):
        lens2 = lens[:-1] + [lens[-1] + cut]
        c2, i2, p2 = G.rows_of_lengths(lens2, k, fmt, seed=9)
        check(Mat(c2, i2, p2, len(lens2), k, fmt), acts[1], 0.3)
    # the other lanes-per-row instances over odd-length rows
    assert G.lpr_of(sum(lens) // len(lens)) == 2
    for lens3, lpr in (([13, 13, 13, 15, 17], 4), ([33, 33, 33, 35, 37, 39, 41], 8), ([65, 65, 65, 67, 69, 71], 16),
                       ([201, 201, 201, 203, 135], 32), ([301, 301, 301, 303], 64)):
        c3, i3, p3 = G.rows_of_lengths(lens3, k, fmt, seed=10)
        assert set(int(b) % 4 for b in p3[:-1]) == {0, 1, 2, 3} and G.lpr_of(len(c3) // len(lens3)) == lpr
        for shift in (0, 3):
            check(Mat(c3, i3, p3, len(lens3), k, fmt, shift=shift), acts[0], 0.25)


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('row_len', [1, 5, 64])
def test_fixed_length_rows_without_an_indptr(fmt, row_len):
    m, k = 257, 333
    codes, indices, indptr = G.fixed_rows(m, k, row_len, fmt, seed=row_len)
    M = Mat(codes, indices, indptr, m, k, fmt, row_len=row_len)
    rng = np.random.default_rng(6)
    check(M, rng.random(k) < 0.3, 0.3, kinds=('bool', 'bits'))
    check(M, rng.random((3, k)) < 0.3, 0.25)
    # nnz is the arrays' length: one below m * row_len is refused before anything is read
    run(M, 'bool', np.ones(k, bool), expect=INVALID, nnz=M.nnz - 1)
    check(M, np.ones(k, bool))


@pytest.mark.parametrize('fmt', FMTS)
def test_an_all_empty_matrix_gives_positive_zeros(fmt):
    m, k = 5, 40
    M = Mat(np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(m + 1, np.int64), m, k, fmt)
    assert M.d_codes.data_ptr() == 0 or M.nnz == 0
    got = run(M, 'bool', np.ones(k, bool), codes=ctypes.c_void_p(0), indices=ctypes.c_void_p(0))
    assert not got.view(np.uint32).any()
    got = run(M, 'bits', np.ones((3, k), bool), codes=ctypes.c_void_p(0), indices=ctypes.c_void_p(0))
    assert got.shape == (3, m) and not got.view(np.uint32).any()


@pytest.mark.parametrize('fmt', FMTS)
def test_every_finite_code_zeros_subnormals_extremes_and_cancellation(fmt):
    fc = K.finite_codes(fmt)
    k = 64
    q = K.q_table(fmt)
    top = int(fc[np.argmax(q[fc])])                                     # +max; top | 0x80 is -max
    assert q[top] == K.Q_MAX[fmt] and q[top | 0x80] == -K.Q_MAX[fmt]
    sub = [1, 2, 3, 0x81, 0x83]                                         # subnormals of either format
    rows = [([int(c) % k], [c]) for c in fc]                            # each code alone
    rows += [(np.arange(len(fc)) % k, fc),                              # every code on one row
             ([5, 9], [0x00, 0x80]),                                    # both zeros
             ([1, 2, 3, 4, 6], sub),
             ([7, 7, 8, 8], [top, top, top | 0x80, top | 0x80]),        # cancels to exactly +0.0 when all are active
             ([7, 8], [top, top]), ([10, 11], [top | 0x80, top | 0x80]),  # |R| = 2 max (e5m2: above 2^32)
             ([12, 13], [0x3c, 0xbc])]                                  # c and -c
    M = Mat(*K.from_rows(rows, k), len(rows), k, fmt)
    all_on = np.ones(k, bool)
    for scale in (1.0, 0.25, 0.3):
        want = check(M, all_on, scale, kinds=('bool', 'float', 'bits'))
        n = len(fc)
        assert want[n + 3].view(np.uint32) == 0 and want[n + 6].view(np.uint32) == 0          # +0.0, not -0.0
        assert want[n + 4] == -want[n + 5] == np.float32(2 * K.Q_MAX[fmt] * 2.0 ** -K.E[fmt] * np.float64(np.float32(scale)))
    if fmt == 'e5m2':
        assert 2 * K.Q_MAX[fmt] > 1 << 32
    half = all_on.copy()
    half[8] = False                                                     # the cancelling row keeps its two +max entries
    check(M, half, 0.3)


@pytest.mark.parametrize('fmt', FMTS)
def test_unsorted_and_duplicated_columns_spike_encodings_and_ids_refused(fmt):
    m, k = 120, 77
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=11)
    assert any(len(set(indices[indptr[i]:indptr[i + 1]])) < indptr[i + 1] - indptr[i] for i in range(m))        # duplicates
    assert any((np.diff(indices[indptr[i]:indptr[i + 1]]) < 0).any() for i in range(m))                        # unsorted
    M = Mat(codes, indices, indptr, m, k, fmt)
    rng = np.random.default_rng(7)
    active = rng.random(k) < 0.4
    want = check(M, active, 0.3, kinds=('bool', 'float', 'bits'))
    run(M, 'bool', active, expect=UNSUPPORTED, sd=A.BE_SPIKE_IDS)
    assert 'BE_SPIKE_IDS' in last_error()
    assert bits_equal(run(M, 'bool', active, 0.3, mv=True), want)                              # a clean call after the refusal


@pytest.mark.parametrize('fmt', FMTS)
def test_batches_equal_one_vector_calls_and_calls_repeat(fmt):
    m, k = 150, 203
    M = Mat(*K.random_matrix(m, k, fmt, seed=12, max_len=90), m, k, fmt)
    rng = np.random.default_rng(8)
    for nb in (1, 3, 33):
        active = rng.random((nb, k)) < 0.3
        active[nb // 2] = False
        for kind in ('bool', 'float', 'bits'):
            got = run(M, kind, active, 0.3)
            assert bits_equal(got, M.expected(active, 0.3))
            assert bits_equal(got, run(M, kind, active, 0.3))                                  # two identical calls, identical bits
            if kind == 'bool' or nb == 3:
                for b in range(nb):
                    assert bits_equal(run(M, kind, active[b], 0.3, mv=True), got[b])


def test_every_error_code_is_followed_by_a_clean_call():
    m, k, fmt = 20, 50, 'e4m3'
    M = Mat(*K.random_matrix(m, k, fmt, seed=13), m, k, fmt)
    active = np.random.default_rng(9).random(k) < 0.5
    want = M.expected(active)
    null = ctypes.c_void_p(0)
    bad = [(INVALID, dict(fmt=2)), (INVALID, dict(fmt=-1)), (INVALID, dict(m=-1)), (INVALID, dict(k=-1)), (INVALID, dict(nnz=-1)),
           (INVALID, dict(m=1 << 32)), (INVALID, dict(k=1 << 32)), (INVALID, dict(nb=-1)), (INVALID, dict(nb=65536)),
           (INVALID, dict(scale=float('nan'))), (INVALID, dict(scale=float('inf'))), (INVALID, dict(scale=1e39)),
           (INVALID, dict(sd=4)), (INVALID, dict(sd=-1)), (INVALID, dict(indptr=null, row_len=-1)), (INVALID, dict(codes=null)),
           (INVALID, dict(indices=null)), (INVALID, dict(spikes=null)), (INVALID, dict(out=null)),
           (WORKSPACE, dict(ws=null)), (WORKSPACE, dict(ws_bytes=0)), (UNSUPPORTED, dict(sd=A.BE_SPIKE_IDS))]
    for code, over in bad:
        if 'ws_bytes' in over:
            over = dict(ws_bytes=fn('be_binary_csrmm_nt_f8_workspace_bytes')(m, k, 1) - 1)
        got = run(M, 'bool', active, expect=code, **over)
        assert (got.view(np.uint32) == 0xFFFFFFFF).all(), over                                 # nothing was written
        assert last_error(), over
        assert bits_equal(run(M, 'bool', active), want), over
    assert fn('be_binary_csrmm_nt_f8_workspace_bytes')(-1, 4, 1) == INVALID
    # zero sizes: BE_OK after the scalar checks, nothing touched (the NULL buffers are not looked at)
    for over in (dict(m=0), dict(k=0), dict(nb=0)):
        got = run(M, 'bool', active, spikes=null, out=null, ws=null, **over)
        run(M, 'bool', active, expect=INVALID, fmt=7, **over)


@pytest.mark.parametrize('lpr', G.LPRS)
def test_one_row_past_a_grid_trip_at_each_instance(lpr):
    fmt = 'e5m2' if lpr in (2, 16) else 'e4m3'
    m, k = G.trip_rows(lpr) + 1, 4099
    row_len = {2: 2, 4: 9, 8: 21, 16: 46, 32: 101, 64: 201}[lpr]
    codes, indices, indptr = G.fixed_rows(m, k, row_len, fmt, seed=lpr)
    M = Mat(codes, indices, indptr, m, k, fmt)
    assert G.lpr_of(M.nnz // m) == lpr and m == 512 * 1024 // lpr + 1
    active = np.random.default_rng(lpr).random(k) < 0.3
    check(M, active, 0.3)


# ------------------------------------------------------------------------------------------------- the mirror's one-byte fill
def fill_u8(codes, indices, indptr, m, k, c0, c1, perm, row_len=-1):
    """be_csr_to_csc_fill_block_u8 over the columns [c0, c1): (cptr of the block, rows, codes, perm or None)."""
    b = _convert.CscBuilder(None if row_len >= 0 else dev(indptr.astype(np.int32)), dev(indices), shape=(m, k), row_len=row_len)
    cptr = b.csc_indptr.cpu().numpy()
    n = int(cptr[c1] - cptr[c0])
    rows = torch.full((n + 64,), -1, dtype=torch.int32, device='cuda')
    out = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    p_out = None if perm is None else torch.full((n + 64,), -1, dtype=perm, device='cuda')
    cursor = torch.empty(max(c1 - c0, 1), dtype=torch.int64, device='cuda')
    d_codes = dev(codes)
    rc = fn('be_csr_to_csc_fill_block_u8')(A.ptr(b.indices), A.ptr(b.indptr), 0, row_len, m, len(indices), c0, c1, A.ptr(b.csc_indptr),
                                           A.ptr(cursor), A.ptr(rows), A.ptr(p_out), int(perm == torch.int64), A.ptr(d_codes), A.ptr(out),
                                           A.stream_ptr())
    assert rc == OK, last_error()
    torch.cuda.synchronize()
    assert bool((rows[n:] == -1).all()) and bool((out[n:] == SENTINEL).all()) and (p_out is None or bool((p_out[n:] == -1).all()))
    return cptr[c0:c1 + 1] - cptr[c0], rows[:n].cpu().numpy(), out[:n].cpu().numpy(), None if p_out is None else p_out[:n].cpu().numpy()


def check_fill(codes, indices, indptr, m, k, c0, c1, perm, row_len=-1):
    """Every column of the block holds exactly its entries' (row, code) pairs; the perm names each slot's source entry."""
    cptr, rows, out, p = fill_u8(codes, indices, indptr, m, k, c0, c1, perm, row_len)
    src_rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(np.asarray(indptr, np.int64)))
    sel = (indices >= c0) & (indices < c1)
    want = np.stack([indices[sel].astype(np.int64), src_rows[sel], codes[sel].astype(np.int64)])
    cols = np.repeat(np.arange(c0, c1, dtype=np.int64), np.diff(cptr))
    got = np.stack([cols, rows.astype(np.int64), out.astype(np.int64)])
    assert got.shape == want.shape
    assert np.array_equal(got[:, np.lexsort(got[::-1])], want[:, np.lexsort(want[::-1])])
    if p is not None:
        assert p.dtype == (np.int64 if perm == torch.int64 else np.int32) and len(np.unique(p)) == len(p)
        assert np.array_equal(indices[p], cols) and np.array_equal(src_rows[p], rows) and np.array_equal(codes[p], out)


@pytest.mark.parametrize('lpr', [1, 4, 16, 64])
def test_the_one_byte_fill_at_each_lanes_per_row_instance(lpr):
    avg = {1: 2, 4: 8, 16: 48, 64: 49}[lpr]
    m, k = 300, 211
    rng = np.random.default_rng(lpr)
    lens = np.full(m, avg)
    lens[0::4] += min(avg, 2)                   # rows around the average, an empty one and one of twice the average
    lens[1::4] -= min(avg, 2)
    lens[2], lens[6] = 0, 2 * avg
    assert lens.sum() == avg * m
    codes, indices, indptr = G.rows_of_lengths(lens, k, 'e4m3', seed=lpr)
    codes = (np.arange(len(codes)) * 7 % 251).astype(np.uint8)                               # any byte moves: not only finite codes
    assert G.fill_lpr_of(len(indices) // m) == lpr
    for perm in (torch.int32, torch.int64, None):
        check_fill(codes, indices, indptr, m, k, 0, k, perm)
    for c0, c1 in ((0, 1), (1, 100), (100, 100), (100, k)):
        check_fill(codes, indices, indptr, m, k, c0, c1, torch.int32)
    # fixed-length rows (no indptr)
    rl = avg
    c, i, p = G.fixed_rows(m, k, rl, 'e5m2', seed=lpr)
    check_fill(c, i, p, m, k, 0, k, None, row_len=rl)
    check_fill(c, i, p, m, k, 7, 150, torch.int64, row_len=rl)


@pytest.mark.parametrize('lpr', [1, 4, 16, 64])
def test_the_one_byte_fill_past_one_grid_trip(lpr):
    m = G.FILL_GRID_CAP * G.FILL_THREADS // lpr + 1
    rl, k = {1: 1, 4: 3, 16: 9, 64: 49}[lpr], 5003
    assert G.fill_lpr_of(rl) == lpr
    c, i, p = G.fixed_rows(m, k, rl, 'e4m3', seed=lpr)
    check_fill(c, i, p, m, k, 0, k, None)


def test_the_public_fill_still_refuses_a_one_byte_weight():
    idx, ptr = dev(np.zeros(4, np.int32)), dev(np.arange(5, dtype=np.int32))
    b = _convert.CscBuilder(ptr, idx, shape=(4, 2))
    buf = torch.zeros(8, dtype=torch.int64, device='cuda')
    rc = fn('be_csr_to_csc_fill_block')(A.ptr(idx), A.ptr(ptr), 0, -1, 4, 4, 0, 2, A.ptr(b.csc_indptr), A.ptr(buf), A.ptr(buf), None, 0,
                                        A.ptr(buf), 1, A.ptr(buf), A.stream_ptr())
    assert rc == INVALID and 'must be 0, 2, 4 or 8' in last_error()
    rc = fn('be_csr_to_csc_fill_block_u8')(A.ptr(idx), A.ptr(ptr), 0, -1, 4, 4, 0, 2, A.ptr(b.csc_indptr), A.ptr(buf), A.ptr(buf), None, 0,
                                           None, A.ptr(buf), A.stream_ptr())
    assert rc == INVALID and 'be_csr_to_csc_fill_block_u8' in last_error()


# ------------------------------------------------------------------------------------------------- through Python
ROUTES = ('kernel', 'planned mirror', 'raw mirror')


def on_route(W, route, monkeypatch):
    """``W`` (either view) serving its gather on ``route``; asserts that it does."""
    if route != 'kernel':
        monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1 if route == 'planned mirror' else 1 << 40)
        assert W.build_mirror() is W
        assert (W._mirror.plan is not None) == (route == 'planned mirror') and W._mirror.nbytes() > 0
        assert (W._mirror.codes is None) == (route == 'planned mirror')             # a planned mirror releases its raw arrays
    else:
        assert W._mirror is None
    return W


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('fmt', FMTS)
def test_events_times_the_transpose_view_on_every_route(fmt, route, monkeypatch):
    m, k = 200, 500
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=9)
    rng = np.random.default_rng(9)
    s, sb = rng.random(k) < 0.3, rng.random((3, k)) < 0.3
    want, wantb = (G.expected_gather(codes, indices, indptr, x, fmt, 0.3) for x in (s, sb))
    W = be.Float8CSR((codes, indices, indptr), shape=(m, k), scale=0.3, fmt=fmt)
    Wt = on_route(W.T, route, monkeypatch)
    assert W._mirror is Wt._mirror and W._plan is None
    r = be.BinaryArray(s) @ Wt                                                       # numpy in -> numpy out
    assert isinstance(r, np.ndarray) and r.dtype == np.float32 and bits_equal(r, want)
    rb = be.BinaryArray(sb) @ W.T
    assert isinstance(rb, np.ndarray) and bits_equal(rb, wantb)
    st = torch.from_numpy(s).cuda()
    rt = be.BinaryArray(st) @ Wt
    assert isinstance(rt, torch.Tensor) and rt.is_cuda and rt.dtype == torch.float32 and bits_equal(rt.cpu().numpy(), want)
    assert bits_equal((be.BitPackedBinary(st) @ Wt).cpu().numpy(), want)             # packed words
    assert bits_equal((be.CompactBinary.from_array(st) @ Wt).cpu().numpy(), want)    # the compacted container
    assert bits_equal((be.BinaryArray(torch.from_numpy(np.where(s, 2.0, -1.0).astype(np.float32)).cuda()) @ Wt).cpu().numpy(), want)
    ring = be.SpikeRing(k, 4)
    ring.push(st)
    ring.push(torch.zeros_like(st))
    assert bits_equal((ring.events(1) @ Wt).cpu().numpy(), want)                     # the spikes of one step ago
    # the same arrays as a Float8CSC of their own: the gather from the left, the scatter from the right
    Cc = on_route(be.Float8CSC((codes, indices, indptr), shape=(k, m), scale=0.3, fmt=fmt), route, monkeypatch)
    assert bits_equal(be.BinaryArray(s) @ Cc, want) and bits_equal(be.BinaryArray(sb) @ Cc, wantb)
    with pytest.raises(NotImplementedError, match=r'gather direction, W8 @ events.*W8\.T'):
        W @ be.BinaryArray(s)
    E = be.Float8CSR((np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(m + 1, np.int32)), shape=(m, k), fmt=fmt)
    assert not (be.BinaryArray(s) @ on_route(E.T, route if route == 'kernel' else 'raw mirror', monkeypatch)).any()


@pytest.mark.parametrize('fmt', FMTS)
def test_a_column_the_sorted_layout_refuses_is_served_by_the_raw_mirror(fmt, monkeypatch):
    """16 385 entries in one column: one more than a q8 row holds, so the mirror keeps its raw arrays and runs the direct scatter."""
    m, k, col = 50, 300, 3
    fc = K.finite_codes(fmt)
    rng = np.random.default_rng(10)
    rows = [(rng.integers(0, k, 20), rng.choice(fc, 20)) for _ in range(m)]
    rows[7] = (np.concatenate([rows[7][0], np.full(K.MAX_ROW + 1, col)]), np.concatenate([rows[7][1], rng.choice(fc, K.MAX_ROW + 1)]))
    codes, indices, indptr = K.from_rows(rows, k)
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1)
    s = rng.random((2, k)) < 0.4
    s[0, col], s[1, col] = True, False
    want = G.expected_gather(codes, indices, indptr, s, fmt, 0.25)
    W = be.Float8CSR((codes, indices, indptr), shape=(m, k), scale=0.25, fmt=fmt)
    assert bits_equal(be.BinaryArray(s) @ W.T, want)                                 # streamed
    W.T.prepare(mirror=True)
    assert W._mirror is not None and W._mirror.plan is None and W._mirror.codes is not None and W._plan is None
    assert bits_equal(be.BinaryArray(s) @ W.T, want) and bits_equal(be.BinaryArray(s[0]) @ W.T, want[0])
    W2 = be.Float8CSR((codes, np.where(indices == col, np.arange(len(indices)) % k, indices).astype(np.int32), indptr), shape=(m, k),
                      scale=0.25, fmt=fmt)
    assert W2.build_mirror()._mirror.plan is not None                                # without that column the plan takes it


@pytest.mark.parametrize('fmt', FMTS)
def test_float8csc_at_events_is_events_at_float8csr_and_plans_are_shared(fmt, monkeypatch):
    m, k = 180, 260
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=14)
    rng = np.random.default_rng(14)
    s, sb = rng.random(m) < 0.3, rng.random((4, m)) < 0.3
    for min_nnz in (1, 1 << 40):
        monkeypatch.setattr(C, 'PLAN_MIN_NNZ', min_nnz)
        R = be.Float8CSR((codes, indices, indptr), shape=(m, k), scale=0.3, fmt=fmt)
        Cc = be.Float8CSC((codes, indices, indptr), shape=(k, m), scale=0.3, fmt=fmt)
        a, b = be.BinaryArray(s) @ R, Cc @ be.BinaryArray(s)
        assert a.shape == b.shape == (k,) and bits_equal(a, b) and bits_equal(a, K.expected(codes, indices, indptr, s, k, fmt, 0.3))
        ab, bb = be.BinaryArray(sb) @ R, Cc @ be.BinaryArray(sb.T)
        assert ab.shape == (4, k) and bb.shape == (k, 4) and bits_equal(ab, np.ascontiguousarray(bb.T))
        assert bits_equal(ab, K.expected(codes, indices, indptr, sb, k, fmt, 0.3))
        assert (Cc._plan is not None) == (min_nnz == 1) and (R._plan is not None) == (min_nnz == 1)
        # a plan built through one view is the one the other view uses; so is a mirror
        V = be.Float8CSR((codes, indices, indptr), shape=(m, k), scale=0.3, fmt=fmt)
        assert V.T.prepare()._plan is V._plan and (V._plan is not None) == (min_nnz == 1) and V._mirror is None
        before = V._plan
        assert bits_equal(be.BinaryArray(s) @ V, a) and bits_equal(V.T @ be.BinaryArray(s), a) and V._plan is before
        V.prepare(mirror=True)
        assert V.T._mirror is V._mirror is not None and V.T.T._mirror is V._mirror
        g = rng.random(k) < 0.3
        assert bits_equal(be.BinaryArray(g) @ V.T, G.expected_gather(codes, indices, indptr, g, fmt, 0.3))


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('fmt', FMTS)
def test_a_captured_gather_replays_with_new_spikes(fmt, route, monkeypatch):
    m, k = 300, 700
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=12)
    W = be.Float8CSR((torch.from_numpy(codes).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(indptr).cuda()), shape=(m, k),
                     scale=0.5, fmt=fmt)
    Wt = on_route(W.T, route, monkeypatch)
    rng = np.random.default_rng(12)
    s = torch.zeros(k, dtype=torch.bool, device='cuda')
    step = be.capture_step(lambda: be.BinaryArray(s) @ Wt)
    for _ in range(3):
        a = rng.random(k) < 0.3
        s.copy_(torch.from_numpy(a))
        assert bits_equal(step().cpu().numpy(), G.expected_gather(codes, indices, indptr, a, fmt, 0.5))


@pytest.mark.parametrize('fmt', FMTS)
def test_csc_quantize_fp8_holds_the_dense_quantisation_at_the_stored_positions(fmt):
    rng = np.random.default_rng(1)
    m, k = 40, 70
    dense = np.where(rng.random((m, k)) < 0.15, rng.standard_normal((m, k)) * 3, 0).astype(np.float32)
    csc = be.CSR.fromdense(dense).tocsc()
    assert isinstance(csc, be.CSC)
    W8 = csc.quantize_fp8(fmt)
    assert isinstance(W8, be.Float8CSC) and W8.fmt == fmt and W8.shape == (m, k) and W8.nse == csc.nse
    assert W8.indices.data_ptr() == csc.indices.data_ptr() and W8.indptr.data_ptr() == csc.indptr.data_ptr()
    D8 = be.quantize_fp8(csc.todense(), fmt, scale=W8.scale)
    assert D8.scale == W8.scale == be.quantize_fp8(dense, fmt).scale
    ptr = W8.indptr.cpu().numpy()
    cols = np.repeat(np.arange(k), np.diff(ptr))
    rows = W8.indices.cpu().numpy()
    assert np.array_equal(W8.codes.view(torch.uint8).cpu().numpy(), D8.codes.view(torch.uint8).cpu().numpy()[rows, cols])
    back = W8.tocsc()
    assert isinstance(back, be.CSC) and back.dtype == torch.float32 and back.shape == W8.shape
    assert np.array_equal(np.asarray(W8.todense()), np.asarray(back.todense())) and W8.tocsc(torch.float16).dtype == torch.float16
    # and its products are the transposed Float8CSR's
    s = rng.random(m) < 0.4
    assert bits_equal((be.BinaryArray(s) @ W8), G.expected_gather(W8.codes.view(torch.uint8).cpu().numpy(), rows, ptr, s, fmt, W8.scale))
