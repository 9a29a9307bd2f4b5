"""The per-synapse products (brainevent_amd/_dt2t.py, csrc/be_dt2t.hip) against three lines of numpy, bit for bit.

The result is one correctly rounded product, and numpy (f16) / torch on the CPU (bf16) form it the same way — the exact f32
product, rounded once — so every comparison is `assert_array_equal` on the bit patterns, for all four dtypes.  `w` and `y` are
drawn as random sign x uniform [0.5, 2): no product is subnormal in any dtype, so the comparison does not depend on a
denormal mode (a choice of inputs, not a tolerance).

Sizes come from CONSTS, the loop geometry of csrc/be_dt2t.hip (tests/test_dt2t_cpu.py compares the table with the source):
V = entries per 16 bytes of the dtype, T = threads * runs_per_thread * V = entries of one block tile, G = the grid cap (blocks
over all batch rows).  After a retune the cases move with the table."""
import numpy as np
import pytest
import torch

import brainevent_amd as be

pytestmark = pytest.mark.gpu

CONSTS = {'threads': 256, 'vec_bytes': 16, 'runs_per_thread': 2, 'grid_cap': 2048}
G = CONSTS['grid_cap']
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def V(dtype) -> int:
    return CONSTS['vec_bytes'] // torch.empty(0, dtype=dtype).element_size()


def T(dtype) -> int:
    return CONSTS['threads'] * CONSTS['runs_per_thread'] * V(dtype)


def dev(x):
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to('cuda')


def draw(rng, shape, dtype) -> torch.Tensor:
    """random sign x uniform [0.5, 2), rounded to `dtype` (CPU tensor)."""
    v = rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype)


def oracle(w: torch.Tensor, y: torch.Tensor, sel: np.ndarray) -> torch.Tensor:
    """`w * y[..., sel]` on the host: numpy, or torch on the CPU for bf16."""
    if w.dtype == torch.bfloat16:
        return w * y[..., torch.from_numpy(np.asarray(sel, dtype=np.int64))]
    return torch.from_numpy(np.asarray(w.numpy() * y.numpy()[..., sel]))


def bits(t) -> np.ndarray:
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    t = t.detach().cpu().contiguous()
    return t.view(BITS[t.element_size()]).numpy()


def assert_bits(got, want):
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    np.testing.assert_array_equal(bits(got), bits(want))


def row_ids(indptr) -> np.ndarray:
    indptr = np.asarray(indptr)
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def csr_from_lens(lens, k, rng, ptr_dtype=np.int32):
    indptr = np.zeros(len(lens) + 1, dtype=ptr_dtype)
    np.cumsum(lens, out=indptr[1:])
    indices = rng.integers(0, k, int(indptr[-1])).astype(np.int32)
    return indices, indptr


def two_entry_rows(nnz):
    """rows of 2 entries, the last one shorter when nnz is odd."""
    lens = np.full((nnz + 1) // 2, 2, dtype=np.int64)
    lens[-1] = nnz - 2 * (len(lens) - 1)
    return lens


def check_csr(rng, lens, k, dtype, transpose, n_batch=None, ptr_dtype=np.int32, check_in_place=False):
    """One CSR case against the oracle: mv (`n_batch=None`) or mm."""
    m = len(lens)
    indices, indptr = csr_from_lens(lens, k, rng, ptr_dtype)
    nnz = len(indices)
    lead = () if n_batch is None else (n_batch,)
    w = draw(rng, lead + (nnz,), dtype)
    y = draw(rng, lead + (k if transpose else m,), dtype)
    want = oracle(w, y, indices if transpose else row_ids(indptr))
    f = be.csrmv_dt2t if n_batch is None else be.csrmm_dt2t
    wd = dev(w)
    got = f(dev(y), wd, dev(indices), dev(indptr), shape=(m, k), transpose=transpose)
    assert_bits(got, want)
    assert_bits(wd, w)                                   # the operand is left alone
    if check_in_place:
        back = f(dev(y), wd, dev(indices), dev(indptr), shape=(m, k), transpose=transpose, out=wd)
        assert back is wd
        assert_bits(wd, want)


# ------------------------------------------------------------------------------------------------ the reference's examples
def test_reference_docstring_examples():
    """The inputs of the reference's docstring examples (`_csr/dt2t.py` csrmv / cscmv / csrmm, `_fcn/dt2t.py` mv / mm; numpy
    in, numpy out); where the reference prints a result, that result."""
    f32 = np.float32
    w = np.array([0.5, 0.3, 0.7, 0.1], f32)
    indices = np.array([0, 2, 1, 2], np.int32)
    indptr = np.array([0, 2, 4], np.int32)
    got = be.csrmv_dt2t(np.array([1.0, 2.0], f32), w, indices, indptr, shape=(2, 3))
    assert isinstance(got, np.ndarray)
    np.testing.assert_array_equal(got, w * np.array([1, 1, 2, 2], f32))
    got = be.csrmv_dt2t(np.array([1.0, 2.0, 3.0], f32), w, indices, indptr, shape=(2, 3), transpose=True)
    np.testing.assert_array_equal(got, w * np.array([1, 3, 2, 3], f32))
    # CSC of a (3, 2) matrix: indptr over the 2 columns, y over the 3 rows
    got = be.cscmv_dt2t(np.array([1.0, 2.0, 3.0], f32), w, indices, indptr, shape=(3, 2))
    np.testing.assert_array_equal(got, w * np.array([1, 3, 2, 3], f32))
    got = be.cscmv_dt2t(np.array([1.0, 2.0], f32), w, indices, indptr, shape=(3, 2), transpose=True)
    np.testing.assert_array_equal(got, w * np.array([1, 1, 2, 2], f32))
    yb = np.array([[1.0, 2.0], [10.0, 20.0]], f32)
    wb = np.array([[0.5, 0.3, 0.7, 0.1], [1.0, 2.0, 3.0, 4.0]], f32)
    got = be.csrmm_dt2t(yb, wb, indices, indptr, shape=(2, 3))
    np.testing.assert_array_equal(got, wb * np.array([[1, 1, 2, 2], [10, 10, 20, 20]], f32))
    # fixed-number connectivity
    fw = np.array([[0.5, 1.0], [1.5, 2.0]], f32)
    fi = np.array([[0, 1], [1, 2]])
    got = be.fcnmv_dt2t(fw, fi, np.array([10.0, 20.0], f32), shape=(2, 3), transpose=False)
    np.testing.assert_array_equal(got, np.array([[5.0, 10.0], [30.0, 40.0]], f32))
    got = be.fcnmv_dt2t(fw, fi, np.array([1.0, 2.0, 3.0], f32), shape=(2, 3), transpose=True)
    np.testing.assert_array_equal(got, np.array([[0.5, 2.0], [3.0, 6.0]], f32))
    fwb = np.array([[[0.5, 1.0], [1.5, 2.0]], [[1.0, 1.0], [1.0, 1.0]]], f32)
    got = be.fcnmm_dt2t(fwb, fi, np.array([[10.0, 20.0], [100.0, 200.0]], f32), shape=(2, 3), transpose=False)
    np.testing.assert_array_equal(got, np.array([[[5, 10], [30, 40]], [[100, 100], [200, 200]]], f32))
    got = be.fcnmm_dt2t(fwb, fi, np.array([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]], f32), shape=(2, 3), transpose=True)
    np.testing.assert_array_equal(got, np.array([[[0.5, 2.0], [3.0, 6.0]], [[10, 20], [20, 30]]], f32))


# ------------------------------------------------------------------------------------------------ random CSR, and as CSC
@pytest.mark.parametrize('n_batch', [1, 3])
@pytest.mark.parametrize('ptr_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_random_csr_and_the_same_arrays_as_csc(dtype, transpose, ptr_dtype, n_batch):
    rng = np.random.default_rng(11)
    m, k = 257, 300
    lens = rng.poisson(5, m)
    indices, indptr = csr_from_lens(lens, k, rng, ptr_dtype)
    nnz = len(indices)
    lead = () if n_batch == 1 else (n_batch,)
    w = draw(rng, lead + (nnz,), dtype)
    y = draw(rng, lead + (k if transpose else m,), dtype)
    want = oracle(w, y, indices if transpose else row_ids(indptr))
    csr, csc = (be.csrmv_dt2t, be.cscmv_dt2t) if n_batch == 1 else (be.csrmm_dt2t, be.cscmm_dt2t)
    args = (dev(y), dev(w), dev(indices), dev(indptr))
    assert_bits(csr(*args, shape=(m, k), transpose=transpose), want)
    # the same arrays are the CSC arrays of the (k, m) transpose: its rows are the stored indices
    assert_bits(csc(*args, shape=(k, m), transpose=not transpose), want)


# ------------------------------------------------------------------------------------------------ tile and vector edges
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_tile_and_vector_edges(dtype, transpose):
    rng = np.random.default_rng(12)
    v, t = V(dtype), T(dtype)
    for nnz in sorted({1, v - 1, v + 1, t - 1, t, t + 1, 2 * t + v + 1}):
        check_csr(rng, two_entry_rows(nnz), 97, dtype, transpose)


# ------------------------------------------------------------------------------------------------ skew: the search path
def skewed_layouts(t):
    empty = 2 * t
    return {
        'one long row between runs of empty rows': np.concatenate([np.zeros(empty), [3 * t + 5], np.zeros(empty)]),
        'long row after short ones, then empty rows': np.concatenate([np.full(50, 3), [3 * t + 5], np.zeros(empty), [2, 0, 1]]),
        'all in the last row': np.concatenate([np.zeros(1000), [2 * t + 3]]),
        'all in the first row': np.concatenate([[2 * t + 3], np.zeros(1000)]),
        'one row': np.array([2 * t + 3]),
    }


@pytest.mark.parametrize('layout', list(skewed_layouts(1)))
@pytest.mark.parametrize('ptr_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('dtype', DTYPES)
def test_skewed_rows(dtype, ptr_dtype, layout):
    rng = np.random.default_rng(13)
    lens = skewed_layouts(T(dtype))[layout].astype(np.int64)
    check_csr(rng, lens, 64, dtype, False, ptr_dtype=ptr_dtype)
    check_csr(rng, lens, 64, dtype, False, n_batch=2, ptr_dtype=ptr_dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_row_ends_on_tile_and_run_boundaries(dtype):
    """Row ends exactly on a thread-run boundary, on the tile boundary, one entry to either side of it, and empty rows that
    sit exactly on the tile boundary."""
    rng = np.random.default_rng(14)
    v, t = V(dtype), T(dtype)
    for lens in ([t - v, v, v, 3, t - 3],                   # ends at t - v (a run boundary), t (the tile boundary), t + v
                 [t, 0, 0, 7, 0, t - 7, 1],                 # the tile boundary followed by empty rows
                 [t - 1, 2, t - 1, 0, 0],                   # a row across the boundary, trailing empty rows
                 [t + 1, t - 1, v]):
        assert sum(lens) >= 2 * t
        check_csr(rng, np.array(lens, dtype=np.int64), 31, dtype, False)


# ------------------------------------------------------------------------------------------------ the grid-stride loop
@pytest.mark.parametrize('n_batch', [None, 2])
def test_second_trip_of_the_grid_stride_loop(n_batch):
    """More tiles than the grid cap: by row (indptr), by row (fixed-length rows) and by column; with a batch the cap is
    shared by the batch rows, so the same bound is crossed at half the entries."""
    rng = np.random.default_rng(15)
    dtype = torch.float32
    t = T(dtype)
    cap = G // (n_batch or 1)
    nnz = cap * t + t + 3                        # CSR: 4-entry rows, the last one of 3
    full = nnz + 1                               # the fixed-number twin: one more entry fills the last row
    assert -(-nnz // t) > cap and full % 4 == 0
    rows, k = full // 4, 1000
    indices = rng.integers(0, k, full).astype(np.int32)
    indptr = np.minimum(np.arange(rows + 1, dtype=np.int64) * 4, nnz).astype(np.int32)
    lead = () if n_batch is None else (n_batch,)
    w = draw(rng, lead + (full,), dtype)
    y_row, y_col = draw(rng, lead + (rows,), dtype), draw(rng, lead + (k,), dtype)
    want_row, want_col = oracle(w, y_row, np.arange(full) // 4), oracle(w, y_col, indices)
    csr = be.csrmv_dt2t if n_batch is None else be.csrmm_dt2t
    fcn = be.fcnmv_dt2t if n_batch is None else be.fcnmm_dt2t
    wd, idx, ptr_ = dev(w), dev(indices), dev(indptr)
    w_csr = wd[..., :nnz].contiguous()
    assert_bits(csr(dev(y_row), w_csr, idx[:nnz], ptr_, shape=(rows, k)), want_row[..., :nnz])
    assert_bits(csr(dev(y_col), w_csr, idx[:nnz], ptr_, shape=(rows, k), transpose=True), want_col[..., :nnz])
    shape3 = lead + (rows, 4)
    assert_bits(fcn(wd.reshape(shape3), idx.reshape(rows, 4), dev(y_row), shape=(rows, k), transpose=False),
                want_row.reshape(shape3))
    assert_bits(fcn(wd.reshape(shape3), idx.reshape(rows, 4), dev(y_col), shape=(rows, k), transpose=True),
                want_col.reshape(shape3))


# ------------------------------------------------------------------------------------------------ views off a 16-byte boundary
@pytest.mark.parametrize('offsets', [(1, 1, 1), (0, 0, 1), (1, 0, 0), (0, 1, 0), (3, 2, 1)], ids=str)
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_misaligned_views_are_used_as_they_are(dtype, transpose, offsets):
    """`w`, `indices` and `out` as views that start `offsets` elements into their allocations: the same bits, the element in
    front of `out` untouched, and `out=w` updates the view's own memory (nothing was cloned)."""
    rng = np.random.default_rng(16)
    ow, oi, oo = offsets
    t, v = T(dtype), V(dtype)
    nnz = t + v + 3
    lens = two_entry_rows(nnz)
    m, k = len(lens), 53
    indices, indptr = csr_from_lens(lens, k, rng)
    w, y = draw(rng, (nnz,), dtype), draw(rng, (k if transpose else m,), dtype)
    want = oracle(w, y, indices if transpose else row_ids(indptr))
    base = torch.full((nnz + ow,), 7.0, dtype=dtype, device='cuda')
    wv = base[ow:]
    wv.copy_(dev(w))
    ibase = torch.zeros(nnz + oi, dtype=torch.int32, device='cuda')
    iv = ibase[oi:]
    iv.copy_(dev(indices))
    obase = torch.full((nnz + oo + 1,), 7.0, dtype=dtype, device='cuda')
    ov = obase[oo:oo + nnz]
    for t_, off in ((wv, ow), (iv, oi), (ov, oo)):
        assert t_.data_ptr() % 16 == (off * t_.element_size()) % 16
    got = be.csrmv_dt2t(dev(y), wv, iv, dev(indptr), shape=(m, k), transpose=transpose, out=ov)
    assert got is ov
    assert_bits(ov, want)
    assert bool((obase[:oo] == 7.0).all()) and float(obase[-1]) == 7.0          # neither side of the view was written
    assert_bits(wv, w)
    # in place: the view's own memory changes, the element in front of it does not
    back = be.csrmv_dt2t(dev(y), wv, iv, dev(indptr), shape=(m, k), transpose=transpose, out=wv)
    assert back is wv and back.data_ptr() == base.data_ptr() + ow * base.element_size()
    assert_bits(base[ow:], want)
    assert bool((base[:ow] == 7.0).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_batch_rows_of_odd_length_start_off_the_boundary(dtype):
    """`w (n_batch, nnz)` with an odd `nnz`: every batch row starts at another phase of the 16-byte grid."""
    rng = np.random.default_rng(17)
    nnz = T(dtype) + V(dtype) + 1
    assert nnz % 2 == 1
    for transpose in (False, True):
        check_csr(rng, two_entry_rows(nnz), 40, dtype, transpose, n_batch=5, check_in_place=True)


# ------------------------------------------------------------------------------------------------ in place, out=
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_in_place_equals_out_of_place(dtype, transpose):
    rng = np.random.default_rng(18)
    check_csr(rng, rng.poisson(6, 700), 90, dtype, transpose, check_in_place=True)
    rows, n_conn, k = 130, 7, 60
    indices = rng.integers(0, k, (rows, n_conn)).astype(np.int32)
    w, y = draw(rng, (rows, n_conn), dtype), draw(rng, (k if transpose else rows,), dtype)
    want = oracle(w.reshape(-1), y, indices.reshape(-1) if transpose else np.repeat(np.arange(rows), n_conn)).reshape(rows, n_conn)
    wd = dev(w)
    assert_bits(be.fcnmv_dt2t(wd, dev(indices), dev(y), shape=(rows, k), transpose=transpose), want)
    assert be.fcnmv_dt2t(wd, dev(indices), dev(y), shape=(rows, k), transpose=transpose, out=wd) is wd
    assert_bits(wd, want)


def test_out_of_a_wrong_kind_is_refused():
    w = torch.ones(4, device='cuda')
    y = torch.ones(2, device='cuda')
    idx = torch.tensor([0, 2, 1, 2], dtype=torch.int32, device='cuda')
    ptr_ = torch.tensor([0, 2, 4], dtype=torch.int32, device='cuda')
    for bad in (torch.empty(5, device='cuda'), torch.empty(4, dtype=torch.float64, device='cuda'), torch.empty(4),
                torch.empty(8, device='cuda')[::2]):
        with pytest.raises(ValueError):
            be.csrmv_dt2t(y, w, idx, ptr_, shape=(2, 3), out=bad)
    with pytest.raises(TypeError):
        be.csrmv_dt2t(y, w, idx, ptr_, shape=(2, 3), out=np.empty(4, np.float32))
    fi = idx.reshape(2, 2)
    with pytest.raises(ValueError):
        be.fcnmv_dt2t(w.reshape(2, 2), fi, y, shape=(2, 3), transpose=False, out=torch.empty(4, device='cuda'))
    with pytest.raises(TypeError):
        be.fcnmm_dt2t(w.reshape(1, 2, 2), fi, y.reshape(1, 2), shape=(2, 3), transpose=False, out=np.empty((1, 2, 2), np.float32))


# ------------------------------------------------------------------------------------------------ fixed-number connectivity
@pytest.mark.parametrize('n_conn', [1, 7, 64])
@pytest.mark.parametrize('dtype', DTYPES)
def test_fcn(dtype, n_conn):
    rng = np.random.default_rng(19)
    rows, k, nb = 130, 75, 3
    indices = rng.integers(0, k, (rows, n_conn)).astype(np.int32)
    by_row = np.repeat(np.arange(rows), n_conn)
    for transpose in (False, True):
        sel = indices.reshape(-1) if transpose else by_row
        n_y = k if transpose else rows
        w, y = draw(rng, (rows, n_conn), dtype), draw(rng, (n_y,), dtype)
        got = be.fcnmv_dt2t(dev(w), dev(indices), dev(y), shape=(rows, k), transpose=transpose)
        assert_bits(got, oracle(w.reshape(-1), y, sel).reshape(rows, n_conn))
        # one shared weight: a full-shaped result all the same
        w1 = draw(rng, (1,), dtype)
        got = be.fcnmv_dt2t(dev(w1), dev(indices), dev(y), shape=(rows, k), transpose=transpose)
        assert_bits(got, oracle(w1.expand(rows * n_conn).contiguous(), y, sel).reshape(rows, n_conn))
        wb, yb = draw(rng, (nb, rows, n_conn), dtype), draw(rng, (nb, n_y), dtype)
        got = be.fcnmm_dt2t(dev(wb), dev(indices), dev(yb), shape=(rows, k), transpose=transpose)
        assert_bits(got, oracle(wb.reshape(nb, -1), yb, sel).reshape(nb, rows, n_conn))
        got = be.fcnmm_dt2t(dev(w1), dev(indices), dev(yb), shape=(rows, k), transpose=transpose)
        assert_bits(got, oracle(w1.expand(nb, rows * n_conn).contiguous(), yb, sel).reshape(nb, rows, n_conn))


def distinct_columns(rng, rows, k, n_conn):
    return np.stack([rng.choice(k, n_conn, replace=False) for _ in range(rows)]).astype(np.int32)


def test_container_methods_follow_the_dense_matrix():
    """`dt2t` scales every stored entry by `y[pre]` (the row of the matrix the container stands for), `dt2t_transposed` by
    `y[post]`, whatever the storage axis: with distinct positions, `todense()` says where every entry sits."""
    rng = np.random.default_rng(20)
    n_pre, n_post, n_conn = 37, 29, 5
    y_pre, y_post = draw(rng, (n_pre,), torch.float32), draw(rng, (n_post,), torch.float32)

    def expect(M, pre_of, post_of, w):
        dense = M.todense()
        np.testing.assert_array_equal(dense[pre_of, post_of], w.numpy().reshape(-1))       # the positions are right
        return ((dense * y_pre.numpy()[:, None])[pre_of, post_of].reshape(w.shape),
                (dense * y_post.numpy()[None, :])[pre_of, post_of].reshape(w.shape))

    # FixedNumPerPre: indices (n_pre, n_conn) are post ids;  FixedNumPerPost: indices (n_post, n_conn) are pre ids
    cases = []
    idx = distinct_columns(rng, n_pre, n_post, n_conn)
    w = draw(rng, idx.shape, torch.float32)
    cases.append((be.FixedNumPerPre((dev(w), dev(idx)), shape=(n_pre, n_post)), np.repeat(np.arange(n_pre), n_conn), idx.reshape(-1), w))
    idx = distinct_columns(rng, n_post, n_pre, n_conn)
    w = draw(rng, idx.shape, torch.float32)
    cases.append((be.FixedNumPerPost((dev(w), dev(idx)), shape=(n_pre, n_post)), idx.reshape(-1), np.repeat(np.arange(n_post), n_conn), w))
    # CSR: rows are pre;  CSC: the stored rows are the post columns
    lens = rng.integers(0, 6, n_pre)
    idx = np.concatenate([rng.choice(n_post, n, replace=False) for n in lens]).astype(np.int32)
    ptr_ = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    w = draw(rng, idx.shape, torch.float32)
    cases.append((be.CSR((dev(w), dev(idx), dev(ptr_)), shape=(n_pre, n_post)), row_ids(ptr_), idx, w))
    lens = rng.integers(0, 6, n_post)
    idx = np.concatenate([rng.choice(n_pre, n, replace=False) for n in lens]).astype(np.int32)
    ptr_ = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    w = draw(rng, idx.shape, torch.float32)
    cases.append((be.CSC((dev(w), dev(idx), dev(ptr_)), shape=(n_pre, n_post)), idx, row_ids(ptr_), w))
    for M, pre_of, post_of, w in cases:
        by_pre, by_post = expect(M, pre_of, post_of, w)
        trace = dev(w).clone()
        assert_bits(M.dt2t(dev(y_pre), trace), torch.from_numpy(by_pre))
        assert_bits(M.dt2t_transposed(dev(y_post), trace), torch.from_numpy(by_post))
        assert isinstance(M.dt2t(y_pre.numpy(), w.numpy()), np.ndarray)                     # numpy in, numpy out
        assert M.dt2t(dev(y_pre), trace, out=trace) is trace                                # a trace beside M.data, in place
        assert_bits(trace, torch.from_numpy(by_pre))


# ------------------------------------------------------------------------------------------------ empty cases
def test_empty_cases():
    i32 = torch.int32
    e = torch.empty
    got = be.csrmv_dt2t(torch.ones(5, device='cuda'), e(0, device='cuda'), e(0, dtype=i32, device='cuda'),
                        torch.zeros(6, dtype=i32, device='cuda'), shape=(5, 4))
    assert tuple(got.shape) == (0,) and got.dtype == torch.float32
    got = be.csrmv_dt2t(e(0, device='cuda'), e(0, device='cuda'), e(0, dtype=i32, device='cuda'),
                        torch.zeros(1, dtype=i32, device='cuda'), shape=(0, 4))
    assert tuple(got.shape) == (0,)
    got = be.csrmm_dt2t(e((0, 2), device='cuda'), e((0, 4), device='cuda'), torch.tensor([0, 2, 1, 2], dtype=i32, device='cuda'),
                        torch.tensor([0, 2, 4], dtype=i32, device='cuda'), shape=(2, 3))
    assert tuple(got.shape) == (0, 4)
    got = be.csrmm_dt2t(torch.ones((3, 5), device='cuda'), e((3, 0), device='cuda'), e(0, dtype=i32, device='cuda'),
                        torch.zeros(6, dtype=i32, device='cuda'), shape=(5, 4), transpose=False)
    assert tuple(got.shape) == (3, 0)
    for transpose in (False, True):
        got = be.fcnmv_dt2t(e((4, 0), device='cuda'), e((4, 0), dtype=i32, device='cuda'), torch.ones(3 if transpose else 4, device='cuda'),
                            shape=(4, 3), transpose=transpose)
        assert tuple(got.shape) == (4, 0)
        got = be.fcnmv_dt2t(torch.ones(1, device='cuda'), e((0, 3), dtype=i32, device='cuda'), torch.ones(5 if transpose else 0, device='cuda'),
                            shape=(0, 5), transpose=transpose)
        assert tuple(got.shape) == (0, 3)
        got = be.fcnmm_dt2t(e((0, 4, 2), device='cuda'), torch.zeros((4, 2), dtype=i32, device='cuda'),
                            e((0, 3 if transpose else 4), device='cuda'), shape=(4, 3), transpose=transpose)
        assert tuple(got.shape) == (0, 4, 2)
    assert isinstance(be.csrmv_dt2t(np.ones(5, np.float32), np.empty(0, np.float32), np.empty(0, np.int32), np.zeros(6, np.int32),
                                    shape=(5, 4)), np.ndarray)


# ------------------------------------------------------------------------------------------------ graph capture
def test_captured_step_follows_y():
    rng = np.random.default_rng(21)
    dtype = torch.float32
    lens = rng.poisson(4, 500)
    m, k = len(lens), 80
    indices, indptr = csr_from_lens(lens, k, rng)
    w, y0, y1 = draw(rng, (len(indices),), dtype), draw(rng, (m,), dtype), draw(rng, (m,), dtype)
    wd, idx, ptr_ = dev(w), dev(indices), dev(indptr)
    y = dev(y0)
    buf = torch.zeros_like(wd)
    step = be.capture_step(lambda: be.csrmv_dt2t(y, wd, idx, ptr_, shape=(m, k), out=buf))
    assert step() is buf
    torch.cuda.synchronize()
    assert_bits(buf, oracle(w, y0, row_ids(indptr)))
    y.copy_(dev(y1))
    step()
    torch.cuda.synchronize()
    assert_bits(buf, oracle(w, y1, row_ids(indptr)))


def test_binned_status_stays_clean():
    """Nothing here goes near the binned scatter route: its status registry is as clean after this module as before."""
    be.check_binned_status()
