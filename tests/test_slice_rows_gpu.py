"""Row slicing (brainevent_amd/_slice.py, csrc/be_slice.hip) against a few lines of numpy, bit for bit.

Per-entry weights: the oracle is `np.add.at` into an f32 (f64 for f64) array in storage order and one rounding to the dtype
(torch on the CPU for bf16) — the kernel's contract — so every comparison is `assert_array_equal` on the bit patterns, for all
four dtypes.  One shared weight: integer counts x w, one product.  Weights are random sign x uniform [0.5, 2) rounded to the
dtype: sums of a few of them are multiples of 2^-11 far above the f32 subnormals, so nothing depends on a denormal mode.  For
CSC / FixedNumPerPost the order inside a mirror row is the builder's business: their weights are small integers (|w| <= 8, exact
in bf16), so every order gives the same bits and the comparisons stay exact.

Sizes come from CONSTS, the geometry of csrc/be_slice.hip (tests/test_slice_rows_cpu.py compares the table with the source):
T = columns of one forward tile, P = threads * entries_per_thread = entries of one pass over a row.

The shared-weight case "4w differs from ((w+w)+w)+w in f16" cannot be built: an exhaustive search over every finite f16 finds
no such w for multiplicities 2 to 5 (the first is 6).  Multiplicity 4 is checked against count x w, and multiplicity 6 with
w = 1 + 2^-10, where six additions in f16 give 6.004 and 6w gives 6.008."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd._misc import build_sub_csr

pytestmark = pytest.mark.gpu

CONSTS = {'threads': 256, 'tile_cols': 4096, 'tile_cols_f64': 2048, 'entries_per_thread': 8, 'vec_bytes': 16, 'grad_split': 8,
          'copy_per_thread': 4}
P = CONSTS['threads'] * CONSTS['entries_per_thread']
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def T(dtype) -> int:
    return CONSTS['tile_cols_f64'] if dtype == torch.float64 else CONSTS['tile_cols']


def dev(x):
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to('cuda')


def draw(rng, shape, dtype) -> torch.Tensor:
    """random sign x uniform [0.5, 2), rounded to `dtype` (CPU tensor)."""
    v = rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype)


def draw_int(rng, shape, dtype) -> torch.Tensor:
    """non-zero integers in [-8, 8] (CPU tensor): every sum of a few of them is exact in every dtype."""
    v = rng.integers(1, 9, shape) * rng.choice([-1, 1], shape)
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype)


def acc_of(t: torch.Tensor) -> np.ndarray:
    """the values in the accumulation type: f64 for f64, f32 otherwise (exact)."""
    return t.numpy() if t.dtype == torch.float64 else t.float().numpy()


def rounded(a: np.ndarray, dtype) -> torch.Tensor:
    """one rounding of an accumulator array to `dtype` (torch on the CPU: round to nearest even, as the kernel's converts)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def bits(t) -> np.ndarray:
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    t = t.detach().cpu().contiguous()
    return t.view(BITS[t.element_size()]).numpy()


def assert_bits(got, want):
    got = torch.from_numpy(got) if isinstance(got, np.ndarray) else got
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    np.testing.assert_array_equal(bits(got), bits(want))


def make_csr(rng, lens, n_cols, ptr_dtype=np.int32):
    indptr = np.zeros(len(lens) + 1, dtype=ptr_dtype)
    np.cumsum(lens, out=indptr[1:])
    indices = rng.integers(0, n_cols, int(indptr[-1])).astype(np.int32)          # unsorted, with duplicates
    return indices, indptr


def dense_rows(w: torch.Tensor, indices, indptr, rows, n_cols) -> torch.Tensor:
    """The oracle: `out[k, indices[j]] += w[j]` over row rows[k] in storage order in the accumulation type, one rounding.
    A row outside the matrix is a zero row.  One shared weight: integer counts x w (+0 where the count is 0)."""
    vals = acc_of(w)
    n_rows = len(indptr) - 1
    out = np.zeros((len(rows), n_cols), dtype=vals.dtype)
    for k, r in enumerate(rows):
        if not 0 <= r < n_rows:
            continue
        cols = indices[indptr[r]:indptr[r + 1]]
        if vals.size == 1 and len(indices) != 1:
            count = np.bincount(cols, minlength=n_cols)
            out[k] = np.where(count > 0, count.astype(vals.dtype) * vals[0], 0)          # (no entry: +0 whatever the sign of w)
        else:
            np.add.at(out[k], cols, vals[indptr[r]:indptr[r + 1]])
    return rounded(out, w.dtype)


def check(w, indices, indptr, rows, n_cols):
    """the functional op on device tensors against the oracle."""
    n_rows = len(indptr) - 1
    got = be.csr_slice_rows(dev(w), dev(indices), dev(indptr), dev(np.asarray(rows, dtype=np.int64)), shape=(n_rows, n_cols))
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.is_contiguous()
    assert_bits(got, dense_rows(w, indices, indptr, rows, n_cols))
    return got


# ------------------------------------------------------------------------------------------------ n_cols on the tile's edges
def edge_cases():
    for dtype in DTYPES:
        t = T(dtype)
        for n_cols in (1, 7, t - 1, t, t + 1, 2 * t + 3):
            yield pytest.param(dtype, n_cols, id=f"{str(dtype)[6:]}-{n_cols}")
    for dtype in (torch.float16, torch.bfloat16):
        yield pytest.param(dtype, 1001, id=f"{str(dtype)[6:]}-1001")             # rows of out start off a 16-byte boundary


@pytest.mark.parametrize('dtype, n_cols', list(edge_cases()))
def test_n_cols_on_the_tile_edges(dtype, n_cols):
    rng = np.random.default_rng(n_cols)
    lens = [0, 3, 40, 1, 7]
    indices, indptr = make_csr(rng, lens, n_cols)
    indices[indptr[2] + 5], indices[indptr[2] + 1] = 0, n_cols - 1              # both ends, out of order
    indices[indptr[4]] = n_cols - 1
    w = draw(rng, len(indices), dtype)
    check(w, indices, indptr, [2, 0, 4, 2, 1, 3], n_cols)
    check(w[:1], indices, indptr, [4, 2, 0], n_cols)                              # one shared weight


# ------------------------------------------------------------------------------------------------ row shapes
@pytest.mark.parametrize('dtype', DTYPES)
def test_a_row_longer_than_one_pass_with_many_duplicates(dtype):
    """P + 1 entries over 300 columns: about 7 entries per column, spread over both passes — the rounds inside a pass and the
    order between passes."""
    rng = np.random.default_rng(1)
    indices, indptr = make_csr(rng, [P + 1, 0, 5], 300)
    w = draw(rng, len(indices), dtype)
    check(w, indices, indptr, [0, 1, 2, 0], 300)
    check(w[:1], indices, indptr, [0, 2], 300)


def test_rows_of_length_zero_no_entries_and_no_selection():
    rng = np.random.default_rng(2)
    indices, indptr = make_csr(rng, [0, 0, 4, 0], 9)
    w = draw(rng, 4, torch.float32)
    got = check(w, indices, indptr, [0, 1, 3], 9)
    assert not got.any()
    none, zeros = np.zeros(0, np.int32), np.zeros(4, np.int32)
    got = check(torch.zeros(0), none, zeros, [0, 2], 9)                          # nse == 0
    assert got.shape == (2, 9) and not got.any()
    got = check(torch.ones(1), none, zeros, [1], 9)                              # nse == 0, a shared weight
    assert not got.any()
    got = check(w, indices, indptr, [], 9)                                        # n_sel == 0
    assert got.shape == (0, 9)


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_whole_matrix_equals_todense(dtype):
    rng = np.random.default_rng(3)
    indices, indptr = make_csr(rng, [5, 0, 17, 2, 9, 1], 13)
    w = draw_int(rng, len(indices), dtype)                                        # (todense sums in the dtype: integers are exact)
    csr = be.CSR((dev(w), dev(indices), dev(indptr)), shape=(6, 13))
    got = csr[:]
    assert got.shape == (6, 13)
    np.testing.assert_array_equal(got.double().cpu().numpy(), csr.todense().astype(np.float64))


# ------------------------------------------------------------------------------------------------ row_indices
def test_duplicate_descending_and_out_of_range_row_indices():
    rng = np.random.default_rng(4)
    indices, indptr = make_csr(rng, [3, 0, 8, 2, 6], 11)
    w = draw(rng, len(indices), torch.float32)
    check(w, indices, indptr, [4, 4, 3, 2, 2, 2, 0], 11)
    got = check(w, indices, indptr, [-1, 2, 5, 0, -6, 1 << 40], 11)               # the functional op: zero rows
    assert not got[[0, 2, 4, 5]].any() and got[1].any()


def test_negative_indices_through_the_containers():
    rng = np.random.default_rng(5)
    indices, indptr = make_csr(rng, [3, 0, 8, 2, 6], 11)
    w = draw(rng, len(indices), torch.float32)
    csr = be.CSR((dev(w), dev(indices), dev(indptr)), shape=(5, 11))
    assert_bits(csr[[3, 2, 2, -1]], dense_rows(w, indices, indptr, [3, 2, 2, 4], 11))
    assert_bits(csr[-3], dense_rows(w, indices, indptr, [2], 11)[0])
    assert_bits(csr[torch.tensor([-5, 4], device='cuda')], dense_rows(w, indices, indptr, [0, 4], 11))
    assert_bits(csr[::-2], dense_rows(w, indices, indptr, [4, 2, 0], 11))
    assert csr[[]].shape == (0, 11)
    with pytest.raises(IndexError):
        csr[5]
    with pytest.raises(IndexError):
        csr[[0, -6]]


def test_seventy_thousand_selected_rows():
    """n_sel beyond 65535: the selection runs along the grid's x."""
    rng = np.random.default_rng(6)
    indices, indptr = make_csr(rng, rng.integers(0, 12, 50), 8)
    w = draw(rng, len(indices), torch.float32)
    rows = rng.integers(0, 50, 70_000)
    got = be.csr_slice_rows(dev(w), dev(indices), dev(indptr), dev(rows), shape=(50, 8))
    assert_bits(got, dense_rows(w, indices, indptr, np.arange(50), 8)[torch.from_numpy(rows)])


# ------------------------------------------------------------------------------------------------ duplicate columns in a row
@pytest.mark.parametrize('dtype', DTYPES)
def test_multiplicities_two_three_and_five(dtype):
    rng = np.random.default_rng(7)
    cols = np.array([4, 9, 4, 0, 9, 6, 6, 9, 6, 11, 6, 6], np.int32)              # 4 twice, 9 three times, 6 five times
    indptr = np.array([0, len(cols)], np.int32)
    w = draw(rng, len(cols), dtype)
    got = check(w, cols, indptr, [0], 12)
    want32 = acc_of(w)
    six = want32[5]
    for j in (6, 8, 10, 11):
        six = six + want32[j]
    assert float(got[0, 6]) == float(rounded(np.asarray(six), dtype))             # (the oracle, spelled out once)


def test_the_sum_runs_in_ascending_storage_order():
    """[1e8, 1.0, -1e8] on one column: (1e8 + 1) - 1e8 = 0 in f32; any other order gives 1."""
    w = torch.tensor([1e8, 1.0, -1e8, 2.0], dtype=torch.float32)
    cols, indptr = np.array([3, 3, 3, 1], np.int32), np.array([0, 4], np.int32)
    got = check(w, cols, indptr, [0], 5)
    assert got[0].tolist() == [0.0, 2.0, 0.0, 0.0, 0.0]


def test_a_shared_weight_is_counted_not_added():
    """out = count x w with one rounding.  Multiplicity 4 (no f16 value tells 4w from repeated addition: see the module's
    docstring) and multiplicity 6 with w = 1 + 2^-10, where repeated addition in f16 gives another result."""
    w = torch.tensor([1.0 + 2.0 ** -10], dtype=torch.float16)
    cols = np.array([2, 5, 2, 2, 5, 2, 5, 5, 5, 5, 0], np.int32)                  # 2 four times, 5 six times
    got = check(w, cols, np.array([0, len(cols)], np.int32), [0], 6)
    added = w.numpy()[0]
    for _ in range(5):
        added = np.float16(added + w.numpy()[0])
    six = np.float16(np.float32(6) * np.float32(w.numpy()[0]))
    assert added != six                                                           # the two rules differ here ...
    assert got[0, 5].item() == float(six) and got[0, 2].item() == float(np.float16(4 * np.float32(w.numpy()[0])))


# ------------------------------------------------------------------------------------------------ structure variants
def test_int64_indptr():
    rng = np.random.default_rng(8)
    indices, indptr = make_csr(rng, [3, 0, 8, 2, 6], 11, ptr_dtype=np.int64)
    w = draw(rng, len(indices), torch.bfloat16)
    check(w, indices, indptr, [4, 1, 2], 11)


@pytest.mark.parametrize('dtype', DTYPES)
def test_fixed_length_rows_through_fixed_num_per_pre(dtype):
    """indptr = NULL + row_len; connectivity drawn with replacement: duplicates in most rows."""
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 10, (6, 7)).astype(np.int32)
    w = draw(rng, (6, 7), dtype)
    M = be.FixedNumPerPre((dev(w), dev(idx)), shape=(6, 10))
    indptr = np.arange(7) * 7
    assert_bits(M[[5, 0, 0, -2]], dense_rows(w.reshape(-1), idx.reshape(-1), indptr, [5, 0, 0, 4], 10))
    assert_bits(M[3], dense_rows(w.reshape(-1), idx.reshape(-1), indptr, [3], 10)[0])
    H = be.FixedNumPerPre((dev(w.reshape(-1)[:1]), dev(idx)), shape=(6, 10))
    assert_bits(H[[1, 4]], dense_rows(w.reshape(-1)[:1], idx.reshape(-1), indptr, [1, 4], 10))


def test_a_host_container_returns_numpy():
    rng = np.random.default_rng(10)
    indices, indptr = make_csr(rng, [3, 0, 8, 2, 6], 11)
    w = draw(rng, len(indices), torch.float32)
    csr = be.CSR((w.numpy(), indices, indptr), shape=(5, 11))
    got = csr[[1, 2]]
    assert isinstance(got, np.ndarray)
    assert_bits(got, dense_rows(w, indices, indptr, [1, 2], 11))
    assert isinstance(csr[2], np.ndarray) and csr[2].shape == (11,)
    got = be.csr_slice_rows(w.numpy(), indices, indptr, np.array(2), shape=(5, 11))
    assert isinstance(got, np.ndarray) and got.shape == (11,)
    assert isinstance(csr.slice_rows([1, 2]).todense(), np.ndarray)


# ------------------------------------------------------------------------------------------------ slice_rows
def canonical(data, indices, indptr):
    """(indptr, the (index, value) pairs of every stored row in sorted order)."""
    data = np.asarray(data.double().cpu() if isinstance(data, torch.Tensor) else data)
    indices, indptr = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t).astype(np.int64) for t in (indices, indptr))
    rows = []
    for r in range(len(indptr) - 1):
        seg = slice(indptr[r], indptr[r + 1])
        vals = np.broadcast_to(data, indices.shape)[seg] if data.size == 1 and indices.size != 1 else data[seg]
        rows.append(sorted(zip(indices[seg].tolist(), vals.tolist())))
    return indptr.tolist(), rows


ROWSETS = [[3, 1, 1, -1], 2, slice(None, None, -2), [0]]


@pytest.mark.parametrize('rows', ROWSETS, ids=['list', 'int', 'slice', 'empty-row'])
@pytest.mark.parametrize('homo', [False, True], ids=['hetero', 'homo'])
def test_csr_slice_rows(rows, homo):
    rng = np.random.default_rng(11)
    indices, indptr = make_csr(rng, [0, 6, 3, 0, 9], 7)
    w = draw(rng, 1 if homo else len(indices), torch.float16)
    csr = be.CSR((dev(w), dev(indices), dev(indptr)), shape=(5, 7))
    sub = csr.slice_rows(rows)
    sel = np.atleast_1d(np.arange(5)[rows])
    assert type(sub) is be.CSR and sub.shape == (len(sel), 7)
    np.testing.assert_array_equal(sub.todense(), csr.todense()[sel])
    # the structure arrays, exactly: the segments of the selected rows one after the other
    gather = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in sel]).astype(np.int64)
    new_ptr = np.concatenate([[0], np.cumsum(indptr[sel + 1] - indptr[sel])])
    np.testing.assert_array_equal(sub.indptr.cpu().numpy(), new_ptr)
    assert sub.indptr.dtype == torch.int32 and sub.indices.dtype == torch.int32
    np.testing.assert_array_equal(sub.indices.cpu().numpy(), indices[gather])
    assert_bits(sub.data, w if homo else w[torch.from_numpy(gather)])


def test_sub_csr_copy_is_balanced_over_long_and_empty_rows():
    """more than one tile of the copy, a row longer than a tile, runs of empty rows, int64 indptr, 8-byte data."""
    rng = np.random.default_rng(12)
    tile = CONSTS['threads'] * CONSTS['copy_per_thread']
    lens = [0, 0, 2 * tile + 5, 0, 1, 0, 0, tile - 1, 3]
    indices, indptr = make_csr(rng, lens, 50, ptr_dtype=np.int64)
    w = draw(rng, len(indices), torch.float64)
    sel = np.array([8, 2, 0, 1, 7, 2, 3, 4, 6])
    data, idx, ptr, shape = build_sub_csr(dev(w), dev(indices), dev(indptr), dev(sel), 50)
    gather = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in sel])
    assert shape == (9, 50) and ptr.dtype == torch.int64
    np.testing.assert_array_equal(ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(indptr[sel + 1] - indptr[sel])]))
    np.testing.assert_array_equal(idx.cpu().numpy(), indices[gather])
    assert_bits(data, w[torch.from_numpy(gather)])
    with pytest.raises(IndexError):
        build_sub_csr(dev(w), dev(indices), dev(indptr), dev(np.array([9])), 50)


@pytest.mark.parametrize('homo', [False, True], ids=['hetero', 'homo'])
def test_fixed_num_per_pre_slice_rows(homo):
    rng = np.random.default_rng(13)
    idx = rng.integers(0, 10, (6, 4)).astype(np.int32)
    w = draw(rng, 1 if homo else (6, 4), torch.float32)
    M = be.FixedNumPerPre((dev(w), dev(idx)), shape=(6, 10))
    for rows in ([5, 0, 0, -2], 3, slice(1, 4)):
        sel = np.atleast_1d(np.arange(6)[rows])
        sub = M.slice_rows(rows)
        assert type(sub) is be.FixedNumPerPre and sub.shape == (len(sel), 10)
        np.testing.assert_array_equal(sub.indices.cpu().numpy(), idx[sel])
        assert_bits(sub.data, w if homo else w[torch.from_numpy(sel)])
        np.testing.assert_array_equal(sub.todense(), M.todense()[sel])


def column_stored(rng, cls, dtype, homo=False):
    """a (6, 5) matrix stored by columns, small integer weights; returns (container, data, the CSR arrays of W in some order)."""
    if cls is be.CSC:
        indices, indptr = make_csr(rng, [4, 0, 6, 3, 5], 6)                      # 5 stored rows = columns of W, ids = rows of W
        w = draw_int(rng, 1 if homo else len(indices), dtype)
        M = be.CSC((dev(w), dev(indices), dev(indptr)), shape=(6, 5))
        col_of = np.repeat(np.arange(5), np.diff(indptr))
        row_of = indices
    else:
        idx = rng.integers(0, 6, (5, 4)).astype(np.int32)                         # FixedNumPerPost: 4 pre ids per post column
        w = draw_int(rng, 1 if homo else (5, 4), dtype)
        M = be.FixedNumPerPost((dev(w), dev(idx)), shape=(6, 5))
        col_of, row_of = np.repeat(np.arange(5), 4), idx.reshape(-1)
    order = np.argsort(row_of, kind='stable')
    r_ptr = np.concatenate([[0], np.cumsum(np.bincount(row_of, minlength=6))]).astype(np.int32)
    flat = w.reshape(-1)
    return M, w, (flat if homo else flat[torch.from_numpy(order)]), col_of[order].astype(np.int32), r_ptr, order


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cls', [be.CSC, be.FixedNumPerPost])
@pytest.mark.parametrize('homo', [False, True], ids=['hetero', 'homo'])
def test_column_stored_containers_read_rows_of_w(cls, dtype, homo):
    rng = np.random.default_rng(14)
    M, _, rw, rcols, rptr, _ = column_stored(rng, cls, dtype, homo)
    assert_bits(M[[5, 2, 2, -6]], dense_rows(rw, rcols, rptr, [5, 2, 2, 0], 5))
    assert_bits(M[1], dense_rows(rw, rcols, rptr, [1], 5)[0])
    np.testing.assert_array_equal(M[:].double().cpu().numpy(), M.todense().astype(np.float64))


@pytest.mark.parametrize('cls, want', [(be.CSC, be.CSC), (be.FixedNumPerPost, be.CSR)])
@pytest.mark.parametrize('homo', [False, True], ids=['hetero', 'homo'])
def test_column_stored_slice_rows(cls, want, homo):
    rng = np.random.default_rng(15)
    M, _, rw, rcols, rptr, _ = column_stored(rng, cls, torch.float32, homo)
    for rows in ([5, 2, 2, -6], 4, slice(None, None, 2)):
        sel = np.atleast_1d(np.arange(6)[rows])
        sub = M.slice_rows(rows)
        assert type(sub) is want and sub.shape == (len(sel), 5)
        np.testing.assert_array_equal(sub.todense(), M.todense()[sel])
        # the structure against the numpy construction (the order inside a stored row is the builder's business)
        gather = np.concatenate([np.arange(rptr[r], rptr[r + 1]) for r in sel]).astype(np.int64)
        s_ptr = np.concatenate([[0], np.cumsum(rptr[sel + 1] - rptr[sel])])
        s_cols, s_w = rcols[gather], (rw if homo else rw[torch.from_numpy(gather)])
        if want is be.CSC:                                                        # ... re-encoded by columns
            s_rows = np.repeat(np.arange(len(sel)), np.diff(s_ptr))
            order = np.argsort(s_cols, kind='stable')
            s_ptr = np.concatenate([[0], np.cumsum(np.bincount(s_cols, minlength=5))])
            s_cols, s_w = s_rows[order], (s_w if homo else s_w[torch.from_numpy(order)])
        assert canonical(sub.data, sub.indices, sub.indptr) == canonical(s_w, s_cols, s_ptr)


# ------------------------------------------------------------------------------------------------ gradient
def grad_oracle(ct: torch.Tensor, indices, indptr, rows) -> np.ndarray:
    """`dw[j] += ct[k, indices[j]]` for k ascending, in the accumulation type (not yet rounded)."""
    g = acc_of(ct)
    dw = np.zeros(len(indices), dtype=g.dtype)
    n_rows = len(indptr) - 1
    for k, r in enumerate(rows):
        if 0 <= r < n_rows:
            seg = slice(indptr[r], indptr[r + 1])
            dw[seg] = dw[seg] + g[k, indices[seg]]
    return dw


@pytest.mark.parametrize('dtype', DTYPES)
def test_grad_bit_for_bit_with_duplicate_rows_and_poisoned_storage(dtype):
    """rows selected three times, rows not selected (exact zeros whatever the allocator hands over: the storage dw is about to
    get is filled with NaN by hand), a row longer than one block's stride, rows out of range."""
    rng = np.random.default_rng(16)
    n_cols = 37
    lens = [5, 0, CONSTS['threads'] * CONSTS['grad_split'] + 3, 4, 7, 2]
    indices, indptr = make_csr(rng, lens, n_cols)
    rows = [4, 2, 4, 0, 4, 2, -1, 2, 6]
    ct = draw(rng, (len(rows), n_cols), dtype)
    args = (dev(ct), dev(indices), dev(indptr), dev(np.asarray(rows)))
    poison = torch.full((len(indices),), float('nan'), dtype=dtype, device='cuda')
    del poison
    got = be.csr_slice_rows_grad(*args, shape=(6, n_cols))
    assert_bits(got, rounded(grad_oracle(ct, indices, indptr, rows), dtype))
    unselected = np.r_[indptr[1]:indptr[2], indptr[3]:indptr[4], indptr[5]:indptr[6]]
    assert not bits(got)[unselected].any()
    # int64 indptr, nothing selected
    got = be.csr_slice_rows_grad(dev(ct[:0]), dev(indices), dev(indptr.astype(np.int64)), dev(np.zeros(0, np.int64)), shape=(6, n_cols))
    assert got.shape == (len(indices),) and not bits(got).any()


def shared_weight_grad(w, indices, indptr, rows, g, shape):
    data = dev(w).requires_grad_()
    out = be.csr_slice_rows(data, dev(indices), dev(indptr), dev(np.asarray(rows)), shape=shape)
    (out * dev(g)).sum().backward()
    return data.grad


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_shared_weight_grad_is_reproducible_and_within_the_summation_bound(dtype):
    """The scalar sum over every selected entry: identical run to run; against the f64 sum within n x 2^-24 x sum|terms|, the
    worst case of any f32 summation order (f64: 2^-53)."""
    rng = np.random.default_rng(17)
    n_cols = 91
    indices, indptr = make_csr(rng, rng.integers(0, 700, 40), n_cols)
    rows = rng.integers(0, 40, 64)
    g = draw(rng, (64, n_cols), dtype)
    w = torch.tensor([0.75], dtype=dtype)
    first = shared_weight_grad(w, indices, indptr, rows, g, (40, n_cols))
    second = shared_weight_grad(w, indices, indptr, rows, g, (40, n_cols))
    assert first.shape == (1,) and first.dtype == dtype
    assert_bits(first, second)
    terms = np.concatenate([g.double().numpy()[k, indices[indptr[r]:indptr[r + 1]]] for k, r in enumerate(rows)])
    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    bound = len(terms) * eps * np.abs(terms).sum()
    err = abs(float(first.double()) - terms.sum())
    print(f"shared-weight grad {dtype}: {len(terms)} terms, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def container_of(cls, rng, dtype, homo=False):
    """(container over a (6, 5) matrix with `data` requiring grad, data, row of W and column of W of every stored entry)."""
    if cls in (be.CSC, be.FixedNumPerPost):
        M, w, _, _, _, _ = column_stored(rng, cls, dtype, homo)
        stored = M._stored_rows()
        idx = stored.indices.cpu().numpy().reshape(-1)
        per = np.diff(M.indptr.cpu().numpy()) if cls is be.CSC else np.full(5, 4)
        row_of, col_of = idx, np.repeat(np.arange(5), per)
    elif cls is be.CSR:
        indices, indptr = make_csr(rng, [4, 0, 6, 3, 5, 2], 5)
        w = draw(rng, 1 if homo else len(indices), dtype)
        M = be.CSR((dev(w), dev(indices), dev(indptr)), shape=(6, 5))
        row_of, col_of = np.repeat(np.arange(6), np.diff(indptr)), indices
    else:
        idx = rng.integers(0, 5, (6, 3)).astype(np.int32)
        w = draw(rng, 1 if homo else (6, 3), dtype)
        M = be.FixedNumPerPre((dev(w), dev(idx)), shape=(6, 5))
        row_of, col_of = np.repeat(np.arange(6), 3), idx.reshape(-1)
    M.data.requires_grad_()
    return M, w, row_of, col_of


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cls', [be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost])
def test_backward_through_the_containers(cls, dtype):
    """`loss = (M[rows] * g).sum()`: data.grad has data's shape; entry j gets the sum of g[k, col(j)] over the k that selected
    its row, ascending."""
    rng = np.random.default_rng(18)
    M, w, row_of, col_of = container_of(cls, rng, dtype)
    rows = [3, 5, 3, 0, 3, -2]
    sel = [3, 5, 3, 0, 3, 4]
    g = draw_int(rng, (len(rows), 5), dtype) if M._stored_transposed else draw(rng, (len(rows), 5), dtype)
    out = M[rows]
    assert out.grad_fn is not None
    (out * dev(g)).sum().backward()
    dense = np.zeros((6, 5), dtype=acc_of(g).dtype)
    for k, r in enumerate(sel):
        dense[r] = dense[r] + acc_of(g)[k]
    assert M.data.grad.shape == M.data.shape and M.data.grad.dtype == dtype
    assert_bits(M.data.grad.reshape(-1), rounded(dense[row_of, col_of], dtype))


@pytest.mark.parametrize('cls', [be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost])
def test_backward_of_a_shared_weight_through_the_containers(cls):
    rng = np.random.default_rng(19)
    M, w, row_of, col_of = container_of(cls, rng, torch.float32, homo=True)
    g = draw_int(rng, (3, 5), torch.float32)
    (M[[1, 4, 4]] * dev(g)).sum().backward()
    want = sum(float(g[k, c]) for k, r in enumerate([1, 4, 4]) for rr, c in zip(row_of, col_of) if rr == r)
    assert M.data.grad.shape == M.data.shape and float(M.data.grad.reshape(-1)[0]) == want
    row = M[2]
    assert row.shape == (5,) and row.grad_fn is not None


@pytest.mark.parametrize('cls', [be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost])
def test_without_requires_grad_the_plain_path_is_taken(cls):
    rng = np.random.default_rng(20)
    M, _, _, _ = container_of(cls, rng, torch.float32)
    M.data.requires_grad_(False)
    assert M[[0, 1]].grad_fn is None and not M[[0, 1]].requires_grad
    M.data.requires_grad_()
    with torch.no_grad():
        assert M[[0, 1]].grad_fn is None
    assert M[[0, 1]].grad_fn is not None


# ------------------------------------------------------------------------------------------------ hygiene
def test_a_cached_released_mirror_is_left_alone():
    """A CSC whose cached mirror gave up its raw arrays reads rows through a private mirror: the cached object stays, nothing
    under `buffers` is replaced."""
    from brainevent_amd._csr import weights_stamp
    rng = np.random.default_rng(21)
    M, _, rw, rcols, rptr, _ = column_stored(rng, be.CSC, torch.float32)
    released = be.Mirror((6, 5), torch.empty(0, device='cuda'), None, None, None, None, weights_stamp(M.data), False)
    assert released.released
    M.buffers['mirror'] = released
    M.buffers['other'] = marker = object()
    before = dict(M.buffers)
    assert_bits(M[[5, 2, 2]], dense_rows(rw, rcols, rptr, [5, 2, 2], 5))
    M.data.requires_grad_()
    (M[[1]] * 2).sum().backward()
    assert M.data.grad is not None
    assert type(M.slice_rows([0, 3])) is be.CSC
    assert set(M.buffers) == set(before) and all(M.buffers[k] is before[k] for k in before)
    assert M.buffers['mirror'] is released and M.buffers['other'] is marker


def test_a_cached_mirror_is_used_and_kept():
    rng = np.random.default_rng(22)
    M, _, rw, rcols, rptr, _ = column_stored(rng, be.FixedNumPerPost, torch.float16)
    assert 'mirror' not in M.buffers
    M[[0]]
    mr = M.buffers['mirror']
    assert mr is not None and not mr.released and mr.perm is not None
    assert_bits(M[[4, 4]], dense_rows(rw, rcols, rptr, [4, 4], 5))
    assert M.buffers['mirror'] is mr
