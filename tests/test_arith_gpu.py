"""Container arithmetic (brainevent_amd/_arith.py, csrc/be_arith.hip: be_entries_dense_op) on the device.

Expected values are torch's (or numpy's) own: for the sample kernel `fn(w, D[row_ids, idx])` computed by torch on the device —
one product (or one division) in f32 (f64 for f64) and one rounding on both sides, so every comparison is on the bit patterns;
for the operators `fn(M.todense(), x)` on integer-valued matrices (every result exact in every dtype).  Where `fn(0, x) != 0`
and the rule keeps the result sparse (`x / M`, a callable given to `apply2`) the stored entries are compared instead.

Sizes come from CONSTS, the geometry of csrc/be_arith.hip (tests/test_arith_cpu.py compares the table with the source):
a tile is `tile` consecutive entries, the grid is capped at `grid_cap` blocks."""
import operator

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd._diag import DiagPlan

pytestmark = pytest.mark.gpu

CONSTS = {'threads': 256, 'tile': 2048, 'grid_cap': 4096}
T = CONSTS['tile']
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
STORED = [be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost]
SHAPE = (37, 53)


def dev(x):
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to('cuda')


def bits(t) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(BITS[t.element_size()]).numpy()


def assert_bits(got, want):
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(bits(got), bits(want))


def draw(rng, shape, dtype) -> torch.Tensor:
    """random sign x uniform [0.5, 2), rounded to `dtype` (device tensor): products and quotients stay far from the subnormals."""
    v = rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
    return dev(np.asarray(v, dtype=np.float64)).to(dtype)


def draw_pow2(rng, shape, dtype) -> torch.Tensor:
    """+-{1, 2, 4}: every product and quotient is exact in every dtype."""
    return dev(rng.choice([1.0, 2.0, 4.0], shape) * rng.choice([-1.0, 1.0], shape)).to(dtype)


def make_csr(rng, lens, n_cols, ptr_dtype=np.int32):
    indptr = np.zeros(len(lens) + 1, dtype=ptr_dtype)
    np.cumsum(lens, out=indptr[1:])
    return rng.integers(0, n_cols, int(indptr[-1])).astype(np.int32), indptr          # unsorted, with duplicates


def torch_op(op, w, d):
    """torch's own answer for one entry array: d are the operand's values on the pattern, already in w's dtype."""
    return {'take': lambda: d.clone(), 'mul': lambda: w * d, 'div': lambda: w / d, 'rdiv': lambda: d / w}[op]()


def sampled(w, indices, indptr, D):
    """`D[row_ids, idx]` in w's dtype, by torch on the device."""
    row_ids = dev(np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)))
    return D[row_ids, dev(indices).long()].to(w.dtype)


def csr_of(w, indices, indptr, shape, ptr_dtype=None):
    return be.CSR((w, dev(indices), dev(indptr)), shape=shape, indptr_dtype=ptr_dtype or 'auto')


def by_op(M, D, op):
    return {'take': lambda: M.apply2(D, lambda a, b: b), 'mul': lambda: M * D, 'div': lambda: M / D,
            'rdiv': lambda: D / M}[op]()


# ------------------------------------------------------------------------------------------------ tile boundaries
def _lens_summing_to(rng, n_rows, total):
    cuts = np.sort(rng.integers(0, total + 1, n_rows - 1))
    return np.diff(np.concatenate([[0], cuts, [total]]))


STRUCTURES = {
    'tile-1': lambda rng: _lens_summing_to(rng, 37, T - 1),
    'tile': lambda rng: _lens_summing_to(rng, 37, T),
    'tile+1': lambda rng: _lens_summing_to(rng, 37, T + 1),
    'a row of more than two tiles': lambda rng: np.array([3, 2 * T + 5, 2]),
    'runs of empty rows': lambda rng: np.array([0] * (T + 3) + [5, 7] + [0] * (T + 3) + [4] + [0] * (T + 3)),
}


@pytest.mark.parametrize('ptr_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('case', sorted(STRUCTURES))
def test_tile_boundaries(case, ptr_dtype):
    rng = np.random.default_rng(sorted(STRUCTURES).index(case))
    lens = STRUCTURES[case](rng)
    n_cols = 19
    indices, indptr = make_csr(rng, lens, n_cols, ptr_dtype)
    w = draw(rng, len(indices), torch.float32)
    D = draw(rng, (len(lens), n_cols), torch.float32)
    M = csr_of(w, indices, indptr, (len(lens), n_cols), torch.int64 if ptr_dtype == np.int64 else torch.int32)
    assert M.indptr.dtype == (torch.int64 if ptr_dtype == np.int64 else torch.int32)
    d = sampled(w, indices, indptr, D)
    for op in ('take', 'mul'):
        assert_bits(by_op(M, D, op).data, torch_op(op, w, d))


@pytest.fixture(scope='module')
def past_the_grid():
    """grid_cap + 2 tiles and a partial one, 64 rows of one length over a 64 x 4096 operand; the expected product once."""
    rng = np.random.default_rng(7)
    n_rows, n_cols = 64, 4096
    k = ((CONSTS['grid_cap'] + 2) * T + 64) // n_rows
    assert (n_rows * k) % T == 64 and n_rows * k > (CONSTS['grid_cap'] + 2) * T
    indices = dev(rng.integers(0, n_cols, n_rows * k).astype(np.int32))
    w = dev(rng.integers(1, 9, n_rows * k).astype(np.float32))
    D = dev(rng.integers(1, 9, (n_rows, n_cols)).astype(np.float32))
    row_ids = torch.arange(n_rows, device='cuda').repeat_interleave(k)
    want = w * D[row_ids, indices.long()]
    return n_rows, n_cols, k, indices, w, D, want


@pytest.mark.parametrize('rows', ['int32', 'int64', 'fixed'])
def test_past_the_grid_cap(past_the_grid, rows):
    n_rows, n_cols, k, indices, w, D, want = past_the_grid
    if rows == 'fixed':
        M = be.FixedNumPerPre((w.reshape(n_rows, k), indices.reshape(n_rows, k)), shape=(n_rows, n_cols), check_indices=False)
        got = (M * D).data.reshape(-1)
    else:
        dt = torch.int32 if rows == 'int32' else torch.int64
        indptr = (torch.arange(n_rows + 1, device='cuda') * k).to(dt)
        M = be.CSR((w, indices, indptr), shape=(n_rows, n_cols), indptr_dtype=dt, check_structure=False)
        got = (M * D).data
    assert_bits(got, want)


# ------------------------------------------------------------------------------------------------ operands
@pytest.fixture(scope='module')
def pattern():
    """67 x 93, rows of 0 to 80 entries (more than one tile in all), unsorted with duplicates."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 81, 67)
    lens[5] = 0
    indices, indptr = make_csr(rng, lens, 93)
    assert len(indices) > T
    return indices, indptr, (67, 93)


@pytest.mark.parametrize('op', ['take', 'mul', 'div', 'rdiv'])
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_every_dtype_and_op_exact_on_powers_of_two(pattern, dtype, op):
    indices, indptr, shape = pattern
    rng = np.random.default_rng(3)
    w, D = draw_pow2(rng, len(indices), dtype), draw_pow2(rng, shape, dtype)
    M = csr_of(w, indices, indptr, shape)
    assert_bits(by_op(M, D, op).data, torch_op(op, w, sampled(w, indices, indptr, D)))


@pytest.mark.parametrize('op', ['take', 'mul', 'div', 'rdiv'])
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_every_dtype_and_op_on_real_values(pattern, dtype, op):
    """One correctly rounded operation and one rounding on both sides: bit for bit."""
    indices, indptr, shape = pattern
    rng = np.random.default_rng(4)
    w, D = draw(rng, len(indices), dtype), draw(rng, shape, dtype)
    M = csr_of(w, indices, indptr, shape)
    got, want = by_op(M, D, op).data, torch_op(op, w, sampled(w, indices, indptr, D))
    differ = int((torch.from_numpy(bits(got)) != torch.from_numpy(bits(want))).sum())
    print(f"{op} {dtype}: {differ} of {got.numel()} entries differ from torch in their bits")
    assert_bits(got, want)


@pytest.mark.parametrize('mask_dtype', [torch.uint8, torch.bool], ids=str)
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_mask_operands_are_read_as_bytes(pattern, dtype, mask_dtype):
    indices, indptr, shape = pattern
    rng = np.random.default_rng(5)
    w = draw(rng, len(indices), dtype)
    D = dev(rng.integers(0, 2 if mask_dtype == torch.bool else 200, shape)).to(mask_dtype)
    M = csr_of(w, indices, indptr, shape)
    d = sampled(w, indices, indptr, D)
    assert_bits((M * D).data, w * d)
    assert_bits((D * M).data, w * d)
    assert_bits(by_op(M, D, 'take').data, d)


def test_strided_views_are_read_in_place(pattern):
    indices, indptr, shape = pattern
    rng = np.random.default_rng(6)
    w = draw(rng, len(indices), torch.float32)
    M = csr_of(w, indices, indptr, shape)
    base = draw(rng, shape, torch.float32)
    wide = torch.zeros((shape[0], shape[1] + 7), device='cuda')
    wide[:, :shape[1]] = base
    flat = torch.zeros(shape[0] * shape[1] + 1, device='cuda')
    flat[1:] = base.reshape(-1)
    views = {'transposed': base.T.contiguous().T, 'row stride > width': wide[:, :shape[1]],
             'offset by one element': flat[1:].view(shape)}
    assert not views['transposed'].is_contiguous() and not views['row stride > width'].is_contiguous()
    assert views['offset by one element'].data_ptr() % 16 == 4
    want = w * sampled(w, indices, indptr, base)
    for name, D in views.items():
        assert torch.equal(D, base), name
        assert_bits((M * D).data, want)


def test_another_operand_dtype_is_converted_once(pattern):
    indices, indptr, shape = pattern
    rng = np.random.default_rng(8)
    w = draw(rng, len(indices), torch.float16)
    D = draw(rng, shape, torch.float32)
    assert_bits((csr_of(w, indices, indptr, shape) * D).data, w * sampled(w, indices, indptr, D.to(torch.float16)))


def test_a_shared_weight_becomes_per_entry(pattern):
    indices, indptr, shape = pattern
    rng = np.random.default_rng(9)
    D = draw(rng, shape, torch.float32)
    w = dev(np.array([1.5], np.float32))
    M = csr_of(w, indices, indptr, shape)
    d = sampled(w, indices, indptr, D)
    for op in ('mul', 'div', 'rdiv', 'take'):
        r = by_op(M, D, op)
        assert tuple(r.data.shape) == (len(indices),)
        assert_bits(r.data, torch_op(op, w.expand(len(indices)), d))
    assert tuple((M * 2).data.shape) == (1,) and float((M * 2).data) == 3.0          # a scalar keeps it shared


# ------------------------------------------------------------------------------------------------ the four containers
def int_matrix(rng, shape, density=0.3):
    """+-{1, 2, 4} on a random pattern with one empty row and one empty column (host array, f32)."""
    mat = rng.choice([1.0, 2.0, 4.0], shape) * rng.choice([-1.0, 1.0], shape) * (rng.random(shape) < density)
    mat[3, :] = 0
    mat[:, 4] = 0
    return mat.astype(np.float32)


def build(cls, mat, tensor=True):
    src = dev(mat) if tensor else mat
    if cls in (be.CSR, be.CSC):
        return cls.fromdense(src)
    view = mat.T if cls is be.FixedNumPerPost else mat
    return cls.fromdense(src, num_conn=int((view != 0).sum(axis=1).max()))


def coords(M):
    """(row, column) of every stored entry in the matrix M stands for, flat, in storage order (device int64)."""
    idx = M.indices.reshape(-1).long()
    if hasattr(M, 'indptr'):
        primary = torch.arange(M.indptr.numel() - 1, device='cuda').repeat_interleave(torch.diff(M.indptr.long()))
    else:
        primary = torch.arange(M.indices.shape[0], device='cuda').repeat_interleave(M.indices.shape[1])
    return (idx, primary) if M._stored_transposed else (primary, idx)


@pytest.fixture(scope='module')
def truth():
    rng = np.random.default_rng(21)
    mat = int_matrix(rng, SHAPE)
    D = (rng.choice([1.0, 2.0, 4.0], SHAPE) * rng.choice([-1.0, 1.0], SHAPE)).astype(np.float32)
    return mat, D


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_swapped_strides_against_the_dense_truth(cls, truth):
    mat, D = truth
    M = build(cls, mat)
    np.testing.assert_array_equal((M * dev(D)).todense(), mat * D)
    np.testing.assert_array_equal((dev(D) * M).todense(), mat * D)
    np.testing.assert_array_equal((M / dev(D)).todense(), mat / D)
    r, c = coords(M)
    assert_bits((dev(D) / M).data.reshape(-1), dev(D)[r, c] / M.data.reshape(-1))
    assert_bits(M.apply2(dev(D), torch.maximum).data.reshape(-1), torch.maximum(M.data.reshape(-1), dev(D)[r, c]))
    assert_bits(M.apply2(dev(D), torch.maximum, reverse=True).data.reshape(-1), torch.maximum(dev(D)[r, c], M.data.reshape(-1)))


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_unary_and_scalar_operators(cls, truth):
    mat, _ = truth
    M = build(cls, mat)
    for got, want in ((-M, -mat), (abs(M), abs(mat)), (+M, mat), (M * 2, mat * 2), (2 * M, 2 * mat), (M / 2, mat / 2),
                      (np.float32(2) * M, 2 * mat), (np.array([2.0], np.float32) * M, 2 * mat), (M * dev(np.float32(2)), mat * 2),
                      (M.apply(torch.square), mat ** 2), (M.apply2(3, operator.mul), mat * 3),
                      (M.apply2(3, operator.mul, reverse=True), mat * 3)):
        assert type(got) is cls and got.shape == M.shape
        assert got.indices is M.indices and getattr(got, 'indptr', None) is getattr(M, 'indptr', None)
        assert got.data.dtype == M.data.dtype and got.data.shape == M.data.shape
        np.testing.assert_array_equal(got.todense(), want)
    # fn(0, x) != 0 and the result stays sparse: the rule is "stored entries only"
    assert_bits((2 / M).data, 2 / M.data)
    assert_bits(M.apply2(2, lambda a, b: a + b).data, M.data + 2)
    assert_bits(M.apply2(2, lambda a, b: a - b, reverse=True).data, 2 - M.data)
    assert M.apply(lambda d: d.double()).data.dtype == torch.float64                  # the dtype may change ...
    with pytest.raises(ValueError, match='shape'):
        M.apply(lambda d: d.reshape(-1)[:3])                                          # ... the shape may not


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_add_and_sub_give_a_dense_result(cls, truth):
    mat, X = truth
    M = build(cls, mat)
    for got, want in ((M + 2, mat + 2), (2 + M, 2 + mat), (M - 2, mat - 2), (2 - M, 2 - mat), (M + dev(X), mat + X),
                      (dev(X) - M, X - mat), (M - dev(X[0]), mat - X[0]), (M + dev(X[:, :1]), mat + X[:, :1])):
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match='broadcast'):
        M + dev(X[:, :7])
    with pytest.raises(ValueError, match='broadcast'):
        dev(X[:5]) - M


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_numpy_in_numpy_out(cls, truth):
    mat, X = truth
    M = build(cls, mat, tensor=False)
    assert M._numpy_result and (M * 2)._numpy_result and (M * X)._numpy_result and (-M)._numpy_result
    np.testing.assert_array_equal((M * X).todense(), mat * X)
    np.testing.assert_array_equal((X * M).todense(), mat * X)
    got = M + X
    assert isinstance(got, np.ndarray)
    np.testing.assert_array_equal(got, mat + X)
    assert isinstance(M - 1.5, np.ndarray) and isinstance(X - M, np.ndarray)
    assert isinstance(M + dev(X), torch.Tensor)                                       # a torch operand gives torch


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_same_structure_sparse_operand(cls, truth):
    mat, _ = truth
    M = build(cls, mat)
    N = M.apply(lambda d: d * 2 + 1)
    for fn in (operator.mul, operator.truediv, operator.add, operator.sub):
        got = fn(M, N)
        assert type(got) is cls and got.indices is M.indices
        assert_bits(got.data, fn(M.data, N.data))
        assert_bits(M.apply2(N, fn, reverse=True).data, fn(N.data, M.data))
    other = build(cls, mat)                                                           # equal arrays, other objects
    for fn in (operator.mul, operator.add):
        with pytest.raises(NotImplementedError, match='sparse'):
            fn(M, other)
    with pytest.raises(NotImplementedError, match='sparse'):
        M * build(be.CSC if cls is be.CSR else be.CSR, mat)
    with pytest.raises(NotImplementedError, match='sparse'):
        M * be.Dense(dev(mat))


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_refusals(cls, truth):
    mat, D = truth
    M = build(cls, mat)
    for bad in (dev(D.T.copy()), dev(D[:, :5]), dev(D[0]), dev(D[:, 0]), D[0], dev(D)[None]):
        with pytest.raises(NotImplementedError, match='dt2t'):
            M * bad
        with pytest.raises(NotImplementedError, match='dt2t'):
            bad / M
    with pytest.raises(be.UnsupportedOperationError, match='requires grad'):
        M * dev(D).requires_grad_()
    with torch.no_grad():
        assert (M * dev(D).requires_grad_()).data.requires_grad is False


@pytest.mark.parametrize('cls', [be.CSR, be.CSC], ids=lambda c: c.__name__)
def test_only_structure_buffers_travel(cls, truth):
    mat, D = truth
    M = build(cls, mat)
    M.prepare(mirror=True)
    M.diag_add(dev(np.ones(min(SHAPE), np.float32)))
    assert {'scatter_plan', 'mirror', 'diag_positions'} <= set(M.buffers)
    plan = M.buffers['diag_positions']
    assert isinstance(plan, DiagPlan)
    for r in (M * 2, -M, M * dev(D), M.apply(torch.abs), M * M):
        assert set(r.buffers) == {'diag_positions'} and r.buffers['diag_positions'] is plan
        assert r.diag_add(dev(np.ones(min(SHAPE), np.float32))).indices is plan.new_indices


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_the_product_of_a_masked_matrix(cls, truth):
    mat, D = truth
    M = build(cls, mat)
    rng = np.random.default_rng(31)
    expected = build(cls, mat * D)
    for n, left in ((SHAPE[0], True), (SHAPE[1], False)):
        spk = be.BinaryArray(dev(rng.random(n) < 0.3))
        got = spk @ (M * dev(D)) if left else (M * dev(D)) @ spk
        want = spk @ expected if left else expected @ spk
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())


# ------------------------------------------------------------------------------------------------ autograd
def _with_grad(cls, mat):
    M = build(cls, mat)
    M.data.requires_grad_()
    r, c = coords(M)
    wp = M.data.detach().clone().reshape(-1).requires_grad_()
    Wd = torch.zeros(SHAPE, device='cuda').index_put((r, c), wp, accumulate=True)
    return M, wp, Wd, (r, c)


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_backward_through_the_dense_operand_product(cls, truth):
    mat, Dh = truth
    rng = np.random.default_rng(41)
    D, G = dev(Dh), dev(rng.integers(-3, 4, SHAPE).astype(np.float32))
    for fn in (lambda m: m * D, lambda m: D * m, lambda m: m / D):
        M, wp, Wd, _ = _with_grad(cls, mat)
        (fn(M)[:] * G).sum().backward()
        (fn(Wd) * G).sum().backward()
        assert_bits(M.data.grad.reshape(-1), wp.grad)


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_backward_through_the_reflected_division(cls, truth):
    """`D / M` keeps the stored entries only, so the truth is per entry: d(D[r, c] / w) = -D[r, c] / w^2.  The zero-weight
    padding of the fixed-number containers is set to 1 first (a quotient by 0 has no gradient to compare)."""
    mat, Dh = truth
    rng = np.random.default_rng(42)
    M = build(cls, mat)
    M = M.with_data(torch.where(M.data == 0, torch.ones_like(M.data), M.data))
    M.data.requires_grad_()
    r, c = coords(M)
    wp = M.data.detach().clone().reshape(-1).requires_grad_()
    g = dev(rng.integers(-3, 4, M.indices.numel()).astype(np.float32))
    ((dev(Dh) / M).data.reshape(-1) * g).sum().backward()
    ((dev(Dh)[r, c] / wp) * g).sum().backward()
    assert_bits(M.data.grad.reshape(-1), wp.grad)


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_backward_through_add_and_a_scaled_product(cls, truth):
    mat, Xh = truth
    rng = np.random.default_rng(43)
    G = dev(rng.integers(-3, 4, SHAPE).astype(np.float32))
    M, wp, Wd, _ = _with_grad(cls, mat)
    ((M + dev(Xh)) * G).sum().backward()
    ((Wd + dev(Xh)) * G).sum().backward()
    assert_bits(M.data.grad.reshape(-1), wp.grad)
    M, wp, Wd, _ = _with_grad(cls, mat)
    spk = dev((rng.random(SHAPE[0]) < 0.4))
    gv = dev(rng.integers(-3, 4, SHAPE[1]).astype(np.float32))
    ((be.BinaryArray(spk) @ (M * 2.0)) * gv).sum().backward()
    ((spk.float() @ (Wd * 2.0)) * gv).sum().backward()
    assert_bits(M.data.grad.reshape(-1), wp.grad)


def test_backward_into_a_shared_weight(truth):
    mat, Dh = truth
    M = build(be.CSR, mat)
    M = be.CSR((dev(np.array([2.0], np.float32)).requires_grad_(), M.indices, M.indptr), shape=SHAPE)
    r, c = coords(M)
    g = dev(np.random.default_rng(44).integers(-3, 4, M.nse).astype(np.float32))
    ((M * dev(Dh)).data * g).sum().backward()
    assert float(M.data.grad) == float((dev(Dh)[r, c] * g).sum())


def test_no_node_without_grad(truth):
    mat, Dh = truth
    M = build(be.CSR, mat)
    for r in (M * dev(Dh), M / dev(Dh), dev(Dh) / M, M * 2):
        assert r.data.grad_fn is None and not r.data.requires_grad
    assert (M + dev(Dh)).grad_fn is None
    M.data.requires_grad_()
    with torch.no_grad():
        assert (M * dev(Dh)).data.grad_fn is None and (M + 1.0).grad_fn is None
    assert (M * dev(Dh)).data.grad_fn is not None and (M * 2).data.grad_fn is not None and (M + 1.0).grad_fn is not None


# ------------------------------------------------------------------------------------------------ Dense and JITC
def test_dense_operators(truth):
    mat, X = truth
    M = be.Dense(dev(mat))
    for got, want in ((-M, -mat), (abs(M), abs(mat)), (M * 2, mat * 2), (2 * M, 2 * mat), (M / 2, mat / 2), (M + 1, mat + 1),
                      (1 - M, 1 - mat), (M * dev(X), mat * X), (X[0] + M, X[0] + mat), (M - be.Dense(dev(X)), mat - X),
                      (np.float32(2) * M, 2 * mat), (M.apply(torch.square), mat ** 2),
                      (M.apply2(dev(X), torch.maximum), np.maximum(mat, X))):
        assert type(got) is be.Dense and got.shape == SHAPE
        np.testing.assert_array_equal(got.todense().cpu().numpy(), want)
    with pytest.raises(ValueError):
        M * dev(X[:, :5])
    with pytest.raises(ValueError):
        M * dev(X)[None]
    with pytest.raises(ValueError):
        M + be.Dense(dev(X.T.copy()))
    with pytest.raises(NotImplementedError):
        M * build(be.CSR, mat)


def test_dense_diag_add(truth):
    mat, _ = truth
    d = np.arange(1, min(SHAPE) + 1, dtype=np.float32)
    for m in (mat, mat.T.copy()):
        want = m.copy()
        want[np.arange(len(d)), np.arange(len(d))] += d
        M = be.Dense(dev(m))
        np.testing.assert_array_equal(M.diag_add(dev(d)).todense().cpu().numpy(), want)
        np.testing.assert_array_equal(M.todense().cpu().numpy(), m)
        with pytest.raises(ValueError):
            M.diag_add(dev(d[:-1]))


@pytest.mark.parametrize('cls', [be.JITCScalarR, be.JITCScalarC, be.JITCUniformR, be.JITCUniformC], ids=lambda c: c.__name__)
def test_jitc_scaling_equals_the_dense_scaling(cls):
    params = (1.5, 0.1, 42) if 'Scalar' in cls.__name__ else (0.5, 1.5, 0.1, 42)
    M = cls(params, shape=(40, 60))
    base = M.mv.todense()
    assert np.count_nonzero(base) > 100
    np.testing.assert_array_equal((M * 2).mv.todense(), 2 * base)
    np.testing.assert_array_equal((2 * M).mv.todense(), 2 * base)
    np.testing.assert_array_equal((M / 2).mv.todense(), base / 2)
    np.testing.assert_array_equal((M + 0.5).mv.todense(), np.where(base != 0, base + np.float32(0.5), 0))


@pytest.mark.parametrize('cls', [be.JITCNormalR, be.JITCNormalC], ids=lambda c: c.__name__)
def test_jitc_normal_scales_loc_alone(cls):
    M = cls((0.5, 0.25, 0.1, 42), shape=(40, 60))
    base = M.mv.todense()
    twice = (M * 2).mv.todense()
    np.testing.assert_array_equal(twice != 0, base != 0)
    np.testing.assert_allclose(twice, np.where(base != 0, base + 0.5, 0), rtol=0, atol=1e-6)          # loc + 0.5, scale as it was
    assert not np.allclose(twice, 2 * base)
    np.testing.assert_allclose((M + 1).mv.todense(), np.where(base != 0, base + 1, 0), rtol=0, atol=1e-6)
