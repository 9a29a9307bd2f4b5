"""``solve`` on the device (csrc/be_solve.hip through ``CSR.solve`` / ``CSC.solve`` / ``Dense.solve`` / ``csr_solve``).

Expectations come from ``numpy.linalg.solve`` in f64 on the densified matrix (for the one size whose dense matrix cannot be
formed: on its dense diagonal blocks).  Two bounds, derived in tests/solve_cases.py and held to the reference itself by
tests/test_solve_cpu.py — none of them tuned:

    residual:  |b - A x|_2   <= rtol |b|_2 + gamma | |A| |x| |_2,      gamma = (longest row + 2) eps(dtype)
    error:     |x - x*|_inf  <= (the same right-hand side) / min_i(|a_ii| - sum_{j != i} |a_ij|)          (Varah)

Sizes are the smallest at which a loop bound of the kernels is crossed; every case prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _solve
import solve_cases as SC

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ['f32', 'f64']
RTOL = {np.float32: 1e-5, np.float64: 1e-10}
#: one element past what the capped vector grid covers in one stride: kSolveVecGridCap workgroups x 256 threads x 4 elements
PAST_ONE_STRIDE = 1024 * 256 * 4 + 3


def csr_of(case, numpy_in=False):
    if numpy_in:
        return be.CSR((case.data, case.indices, case.indptr), shape=(case.n, case.n))
    return be.CSR((torch.from_numpy(case.data), torch.from_numpy(case.indices), torch.from_numpy(case.indptr)),
                  shape=(case.n, case.n))


def solve_and_check(case, x_star=None, **kw):
    rtol = kw.get('rtol') or RTOL[case.dtype.type]
    x, info = csr_of(case).solve(torch.from_numpy(case.b), return_info=True, **kw)
    assert isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.from_numpy(case.b).dtype and tuple(x.shape) == (case.n,)
    print(case.name, info)
    assert info['converged'] and info['residual'] <= rtol
    if x_star is None:
        x_star = np.linalg.solve(case.A, case.b.astype(np.float64))
    SC.check_solution(case, x.cpu().numpy(), x_star, rtol)
    return x, info


# ------------------------------------------------------------------------------------------------ sizes and row shapes
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 257])
def test_sizes_around_the_wave_and_the_workgroup(n, dtype):
    solve_and_check(SC.dominant_case(n, 3, 100 + n, dtype, name=f'n{n}'))


@functools.lru_cache(maxsize=None)
def past_one_stride_case(dtype):
    """Built once per dtype and left unchanged: the case and its exact f64 solution."""
    case = SC.block_case(PAST_ONE_STRIDE, 4, 5, dtype, name='past one stride')
    return case, SC.block_solve(case, 4)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_one_size_past_what_the_capped_grids_cover_in_one_stride(dtype):
    """Both capped grids take a second stride here: the vector kernels (1024 x 256 x 4 elements) and the matrix passes (2048
    workgroups x 256 rows at four lanes per row).  Dense 4 x 4 diagonal blocks keep an exact f64 reference."""
    case, x_star = past_one_stride_case(dtype)
    solve_and_check(case, x_star)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n,per_row,lanes', [(65, 3, 4), (65, 23, 4), (65, 24, 16), (257, 159, 16), (257, 160, 64)])
def test_row_lengths_that_select_each_lanes_per_row_class(n, per_row, lanes, dtype):
    case = SC.dominant_case(n, per_row, 7, dtype, name=f'{lanes} lanes per row')
    avg = case.data.size // n                                  # (per_row + 1: the diagonal)
    assert (4 if avg <= 24 else 16 if avg <= 160 else 64) == lanes
    solve_and_check(case)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_one_full_row_among_short_ones(dtype):
    counts = np.full(257, 3)
    counts[100] = 256
    case = SC.dominant_case(257, counts, 7, dtype, name='full row')
    assert case.longest_row == 257
    solve_and_check(case)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_rows_with_only_the_diagonal_among_others(dtype):
    counts = np.where(np.arange(130) % 3 == 0, 0, 4)
    solve_and_check(SC.dominant_case(130, counts, 8, dtype, name='diagonal-only rows'))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('opts', [dict(shuffle=True), dict(dup_offdiag=True), dict(dup_diag=True),
                                  dict(shuffle=True, dup_offdiag=True, dup_diag=True)],
                         ids=['unsorted', 'duplicated off-diagonals', 'diagonal stored twice', 'all three'])
def test_unsorted_rows_and_duplicates(opts, dtype):
    solve_and_check(SC.dominant_case(65, 5, 9, dtype, name=str(sorted(opts)), **opts))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_int64_indptr_gives_the_same_bytes(dtype):
    case = SC.dominant_case(257, 6, 10, dtype, name='int32 indptr')
    wide = SC.Case(case.data, case.indices, case.indptr.astype(np.int64), case.b, case.n, 'int64 indptr')
    x32, _ = solve_and_check(case)
    x64, _ = solve_and_check(wide)
    assert torch.equal(x32, x64)


# ------------------------------------------------------------------------------------------------ the diagonal matrix
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n', [1, 65, 1027])
def test_diagonal_matrix_is_one_division(n, dtype):
    """``x == b / d`` to one rounding — the correctly rounded quotient, bit for bit — in at most one iteration."""
    case = SC.dominant_case(n, 0, 11, dtype, name='diagonal')
    x, info = csr_of(case).solve(torch.from_numpy(case.b), return_info=True)
    print(info)
    assert info['converged'] and info['iterations'] <= 1
    np.testing.assert_array_equal(x.cpu().numpy(), case.b / case.data)


# ------------------------------------------------------------------------------------------------ a missing diagonal
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_row_without_a_stored_diagonal_does_what_the_recurrence_does(dtype):
    """Row 5 of an otherwise dominant matrix loses its diagonal entry: the preconditioner falls back to 1 there.  Whether the
    solve converges is what the f64 CPU run of the same recurrence says (tests/solve_cases.py), not an assumption."""
    full = SC.dominant_case(33, 4, 12, dtype)
    keep = ~((full.rows == 5) & (full.indices == 5))
    indptr = np.zeros(34, dtype=np.int32)
    np.cumsum(np.bincount(full.rows[keep], minlength=33), out=indptr[1:])
    case = SC.Case(full.data[keep], full.indices[keep], indptr, full.b, 33, 'no diagonal in row 5')
    assert case.A[5, 5] == 0.0 and np.count_nonzero(case.A[5]) == 4
    rtol = RTOL[dtype]
    _, expect = SC.bicgstab_reference(case.A, case.b, rtol)
    print('reference recurrence:', expect)
    if expect['converged']:
        x, info = csr_of(case).solve(torch.from_numpy(case.b), return_info=True)
        print('device:', info)
        assert info['converged']
        x64 = x.cpu().numpy().astype(np.float64)
        res = np.linalg.norm(case.b.astype(np.float64) - case.A @ x64)
        assert res <= SC.residual_bound(case, x64, rtol)
    else:
        with pytest.raises(be.MathError):
            csr_of(case).solve(torch.from_numpy(case.b))


# ------------------------------------------------------------------------------------------------ operands
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_shared_weight_is_expanded(dtype):
    """One shared weight w: the diagonal is stored five times beside two off-diagonal entries per row and per column, so
    A = w (5 I + P1 + P7) is dominant by row and by column and the two bounds apply."""
    n = 40
    rows = np.arange(n)
    indices = np.stack([rows] * 5 + [(rows + 1) % n, (rows + 7) % n], axis=1).reshape(-1).astype(np.int32)
    indptr = (np.arange(n + 1) * 7).astype(np.int32)
    b = np.random.default_rng(3).standard_normal(n).astype(dtype)
    case = SC.Case(np.full(7 * n, -1.5, dtype=dtype), indices, indptr, b, n, 'shared weight')
    assert SC.row_gap(case) == 4.5 and SC.col_gap(case) == 4.5
    x, info = be.CSR((np.array([-1.5], dtype=dtype), indices, indptr), shape=(n, n)).solve(b, return_info=True)
    print(info)
    assert isinstance(x, np.ndarray) and x.dtype == dtype and info['converged'] and info['iterations'] >= 1
    SC.check_solution(case, x, np.linalg.solve(case.A, b.astype(np.float64)), RTOL[dtype])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_numpy_in_numpy_out_and_b_is_converted(dtype):
    case = SC.dominant_case(65, 4, 13, dtype, name='numpy')
    x_star = np.linalg.solve(case.A, case.b.astype(np.float64))
    x = csr_of(case, numpy_in=True).solve(case.b)
    assert isinstance(x, np.ndarray) and x.dtype == dtype
    SC.check_solution(case, x, x_star, RTOL[dtype])
    xt = csr_of(case).solve(torch.from_numpy(case.b))
    assert isinstance(xt, torch.Tensor) and np.array_equal(xt.cpu().numpy(), x)
    other = np.float64 if dtype == np.float32 else np.float32
    xo = csr_of(case, numpy_in=True).solve(case.b.astype(other))                     # b in the other dtype: converted
    assert xo.dtype == dtype
    xf = be.csr_solve(case.data, case.indices, case.indptr, case.b)                   # the functional form, shape implied
    assert isinstance(xf, np.ndarray) and np.array_equal(xf, x)
    xf2 = be.csr_solve(torch.from_numpy(case.data), case.indices, case.indptr, case.b, 1e-6, 1, shape=(65, 65))
    assert isinstance(xf2, torch.Tensor) and np.array_equal(xf2.cpu().numpy(), x)
    assert be.csr_solve_p.call(torch.from_numpy(case.data).cuda(), torch.from_numpy(case.indices).cuda(),
                               torch.from_numpy(case.indptr).cuda(), torch.from_numpy(case.b).cuda(), shape=(65, 65))[0][1]['converged']


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_warm_start(dtype):
    case = SC.dominant_case(257, 6, 14, dtype, name='warm start')
    x_star = np.linalg.solve(case.A, case.b.astype(np.float64))
    _, cold = solve_and_check(case, x_star)
    near = (x_star * (1 + 1e-4)).astype(dtype)
    x, warm = solve_and_check(case, x_star, x0=torch.from_numpy(near))
    assert 0 < warm['iterations'] < cold['iterations']
    _, exact = solve_and_check(case, x_star, x0=x)                                   # already inside rtol: nothing to iterate
    assert exact['iterations'] == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_zero_right_hand_side(dtype):
    case = SC.dominant_case(65, 4, 15, dtype)
    x, info = csr_of(case).solve(torch.zeros(65, dtype=torch.from_numpy(case.b).dtype), return_info=True)
    assert torch.count_nonzero(x) == 0 and x.dtype == torch.from_numpy(case.b).dtype
    assert info == {'iterations': 0, 'residual': 0.0, 'restarts': 0, 'converged': True}


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_two_calls_return_identical_bytes(dtype):
    case = SC.dominant_case(4099, 9, 16, dtype, name='twice')
    M, b = csr_of(case), torch.from_numpy(case.b).cuda()
    x1, i1 = M.solve(b, return_info=True)
    x2, i2 = M.solve(b, return_info=True)
    assert i1 == i2 and i1['converged'] and i1['iterations'] > 1
    assert torch.equal(x1.view(torch.uint8), x2.view(torch.uint8))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_two_calls_return_identical_bytes_on_full_grids(dtype):
    """The same at the size where both grids are at their caps (1024 and 2048 workgroups): every consumer sums 1024 or 2048
    partials, and the status gating spans every workgroup the kernels can have."""
    case, _ = past_one_stride_case(dtype)
    M, b = csr_of(case), torch.from_numpy(case.b).cuda()
    x1, i1 = M.solve(b, return_info=True)
    x2, i2 = M.solve(b, return_info=True)
    print(i1)
    assert i1 == i2 and i1['converged'] and i1['iterations'] > 1
    assert torch.equal(x1.view(torch.uint8), x2.view(torch.uint8))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_half_step_exit_on_a_full_grid_updates_every_element(dtype):
    """Convergence at the half step, ``|s|^2 <= rtol^2 |b|^2``, on 1024 workgroups: every one of them owes ``x += alpha y``
    whichever of them is first to report the exit.

    Row ``i`` stores ``d_i`` and the pair ``+w_i, -w_i`` at column ``i + 1`` with ``|w_i| <= |d_i| / 4``: not a diagonal matrix
    to the setup pass (it has nonzero off-diagonal entries), so the recurrence runs, and ``A = D`` exactly.  With ``x0 = 0``:
    ``y = fl(b / d)``, ``v = A y`` is ``b`` to a few roundings per row — ``|v_i - b_i| <= 4 eps (|b_i| + 2 |w_i y_(i+1)|)`` —
    so ``alpha = 1 + O(eps)`` and ``|s_i| = |b_i - alpha v_i|`` stays below ``~20 eps max|b|``: ``|s|^2 <= 400 eps^2 |b|^2``,
    far under ``rtol^2 |b|^2`` (6e-12 against 1e-10 in f32, 2e-29 against 1e-20 in f64).  The first iteration therefore leaves
    at the half step, with no restart; the solution is ``b / d`` and is held to the module's two bounds, and two calls
    return the same bytes."""
    n = PAST_ONE_STRIDE
    rng = np.random.default_rng(23)
    d = (rng.uniform(1.0, 2.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(dtype)
    w = rng.uniform(0.1, 0.25, n).astype(dtype)
    b = rng.uniform(0.5, 1.0, n).astype(dtype)
    i = np.arange(n)
    nxt = (i + 1) % n
    case = SC.Case(np.stack([d, w, -w], axis=1).reshape(-1), np.stack([i, nxt, nxt], axis=1).reshape(-1).astype(np.int32),
                   (3 * np.arange(n + 1)).astype(np.int32), b, n, 'half step')
    assert SC.row_gap(case) >= 0.5 and SC.col_gap(case) >= 0.5
    M, bt = csr_of(case), torch.from_numpy(b).cuda()
    x1, i1 = M.solve(bt, return_info=True)
    x2, i2 = M.solve(bt, return_info=True)
    print(i1)
    assert i1 == i2 and i1['converged'] and i1['iterations'] == 1 and i1['restarts'] == 0
    assert torch.equal(x1.view(torch.uint8), x2.view(torch.uint8))
    SC.check_solution(case, x1.cpu().numpy(), b.astype(np.float64) / d.astype(np.float64), RTOL[dtype])


# ------------------------------------------------------------------------------------------------ CSC and Dense
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_csc_solves_with_the_matrix_not_its_transpose(dtype):
    case = SC.dominant_case(65, 5, 17, dtype, name='csc')
    A = case.A
    assert np.abs(A - A.T).max() > 0.1                                               # non-symmetric
    x_star = np.linalg.solve(A, case.b.astype(np.float64))
    x_t = np.linalg.solve(A.T, case.b.astype(np.float64))
    csr = csr_of(case)
    csc = csr.tocsc()
    assert isinstance(csc, be.CSC) and csc.shape == (65, 65)
    xc = csc.solve(torch.from_numpy(case.b))
    xr = csr.solve(torch.from_numpy(case.b))
    rtol = RTOL[dtype]
    _, bound, _, err_bound = SC.check_solution(case, xc.cpu().numpy(), x_star, rtol)
    SC.check_solution(case, xr.cpu().numpy(), x_star, rtol)
    assert np.max(np.abs(xc.cpu().numpy().astype(np.float64) - xr.cpu().numpy())) <= 2 * err_bound
    assert np.max(np.abs(xc.cpu().numpy() - x_t)) > 100 * err_bound                  # not the transposed system's solution
    # a CSC built directly from column-major arrays
    direct = be.CSC.fromdense(torch.from_numpy(A.astype(dtype)))
    SC.check_solution(case, direct.solve(torch.from_numpy(case.b)).cpu().numpy(), x_star, rtol)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_dense_solve_is_torch_linalg_solve(dtype):
    case = SC.dominant_case(33, 6, 18, dtype)
    Ad = torch.from_numpy(case.A.astype(dtype)).cuda()
    b = torch.from_numpy(case.b).cuda()
    x = be.Dense(Ad).solve(b, 1e-6, 1)
    assert torch.equal(x, torch.linalg.solve(Ad, b))
    xn = be.Dense(case.A.astype(dtype)).solve(case.b)
    assert isinstance(xn, np.ndarray) and np.array_equal(xn, x.cpu().numpy())
    with pytest.raises(AssertionError, match='square'):
        be.Dense(Ad[:, :5].contiguous()).solve(b)
    with pytest.raises(AssertionError, match='right-hand side'):
        be.Dense(Ad).solve(b[:5])
    # the info of a direct solve carries the MEASURED residual: it agrees with the f64 residual of the returned x to the
    # rounding of the device's own residual pass, gamma | |A| |x| |_2 with gamma = (n + 2) eps (tests/solve_cases.py)
    xi, info = be.Dense(Ad).solve(b, return_info=True)
    assert torch.equal(xi, x) and info['iterations'] == 0 and info['restarts'] == 0 and info['converged'] is True
    A64, x64, b64 = Ad.cpu().numpy().astype(np.float64), x.cpu().numpy().astype(np.float64), case.b.astype(np.float64)
    true = np.linalg.norm(b64 - A64 @ x64)
    slack = (33 + 2) * np.finfo(dtype).eps * np.linalg.norm(np.abs(A64) @ np.abs(x64))
    print(f"dense residual {info['residual']:.3e}, f64 {true / np.linalg.norm(b64):.3e}")
    assert abs(info['residual'] * np.linalg.norm(b64) - true) <= slack


# ------------------------------------------------------------------------------------------------ failure paths
def test_zero_row_raises_math_error():
    full = SC.dominant_case(33, 4, 19, np.float32)
    data = full.data.copy()
    data[full.rows == 7] = 0.0
    M = be.CSR((data, full.indices, full.indptr), shape=(33, 33))
    with pytest.raises(be.MathError, match=r'relative residual .* after \d+ iterations'):
        M.solve(full.b, maxiter=200)
    x, info = M.solve(full.b, maxiter=200, return_info=True)
    assert not info['converged'] and isinstance(x, np.ndarray)
    # a structurally empty row as well
    keep = full.rows != 7
    indptr = np.zeros(34, dtype=np.int32)
    np.cumsum(np.bincount(full.rows[keep], minlength=33), out=indptr[1:])
    with pytest.raises(be.MathError):
        be.CSR((full.data[keep], full.indices[keep], indptr), shape=(33, 33)).solve(full.b, maxiter=200)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_maxiter_one_on_a_non_diagonal_matrix(dtype):
    case = SC.dominant_case(65, 5, 20, dtype)
    M = csr_of(case)
    with pytest.raises(be.MathError, match='after 1 iterations'):
        M.solve(torch.from_numpy(case.b), maxiter=1)
    x, info = M.solve(torch.from_numpy(case.b), maxiter=1, return_info=True)
    assert info['converged'] is False and info['iterations'] == 1 and info['residual'] > RTOL[dtype]
    assert torch.all(torch.isfinite(x))


def test_host_side_refusals():
    case = SC.dominant_case(12, 3, 21, np.float32)
    M = csr_of(case)
    b = torch.from_numpy(case.b)
    with pytest.raises(ValueError, match='square'):
        be.CSR((case.data[:3], case.indices[:3], np.array([0, 1, 3], dtype=np.int32)), shape=(2, 12)).solve(b[:2])
    with pytest.raises(ValueError, match='square'):
        be.CSC((case.data[:3], case.indices[:3], np.array([0, 1, 3], dtype=np.int32)), shape=(12, 2)).solve(b)
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match='float32 or float64'):
            M.with_data(M.data.to(bad)).solve(b)
    with pytest.raises(NotImplementedError, match='1-D'):
        M.solve(torch.stack([b, b], dim=1))
    with pytest.raises(AssertionError, match='The number of rows in the matrix must match the size of the right-hand side vector b'):
        M.solve(b[:5])


# ------------------------------------------------------------------------------------------------ gradients
GRAD_RTOL = 1e-13


def _grad_reference(case, g):
    """x = A^-1 b and the gradients of L = g . x by torch autograd through ``torch.linalg.solve`` on the CPU, f64."""
    data = torch.from_numpy(case.data.astype(np.float64)).requires_grad_()
    b = torch.from_numpy(case.b.astype(np.float64)).requires_grad_()
    dense = torch.zeros(case.n, case.n, dtype=torch.float64).index_put((torch.from_numpy(case.rows), torch.from_numpy(
        case.indices.astype(np.int64))), data, accumulate=True)
    x = torch.linalg.solve(dense, b)
    (x * torch.from_numpy(g)).sum().backward()
    return x.detach().numpy(), b.grad.numpy(), data.grad.numpy()


@pytest.mark.parametrize('n', [7, 33])
def test_gradients_against_the_dense_solve(n):
    """With L = g . x: db = A^-T g =: lam comes from one more device solve, on A.T, to the same rtol, so by the module's two
    bounds applied to A.T (whose ROW dominance is A's COLUMN dominance — why the generator is column-dominant too)

        |db - lam|_inf          <= (rtol |g|_2 + gamma | |A.T| |db| |_2) / min_j(|a_jj| - sum_{i != j} |a_ij|)  =: E
        |ddata - ddata*|_inf    <= E * |x|_inf            (ddata[e] = -db[row(e)] x[col(e)])"""
    case = SC.dominant_case(n, 3, 30 + n, np.float64, shuffle=True, name=f'grad n{n}')
    g = np.cos(np.arange(n) * 0.7) + 0.1
    x_ref, db_ref, dw_ref = _grad_reference(case, g)
    data = torch.from_numpy(case.data).cuda().requires_grad_()
    b = torch.from_numpy(case.b).cuda().requires_grad_()
    M = be.CSR((data, torch.from_numpy(case.indices), torch.from_numpy(case.indptr)), shape=(n, n))
    x = M.solve(b, rtol=GRAD_RTOL)
    assert x.grad_fn is not None
    SC.check_solution(case, x.detach().cpu().numpy(), x_ref, GRAD_RTOL)
    (x * torch.from_numpy(g).cuda()).sum().backward()
    db, dw = b.grad.cpu().numpy(), data.grad.cpu().numpy()
    gamma = (case.longest_row + 2) * np.finfo(np.float64).eps
    E = (GRAD_RTOL * np.linalg.norm(g) + gamma * np.linalg.norm(np.abs(case.A.T) @ np.abs(db))) / SC.col_gap(case)
    x_inf = float(np.max(np.abs(x_ref)))
    print(f'db error {np.max(np.abs(db - db_ref)):.3e} <= {E:.3e}; ddata error {np.max(np.abs(dw - dw_ref)):.3e} <= {E * x_inf:.3e}')
    assert dw.shape == case.data.shape and db.shape == (n,)
    assert np.max(np.abs(db - db_ref)) <= E
    assert np.max(np.abs(dw - dw_ref)) <= E * x_inf
    # b alone, data alone
    b2 = torch.from_numpy(case.b).cuda().requires_grad_()
    (csr_of(case).solve(b2, rtol=GRAD_RTOL) * torch.from_numpy(g).cuda()).sum().backward()
    assert torch.equal(b2.grad, b.grad)
    d2 = torch.from_numpy(case.data).cuda().requires_grad_()
    M2 = be.CSR((d2, torch.from_numpy(case.indices), torch.from_numpy(case.indptr)), shape=(n, n))
    (M2.solve(torch.from_numpy(case.b), rtol=GRAD_RTOL) * torch.from_numpy(g).cuda()).sum().backward()
    assert torch.equal(d2.grad, data.grad)
    # CSC: the gradient arrives in the CSC order of data
    csc = csr_of(case).tocsc()
    d3 = csc.data.clone().requires_grad_()
    (csc.with_data(d3).solve(torch.from_numpy(case.b), rtol=GRAD_RTOL) * torch.from_numpy(g).cuda()).sum().backward()
    ref = -np.outer(db_ref, x_ref)
    cols = np.repeat(np.arange(n), np.diff(csc.indptr.cpu().numpy()))
    assert np.max(np.abs(d3.grad.cpu().numpy() - ref[csc.indices.cpu().numpy(), cols])) <= E * x_inf


def test_shared_weight_gradient_is_the_sum():
    """A = w (3 I + P5): the diagonal stored three times beside one off-diagonal entry, w shared.  dL/dw is the sum of the
    per-entry gradients of the twin with per-entry data (to the rounding of a sum of 4 n terms), and equals
    -sum_i lam_i (3 x_i + x_(i+5))."""
    n = 33
    rows = np.arange(n)
    indices = np.stack([rows, rows, rows, (rows + 5) % n], axis=1).reshape(-1).astype(np.int32)
    indptr = (np.arange(n + 1) * 4).astype(np.int32)
    bnp = np.sin(np.arange(n) + 1.0)
    g = torch.from_numpy(np.cos(np.arange(n) * 0.7) + 0.1).cuda()
    w = torch.tensor([1.5], dtype=torch.float64, device='cuda', requires_grad=True)
    full = torch.full((4 * n,), 1.5, dtype=torch.float64, device='cuda', requires_grad=True)
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(rows, 4), indices), 1.5)
    xs = be.CSR((w, indices, indptr), shape=(n, n)).solve(torch.from_numpy(bnp), rtol=GRAD_RTOL)
    xf = be.CSR((full, indices, indptr), shape=(n, n)).solve(torch.from_numpy(bnp), rtol=GRAD_RTOL)
    assert torch.equal(xs, xf)
    (xs * g).sum().backward()
    (xf * g).sum().backward()
    assert w.grad.shape == (1,)
    terms = full.grad.cpu().numpy()
    bound = 4 * n * np.finfo(np.float64).eps * np.abs(terms).sum()            # a sum of 4 n terms in any order
    assert abs(float(w.grad[0]) - terms.sum()) <= bound
    lam = np.linalg.solve(A.T, g.cpu().numpy())
    x_ref = np.linalg.solve(A, bnp)
    exact = -(lam * (3 * x_ref + np.roll(x_ref, -5))).sum()
    # every term is off by at most E |x|_inf (test_gradients_against_the_dense_solve); there are 4 n of them
    gamma = (4 + 2) * np.finfo(np.float64).eps
    E = (GRAD_RTOL * np.linalg.norm(g.cpu().numpy()) + gamma * np.linalg.norm(np.abs(A.T) @ np.abs(lam))) / 3.0
    assert abs(float(w.grad[0]) - exact) <= 4 * n * E * np.max(np.abs(x_ref)) + bound


def test_without_grad_there_is_no_node_and_the_bytes_are_the_same():
    case = SC.dominant_case(33, 3, 40, np.float64)
    data = torch.from_numpy(case.data).cuda()
    idx, ptr, b = torch.from_numpy(case.indices), torch.from_numpy(case.indptr), torch.from_numpy(case.b).cuda()
    plain = be.CSR((data, idx, ptr), shape=(33, 33)).solve(b)
    assert plain.grad_fn is None and not plain.requires_grad
    recorded = be.CSR((data.clone().requires_grad_(), idx, ptr), shape=(33, 33)).solve(b)
    assert recorded.grad_fn is not None
    assert torch.equal(plain.view(torch.uint8), recorded.detach().view(torch.uint8))
    with torch.no_grad():
        quiet = be.CSR((data.clone().requires_grad_(), idx, ptr), shape=(33, 33)).solve(b)
    assert quiet.grad_fn is None and torch.equal(quiet, plain)
