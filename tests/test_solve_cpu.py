"""``solve`` without a device: the ABI bookkeeping of csrc/be_solve.hip, the public surface, the refusals that need no kernel, the
constants tests/test_solve_gpu.py sizes its cases by, and the test-matrix generator (tests/solve_cases.py) held to its own
claim — dominance by row and by column, Varah's bound against ``numpy.linalg.inv``, and ``numpy.linalg.solve`` itself inside
every bound the GPU file uses (otherwise those bounds would test nothing).  No GPU needed."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi, _solve
from brainevent_amd import _autograd as AG
import solve_cases as SC

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'brainevent_amd.h'
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_solve.hip'
ENTRY_POINTS = {'be_solve_workspace_bytes': 2, 'be_solve_setup': 10, 'be_solve_residual': 12, 'be_solve_diagonal': 7,
                'be_solve_iterate': 13}


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_entry_points_are_in_the_header_and_the_table_with_equal_argument_counts():
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    for name, arity in ENTRY_POINTS.items():
        m = re.findall(r'\b(?:int|int64_t)\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, re.S)
        assert len(m) == 1, name
        assert len(m[0].split(',')) == len(_abi.PROTOTYPES[name][1]) == arity, name
    from test_host_cpu import declared_symbols
    assert set(ENTRY_POINTS) <= set(declared_symbols())


def test_entry_points_follow_diag_fill_in_the_header_and_the_table():
    text = HEADER.read_text()
    names = ['be_diag_fill'] + list(ENTRY_POINTS)
    order = [text.index(f' {n}(') for n in names]
    assert order == sorted(order)
    table = list(_abi.PROTOTYPES)
    at = table.index('be_diag_fill')
    assert table[at:at + 6] == names


def test_mirrored_constants_equal_the_source():
    text = SOURCE.read_text()
    for pattern, value in ((r'constexpr int kSolveThreads = (\d+);', 256), (r'constexpr int kSolveVecGridCap = (\d+);', 1024),
                           (r'constexpr int kSolveSpmvGridCap = (\d+);', 2048)):
        found = re.findall(pattern, text)
        assert len(found) == 1 and int(found[0]) == value, (pattern, found)
    assert 'sizeof(SolveState) == 72' in text and _solve._STATE.itemsize == 72
    assert _solve._STATE.fields['status'][1] == 40 and _solve._STATE.fields['iters'][1] == 44
    assert 'return avg <= 24 ? 4 : (avg <= 160 ? 16 : 64);' in text        # the lanes-per-row classes of the GPU cases
    code = re.sub(r'//[^\n]*', '', text)
    assert 'atomic' not in code and 'Cooperative' not in code                # fixed-order sums, launch boundaries only
    assert _solve.CHUNK == 8 and _solve.MAX_RESTARTS == 3


# ------------------------------------------------------------------------------------------------ surface
@pytest.mark.parametrize('f', [be.CSR.solve, be.CSC.solve, be.Dense.solve, be.DataRepresentation.solve],
                         ids=['CSR', 'CSC', 'Dense', 'DataRepresentation'])
def test_methods_begin_with_the_reference_signature(f):
    p = list(inspect.signature(f).parameters.values())
    assert [q.name for q in p[:4]] == ['self', 'b', 'tol', 'reorder']
    assert p[1].default is inspect.Parameter.empty and p[2].default == 1e-6 and p[3].default == 1
    assert all(q.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for q in p[:4])


def test_method_keywords():
    for f in (be.CSR.solve, be.CSC.solve, be.Dense.solve):
        p = inspect.signature(f).parameters
        assert [(k, p[k].default) for k in ('rtol', 'maxiter', 'x0', 'return_info')] == [
            ('rtol', None), ('maxiter', 1000), ('x0', None), ('return_info', False)]
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('rtol', 'maxiter', 'x0', 'return_info'))
        assert 'unused' in f.__doc__
    for f in (be.CSR.solve, be.CSC.solve):
        assert 'ITERATIVE' in f.__doc__ and '2698-2734' in f.__doc__
    assert 'ITERATIVE' in be.csr_solve.__doc__ and 'unused' in be.csr_solve.__doc__


def test_functional_signature():
    p = list(inspect.signature(be.csr_solve).parameters.values())
    assert [q.name for q in p[:6]] == ['data', 'indices', 'indptr', 'b', 'tol', 'reorder']
    assert p[4].default == 1e-6 and p[5].default == 1
    assert p[6].name == 'shape' and p[6].kind is inspect.Parameter.KEYWORD_ONLY and p[6].default is None
    assert be.csr_solve is _solve.csr_solve and be.csr_solve_p is _solve.csr_solve_p


def test_registry_finds_the_primitive_by_its_tags():
    p = be.csr_solve_p
    assert isinstance(p, be.OpKernel) and p.name == 'csr_solve' and p.available_backends() == ['hip']
    assert {'csr', 'float', 'solve'} <= p.tags
    assert be.get_primitives_by_tags({'csr', 'float', 'solve'})['csr_solve'] is p
    assert 'csr_solve' in be.get_all_primitive_names()
    assert 'Solve' in AG.__all__ and issubclass(AG.Solve, torch.autograd.Function)


def test_the_base_class_refuses():
    class M(be.DataRepresentation):
        pass
    with pytest.raises(NotImplementedError, match='solve'):
        M().solve(np.zeros(3))


# ------------------------------------------------------------------------------------------------ refusals without a device
def _tiny(dtype=np.float32):
    return np.array([2, 1, 3], dtype=dtype), np.array([0, 1, 1], dtype=np.int32), np.array([0, 2, 3], dtype=np.int32)


def test_refusals_need_no_device(monkeypatch):
    from brainevent_amd import _lib
    monkeypatch.setattr(_lib, '_device_ok', False)
    data, idx, ptr = _tiny()
    with pytest.raises(NotImplementedError, match='1-D'):
        be.csr_solve(data, idx, ptr, np.zeros((2, 2), dtype=np.float32))
    with pytest.raises(AssertionError, match='The number of rows in the matrix must match the size of the right-hand side'):
        be.csr_solve(data, idx, ptr, np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError, match='square'):
        be.csr_solve(data, idx, ptr, np.zeros(2, dtype=np.float32), shape=(2, 3))
    for bad in (np.float16, torch.bfloat16):
        d = torch.tensor([2, 1, 3], dtype=bad) if bad is torch.bfloat16 else data.astype(bad)
        with pytest.raises(ValueError, match='float32 or float64'):
            be.csr_solve(d, idx, ptr, np.zeros(2, dtype=np.float32))
    with pytest.raises(be.KernelNotAvailableError):                        # valid operands get as far as the device
        be.csr_solve(data, idx, ptr, np.ones(2, dtype=np.float32))


def test_call_function_refusals():
    data, idx, ptr = (torch.from_numpy(a) for a in _tiny())
    b = torch.ones(2)
    with pytest.raises(ValueError, match='maxiter'):
        be.csr_solve_p_call(data, idx, ptr, b, shape=(2, 2), maxiter=0)
    with pytest.raises(ValueError, match='rtol'):
        be.csr_solve_p_call(data, idx, ptr, b, shape=(2, 2), rtol=0.0)
    with pytest.raises(ValueError, match='x0'):
        be.csr_solve_p_call(data, idx, ptr, b, shape=(2, 2), x0=torch.ones(3))
    assert _solve.default_rtol(torch.float32) == 1e-5 and _solve.default_rtol(torch.float64) == 1e-10


# ------------------------------------------------------------------------------------------------ the generator's own claim
def _small_cases(dtype):
    yield SC.dominant_case(1, 0, 1, dtype, name='n1')
    yield SC.dominant_case(2, 1, 2, dtype, name='n2')
    yield SC.dominant_case(7, 3, 3, dtype, name='n7')
    yield SC.dominant_case(33, 5, 4, dtype, shuffle=True, name='n33')
    yield SC.dominant_case(65, 40, 5, dtype, name='lpr16')
    yield SC.dominant_case(64, 3, 6, dtype, dup_offdiag=True, dup_diag=True, shuffle=True, name='dups')
    counts = np.full(257, 3)
    counts[100] = 256
    yield SC.dominant_case(257, counts, 7, dtype, name='full row')
    yield SC.dominant_case(257, 200, 8, dtype, indptr_dtype=np.int64, name='lpr64')
    yield SC.block_case(23, 4, 9, dtype, name='blocks')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_generator_is_dominant_by_row_and_by_column_with_mixed_signs(dtype):
    for case in _small_cases(dtype):
        A = case.A
        assert case.data.dtype == dtype and case.b.dtype == dtype and case.indices.dtype == np.int32
        d = np.abs(np.diag(A))
        off = np.abs(A) - np.diag(d)
        assert np.all(off.sum(axis=1) <= 0.5 * d), case.name
        assert np.all(off.sum(axis=0) <= 0.5 * d), case.name
        if case.n > 1:
            assert np.diag(A).min() < 0 < np.diag(A).max(), case.name
        assert np.isclose(SC.row_gap(case), np.min(d - off.sum(axis=1)), rtol=1e-12)
        assert np.isclose(SC.col_gap(case), np.min(d - off.sum(axis=0)), rtol=1e-12)
        assert SC.row_gap(case) >= 0.25 and SC.col_gap(case) >= 0.25
        np.testing.assert_allclose(case.matvec(case.b), A @ case.b.astype(np.float64), rtol=1e-12, atol=1e-12)


def test_generator_options_do_what_they_say():
    plain = SC.dominant_case(64, 3, 6, np.float32)
    dups = SC.dominant_case(64, 3, 6, np.float32, dup_offdiag=True, dup_diag=True, shuffle=True)
    assert dups.data.size == 2 * plain.data.size
    r, c = dups.rows, dups.indices
    assert all(np.sum((r == i) & (c == i)) == 2 for i in range(64))                      # every diagonal stored twice
    assert any(np.any(np.diff(c[r == i]) < 0) for i in range(64))                        # ... and rows out of order
    np.testing.assert_allclose(dups.A, plain.A, rtol=1e-6)
    counts = np.full(257, 3)
    counts[100] = 256
    full = SC.dominant_case(257, counts, 7, np.float32)
    assert full.longest_row == 257 and np.median(np.diff(full.indptr)) == 4
    assert SC.dominant_case(257, 200, 8, np.float64, indptr_dtype=np.int64).indptr.dtype == np.int64


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_varah_bound_holds_against_the_inverse(dtype):
    for case in _small_cases(dtype):
        inv = np.linalg.inv(case.A)
        assert np.abs(inv).sum(axis=1).max() <= 1.0 / SC.row_gap(case) * (1 + 1e-12), case.name
        assert np.abs(inv.T).sum(axis=1).max() <= 1.0 / SC.col_gap(case) * (1 + 1e-12), case.name          # A.T: the backward solve


@pytest.mark.parametrize('dtype,rtol', [(np.float32, 1e-5), (np.float64, 1e-10), (np.float64, 1e-13)],
                         ids=['f32', 'f64', 'f64-grad'])
def test_numpy_solve_stays_inside_every_bound_the_gpu_file_uses(dtype, rtol):
    """The reference rounded to the dtype (what a perfect solver would return) passes the residual and the error bound, for
    ``A`` and — with the column gap — for ``A.T``; with ``rtol = 0`` the residual bound alone would NOT hold for it, so the
    bound is not vacuous."""
    for case in _small_cases(dtype):
        x_star = np.linalg.solve(case.A, case.b.astype(np.float64))
        SC.check_solution(case, x_star.astype(dtype), x_star, rtol)
        g = np.cos(np.arange(case.n)).astype(dtype)
        t = SC.Case(case.data, case.indices, case.indptr, g, case.n, case.name + '.T')
        t._dense = case.A.T                                                   # (matvec is only used through the dense matrix)
        lam = np.linalg.solve(case.A.T, g.astype(np.float64))
        res = float(np.linalg.norm(g.astype(np.float64) - case.A.T @ lam.astype(dtype).astype(np.float64)))
        bound = rtol * np.linalg.norm(g.astype(np.float64)) + (case.longest_row + 2) * np.finfo(dtype).eps * np.linalg.norm(
            np.abs(case.A.T) @ np.abs(lam))
        assert res <= bound and np.max(np.abs(lam.astype(dtype) - lam)) <= bound / SC.col_gap(case), case.name
    big = SC.dominant_case(257, 200, 8, dtype)
    x_star = np.linalg.solve(big.A, big.b.astype(np.float64))
    wrong = x_star * (1 + 100 * rtol)
    with pytest.raises(AssertionError):
        SC.check_solution(big, wrong, x_star, rtol)


def test_block_solve_is_the_dense_solve():
    case = SC.block_case(23, 4, 9, np.float64)
    np.testing.assert_allclose(SC.block_solve(case, 4), np.linalg.solve(case.A, case.b), rtol=1e-12)
    A = case.A
    for i in range(23):
        assert np.all(A[i, :(i // 4) * 4] == 0) and np.all(A[i, (i // 4) * 4 + 4:] == 0)
        assert np.count_nonzero(A[i]) == min(4, 23 - (i // 4) * 4)


# ------------------------------------------------------------------------------------------------ the reference recurrence
@pytest.mark.parametrize('dtype,rtol', [(np.float32, 1e-5), (np.float64, 1e-10)], ids=['f32', 'f64'])
def test_reference_recurrence_converges_on_the_generator(dtype, rtol):
    for case in _small_cases(dtype):
        x, info = SC.bicgstab_reference(case.A, case.b, rtol)
        assert info['converged'] and info['iterations'] <= 60 and info['residual'] <= rtol, (case.name, info)
        SC.check_solution(case.with_dtype(np.float64), x, np.linalg.solve(case.A, case.b.astype(np.float64)), rtol)
    diag = SC.dominant_case(65, 0, 11, dtype)
    x, info = SC.bicgstab_reference(diag.A, diag.b, rtol)
    assert info['converged'] and info['iterations'] <= 1


def test_reference_recurrence_reports_failure():
    case = SC.dominant_case(33, 5, 4, np.float64)
    _, info = SC.bicgstab_reference(case.A, case.b, 1e-10, maxiter=1)
    assert not info['converged'] and info['iterations'] == 1
    A = case.A.copy()
    A[5] = 0.0
    _, info = SC.bicgstab_reference(A, case.b, 1e-10, maxiter=200)
    assert not info['converged']
    P = np.array([[0.0, 1.0], [1.0, 0.0]])                  # a permutation, no diagonal at all: rh.v = 0 at once (breakdown)
    _, info = SC.bicgstab_reference(P, np.array([1.0, 0.0]), 1e-10)
    assert not info['converged'] and info['iterations'] == 0
    _, info = SC.bicgstab_reference(case.A, np.zeros(33), 1e-10)
    assert info['converged'] and info['iterations'] == 0
