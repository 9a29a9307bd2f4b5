"""The host side of row slicing (brainevent_amd/_slice.py, the two helpers in _misc.py): names, registry, header, the row
selector, validators, the refusing stubs — and the kernel geometry tests/test_slice_rows_gpu.py places its cases by (its CONSTS
table) against csrc/be_slice.hip read as text and against the library's own answer.  No GPU needed.  When the last part fails
after a retune, move the table with the source: the GPU cases follow it."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi, _lib, _slice
from brainevent_amd._error import KernelNotAvailableError
from brainevent_amd._misc import build_sub_csr, normalize_row_index
from test_slice_rows_gpu import CONSTS

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_slice.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'

FUNCTIONS = ['csr_slice_rows', 'csr_slice_rows_p_call', 'csr_slice_rows_grad', 'csr_slice_rows_grad_p_call']
PRIMITIVES = ['csr_slice_rows_p', 'csr_slice_rows_grad_p']
ENTRY_POINTS = {'be_slice_rows': 14, 'be_slice_rows_grad': 19, 'be_slice_rows_copy': 15}


@pytest.fixture
def no_device(monkeypatch):
    """The library's view of a machine without a HIP device, wherever the test runs."""
    monkeypatch.setattr(_lib, '_device_ok', False)


# ------------------------------------------------------------------------------------------------ surface
def test_names_are_exported():
    assert sorted(_slice.__all__) == sorted(FUNCTIONS + PRIMITIVES)
    for name in FUNCTIONS:
        assert callable(getattr(be, name)) and getattr(be, name) is getattr(_slice, name)
    for name in PRIMITIVES:
        p = getattr(be, name)
        assert isinstance(p, be.OpKernel) and p.name == name[:-2] and p.available_backends() == ['hip']
        assert p._call_fn is getattr(_slice, name + '_call')


def test_registry_finds_the_primitives_by_tag():
    found = be.get_primitives_by_tags({'csr', 'slice'})
    assert found['csr_slice_rows'] is be.csr_slice_rows_p and found['csr_slice_rows_grad'] is be.csr_slice_rows_grad_p
    assert {'csr', 'slice'} <= be.csr_slice_rows_p.tags and {'csr', 'slice', 'grad'} <= be.csr_slice_rows_grad_p.tags
    assert {'csr_slice_rows', 'csr_slice_rows_grad'} <= set(be.get_all_primitive_names())


@pytest.mark.parametrize('name', sorted(ENTRY_POINTS))
def test_header_declares_the_entry_point(name):
    """(tests/test_host_cpu.py::test_library_exports_every_declared_symbol then holds the library to it)"""
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', HEADER.read_text(), re.S)
    assert m, f"{name} is not declared"
    assert len(m.group(1).split(',')) == len(_abi.PROTOTYPES[name][1]) == ENTRY_POINTS[name]
    from test_host_cpu import declared_symbols
    assert name in declared_symbols()


def test_entry_points_follow_dt2t_in_the_header_and_the_table():
    text = HEADER.read_text()
    order = [text.index(f' {n}(') for n in ('be_dt2t', 'be_slice_rows_tile_cols', 'be_slice_rows', 'be_slice_rows_grad_workspace_bytes',
                                             'be_slice_rows_grad', 'be_slice_rows_copy', 'be_jitmm_float_workspace_bytes')]
    assert order == sorted(order)
    names = list(_abi.PROTOTYPES)
    at = names.index('be_dt2t')
    assert names[at + 1:at + 6] == ['be_slice_rows_tile_cols', 'be_slice_rows', 'be_slice_rows_grad_workspace_bytes',
                                    'be_slice_rows_grad', 'be_slice_rows_copy']


# ------------------------------------------------------------------------------------------------ the row selector
def test_an_int_is_marked_as_scalar_and_wraps():
    for index, want in ((3, 3), (-1, 9), (0, 0), (-10, 0), (np.int32(4), 4)):
        rows = normalize_row_index(index, 10)
        assert isinstance(rows, np.ndarray) and rows.ndim == 0 and rows.dtype == np.int64 and int(rows) == want


@pytest.mark.parametrize('make', [list, tuple, lambda x: np.asarray(x, np.int32), lambda x: np.asarray(x, np.int64),
                                  lambda x: np.asarray(x, np.uint8) if min(x) >= 0 else np.asarray(x, np.int16)])
def test_sequences_give_1d_int64_with_negatives_wrapped(make):
    rows = normalize_row_index(make([3, 7, 7, -1]), 10)
    assert isinstance(rows, np.ndarray) and rows.dtype == np.int64
    np.testing.assert_array_equal(rows, [3, 7, 7, 9])


def test_a_tensor_stays_a_tensor():
    rows = normalize_row_index(torch.tensor([3, 7, 7, -1], dtype=torch.int32), 10)
    assert isinstance(rows, torch.Tensor) and rows.dtype == torch.int64 and rows.tolist() == [3, 7, 7, 9]
    rows = normalize_row_index(torch.tensor(-2), 10)
    assert isinstance(rows, torch.Tensor) and rows.ndim == 0 and int(rows) == 8


def test_slices_are_resolved_against_n_rows():
    np.testing.assert_array_equal(normalize_row_index(slice(None, None, -2), 7), [6, 4, 2, 0])
    np.testing.assert_array_equal(normalize_row_index(slice(None), 4), [0, 1, 2, 3])
    np.testing.assert_array_equal(normalize_row_index(slice(-3, 100), 5), [2, 3, 4])
    assert normalize_row_index(slice(3, 3), 5).shape == (0,)
    assert normalize_row_index(slice(None, None, -2), 7).dtype == np.int64


def test_empty_selections():
    for index in ([], (), np.zeros(0, np.int64), torch.zeros(0, dtype=torch.int64), slice(0, 0)):
        rows = normalize_row_index(index, 5)
        assert tuple(rows.shape) == (0,)
    assert tuple(normalize_row_index([], 0).shape) == (0,)


@pytest.mark.parametrize('index', [True, [True, False], np.array([True, False]), torch.tensor([True, False]), 1.0, [0.0, 1.0],
                                   np.array([1.0], np.float32), torch.tensor([1.0]), torch.tensor([1.0], dtype=torch.bfloat16)])
def test_bool_and_float_selectors_raise(index):
    with pytest.raises(IndexError, match='integer'):
        normalize_row_index(index, 5)


@pytest.mark.parametrize('index', [5, -6, [0, 5], [-6, 0], np.array([4, 5]), torch.tensor([-6])])
def test_out_of_bounds_raises(index):
    """n_rows and -n_rows - 1 are the first numbers outside."""
    with pytest.raises(IndexError, match='out of bounds for axis 0 with size 5'):
        normalize_row_index(index, 5)
    with pytest.raises(IndexError):
        normalize_row_index(0, 0)


def test_a_2d_selector_raises():
    with pytest.raises(IndexError, match='1-D'):
        normalize_row_index([[0, 1]], 5)


# ------------------------------------------------------------------------------------------------ validators
W4, IDX, PTR, ROWS = np.ones(4, np.float32), np.array([0, 2, 1, 2], np.int32), np.array([0, 2, 4], np.int32), np.array([1, 0])
SLICE_BAD = {
    'data 2-D': dict(data=W4.reshape(2, 2)),
    'indices 2-D': dict(indices=IDX.reshape(2, 2)),
    'indptr 2-D': dict(indptr=PTR.reshape(1, 3)),
    'row_indices 2-D': dict(row_indices=ROWS.reshape(1, 2)),
    'float indices': dict(indices=IDX.astype(np.float32)),
    'float indptr': dict(indptr=PTR.astype(np.float64)),
    'float row_indices': dict(row_indices=ROWS.astype(np.float32)),
    'bool row_indices': dict(row_indices=np.array([True, False])),
    'integer data': dict(data=W4.astype(np.int32)),
    'data of another length': dict(data=W4[:3]),
    'indptr of another row count': dict(indptr=np.array([0, 2, 4, 4], np.int32)),
    'shape of length 3': dict(shape=(2, 3, 1)),
}


@pytest.mark.parametrize('case', sorted(SLICE_BAD))
@pytest.mark.parametrize('as_tensor', [False, True])
def test_slice_validator_fires_before_any_device_use(case, as_tensor, no_device):
    kw = dict(data=W4, indices=IDX, indptr=PTR, row_indices=ROWS, shape=(2, 3))
    kw.update(SLICE_BAD[case])
    shape = kw.pop('shape')
    if as_tensor:
        kw = {k: torch.from_numpy(v) for k, v in kw.items()}
    with pytest.raises(AssertionError):
        be.csr_slice_rows_p_call(kw['data'], kw['indices'], kw['indptr'], kw['row_indices'], shape=shape)
    with pytest.raises(AssertionError):
        be.csr_slice_rows(kw['data'], kw['indices'], kw['indptr'], kw['row_indices'], shape=shape)


CT = np.ones((2, 3), np.float32)
GRAD_BAD = {
    'ct 1-D': dict(ct=CT.reshape(-1)),
    'ct 3-D': dict(ct=CT.reshape(2, 3, 1)),
    'indices 2-D': dict(indices=IDX.reshape(2, 2)),
    'indptr 2-D': dict(indptr=PTR.reshape(1, 3)),
    'row_indices 2-D': dict(row_indices=ROWS.reshape(1, 2)),
    'float indices': dict(indices=IDX.astype(np.float32)),
    'float indptr': dict(indptr=PTR.astype(np.float32)),
    'float row_indices': dict(row_indices=ROWS.astype(np.float64)),
    'integer ct': dict(ct=CT.astype(np.int64)),
    'ct of another selection': dict(ct=np.ones((3, 3), np.float32)),
    'ct of another width': dict(ct=np.ones((2, 4), np.float32)),
    'indptr of another row count': dict(indptr=np.array([0, 4], np.int32)),
}


@pytest.mark.parametrize('case', sorted(GRAD_BAD))
@pytest.mark.parametrize('as_tensor', [False, True])
def test_grad_validator_fires_before_any_device_use(case, as_tensor, no_device):
    kw = dict(ct=CT, indices=IDX, indptr=PTR, row_indices=ROWS)
    kw.update(GRAD_BAD[case])
    if as_tensor:
        kw = {k: torch.from_numpy(v) for k, v in kw.items()}
    with pytest.raises(AssertionError):
        be.csr_slice_rows_grad_p_call(kw['ct'], kw['indices'], kw['indptr'], kw['row_indices'], shape=(2, 3))
    with pytest.raises(AssertionError):
        be.csr_slice_rows_grad(kw['ct'], kw['indices'], kw['indptr'], kw['row_indices'], shape=(2, 3))


def test_valid_input_without_a_device_is_a_missing_kernel(no_device):
    """No quiet host fallback: a well-formed call on a machine without a HIP device says so."""
    with pytest.raises(KernelNotAvailableError):
        be.csr_slice_rows(W4, IDX, PTR, ROWS, shape=(2, 3))
    with pytest.raises(KernelNotAvailableError):
        be.csr_slice_rows(W4[:1], IDX, PTR, np.int64(1), shape=(2, 3))
    with pytest.raises(KernelNotAvailableError):
        be.csr_slice_rows_grad(CT, IDX, PTR, ROWS, shape=(2, 3))
    with pytest.raises(KernelNotAvailableError):
        build_sub_csr(W4, IDX, PTR, ROWS, 3)


# ------------------------------------------------------------------------------------------------ containers
def test_containers_have_both_methods_and_the_contract_declares_them():
    for cls in (be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost):
        assert callable(cls.__getitem__) and callable(cls.slice_rows)
        assert cls.__getitem__ is not be.DataRepresentation.__getitem__ and cls.slice_rows is not be.DataRepresentation.slice_rows
    assert be.Dense.__getitem__ is not be.DataRepresentation.__getitem__


def test_the_stubs_refuse():
    with pytest.raises(NotImplementedError, match='__getitem__'):
        be.DataRepresentation()[0]
    with pytest.raises(NotImplementedError, match='slice_rows'):
        be.DataRepresentation().slice_rows([0])
    for cls in (be.JITCScalarR, be.JITCNormalC, be.JITCUniformR):
        assert cls.__getitem__ is be.DataRepresentation.__getitem__ and cls.slice_rows is be.DataRepresentation.slice_rows
    planned = object.__new__(be.PlannedMatrix)
    with pytest.raises(NotImplementedError, match='raw structure'):
        planned[0]
    with pytest.raises(NotImplementedError, match='raw structure'):
        planned.slice_rows([0])


def _bare(cls, indices, indptr, shape):
    """A container around host arrays (its constructor moves them to the device)."""
    M = object.__new__(cls)
    M.indices, M.shape, M.backend, M.buffers, M._numpy_result = torch.from_numpy(indices), shape, None, {}, True
    M.data = torch.ones(indices.shape)
    if indptr is not None:
        M.indptr = torch.from_numpy(indptr)
    return M


@pytest.mark.parametrize('cls', [be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost])
def test_container_selectors_are_checked_before_any_device_use(cls, no_device):
    """shape[0] of the matrix, whatever the storage axis: 2 rows for the row-stored pair, 3 for the column-stored one."""
    fixed = cls in (be.FixedNumPerPre, be.FixedNumPerPost)
    shape = (2, 3) if cls in (be.CSR, be.FixedNumPerPre) else (3, 2)
    M = _bare(cls, IDX.reshape(2, 2) if fixed else IDX, None if fixed else PTR, shape)
    for method in (M.__getitem__, M.slice_rows):
        with pytest.raises(IndexError, match=f'size {shape[0]}'):
            method(shape[0])
        with pytest.raises(IndexError, match=f'size {shape[0]}'):
            method([-shape[0] - 1])
        with pytest.raises(IndexError, match='integer'):
            method([True, False])
        with pytest.raises(IndexError, match='integer'):
            method(0.5)


# ------------------------------------------------------------------------------------------------ the kernel's geometry
PATTERNS = {
    'threads': r'constexpr int kThreads = (\d+);',
    'tile_cols': r'constexpr int kTileCols = (\d+);',
    'tile_cols_f64': r'constexpr int kTileColsF64 = (\d+);',
    'entries_per_thread': r'constexpr int kPer = (\d+);',
    'vec_bytes': r'constexpr int kVecBytes = (\d+);',
    'grad_split': r'constexpr int kGradSplit = (\d+);',
    'copy_per_thread': r'constexpr int kCopyPer = (\d+);',
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    found = re.findall(PATTERNS[key], SOURCE.read_text())
    assert len(found) == 1, f"{key}: {SOURCE.name} holds /{PATTERNS[key]}/ {len(found)} times"
    assert int(found[0]) == CONSTS[key], (f"{key}: {SOURCE.name} says {found[0]}, tests/test_slice_rows_gpu.py assumes "
                                          f"{CONSTS[key]}: move the table, its cases follow")


def test_the_geometry_is_built_from_the_constants_as_the_gpu_cases_assume():
    """One pass of a row is threads * entries_per_thread entries; the tile is chosen by the accumulator's width; one launch
    bound for every kernel of the file."""
    text = SOURCE.read_text()
    assert len(re.findall(r'sizeof\(typename PB<W>::acc\) == 8 \? kTileColsF64 : kTileCols;', text)) == 1
    assert len(re.findall(r'base \+= \(int64_t\)kThreads \* kPer\)', text)) == 1
    assert len(re.findall(r'constexpr int64_t kTile = \(int64_t\)kThreads \* kCopyPer;', text)) == 1
    assert len(re.findall(r'dim3\(gx, kGradSplit\), dim3\(kThreads\)', text)) == 1
    assert len(re.findall(r'__launch_bounds__\(\w+\)', text)) == len(re.findall(r'__launch_bounds__\(kThreads\)', text)) == 4
    assert 'atomicAdd(&s_own' in text and 'atomicMin(&s_own' in text and not re.search(r'atomicAdd\([^&]', text)


def test_the_library_reports_the_same_tile():
    """`be_slice_rows_tile_cols` needs no device: the answer is a constant of the build."""
    if _lib.needs_build():
        _lib.build()
    f = _lib.fn('be_slice_rows_tile_cols')
    assert [f(code) for code in (0, 2, 3)] == [CONSTS['tile_cols']] * 3          # f32, f16, bf16
    assert f(1) == CONSTS['tile_cols_f64']
    assert f(7) == -1
    ws = _lib.fn('be_slice_rows_grad_workspace_bytes')
    assert ws(1000, 0) >= 4000 and ws(1000, 1) >= 8000 and ws(0, 0) > 0
