"""The host side of the per-synapse products (brainevent_amd/_dt2t.py): names, registry, header, validators, container routing —
and the loop geometry tests/test_dt2t_gpu.py sizes its cases by (its CONSTS table) against csrc/be_dt2t.hip read as text.  No
GPU needed.  When the last part fails after a retune, move the table with the source: the GPU cases follow it."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi, _dt2t, _lib
from brainevent_amd._error import KernelNotAvailableError
from test_dt2t_gpu import CONSTS

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_dt2t.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'

FUNCTIONS = ['csrmv_dt2t', 'csrmm_dt2t', 'cscmv_dt2t', 'cscmm_dt2t', 'fcnmv_dt2t', 'fcnmm_dt2t',
             'csrmv_dt2t_p_call', 'csrmm_dt2t_p_call', 'fcnmv_dt2t_p_call', 'fcnmm_dt2t_p_call']
PRIMITIVES = ['csrmv_dt2t_p', 'csrmm_dt2t_p', 'fcnmv_dt2t_p', 'fcnmm_dt2t_p']


@pytest.fixture
def no_device(monkeypatch):
    """The library's view of a machine without a HIP device, wherever the test runs."""
    monkeypatch.setattr(_lib, '_device_ok', False)


# ------------------------------------------------------------------------------------------------ surface
def test_names_are_exported():
    assert sorted(_dt2t.__all__) == sorted(FUNCTIONS + PRIMITIVES)
    for name in FUNCTIONS:
        assert callable(getattr(be, name)) and getattr(be, name) is getattr(_dt2t, name)
    for name in PRIMITIVES:
        p = getattr(be, name)
        assert isinstance(p, be.OpKernel) and p.name == name[:-2] and p.available_backends() == ['hip']
        assert p._call_fn is getattr(_dt2t, name + '_call')


def test_registry_finds_the_primitives_by_tag():
    csr = be.get_primitives_by_tags({'csr', 'float'})
    fcn = be.get_primitives_by_tags({'fcn', 'float'})
    assert csr['csrmv_dt2t'] is be.csrmv_dt2t_p and csr['csrmm_dt2t'] is be.csrmm_dt2t_p
    assert fcn['fcnmv_dt2t'] is be.fcnmv_dt2t_p and fcn['fcnmm_dt2t'] is be.fcnmm_dt2t_p
    assert {'csrmv_dt2t', 'csrmm_dt2t', 'fcnmv_dt2t', 'fcnmm_dt2t'} <= set(be.get_all_primitive_names())


def test_header_declares_the_entry_point():
    """(tests/test_host_cpu.py::test_library_exports_every_declared_symbol then holds the library to it)"""
    m = re.search(r'\bint\s+be_dt2t\s*\(([^;]*?)\)\s*;', HEADER.read_text(), re.S)
    assert m, "be_dt2t is not declared"
    assert len(m.group(1).split(',')) == len(_abi.PROTOTYPES['be_dt2t'][1]) == 15
    from test_host_cpu import declared_symbols
    assert 'be_dt2t' in declared_symbols()


# ------------------------------------------------------------------------------------------------ validators
Y2, W4 = np.ones(2, np.float32), np.ones(4, np.float32)
IDX, PTR = np.array([0, 2, 1, 2], np.int32), np.array([0, 2, 4], np.int32)
CSR_BAD = {
    'dtypes differ': dict(y=Y2.astype(np.float64)),
    'indptr 2-D': dict(indptr=PTR.reshape(1, 3)),
    'indices 2-D': dict(indices=IDX.reshape(2, 2), w=W4.reshape(2, 2)),
    'y 2-D': dict(y=Y2.reshape(1, 2)),
    'w 2-D': dict(w=W4.reshape(1, 4)),
    'float indices': dict(indices=IDX.astype(np.float32)),
    'float indptr': dict(indptr=PTR.astype(np.float32)),
    'integer weights': dict(y=Y2.astype(np.int32), w=W4.astype(np.int32)),
    'w shorter than indices': dict(w=W4[:3]),
    'y of the other axis': dict(y=np.ones(3, np.float32)),
    'y of the other axis, transposed': dict(transpose=True),
    'indptr of another row count': dict(indptr=np.array([0, 2, 4, 4], np.int32)),
}


@pytest.mark.parametrize('case', sorted(CSR_BAD))
@pytest.mark.parametrize('as_tensor', [False, True])
def test_csrmv_validator_fires_before_any_device_use(case, as_tensor, no_device):
    kw = dict(y=Y2, w=W4, indices=IDX, indptr=PTR, transpose=False)
    kw.update(CSR_BAD[case])
    transpose = kw.pop('transpose')
    if as_tensor:
        kw = {k: torch.from_numpy(v) for k, v in kw.items()}
    with pytest.raises(AssertionError):
        be.csrmv_dt2t_p_call(kw['y'], kw['w'], kw['indices'], kw['indptr'], shape=(2, 3), transpose=transpose)
    with pytest.raises(AssertionError):
        be.csrmv_dt2t(kw['y'], kw['w'], kw['indices'], kw['indptr'], shape=(2, 3), transpose=transpose)


YB, WB = np.ones((2, 2), np.float32), np.ones((2, 4), np.float32)
CSRMM_BAD = {
    'dtypes differ': dict(y=YB.astype(np.float16)),
    'y 1-D': dict(y=Y2),
    'w 1-D': dict(w=W4),
    'batch mismatch': dict(w=np.ones((3, 4), np.float32)),
    'w shorter than indices': dict(w=WB[:, :3]),
    'y of the other axis': dict(y=np.ones((2, 3), np.float32)),
    'integer weights': dict(y=YB.astype(np.int64), w=WB.astype(np.int64)),
    'float indices': dict(indices=IDX.astype(np.float64)),
}


@pytest.mark.parametrize('case', sorted(CSRMM_BAD))
def test_csrmm_validator_fires_before_any_device_use(case, no_device):
    kw = dict(y=YB, w=WB, indices=IDX, indptr=PTR)
    kw.update(CSRMM_BAD[case])
    with pytest.raises(AssertionError):
        be.csrmm_dt2t(kw['y'], kw['w'], kw['indices'], kw['indptr'], shape=(2, 3))
    with pytest.raises(AssertionError):
        be.cscmm_dt2t(kw['y'], kw['w'], kw['indices'], kw['indptr'], shape=(3, 2), transpose=True)


FW, FI = np.ones((2, 2), np.float32), np.array([[0, 1], [1, 2]])
FCN_BAD = {
    'indices 1-D': (dict(indices=FI.reshape(-1)), 'indices must be 2D'),
    'shape of length 3': (dict(shape=(2, 3, 1)), 'shape must be length-2'),
    'integer weights': (dict(weights=FW.astype(np.int32)), 'floating-point'),
    'weights of another shape': (dict(weights=np.ones((2, 3), np.float32)), 'size-1 or match indices shape'),
    'y 2-D': (dict(y=np.ones((1, 2), np.float32)), 'y must be 1D'),
    'y of the other axis': (dict(y=np.ones(3, np.float32)), 'does not match expected 2'),
    'y of the other axis, transposed': (dict(transpose=True), 'does not match expected 3'),
    'rows of another matrix': (dict(shape=(3, 3), y=np.ones(3, np.float32)), 'rows'),
    'float indices': (dict(indices=FI.astype(np.float32)), 'integer type'),
}


@pytest.mark.parametrize('case', sorted(FCN_BAD))
def test_fcnmv_validator_fires_before_any_device_use(case, no_device):
    kw = dict(weights=FW, indices=FI, y=Y2, shape=(2, 3), transpose=False)
    change, message = FCN_BAD[case]
    kw.update(change)
    with pytest.raises(ValueError, match=message):
        be.fcnmv_dt2t(kw['weights'], kw['indices'], kw['y'], shape=kw['shape'], transpose=kw['transpose'])
    with pytest.raises(ValueError, match=message):
        be.fcnmv_dt2t_p_call(torch.from_numpy(kw['weights']), torch.from_numpy(kw['indices']), torch.from_numpy(kw['y']),
                             shape=kw['shape'], transpose=kw['transpose'])


FWB = np.ones((2, 2, 2), np.float32)
FCNMM_BAD = {
    'indices 3-D': (dict(indices=FI.reshape(1, 2, 2)), 'indices must be 2D'),
    'shape of length 1': (dict(shape=(2,)), 'shape must be length-2'),
    'integer weights': (dict(weights=FWB.astype(np.int8)), 'floating-point'),
    'y 1-D': (dict(y=Y2), 'y must be 2D'),
    'y of the other axis': (dict(y=np.ones((2, 3), np.float32)), 'trailing dimension 3 does not match expected 2'),
    'weights without the batch axis': (dict(weights=FW), r'size-1 or have shape \(2, 2, 2\)'),
    'weights of another batch': (dict(weights=np.ones((3, 2, 2), np.float32)), r'size-1 or have shape \(2, 2, 2\)'),
}


@pytest.mark.parametrize('case', sorted(FCNMM_BAD))
def test_fcnmm_validator_fires_before_any_device_use(case, no_device):
    kw = dict(weights=FWB, indices=FI, y=YB, shape=(2, 3), transpose=False)
    change, message = FCNMM_BAD[case]
    kw.update(change)
    with pytest.raises(ValueError, match=message):
        be.fcnmm_dt2t(kw['weights'], kw['indices'], kw['y'], shape=kw['shape'], transpose=kw['transpose'])


def test_out_is_checked_before_any_device_use(no_device):
    with pytest.raises(TypeError, match='device tensor'):
        be.csrmv_dt2t(Y2, W4, IDX, PTR, shape=(2, 3), out=np.empty(4, np.float32))
    with pytest.raises(ValueError, match='shape'):
        be.csrmv_dt2t(Y2, W4, IDX, PTR, shape=(2, 3), out=torch.empty(5))
    with pytest.raises(ValueError, match='dtype'):
        be.csrmv_dt2t(Y2, W4, IDX, PTR, shape=(2, 3), out=torch.empty(4, dtype=torch.float64))
    with pytest.raises(ValueError, match='on the device'):
        be.csrmv_dt2t(Y2, W4, IDX, PTR, shape=(2, 3), out=torch.empty(4))
    with pytest.raises(TypeError, match='device tensor'):
        be.fcnmv_dt2t(FW, FI, Y2, shape=(2, 3), transpose=False, out=np.empty((2, 2), np.float32))


def test_valid_input_without_a_device_is_a_missing_kernel(no_device):
    """No quiet host fallback: a well-formed call on a machine without a HIP device says so."""
    with pytest.raises(KernelNotAvailableError):
        be.csrmv_dt2t(Y2, W4, IDX, PTR, shape=(2, 3))
    with pytest.raises(KernelNotAvailableError):
        be.cscmv_dt2t(np.ones(3, np.float32), W4, IDX, PTR, shape=(3, 2))
    with pytest.raises(KernelNotAvailableError):
        be.csrmm_dt2t(YB, WB, IDX, PTR, shape=(2, 3))
    with pytest.raises(KernelNotAvailableError):
        be.fcnmv_dt2t(FW, FI, Y2, shape=(2, 3), transpose=False)
    with pytest.raises(KernelNotAvailableError):
        be.fcnmm_dt2t(FWB, FI, YB, shape=(2, 3), transpose=False)


# ------------------------------------------------------------------------------------------------ containers
def test_containers_have_both_methods_and_the_contract_declares_them():
    for cls in (be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost):
        assert callable(cls.dt2t) and callable(cls.dt2t_transposed)
        assert cls.dt2t is not be.DataRepresentation.dt2t and cls.dt2t_transposed is not be.DataRepresentation.dt2t_transposed
    for name in ('dt2t', 'dt2t_transposed'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(be.DataRepresentation(), name)(Y2, W4)
        with pytest.raises(NotImplementedError, match='raw structure'):
            getattr(object.__new__(be.PlannedMatrix), name)(Y2, W4)


def _bare(cls, indices, indptr, shape):
    """A container around host arrays (its constructor moves them to the device)."""
    M = object.__new__(cls)
    M.indices, M.shape, M.backend, M.buffers = torch.from_numpy(indices), shape, None, {}
    if indptr is not None:
        M.indptr = torch.from_numpy(indptr)
    return M


@pytest.mark.parametrize('cls, method, want', [
    (be.CSR, 'dt2t', False), (be.CSR, 'dt2t_transposed', True), (be.CSC, 'dt2t', True), (be.CSC, 'dt2t_transposed', False),
])
def test_csr_and_csc_route_as_the_reference(cls, method, want, monkeypatch):
    """CSR: its own shape, `dt2t` by the row.  CSC (3 columns here: the stored rows): the reversed shape, `dt2t` by the stored
    index (reference `_csr/main.py:1850`, `:1885`, `:2770`, `:2808`)."""
    seen = {}

    def spy(y, w, indices, indptr, *, shape, transpose, backend=None, out=None):
        seen.update(shape=tuple(shape), transpose=transpose, y=y, w=w, indices=indices, indptr=indptr)
        return [torch.zeros(4)]
    monkeypatch.setattr(_dt2t, 'csrmv_dt2t_p_call', spy)
    shape = (2, 3) if cls is be.CSR else (3, 2)           # CSC of a (3, 2) matrix: an indptr over 2 columns
    M = _bare(cls, IDX, PTR, shape)
    y, w = torch.ones(3), torch.ones(4)
    getattr(M, method)(y, w)
    assert seen['shape'] == (2, 3) and seen['transpose'] is want
    assert seen['y'] is y and seen['w'] is w and seen['indices'] is M.indices and seen['indptr'] is M.indptr


@pytest.mark.parametrize('cls, method, want', [
    (be.FixedNumPerPre, 'dt2t', False), (be.FixedNumPerPre, 'dt2t_transposed', True),
    (be.FixedNumPerPost, 'dt2t', True), (be.FixedNumPerPost, 'dt2t_transposed', False),
])
def test_fixed_number_containers_route_as_the_reference(cls, method, want, monkeypatch):
    """`shape=_a_shape` (the stored structure), `transpose=_ell_transpose(...)` (reference `_fcn/main.py:387`, `:417`, `:853`,
    `:1114`): the pre axis is the row of a `FixedNumPerPre`, the stored index of a `FixedNumPerPost`."""
    seen = {}

    def spy(weights, indices, y, *, shape, transpose, backend=None, out=None):
        seen.update(shape=tuple(shape), transpose=transpose, weights=weights, y=y)
        return [torch.zeros(2, 2)]
    monkeypatch.setattr(_dt2t, 'fcnmv_dt2t_p_call', spy)
    # 2 stored rows over 3 ids: a (2, 3) FixedNumPerPre, a (3, 2) FixedNumPerPost
    M = _bare(cls, FI.astype(np.int32), None, (2, 3) if cls is be.FixedNumPerPre else (3, 2))
    y, w = torch.ones(3), torch.ones(2, 2)
    getattr(M, method)(y, w)
    assert seen['shape'] == (2, 3) and seen['transpose'] is want and seen['weights'] is w and seen['y'] is y


# ------------------------------------------------------------------------------------------------ the kernel's geometry
PATTERNS = {
    'threads': r'constexpr int kThreads = (\d+);',
    'vec_bytes': r'constexpr int kVecBytes = (\d+);',
    'runs_per_thread': r'constexpr int kRuns = (\d+);',
    'grid_cap': r'constexpr int kGridCap = (\d+);',
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    found = re.findall(PATTERNS[key], SOURCE.read_text())
    assert len(found) == 1, f"{key}: {SOURCE.name} holds /{PATTERNS[key]}/ {len(found)} times"
    assert int(found[0]) == CONSTS[key], (f"{key}: {SOURCE.name} says {found[0]}, tests/test_dt2t_gpu.py assumes {CONSTS[key]}: "
                                          f"move the table, its cases follow")


def test_tile_and_grid_are_built_from_the_constants_as_the_gpu_cases_assume():
    """T = threads * runs * V with V = vec_bytes / sizeof(element), in the kernel and in its launcher; the grid cap is shared
    by the batch rows; one launch bound."""
    text = SOURCE.read_text()
    assert len(re.findall(r'constexpr int V = kVecBytes / \(int\)sizeof\(B\);', text)) == 2
    assert len(re.findall(r'constexpr int64_t kTile = \(int64_t\)kThreads \* kRuns \* V;', text)) == 2
    assert len(re.findall(r'kGridCap / n_batch', text)) == 2
    assert len(re.findall(r'grid_for\(nnz \+ V - 1, \(int\)kTile, \(int\)cap\)', text)) == 1
    assert len(re.findall(r'__launch_bounds__\(kThreads\)', text)) == 1
    assert len(re.findall(r'dim3\(gx, \(unsigned\)n_batch\), dim3\(kThreads\)', text)) == 1
