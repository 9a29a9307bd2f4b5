"""The host side of diag_add (brainevent_amd/_diag.py): names, header, the offset dtype rule, the validators — and the diagonal
rule restated as a short numpy loop (`diag_rule` / `diag_values`), held against the reference's docstring example here and
reused by tests/test_diag_add_gpu.py as the expected answer.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi, _diag, _lib

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_arith.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'
ENTRY_POINTS = {'be_diag_scan': 8, 'be_diag_move': 16, 'be_diag_fill': 13}


# ------------------------------------------------------------------------------------------------ the rule
def diag_rule(indptr, indices, n_diag):
    """The structure of `A + diag(d)`: a row i < n_diag without a stored index i gains one entry, before its first stored entry
    with an index > i in storage order (at the row's end if there is none); where the diagonal is stored more than once the LAST
    copy is the diagonal.  Returns (new_indptr, new_indices, old_to_new, diag_dest) as int64 / int32 / int64 / int64."""
    n_rows = len(indptr) - 1
    new_indptr, new_indices, old_to_new, diag_dest = [0], [], np.zeros(len(indices), np.int64), np.zeros(n_diag, np.int64)
    for i in range(n_rows):
        row = list(range(int(indptr[i]), int(indptr[i + 1])))
        cols = [int(indices[j]) for j in row]
        at = None
        if i < n_diag and i not in cols:
            at = next((k for k, c in enumerate(cols) if c > i), len(cols))
        for k, j in enumerate(row):
            if k == at:
                diag_dest[i] = len(new_indices)
                new_indices.append(i)
            old_to_new[j] = len(new_indices)
            if i < n_diag and cols[k] == i:
                diag_dest[i] = len(new_indices)
            new_indices.append(cols[k])
        if at == len(cols):
            diag_dest[i] = len(new_indices)
            new_indices.append(i)
        new_indptr.append(len(new_indices))
    return np.asarray(new_indptr, np.int64), np.asarray(new_indices, np.int32), old_to_new, diag_dest


def diag_values(data, d, positions):
    """`nd = 0; nd[old_to_new] = data; nd[diag_dest] += d` in float64 (exact for the tests' values)."""
    _, new_indices, old_to_new, diag_dest = positions
    nd = np.zeros(len(new_indices), np.float64)
    nd[old_to_new] = np.broadcast_to(np.asarray(data, np.float64), old_to_new.shape)
    nd[diag_dest] += np.asarray(d, np.float64)
    return nd


def test_the_rule_gives_the_reference_docstring_example():
    indptr, indices = np.array([0, 1, 2, 4], np.int32), np.array([0, 2, 0, 2], np.int32)
    pos = diag_rule(indptr, indices, 3)
    np.testing.assert_array_equal(pos[0], [0, 1, 3, 5])
    np.testing.assert_array_equal(pos[1], [0, 1, 2, 0, 2])
    np.testing.assert_array_equal(pos[2], [0, 2, 3, 4])
    np.testing.assert_array_equal(pos[3], [0, 1, 4])
    np.testing.assert_allclose(diag_values(np.ones(4), [0.1, 0.2, 0.3], pos), [1.1, .2, 1, 1, 1.3], rtol=0, atol=1e-12)


def test_the_rule_on_duplicates_unsorted_rows_and_rectangles():
    # row 0: the diagonal stored twice (the last copy counts); row 1: unsorted, the diagonal goes before the FIRST index > 1;
    # row 2: nothing above the diagonal (appended); row 3: beyond n_diag = 3 columns... of a 4 x 3 matrix: copied
    indptr, indices = np.array([0, 3, 6, 7, 9]), np.array([0, 2, 0, 2, 0, 2, 1, 2, 0], np.int32)
    p, idx, o2n, dest = diag_rule(indptr, indices, 3)
    np.testing.assert_array_equal(p, [0, 3, 7, 9, 11])
    np.testing.assert_array_equal(idx, [0, 2, 0, 1, 2, 0, 2, 1, 2, 2, 0])
    np.testing.assert_array_equal(o2n, [0, 1, 2, 4, 5, 6, 7, 9, 10])
    np.testing.assert_array_equal(dest, [2, 3, 8])
    # a 2 x 5 matrix: n_diag = 2, every row below it
    p, idx, _, dest = diag_rule(np.array([0, 0, 2]), np.array([4, 0], np.int32), 2)
    np.testing.assert_array_equal(p, [0, 1, 4])
    np.testing.assert_array_equal(idx, [0, 1, 4, 0])
    np.testing.assert_array_equal(dest, [0, 1])


# ------------------------------------------------------------------------------------------------ surface
def test_names_are_exported():
    assert {'csr_diag_position', 'csr_diag_add', 'DiagPlan', 'offset_dtype'} <= set(_diag.__all__)
    assert be.csr_diag_position is _diag.csr_diag_position and be.csr_diag_add is _diag.csr_diag_add
    for cls in (be.CSR, be.CSC, be.Dense):
        assert callable(cls.diag_add)
    for cls in (be.FixedNumPerPre, be.FixedNumPerPost, be.JITCScalarR, be.JITCNormalC, be.PlannedMatrix):
        assert not hasattr(cls, 'diag_add')


@pytest.mark.parametrize('name', sorted(ENTRY_POINTS))
def test_header_declares_the_entry_point(name):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', HEADER.read_text(), re.S)
    assert m, f"{name} is not declared"
    assert len(m.group(1).split(',')) == len(_abi.PROTOTYPES[name][1]) == ENTRY_POINTS[name]


def test_the_kernels_geometry_matches_the_gpu_cases():
    from test_diag_add_gpu import CONSTS
    text = SOURCE.read_text()
    for key, pattern in (('threads', r'constexpr int kThreads = (\d+);'), ('tile', r'constexpr int kTile = (\d+);'),
                         ('grid_cap', r'constexpr int kGridCap = (\d+);')):
        found = re.findall(pattern, text)
        assert len(found) == 1 and int(found[0]) == CONSTS[key], (key, found)
    assert len(re.findall(r'constexpr int kScanPer = kTile / kThreads;', text)) == 1
    assert CONSTS['scan_per'] == CONSTS['tile'] // CONSTS['threads']
    # integer atomics only, on the scan's two words per row
    assert len(re.findall(r'atomicMax\(', text)) == 1 and len(re.findall(r'atomicMin\(', text)) == 1
    assert 'atomicAdd' not in text and 'hipMemset' not in text


# ------------------------------------------------------------------------------------------------ the offset dtype
def test_offsets_are_int64_where_int32_cannot_hold_them():
    i32 = np.iinfo(np.int32).max
    assert _diag.offset_dtype(torch.int32, 5) == torch.int32
    assert _diag.offset_dtype(torch.int32, i32) == torch.int32
    assert _diag.offset_dtype(torch.int32, i32 + 1) == torch.int64           # the diagonal pushed the count past int32
    assert _diag.offset_dtype(torch.int64, 5) == torch.int64                 # an int64 indptr stays int64
    assert _diag.offset_dtype(torch.int64, 3 * 10 ** 9) == torch.int64


# ------------------------------------------------------------------------------------------------ validators
@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, '_device_ok', False)


PTR, IDX = np.array([0, 1, 2, 4], np.int32), np.array([0, 2, 0, 2], np.int32)


def test_position_validators_fire_before_any_device_use(no_device):
    for kw in (dict(indptr=PTR.reshape(1, 4)), dict(indices=IDX.reshape(2, 2)), dict(shape=(3, 3, 1)), dict(shape=(0, 3)),
               dict(shape=[3.0, 3]), dict(indptr=PTR.astype(np.float32)), dict(indices=IDX.astype(np.float64)),
               dict(indptr=PTR[:2])):
        args = dict(indptr=PTR, indices=IDX, shape=(3, 3))
        args.update(kw)
        with pytest.raises(AssertionError):
            be.csr_diag_position(args['indptr'], args['indices'], shape=args['shape'])
    with pytest.raises(be.KernelNotAvailableError):
        be.csr_diag_position(PTR, IDX, shape=(3, 3))


def test_diag_add_validators_fire_before_any_device_use(no_device):
    pos = diag_rule(PTR, IDX, 3)
    w, d = np.ones(4, np.float32), np.ones(3, np.float32)
    for bad in (dict(w=w.reshape(2, 2)), dict(d=d.reshape(1, 3)), dict(d=d.astype(np.float64)), dict(w=w[:3]), dict(d=d[:2]),
                dict(pos=(pos[0], pos[1], pos[2].astype(np.float32), pos[3])), dict(pos=(pos[0], pos[1], pos[2], pos[3].reshape(1, 3)))):
        args = dict(w=w, pos=pos, d=d)
        args.update(bad)
        with pytest.raises(AssertionError):
            be.csr_diag_add(args['w'], args['pos'], args['d'])
    with pytest.raises(be.KernelNotAvailableError):
        be.csr_diag_add(w, pos, d)


def _bare(cls, shape):
    M = object.__new__(cls)
    M.indices, M.indptr, M.shape, M.backend, M.buffers, M._numpy_result = torch.from_numpy(IDX), torch.from_numpy(PTR), shape, None, {}, True
    M.data = torch.ones(4)
    return M


@pytest.mark.parametrize('cls', [be.CSR, be.CSC])
def test_container_checks_the_diagonal_before_any_device_use(cls, no_device):
    M = _bare(cls, (3, 3))
    with pytest.raises(ValueError, match=r'\(3,\)'):
        M.diag_add(np.ones(4, np.float32))
    with pytest.raises(ValueError, match=r'\(3,\)'):
        M.diag_add(np.ones((3, 1), np.float32))
    with pytest.raises(AssertionError):
        M.diag_add(np.ones(3, np.int32))
    with pytest.raises(AssertionError, match='sparse'):
        M.diag_add(_bare(cls, (3, 3)))
    with pytest.raises(be.KernelNotAvailableError):
        M.diag_add(np.ones(3, np.float32))
