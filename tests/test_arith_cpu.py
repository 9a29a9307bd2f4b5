"""The host side of container arithmetic (brainevent_amd/_arith.py): names, registry, header, the operator methods on every
class, the JITC parameter rules, the refusals that need no device — and the kernel geometry tests/test_arith_gpu.py places its
cases by (its CONSTS table) against csrc/be_arith.hip read as text.  No GPU needed.  When the last part fails after a retune,
move the table with the source: the GPU cases follow it."""
import operator
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi, _arith, _lib
from test_arith_gpu import CONSTS

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_arith.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'

OPERATORS = ['apply', 'apply2', '__abs__', '__neg__', '__pos__', '__mul__', '__truediv__', '__add__', '__sub__', '__rmul__',
             '__rtruediv__', '__radd__', '__rsub__']
CLASSES = [be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost, be.Dense, be.JITCScalarR, be.JITCScalarC, be.JITCUniformR,
           be.JITCUniformC, be.JITCNormalR, be.JITCNormalC]


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, '_device_ok', False)


# ------------------------------------------------------------------------------------------------ surface
def test_names_are_exported():
    assert be.ArithmeticMixin is _arith.ArithmeticMixin and be.entries_dense_op_p is _arith.entries_dense_op_p
    p = be.entries_dense_op_p
    assert isinstance(p, be.OpKernel) and p.name == 'entries_dense_op' and p.available_backends() == ['hip']
    assert _arith.OPS == {'take': 0, 'mul': 1, 'div': 2, 'rdiv': 3}


def test_registry_finds_the_primitive_by_tag():
    assert be.get_primitives_by_tags({'csr', 'arith'})['entries_dense_op'] is be.entries_dense_op_p
    assert {'csr', 'arith'} <= be.entries_dense_op_p.tags and 'entries_dense_op' in be.get_all_primitive_names()


def test_header_declares_the_entry_point():
    m = re.search(r'\bint\s+be_entries_dense_op\s*\(([^;]*?)\)\s*;', HEADER.read_text(), re.S)
    assert m, "be_entries_dense_op is not declared"
    assert len(m.group(1).split(',')) == len(_abi.PROTOTYPES['be_entries_dense_op'][1]) == 17
    from test_host_cpu import declared_symbols
    assert 'be_entries_dense_op' in declared_symbols()


def test_entry_points_follow_sddmm_in_the_header_and_the_table():
    text = HEADER.read_text()
    names = ['be_sddmm_rows', 'be_entries_dense_op', 'be_diag_scan', 'be_diag_move', 'be_diag_fill']
    order = [text.index(f' {n}(') for n in names]
    assert order == sorted(order)
    table = list(_abi.PROTOTYPES)
    at = table.index('be_sddmm_rows')
    assert table[at:at + 5] == names


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: c.__name__)
def test_every_class_has_the_operators(cls):
    assert issubclass(cls, be.ArithmeticMixin)
    for name in OPERATORS:
        assert getattr(cls, name) is getattr(be.ArithmeticMixin, name), name
    for hook in ('_unitary_op', '_binary_op', '_binary_rop'):
        assert getattr(cls, hook) is not getattr(be.ArithmeticMixin, hook), hook
    assert cls.__array_ufunc__ is None                     # numpy on the left defers to __rmul__ and its kin


def test_the_objects_that_stand_for_a_matrix_get_nothing():
    for cls in (be.PlannedMatrix, be.Mirror, be.JITCScatterShard, be.JITCGatherShard):
        assert not issubclass(cls, be.ArithmeticMixin) and not hasattr(cls, '__mul__') and not hasattr(cls, 'apply2')
    bare = be.ArithmeticMixin()
    for call in (lambda: -bare, lambda: bare * 2, lambda: 2 - bare):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------------------------------------ JITC: parameter arithmetic
@pytest.mark.parametrize('cls', [be.JITCScalarR, be.JITCScalarC], ids=lambda c: c.__name__)
def test_jitc_scalar_acts_on_the_weight(cls):
    M = cls((1.5, 0.1, 42), shape=(10, 20), corder=True)
    cases = ((M * 2, 3.0), (2 * M, 3.0), (M / 2, 0.75), (3 / M, 2.0), (M + 0.5, 2.0), (0.5 + M, 2.0), (M - 0.5, 1.0), (2 - M, 0.5),
             (-M, -1.5), (abs(-M), 1.5), (+M, 1.5), (M.apply(lambda w: w * w), 2.25), (np.float32(2) * M, 3.0),
             (np.array([2.0]) * M, 3.0), (M * torch.tensor(2.0), 3.0), (M.apply2(2, operator.pow), 2.25),
             (M.apply2(2, operator.pow, reverse=True), 2 ** 1.5))
    for got, want in cases:
        assert type(got) is cls and float(got.weight) == pytest.approx(want, rel=1e-7)
        assert (got.prob, got.seed, got.shape, got.corder) == (M.prob, M.seed, M.shape, M.corder) and got.buffers == {}


@pytest.mark.parametrize('cls', [be.JITCUniformR, be.JITCUniformC], ids=lambda c: c.__name__)
def test_jitc_uniform_acts_on_both_bounds(cls):
    M = cls((0.5, 1.5, 0.1, 42), shape=(10, 20))
    for got, want in ((M * 2, (1.0, 3.0)), (2 * M, (1.0, 3.0)), (M / 2, (0.25, 0.75)), (M + 1, (1.5, 2.5)), (1 + M, (1.5, 2.5)),
                      (M - 1, (-0.5, 0.5)), (+M, (0.5, 1.5)), (abs(M), (0.5, 1.5))):
        assert type(got) is cls and (float(got.wlow), float(got.whigh)) == want
        assert (got.prob, got.seed, got.shape, got.corder) == (M.prob, M.seed, M.shape, M.corder)
    # what flips the bounds is refused by the constructor, as in the reference
    for flip in (lambda: -M, lambda: M * -1, lambda: 1 - M, lambda: 1 / M):
        with pytest.raises(ValueError, match='wlow must be <= whigh'):
            flip()
    point = cls((0.5, 0.5, 0.1, 42), shape=(10, 20))
    assert (float((-point).wlow), float((-point).whigh)) == (-0.5, -0.5)


@pytest.mark.parametrize('cls', [be.JITCNormalR, be.JITCNormalC], ids=lambda c: c.__name__)
def test_jitc_normal_acts_on_loc_alone(cls):
    M = cls((0.5, 0.25, 0.1, 42), shape=(10, 20))
    for got, loc in ((M * 2, 1.0), (2 * M, 1.0), (M / 2, 0.25), (M + 1, 1.5), (1 - M, 0.5), (-M, -0.5), (abs(-M), 0.5)):
        assert type(got) is cls and float(got.wloc) == loc and float(got.wscale) == 0.25
        assert (got.prob, got.seed, got.shape, got.corder) == (M.prob, M.seed, M.shape, M.corder)


@pytest.mark.parametrize('cls', [be.JITCScalarR, be.JITCUniformC, be.JITCNormalR], ids=lambda c: c.__name__)
def test_jitc_refuses_anything_but_a_size_1_operand(cls):
    M = cls((0.5, 0.1, 42) if cls is be.JITCScalarR else (0.5, 1.5, 0.1, 42), shape=(4, 6))
    for bad in (np.ones(6), np.ones((4, 6)), torch.ones(4, 6), [1.0, 2.0]):
        for fn in (operator.mul, operator.add):
            with pytest.raises(NotImplementedError, match='size-1'):
                fn(M, bad)
    with pytest.raises(NotImplementedError, match='size-1'):
        np.ones(6) * M
    with pytest.raises(NotImplementedError, match='sparse'):
        M * M
    with pytest.raises(NotImplementedError, match='sparse'):
        M + be.Dense.__new__(be.Dense)


def test_the_docstrings_name_what_equals_the_dense_operation():
    doc = be.JITCMatrix._unitary_op.__doc__
    for word in ('Scalar', 'Uniform', 'Normal', 'todense()', 'scale', 'ValueError'):
        assert word in doc
    assert 'in place' in be.ArithmeticMixin.apply.__doc__ and 'plastic' in be.CSR._unitary_op.__doc__


# ------------------------------------------------------------------------------------------------ stored rows: no device needed
IDX, PTR = np.array([0, 2, 1, 2], np.int32), np.array([0, 2, 4], np.int32)


def _bare(cls, shape=None):
    fixed = cls in (be.FixedNumPerPre, be.FixedNumPerPost)
    M = object.__new__(cls)
    M.indices = torch.from_numpy(IDX.reshape(2, 2) if fixed else IDX)
    M.shape = shape or ((2, 3) if cls in (be.CSR, be.FixedNumPerPre) else (3, 2))
    M.backend, M.buffers, M._numpy_result = None, {'scatter_plan': object(), 'mirror': object(), 'diag_positions': 'plan'}, True
    M.data = torch.tensor([1.0, -2.0, 4.0, -1.0]).reshape(M.indices.shape)
    if not fixed:
        M.indptr = torch.from_numpy(PTR)
    return M


STORED = [be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost]


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_data_only_operations_share_the_structure(cls, monkeypatch):
    """Unary operations and size-1 operands are torch on `data`: they run wherever `data` lives."""
    monkeypatch.setattr(_arith.A, 'device', lambda: torch.device('cpu'))
    M = _bare(cls)
    for got, want in ((-M, -M.data), (abs(M), M.data.abs()), (+M, M.data), (M * 2, M.data * 2), (2 * M, M.data * 2),
                      (M / 2, M.data / 2), (2 / M, 2 / M.data), (np.float32(2) * M, M.data * 2), (np.array([2.0]) * M, M.data * 2),
                      (M * torch.tensor([2.0], dtype=torch.float64), M.data * 2), (M.apply(torch.square), M.data ** 2),
                      (M.apply2(2, lambda a, b: a + b), M.data + 2), (M.apply2(M, operator.sub), M.data * 0),
                      (M + M, M.data * 2), (M.apply2(-M, operator.truediv, reverse=True), M.data * 0 - 1)):
        assert type(got) is cls and got.shape == M.shape and got._numpy_result is True
        assert got.indices is M.indices and getattr(got, 'indptr', None) is getattr(M, 'indptr', None)
        assert got.data.dtype == torch.float32 and torch.equal(got.data, want)
        assert got.buffers == {'diag_positions': 'plan'}               # plans and mirrors embed weights: they do not travel
    assert M.apply(lambda d: d.double()).data.dtype == torch.float64
    with pytest.raises(ValueError, match='shape'):
        M.apply(lambda d: d.reshape(-1)[:2])


@pytest.mark.parametrize('cls', STORED, ids=lambda c: c.__name__)
def test_refusals_fire_before_any_device_use(cls, no_device):
    M = _bare(cls)
    n0, n1 = M.shape
    for bad in (np.ones(n1, np.float32), np.ones((n0, 1), np.float32), np.ones((n1, n0 + 5), np.float32), torch.ones(1, n0, n1)):
        for call in (lambda: M * bad, lambda: bad / M, lambda: M.apply2(bad, torch.maximum)):
            with pytest.raises(NotImplementedError, match='dt2t'):
                call()
    other = _bare(cls)
    for fn in (operator.mul, operator.truediv, operator.add, operator.sub):
        with pytest.raises(NotImplementedError, match='sparse'):
            fn(M, other)
    with pytest.raises(NotImplementedError, match='sparse'):
        M * be.JITCScalarR((1.0, 0.1, 1), shape=M.shape)
    with pytest.raises(be.UnsupportedOperationError, match='requires grad'):
        M * torch.ones(n0, n1, requires_grad=True)
    with pytest.raises(ValueError, match='broadcast'):
        M + np.ones((n0, n1 + 1), np.float32)
    with pytest.raises(be.KernelNotAvailableError):                    # no quiet host fallback for the sample kernel
        M * np.ones((n0, n1), np.float32)


def test_dense_operand_rule_without_a_device(monkeypatch):
    monkeypatch.setattr(be._dense.A, 'device', lambda: torch.device('cpu'))
    M = object.__new__(be.Dense)
    M.data, M.shape, M.backend, M.buffers, M._numpy_result = torch.arange(6.0).reshape(2, 3), (2, 3), None, {}, False
    for bad in (np.ones((3, 2)), np.ones(2), torch.ones(1, 2, 3)):
        with pytest.raises(ValueError):
            M._binary_operand_data(bad)
    with pytest.raises(NotImplementedError):
        M._binary_operand_data(_bare(be.CSR))
    with pytest.raises(ValueError, match=r'\(2,\)'):
        M.diag_add(np.ones(3, np.float32))


# ------------------------------------------------------------------------------------------------ the kernel's geometry
PATTERNS = {
    'threads': r'constexpr int kThreads = (\d+);',
    'tile': r'constexpr int kTile = (\d+);',
    'grid_cap': r'constexpr int kGridCap = (\d+);',
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    found = re.findall(PATTERNS[key], SOURCE.read_text())
    assert len(found) == 1, f"{key}: {SOURCE.name} holds /{PATTERNS[key]}/ {len(found)} times"
    assert int(found[0]) == CONSTS[key], (f"{key}: {SOURCE.name} says {found[0]}, tests/test_arith_gpu.py assumes "
                                          f"{CONSTS[key]}: move the table, its cases follow")


def test_the_geometry_is_built_from_the_constants_as_the_gpu_cases_assume():
    text = SOURCE.read_text()
    assert len(re.findall(r'tile \+= \(int64_t\)gridDim\.x \* kTile\)', text)) == 3           # sample, scan, move
    assert len(re.findall(r'grid_for\(nse, kTile, kGridCap\)', text)) == 3
    assert len(re.findall(r'__launch_bounds__\(\w+\)', text)) == len(re.findall(r'__launch_bounds__\(kThreads\)', text)) == 4
    assert '__shared__' not in text                                                           # no LDS
    assert len(re.findall(r'__builtin_nontemporal_load\(col \+ e\)', text)) == 3
    assert '__builtin_nontemporal_store(PB<W>::put(v), out + e)' in text
