"""The host side of the JIT-connectivity per-synapse products (brainevent_amd/_jitc.py: jit{s,u,n}mv_dt2t, JITC*.dt2t,
materialize(canonical=True)): names, the ABI entry, the validators, the empty results — and the two constants of the sorted
fill that tests/test_jitc_dt2t_gpu.py sizes its cases by, against csrc/be_jitc.hip read as text.  No GPU needed."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi, _jitc, _lib

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_jitc.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'

FUNCTIONS = ['jitsmv_dt2t', 'jitumv_dt2t', 'jitnmv_dt2t']
CLASSES = ['JITCScalarR', 'JITCScalarC', 'JITCUniformR', 'JITCUniformC', 'JITCNormalR', 'JITCNormalC']
F32 = np.float32


@pytest.fixture
def no_device(monkeypatch):
    """The library's view of a machine without a HIP device, wherever the test runs."""
    monkeypatch.setattr(_lib, '_device_ok', False)


def _call(family, y, *, w=None, prob=0.2, seed=3, **kw):
    w = w if w is not None else {'s': (F32(0.5),), 'u': (F32(0.1), F32(0.9)), 'n': (F32(0.2), F32(1.3))}[family]
    return getattr(be, f'jit{family}mv_dt2t')(*w, prob, y, seed, **kw)


# ------------------------------------------------------------------------------------------------ surface
def test_names_are_exported():
    for name in FUNCTIONS:
        assert name in _jitc.__all__
        assert callable(getattr(be, name)) and getattr(be, name) is getattr(_jitc, name)
        sig = inspect.signature(getattr(be, name))
        kw = [p.name for p in sig.parameters.values() if p.kind is p.KEYWORD_ONLY]
        assert kw == ['shape', 'transpose', 'corder', 'backend', 'out']
        assert sig.parameters['transpose'].default is False and sig.parameters['corder'].default is True
        assert sig.parameters['seed'].default is None
    assert list(inspect.signature(be.jitsmv_dt2t).parameters)[:4] == ['weight', 'prob', 'y', 'seed']
    assert list(inspect.signature(be.jitumv_dt2t).parameters)[:5] == ['w_low', 'w_high', 'prob', 'y', 'seed']
    assert list(inspect.signature(be.jitnmv_dt2t).parameters)[:5] == ['w_loc', 'w_scale', 'prob', 'y', 'seed']


def test_containers_have_both_methods_and_the_canonical_keyword():
    for name in CLASSES:
        cls = getattr(be, name)
        assert cls.dt2t is not be.DataRepresentation.dt2t and cls.dt2t_transposed is not be.DataRepresentation.dt2t_transposed
        for meth in (cls.dt2t, cls.dt2t_transposed):
            assert list(inspect.signature(meth).parameters) == ['self', 'y', 'w', 'out']
        for meth in (cls.materialize, cls.tocsr, cls.tocsc):
            p = inspect.signature(meth).parameters['canonical']
            assert p.kind is p.KEYWORD_ONLY and p.default is False
    for meth in ('todense', 'tocsr', 'tocsc'):
        p = inspect.signature(getattr(_jitc._JITCModeView, meth)).parameters['canonical']
        assert p.kind is p.KEYWORD_ONLY and p.default is False


def test_header_declares_the_entry_point_and_the_table_holds_it():
    """(tests/test_abi_table_cpu.py compares the two argument by argument; tests/test_host_cpu.py holds the library to it)"""
    m = re.search(r'\bint\s+be_jitc_fill_sorted\s*\(([^;]*?)\)\s*;', HEADER.read_text(), re.S)
    assert m, "be_jitc_fill_sorted is not declared"
    assert len(m.group(1).split(',')) == len(_abi.PROTOTYPES['be_jitc_fill_sorted'][1]) == 15
    from test_host_cpu import declared_symbols
    assert 'be_jitc_fill_sorted' in declared_symbols()


# ------------------------------------------------------------------------------------------------ the kernel's geometry
PATTERNS = {
    'JIT_SORTED_WINDOW': r'constexpr int kSortedWindow = (\d+);',
    'JIT_SORTED_GRID_CAP': r'constexpr int kSortedGridCap = (\d+);',
}


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    found = re.findall(PATTERNS[key], SOURCE.read_text())
    assert len(found) == 1, f"{key}: {SOURCE.name} holds /{PATTERNS[key]}/ {len(found)} times"
    assert int(found[0]) == getattr(_jitc, key), f"{key}: {SOURCE.name} says {found[0]}, _jitc.py says {getattr(_jitc, key)}"


def test_the_sorted_fill_is_launched_as_the_gpu_cases_assume():
    """One owner row per workgroup, at most the cap per launch; a window is a multiple of the words the block's threads take."""
    text = SOURCE.read_text()
    assert len(re.findall(r'std::min<int64_t>\(n_rows, kSortedGridCap\)', text)) == 1
    assert len(re.findall(r'row \+= gridDim\.x', text)) >= 1
    assert _jitc.JIT_SORTED_WINDOW % (32 * 256) == 0


# ------------------------------------------------------------------------------------------------ validators
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
@pytest.mark.parametrize('as_tensor', [False, True])
def test_validators_fire_before_any_device_use(family, as_tensor, no_device):
    conv = torch.from_numpy if as_tensor else (lambda a: a)
    with pytest.raises(AssertionError, match='1D'):
        _call(family, conv(np.ones((1, 3), F32)), shape=(3, 4))
    with pytest.raises(AssertionError, match='non-transpose'):
        _call(family, conv(np.ones(4, F32)), shape=(3, 4))
    with pytest.raises(AssertionError, match='transpose'):
        _call(family, conv(np.ones(3, F32)), shape=(3, 4), transpose=True)
    for corder in (False, True):
        with pytest.raises(ValueError, match='float32'):
            _call(family, conv(np.ones(3, np.float64)), shape=(3, 4), corder=corder)
        with pytest.raises(ValueError, match='float32'):
            _call(family, conv(np.ones(3, np.float16)), shape=(3, 4), corder=corder)
    w64 = {'s': (np.float64(0.5),), 'u': (np.float64(0.1), F32(0.9)), 'n': (F32(0.2), np.float64(1.3))}[family]
    w16 = {'s': (np.float16(0.5),), 'u': (np.float16(0.1), np.float16(0.9)), 'n': (np.float16(0.2), np.float16(1.3))}[family]
    for w in (w64, w16):
        with pytest.raises(ValueError, match='float32'):
            _call(family, conv(np.ones(3, F32)), w=w, shape=(3, 4))
    with pytest.raises(ValueError, match='prob'):
        _call(family, conv(np.ones(3, F32)), prob=1.5, shape=(3, 4))
    with pytest.raises(ValueError, match='backend'):
        _call(family, conv(np.ones(3, F32)), shape=(3, 4), backend='triton')


@pytest.mark.parametrize('cls_name', CLASSES)
def test_container_validators_fire_before_any_device_use(cls_name, no_device):
    fam = {'S': 's', 'U': 'u', 'N': 'n'}[cls_name[4]]
    params = {'s': (F32(0.5),), 'u': (F32(0.1), F32(0.9)), 'n': (F32(0.2), F32(1.3))}[fam]
    for corder in (False, True):
        M = getattr(be, cls_name)((*params, 0.2, 3), shape=(3, 4), corder=corder)
        with pytest.raises(AssertionError, match='non-transpose'):
            M.dt2t(np.ones(4, F32))
        with pytest.raises(AssertionError, match='transpose'):
            M.dt2t_transposed(np.ones(3, F32))
        with pytest.raises(AssertionError, match='1D'):
            M.dt2t(np.ones((3, 1), F32))
        with pytest.raises(ValueError, match='float32'):
            M.dt2t(np.ones(3, np.float64))
        with pytest.raises(TypeError, match='device tensor'):
            M.dt2t(np.ones(3, F32), out=np.empty(2, F32))
        with pytest.raises(ValueError, match='dtype'):
            M.dt2t(np.ones(3, F32), out=torch.empty(2, dtype=torch.float64))
        with pytest.raises(ValueError, match='on the device'):
            M.dt2t(np.ones(3, F32), out=torch.empty(2))
    M64 = getattr(be, cls_name)((*[np.float64(p) for p in params], 0.2, 3), shape=(3, 4), corder=True)
    with pytest.raises(ValueError, match='float32'):
        M64.dt2t(np.ones(3, F32))


def test_valid_input_without_a_device_is_a_missing_kernel(no_device):
    """No quiet host fallback: a well-formed call on a machine without a HIP device says so."""
    from brainevent_amd._error import KernelNotAvailableError
    for corder in (False, True):
        with pytest.raises(KernelNotAvailableError):
            be.jitsmv_dt2t(F32(0.5), 0.2, np.ones(3, F32), 3, shape=(3, 4), corder=corder)


# ------------------------------------------------------------------------------------------------ nothing drawn
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('corder', [False, True])
def test_prob_zero_and_empty_shapes_give_an_empty_result(family, transpose, corder, no_device):
    """(host arrays in: a host array of length 0 out, no device touched — the reference returns ``zeros(0)`` the same way)"""
    for shape, prob in (((3, 4), 0.0), ((0, 4), 0.2), ((3, 0), 0.2)):
        y = np.ones(shape[1] if transpose else shape[0], F32)
        r = _call(family, y, prob=prob, shape=shape, transpose=transpose, corder=corder)
        assert isinstance(r, np.ndarray) and r.shape == (0,) and r.dtype == F32
    for cls_kind in 'RC':
        cls = getattr(be, {'s': 'JITCScalar', 'u': 'JITCUniform', 'n': 'JITCNormal'}[family] + cls_kind)
        params = {'s': (F32(0.5),), 'u': (F32(0.1), F32(0.9)), 'n': (F32(0.2), F32(1.3))}[family]
        M = cls((*params, 0.0, 3), shape=(3, 4), corder=corder)
        r = (M.dt2t_transposed if transpose else M.dt2t)(np.ones(4 if transpose else 3, F32))
        assert isinstance(r, np.ndarray) and r.shape == (0,) and r.dtype == F32
