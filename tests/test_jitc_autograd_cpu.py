"""The autograd rules of the JIT-connectivity products (brainevent_amd/_autograd.py: JitProduct) against torch autograd on the
oracle's dense generator matrices, the ABI bookkeeping of be_jit_param_grad (csrc/be_jitc_grad.hip), the constants
tests/test_jitc_autograd_gpu.py sizes its cases by against the kernel source read as text, and the validation that needs no
device.  No GPU needed."""
import functools
import re
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi, _jitc, _lib
from brainevent_amd import _autograd as AG
from brainevent_amd._error import KernelNotAvailableError
from oracle import oracle_np

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_jitc_grad.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'
NAMES = ('be_jit_param_grad_workspace_bytes', 'be_jit_param_grad')


@pytest.fixture
def no_device(monkeypatch):
    """The library's view of a machine without a HIP device, wherever the test runs."""
    monkeypatch.setattr(_lib, '_device_ok', False)


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_entry_points_are_declared_once_and_last():
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)             # (comments hold commas and names)
    arity = {'be_jit_param_grad_workspace_bytes': 4, 'be_jit_param_grad': 15}
    for name in NAMES:
        m = re.findall(r'\b(?:int|int64_t)\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, re.S)
        assert len(m) == 1, name
        assert len(m[0].split(',')) == len(_abi.PROTOTYPES[name][1]) == arity[name]
    assert tuple(_abi.PROTOTYPES)[-2:] == NAMES                                  # appended: the entries before keep their order
    declared = re.findall(r'\b(be_\w+)\s*\(', text)
    assert tuple(declared[-2:]) == NAMES                                         # ... and the header ends with them
    assert 'be_jit_param_grad' in (ROOT / 'INTEGRATION.md').read_text()


def test_mirrored_constants_equal_the_source():
    text = SOURCE.read_text()
    for pattern, value in ((r'constexpr int kParamGradThreads = (\d+);', _jitc.JIT_PARAM_GRAD_THREADS),
                           (r'constexpr int kParamGradGridCap = (\d+);', _jitc.JIT_PARAM_GRAD_GRID_CAP)):
        found = re.findall(pattern, text)
        assert len(found) == 1 and int(found[0]) == value, (pattern, found, value)
    # the geometry the GPU cases assume: stride lanes per row, a grid capped over (row block, chunk) tasks taken grid-stride
    for pat in (r'const int64_t tpb = kParamGradThreads / S;', r'std::min<int64_t>\(tasks, kParamGradGridCap\)',
                r'for \(int64_t t = blockIdx.x; t < tasks; t \+= gridDim.x\)'):
        assert len(re.findall(pat, text)) == 1, pat
    assert 'atomic' not in text.replace('No float atomics', '')                 # fixed-order sums only


def test_surface():
    assert callable(be.jit_param_sums) and be.jit_param_sums is _jitc.jit_param_sums
    assert getattr(AG.JitProduct.backward, '__wrapped__', None) is not None     # once_differentiable
    assert 'JITC families excluded' not in (ROOT / 'DESIGN.md').read_text()


# ------------------------------------------------------------------------------------------------ the rules vs torch autograd
@functools.lru_cache(maxsize=None)
def _generator(family, shape, transpose, corder, mode, prob=0.2, seed=7):
    """(C, T): the structure (0/1) and t on the structure, both in the generator's orientation, float64."""
    kw = dict(shape=shape, transpose=transpose, corder=corder, matrix_mode=mode, dtype=np.float64)
    C = oracle_np.jit_generator_matrix('s', 1.0, 0.0, prob, seed, **kw)
    T = C * 0.0 if family == 's' else oracle_np.jit_generator_matrix(family, 0.0, 1.0, prob, seed, **kw)
    for M in (C, T):
        M.setflags(write=False)
    return C, T


@pytest.mark.parametrize('shape', [(13, 17), (37, 9)])
@pytest.mark.parametrize('mode', ['mv', 'mm'])
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('corder', [False, True])
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_rule_table_matches_dense_autograd(family, corder, transpose, mode, shape):
    rng = np.random.default_rng(zlib.crc32(repr((family, corder, transpose, mode, shape)).encode()))
    C, T = (torch.tensor(M) for M in _generator(family, shape, transpose, corder, mode))
    assert C.sum() > 10
    in_len, out_len = (shape[0], shape[1]) if transpose else (shape[1], shape[0])
    nb = 1 if mode == 'mv' else 5
    a = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(1.7, dtype=torch.float64, requires_grad=True)
    G = {'s': a * C, 'u': a * C + T * (b - a), 'n': a * C + b * T}[family]          # w = w0 + t w1 on the structure
    D = G if corder else G.T                                                      # (out_len, in_len)
    X = torch.tensor(rng.standard_normal((in_len, nb)), requires_grad=True)
    g = torch.from_numpy(rng.standard_normal((out_len, nb)))
    (D @ X).backward(g)
    # the parameter rule
    P, Q = AG.jit_pq(corder, g, X.detach())
    PQ = P @ Q.T
    assert PQ.shape == C.shape
    s0, s1 = (C * PQ).sum(), (T * PQ).sum()
    tol = 1e-12 * float((C * PQ.abs()).sum())
    ga, gb = AG.jit_param_grads(family, s0, s1)
    assert abs(float(ga - a.grad)) <= tol
    if family == 's':
        assert gb is None
    else:
        assert abs(float(gb - b.grad)) <= tol
    # the operand rule: the twin's flags draw the same generator, and its product is M.T @ g
    t_transpose, t_corder = AG.jit_twin_flags(transpose, corder)
    C2, T2 = (torch.tensor(M) for M in _generator(family, shape, t_transpose, t_corder, mode))
    assert torch.equal(C2, C) and torch.equal(T2, T)
    G2 = G.detach()
    D2 = G2 if t_corder else G2.T
    assert D2.shape == (in_len, out_len)
    np.testing.assert_allclose((D2 @ g).numpy(), X.grad.numpy(), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ what is recorded
def test_needed_follows_grad_mode_and_parameter_kind():
    p = torch.nn.Parameter(torch.tensor(0.5))
    x = torch.ones(4, requires_grad=True)
    assert AG.jit_needed((p, 1.0), np.ones(4, np.float32))
    assert AG.jit_needed((torch.nn.Parameter(torch.ones(1)),), torch.ones(4))
    assert AG.jit_needed((0.5, 1.0), x)
    assert AG.jit_needed((0.5,), be.BinaryArray(x))
    assert not AG.jit_needed((0.5, np.float32(1.0)), torch.ones(4))
    assert not AG.jit_needed((torch.tensor(0.5),), torch.ones(4))
    assert not AG.jit_needed((torch.ones(2, requires_grad=True),), torch.ones(4))             # not a size-1 parameter
    assert not AG.jit_needed((0.5,), torch.ones(4, dtype=torch.int32))
    assert not AG.jit_needed((0.5,), be.BitPackedBinary(x))                                   # bit-packed: parameter gradients only
    with torch.no_grad():
        assert not AG.jit_needed((p,), x)


# ------------------------------------------------------------------------------------------------ validation without a device
def test_validators_fire_before_any_device_use(no_device):
    P, Q = torch.ones(3, 2), torch.ones(4, 2)
    kw = dict(clen=10, seed=1, shape1=4, stride=32)
    with pytest.raises(ValueError, match='family'):
        be.jit_param_sums('x', P, Q, **kw)
    with pytest.raises(ValueError, match='stride'):
        be.jit_param_sums('n', P, Q, **{**kw, 'stride': 8})
    with pytest.raises(TypeError):
        be.jit_param_sums('n', P.numpy(), Q, **kw)
    with pytest.raises(ValueError, match='nb'):
        be.jit_param_sums('n', P, torch.ones(4, 3), **kw)
    with pytest.raises(ValueError, match='dtype'):
        be.jit_param_sums('n', P, Q.double(), **kw)
    with pytest.raises(ValueError, match='dtype'):
        be.jit_param_sums('n', P.int(), Q.int(), **kw)
    p = torch.nn.Parameter(torch.tensor(0.5))
    with pytest.raises(AssertionError):                                          # the functionals' own shape checks come first
        be.jitsmv(p, 0.2, torch.ones(5), 1, shape=(3, 4))
    with pytest.raises(AssertionError):
        be.binary_jitnmm(p, 1.0, 0.2, torch.ones(5, 2), 1, shape=(3, 4))


def test_a_gradient_without_a_device_is_a_missing_kernel(no_device):
    """No cut graph and no host fallback: the call that would have to record a node says that there is no device."""
    p = torch.nn.Parameter(torch.tensor(0.5))
    x = torch.ones(4, requires_grad=True)
    with pytest.raises(KernelNotAvailableError):
        be.jitsmv(p, 0.2, torch.ones(4), 1, shape=(3, 4))
    with pytest.raises(KernelNotAvailableError):
        be.binary_jitnmv(p, 1.0, 0.2, x, 1, shape=(3, 4))
    with pytest.raises(KernelNotAvailableError):
        be.JITCNormalR((p, 1.0, 0.2, 1), shape=(3, 4)) @ x
    with pytest.raises(KernelNotAvailableError):
        be.BinaryArray(np.ones(3, bool)) @ be.JITCUniformC((p, 1.0, 0.2, 1), shape=(3, 4))
    with pytest.raises(KernelNotAvailableError):
        be.jit_param_sums('n', torch.ones(3, 2), torch.ones(4, 2), clen=10, seed=1, shape1=4, stride=4)
