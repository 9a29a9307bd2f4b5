"""Host model of the sampled dense-dense product (csrc/be_sddmm.hip) and of the autograd rules of the float-operand products
(brainevent_amd/_autograd.py: FloatRowsProduct), checked against torch autograd on dense CPU tensors; the validation that
needs no device; and the loop geometry tests/test_float_autograd_gpu.py sizes its cases by (its CONSTS table) against the
kernel source read as text.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi
from brainevent_amd import _autograd as AG
from test_autograd_cpu import acc_dtype, random_csr, round_to

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_sddmm.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'


# ------------------------------------------------------------------------------------------------ the host model
def model_sddmm(indices, rows, P, Q, wdtype: torch.dtype) -> torch.Tensor:
    """``out[e] = sum_b P[rows[e], b] * Q[indices[e], b]``: ``P`` / ``Q`` hold values of the weight dtype (as float64), the
    sum runs in f32 (f64 for f64) in ascending ``b`` and is rounded once.  The kernel sums the same products in another — fixed
    — order and with fused multiply-adds, so the two agree bit for bit where no partial sum rounds: ``nb = 1`` (one product,
    one rounding) and integer-valued operands; elsewhere the GPU tests hold the kernel to an error bound."""
    ad = acc_dtype(wdtype)
    indices = np.asarray(indices).reshape(-1).astype(np.int64)
    rows = np.asarray(rows).reshape(-1).astype(np.int64)
    P = np.asarray(P, dtype=np.float64).astype(ad)
    Q = np.asarray(Q, dtype=np.float64).astype(ad)
    acc = np.zeros(indices.shape[0], dtype=ad)
    for b in range(P.shape[1]):
        acc = acc + P[rows, b] * Q[indices, b]
    return round_to(acc, wdtype)


def model_shared(indices, rows, P, Q) -> float:
    """One shared weight: ``sum(P * (A1 @ Q))`` with ``A1`` the structure with weight 1, in f64."""
    indices = np.asarray(indices).reshape(-1).astype(np.int64)
    rows = np.asarray(rows).reshape(-1).astype(np.int64)
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    a1q = np.zeros_like(P)
    np.add.at(a1q, rows, Q[indices])
    return float((P * a1q).sum())


def test_model_accumulates_in_f32_and_rounds_once():
    # f32: 1 + 2^-24 + 2^-24 stays 1 in ascending order; f16: the f32 sum 1 + 2^-11 + 2^-11 rounds once to 1 + 2^-10
    one = np.array([[1.0, 1.0, 1.0]])
    got = model_sddmm([0], [0], one, np.array([[1.0, 2.0 ** -24, 2.0 ** -24]]), torch.float32)
    assert got.item() == 1.0
    got16 = model_sddmm([0], [0], one, np.array([[1.0, 2.0 ** -11, 2.0 ** -11]]), torch.float16)
    assert got16.item() == 1.0 + 2.0 ** -10
    got64 = model_sddmm([0], [0], one, np.array([[1.0, 2.0 ** -24, 2.0 ** -24]]), torch.float64)
    assert got64.item() == 1.0 + 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the rules vs torch autograd
def _dense_from(w, rows, indices, m, k):
    return torch.zeros(m, k, dtype=torch.float64).index_put((torch.from_numpy(rows), torch.from_numpy(indices.astype(np.int64))), w,
                                                            accumulate=True)


@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('nb', [1, 3, 33])
def test_rules_match_dense_autograd(transpose, nb):
    """``A @ X``: dw = sddmm(P = g, Q = X), dX = A.T @ g.  ``A.T @ X``: dw = sddmm(P = X, Q = g), dX = A @ g."""
    rng = np.random.default_rng(11 * nb + transpose)
    m, k = 9, 13
    indices, indptr, rows = random_csr(rng, m, k)
    w = torch.tensor(rng.standard_normal(indices.size), dtype=torch.float64, requires_grad=True)
    dense = _dense_from(w, rows, indices, m, k)
    X = torch.tensor(rng.standard_normal((m if transpose else k, nb)), requires_grad=True)
    g = rng.standard_normal((k if transpose else m, nb))
    y = dense.T @ X if transpose else dense @ X
    y.backward(torch.from_numpy(g))
    P, Q = (X.detach().numpy(), g) if transpose else (g, X.detach().numpy())
    got = model_sddmm(indices, rows, P, Q, torch.float64)
    np.testing.assert_allclose(got.numpy(), w.grad.numpy(), rtol=1e-12, atol=1e-12)
    dX = (dense.detach() @ torch.from_numpy(g)) if transpose else (dense.detach().T @ torch.from_numpy(g))
    np.testing.assert_allclose(dX.numpy(), X.grad.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('transpose', [False, True])
def test_shared_weight_rule_matches_dense_autograd(transpose):
    rng = np.random.default_rng(5 + transpose)
    m, k, nb = 7, 10, 4
    indices, indptr, rows = random_csr(rng, m, k, 0.4)
    w = torch.tensor(1.7, dtype=torch.float64, requires_grad=True)
    dense = _dense_from(w.expand(indices.size), rows, indices, m, k)
    X = torch.tensor(rng.standard_normal((m if transpose else k, nb)))
    g = rng.standard_normal((k if transpose else m, nb))
    (dense.T @ X if transpose else dense @ X).backward(torch.from_numpy(g))
    P, Q = (X.numpy(), g) if transpose else (g, X.numpy())
    assert model_shared(indices, rows, P, Q) == pytest.approx(w.grad.item(), rel=1e-12, abs=1e-12)
    # ... which is the sum of the per-entry rule
    assert model_shared(indices, rows, P, Q) == pytest.approx(model_sddmm(indices, rows, P, Q, torch.float64).sum().item(), rel=1e-12)


# ------------------------------------------------------------------------------------------------ validation without a device
def test_float_needed_follows_grad_mode_and_operand_kind():
    w = torch.ones(4, requires_grad=True)
    x = torch.ones(4, requires_grad=True)
    assert AG.float_needed(w, torch.ones(4))
    assert AG.float_needed(torch.ones(4), x)
    assert not AG.float_needed(torch.ones(4), torch.ones(4))
    assert not AG.float_needed(w, np.ones(4, np.float32))          # numpy operands: numpy results, no autograd
    with torch.no_grad():
        assert not AG.float_needed(w, x)
    assert getattr(AG.FloatRowsProduct.backward, '__wrapped__', None) is not None        # once_differentiable


def test_sddmm_argument_checks_need_no_device():
    A, B = np.ones((3, 2), np.float32), np.ones((2, 4), np.float32)
    with pytest.raises(AssertionError):
        be.sddmm_indices(A[0], B, np.zeros((1, 2), np.int32))                   # A.ndim == 2
    with pytest.raises(AssertionError):
        be.sddmm_indices(A, B[0], np.zeros((1, 2), np.int32))                   # B.ndim == 2
    with pytest.raises(AssertionError):
        be.sddmm_indices(A, np.ones((3, 4), np.float32), np.zeros((1, 2), np.int32))      # A.shape[1] == B.shape[0]
    with pytest.raises(AssertionError):
        be.sddmm_indices(A, B, np.zeros(2, np.int32))                           # indices.ndim == 2
    with pytest.raises(AssertionError):
        be.sddmm_indices(A, B, np.zeros((1, 3), np.int32))                      # indices.shape[1] == 2
    with pytest.raises(AssertionError):
        be.sddmm_coo_indices(A, B, np.zeros((1, 1), np.int32), np.zeros(1, np.int32))     # pre_idx.ndim == 1
    with pytest.raises(AssertionError):
        be.sddmm_coo_indices(A, B, np.zeros(2, np.int32), np.zeros(3, np.int32))          # same shape
    with pytest.raises(AssertionError):
        be.sddmm_coo_indices(A.astype(np.int32), B, np.zeros(2, np.int32), np.zeros(2, np.int32))    # floating operands


def test_sddmm_is_registered_and_exported():
    assert 'sddmm' in be.get_all_primitive_names()
    assert be.sddmm_p.tags == {'coo', 'float'}
    assert be.sddmm_p.available_backends() == ['hip']
    for cls in (be.CSR, be.CSC, be.FixedNumPerPre, be.FixedNumPerPost):
        assert callable(getattr(cls, 'sddmm'))
    assert 'no autodiff' not in (ROOT / 'brainevent_amd' / '_float.py').read_text()


def test_entry_point_is_declared_once_with_14_arguments():
    m = re.findall(r'\bint\s+be_sddmm_rows\s*\(([^;]*?)\)\s*;', HEADER.read_text(), re.S)
    assert len(m) == 1
    assert len(m[0].split(',')) == len(_abi.PROTOTYPES['be_sddmm_rows'][1]) == 14


# ------------------------------------------------------------------------------------------------ the GPU cases' constants
PATTERNS = {
    'threads': r'constexpr int kThreads = (\d+);',
    'tile': r'constexpr int kTile = (\d+);',
    'grid_cap': r'constexpr int kGridCap = (\d+);',
    'vec_bytes': r'constexpr int kVecBytes = (\d+);',
    'max_lanes': r'constexpr int kMaxLanes = (\d+);',
}


def _consts():
    from test_float_autograd_gpu import CONSTS          # (here: that module imports the host model from this one)
    return CONSTS


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(_consts())


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    found = re.findall(PATTERNS[key], SOURCE.read_text())
    assert len(found) == 1, f"{key}: be_sddmm.hip holds /{PATTERNS[key]}/ {len(found)} times"
    assert int(found[0]) == _consts()[key], (f"{key}: be_sddmm.hip says {found[0]}, tests/test_float_autograd_gpu.py assumes "
                                             f"{_consts()[key]}: re-size the cases its docstring lists for this bound")


def test_lane_thresholds_and_grid_are_the_ones_the_cases_assume():
    """lanes_for: 1 lane up to V elements, 2 up to 2 V, 4, 8, kMaxLanes beyond 8 V; the grid is capped over tiles of kTile."""
    text = SOURCE.read_text()
    for pat in (r'if \(nb <= v\) return 1;', r'if \(nb <= 2 \* v\) return 2;', r'if \(nb <= 4 \* v\) return 4;',
                r'if \(nb <= 8 \* v\) return 8;', r'return kMaxLanes;', r'const int64_t v = kVecBytes / elem_bytes;',
                r'grid_for\(nse, kTile, kGridCap\)', r'constexpr int G = kThreads / LPE;', r'u < kTile / G'):
        assert len(re.findall(pat, text)) == 1, pat
    from test_float_autograd_gpu import lanes_for, nb_boundaries
    assert [lanes_for(n, torch.float32) for n in (1, 4, 5, 8, 9, 16, 17, 32, 33, 257)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [lanes_for(n, torch.float64) for n in (1, 2, 3, 4, 5, 8, 9, 16, 17)] == [1, 1, 2, 2, 4, 4, 8, 8, 16]
    assert [lanes_for(n, torch.bfloat16) for n in (8, 9, 16, 17, 32, 33, 64, 65)] == [1, 2, 2, 4, 4, 8, 8, 16]
    assert nb_boundaries(torch.float32) == [1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33]
    assert nb_boundaries(torch.float16)[-3:] == [33, 63, 64]
