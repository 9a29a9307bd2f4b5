"""Spike-triggered plasticity, host side: the host model the GPU tests check against reproduces the reference's known answers,
and the public functions reject bad arguments before any device work (no GPU needed)."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _array, _plasticity


# ------------------------------------------------------------------------------------------------------------ host model
def _clip(w, lo, hi):
    """min(max(w, lo), hi) in w's own dtype (the reference's u.math.clip; NaN stays NaN, lo > hi gives hi)."""
    if isinstance(w, torch.Tensor):
        return torch.clamp(w, min=lo, max=hi) if (lo is not None or hi is not None) else w
    if lo is not None:
        w = np.maximum(w, w.dtype.type(lo))
    if hi is not None:
        w = np.minimum(w, w.dtype.type(hi))
    return w


def model_update(w, pos, tidx, trace, lo=None, hi=None):
    """w[pos] = w[pos] + trace[tidx] (trace cast to w's dtype first, one rounding), then clip the WHOLE array.
    ``w``: numpy (f16 / f32 / f64) or a CPU torch tensor (bf16)."""
    w = w.copy() if isinstance(w, np.ndarray) else w.clone()
    if isinstance(w, np.ndarray):
        tr = np.asarray(trace).astype(w.dtype)
        w[pos] = w[pos] + tr[tidx]
    else:
        tr = torch.as_tensor(np.asarray(trace, dtype=np.float64)).to(w.dtype)
        p, t = torch.as_tensor(pos, dtype=torch.int64), torch.as_tensor(tidx, dtype=torch.int64)
        w[p] = w[p] + tr[t]
    return _clip(w, lo, hi)


def row_of(indptr):
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def model_rows(w, indices, indptr, spikes, trace, lo=None, hi=None):
    """Row-driven: every entry of an active stored row gets + trace[indices[e]]."""
    act = np.asarray(spikes) != 0
    pos = np.nonzero(act[row_of(indptr)])[0]
    return model_update(w, pos, np.asarray(indices, dtype=np.int64)[pos], trace, lo, hi)


def model_cols(w, indices, indptr, spikes, trace, lo=None, hi=None):
    """Column-driven: every entry whose stored column is active gets + trace[row(e)]."""
    act = np.asarray(spikes) != 0
    idx = np.asarray(indices, dtype=np.int64)
    pos = np.nonzero(act[idx])[0]
    return model_update(w, pos, row_of(indptr)[pos], trace, lo, hi)


# ------------------------------------------------------------------------------------------------------------ known answers
def test_model_reproduces_reference_kat_pre():
    # brainevent/_csr/plasticity_binary_test.py:469-481 (int64_structure, _csr/_test_util.py:323-339)
    w = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    got = model_rows(w, [0, 2, 1, 2], [0, 2, 4], [True, False], np.array([0.5, 1.5, 2.5], np.float32))
    np.testing.assert_array_equal(got, np.array([1.5, 4.5, 3.0, 4.0], np.float32))


def test_model_reproduces_reference_kat_post():
    # brainevent/_csr/plasticity_binary_test.py:484-497: CSC arrays (indices = pre ids) + the CSC -> CSR permutation
    w = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    csc_indices, csc_indptr, perm = np.array([0, 1, 0, 1]), np.array([0, 2, 4]), np.array([0, 2, 1, 3])
    act = np.array([False, True])
    slots = np.nonzero(act[row_of(csc_indptr)])[0]
    got = model_update(w, perm[slots], csc_indices[slots], np.array([0.5, 1.5], np.float32))
    np.testing.assert_array_equal(got, np.array([1.0, 2.5, 3.0, 5.5], np.float32))


def test_model_reproduces_docstring_examples():
    # update_csr_on_binary_pre (brainevent/_csr/plasticity_binary.py:141-153)
    got = model_rows(np.array([0.5, 0.3, 0.8, 0.2], np.float32), [0, 1, 0, 2], [0, 2, 4], [True, False],
                     np.array([0.1, 0.2, 0.05], np.float32))
    np.testing.assert_array_equal(got, np.array([0.5, 0.3, 0.8, 0.2], np.float32) + np.array([0.1, 0.2, 0, 0], np.float32))
    # update_fixed_post_conn_on_binary_pre (brainevent/_fcn/plasticity_binary.py:253-261)
    data = np.array([[0.5, 0.3], [0.8, 0.2]], np.float32)
    got = model_rows(data.reshape(-1), [0, 1, 1, 2], [0, 2, 4], [True, False], np.array([0.1, 0.2, 0.05], np.float32))
    np.testing.assert_array_equal(got.reshape(2, 2), np.array([[0.5 + np.float32(0.1), 0.3 + np.float32(0.2)], [0.8, 0.2]],
                                                              np.float32))
    # update_csc_on_binary_pre / _post (brainevent/_csr/plasticity_binary.py:1036-1048, :1136-1148): W = [[.5, 0, .8], [0, .3, .2]]
    W = np.array([[0.5, 0.0, 0.8], [0.0, 0.3, 0.2]], np.float32)
    cols, rows = np.nonzero(W.T)                       # CSC: stored rows = columns, indices = pre ids
    data, indptr = W[rows, cols], np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=3))])
    pre = model_cols(data, rows, indptr, [True, False], np.array([0.1, 0.2, 0.05], np.float32))
    exp = W.copy()
    exp[0, 0] += np.float32(0.1)
    exp[0, 2] += np.float32(0.05)
    np.testing.assert_array_equal(pre, exp[rows, cols])
    post = model_rows(data, rows, indptr, [True, False, True], np.array([0.1, -0.05], np.float32))
    exp = W.copy()
    exp[0, 0] += np.float32(0.1)
    exp[0, 2] += np.float32(0.1)
    exp[1, 2] += np.float32(-0.05)
    np.testing.assert_array_equal(post, exp[rows, cols])


def test_model_clip_order_and_nan():
    w = np.array([np.nan, -1.0, 0.5, 3.0], np.float32)
    np.testing.assert_array_equal(_clip(w, 0.0, 1.0), np.array([np.nan, 0.0, 0.5, 1.0], np.float32))
    np.testing.assert_array_equal(_clip(w, 2.0, 1.0), np.array([np.nan, 1.0, 1.0, 1.0], np.float32))   # w_min > w_max -> w_max
    t = torch.tensor([float('nan'), -1.0, 3.0], dtype=torch.bfloat16)
    assert torch.isnan(_clip(t, 0.0, 1.0)[0]) and _clip(t, 2.0, 1.0)[1:].tolist() == [1.0, 1.0]


# ------------------------------------------------------------------------------------------------------------ validation
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the library or the device fails the test."""
    def boom(*a, **k):
        raise AssertionError("device work before validation")
    monkeypatch.setattr(_plasticity, 'fn', boom)
    monkeypatch.setattr(_array, 'to_device', boom)
    monkeypatch.setattr(_array, 'device', boom)


def _csr_args():
    return (np.ones(4, np.float32), np.array([0, 2, 1, 2], np.int32), np.array([0, 2, 4], np.int32), np.array([True, False]),
            np.ones(3, np.float32))


def test_homogeneous_weight_is_refused(no_device):
    _, idx, ptr, spk, tr = _csr_args()
    for f, args in [(be.update_csr_on_binary_pre, (np.ones(1, np.float32), idx, ptr, spk, tr)),
                    (be.update_csc_on_binary_post, (np.ones(1, np.float32), idx, ptr, np.ones(3, np.float32), np.ones(2, bool))),
                    (be.update_csr_on_binary_post, (np.ones(1, np.float32), idx, np.array([0, 2, 4]), idx,
                                                    np.ones(3, np.float32), np.ones(2, bool)))]:
        with pytest.raises(ValueError, match='per-synapse'):
            f(*args, shape=(2, 3))
    with pytest.raises(ValueError, match='per-synapse'):
        be.update_fixed_post_conn_on_binary_pre(np.ones(1, np.float32), np.zeros((2, 3), np.int32), spk, tr, shape=(2, 3))
    with pytest.raises(ValueError, match='per-synapse'):
        be.update_fixed_pre_conn_on_binary_post(np.float32(1.0), np.zeros((3, 2), np.int32), spk, tr, shape=(2, 3))


def test_shape_mismatch_is_refused(no_device):
    w, idx, ptr, spk, tr = _csr_args()
    with pytest.raises(ValueError):
        be.update_csr_on_binary_pre(w, idx, ptr, np.ones(3, bool), tr, shape=(2, 3))          # pre_spike length
    with pytest.raises(ValueError):
        be.update_csr_on_binary_pre(w, idx, ptr, spk, np.ones(2, np.float32), shape=(2, 3))   # post_trace length
    with pytest.raises(ValueError):
        be.update_csr_on_binary_pre(w[:3], idx, ptr, spk, tr, shape=(2, 3))                  # weight vs indices
    with pytest.raises(ValueError):
        be.update_dense_on_binary_pre(np.ones((2, 3), np.float32), spk, np.ones(4, np.float32))
    with pytest.raises(ValueError):
        be.update_dense_on_binary_post(np.ones((2, 3), np.float32), np.ones(2, np.float32), np.ones(2, bool))
    with pytest.raises(ValueError):
        be.update_fixed_post_conn_on_binary_pre(np.ones((2, 3), np.float32), np.zeros((2, 2), np.int32), spk, tr, shape=(2, 3))


def test_non_scalar_bound_is_refused(no_device):
    w, idx, ptr, spk, tr = _csr_args()
    for bad in (np.array([0.0, 1.0]), [0.0], 'x', torch.zeros(2)):
        with pytest.raises(ValueError):
            be.update_csr_on_binary_pre(w, idx, ptr, spk, tr, bad, None, shape=(2, 3))
        with pytest.raises(ValueError):
            be.update_dense_on_binary_post(np.ones((2, 3), np.float32), np.ones(2, np.float32), np.ones(3, bool), None, bad)


def test_plasticity_names_are_exported():
    for name in _plasticity.__all__:
        assert getattr(be, name) is getattr(_plasticity, name)
    for cls in (be.CSR, be.CSC, be.Dense, be.FixedNumPerPre, be.FixedNumPerPost):
        assert callable(cls.update_on_pre) and callable(cls.update_on_post)
