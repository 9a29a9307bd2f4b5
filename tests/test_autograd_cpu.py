"""Host model of the autograd rules (brainevent_amd/_autograd.py, csrc/be_grad.hip), checked against torch autograd on dense
CPU tensors, plus the validation that needs no device.  The GPU tests compare the kernels against these models bit for bit."""
import numpy as np
import pytest
import torch

from brainevent_amd import _autograd as AG
from brainevent_amd._event import BinaryArray, BitPackedBinary


# ------------------------------------------------------------------------------------------------ the host model
def active(s_bm: np.ndarray) -> np.ndarray:
    """The product's spike rule: != 0 for bool / integer spikes, > 0 for float spikes."""
    s_bm = np.asarray(s_bm)
    return s_bm > 0 if np.issubdtype(s_bm.dtype, np.floating) else s_bm != 0


def acc_dtype(wdtype: torch.dtype):
    return np.float64 if wdtype == torch.float64 else np.float32


def round_to(acc: np.ndarray, wdtype: torch.dtype) -> torch.Tensor:
    """One rounding of the accumulator to the weight dtype (round to nearest even, as the kernels do)."""
    return torch.from_numpy(np.ascontiguousarray(acc)).to(wdtype)


def row_of(indptr: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def model_rows_dw(indices, rows, transpose: bool, act_bm, g_bm, wdtype: torch.dtype) -> torch.Tensor:
    """Per-entry weight gradient.  ``transpose`` (s @ A): dw[j] = sum_b a[b, r(j)] g[b, c(j)]; else dw[j] = sum_b g[b, r(j)]
    a[b, c(j)].  ``act_bm [nb, n_spk]`` bool, ``g_bm [nb, n_out]`` in the weight dtype (as float64 values).  Sum in f32 (f64
    for f64) over the active b only, ascending b, rounded once."""
    ad = acc_dtype(wdtype)
    indices = np.asarray(indices).reshape(-1).astype(np.int64)
    rows = np.asarray(rows).astype(np.int64)
    sidx, gidx = (rows, indices) if transpose else (indices, rows)
    acc = np.zeros(indices.shape[0], dtype=ad)
    g_bm = np.asarray(g_bm, dtype=np.float64)
    for b in range(act_bm.shape[0]):
        on = act_bm[b, sidx]
        acc[on] = acc[on] + g_bm[b, gidx[on]].astype(ad)
    return round_to(acc, wdtype)


def model_rows_homo(indices, rows, transpose: bool, act_bm, g_bm) -> float:
    """Shared weight: the f64 sum over every entry of the per-entry rule."""
    indices = np.asarray(indices).reshape(-1).astype(np.int64)
    rows = np.asarray(rows).astype(np.int64)
    sidx, gidx = (rows, indices) if transpose else (indices, rows)
    a = act_bm[:, sidx].astype(np.float64)
    return float((a * np.asarray(g_bm, np.float64)[:, gidx]).sum())


def model_dense_dw(transpose: bool, act_bm, g_bm, wdtype: torch.dtype) -> torch.Tensor:
    """``transpose`` (s @ W, W [R, C]): dW[i, j] = sum_b a[b, i] g[b, j]; else (W @ s): dW[i, j] = sum_b g[b, i] a[b, j]."""
    ad = acc_dtype(wdtype)
    g_bm = np.asarray(g_bm, dtype=np.float64)
    nb = act_bm.shape[0]
    if transpose:
        acc = np.zeros((act_bm.shape[1], g_bm.shape[1]), dtype=ad)
        for b in range(nb):
            acc[act_bm[b]] = acc[act_bm[b]] + g_bm[b].astype(ad)[None, :]
    else:
        acc = np.zeros((g_bm.shape[1], act_bm.shape[1]), dtype=ad)
        for b in range(nb):
            acc[:, act_bm[b]] = acc[:, act_bm[b]] + g_bm[b].astype(ad)[:, None]
    return round_to(acc, wdtype)


def random_csr(rng, m, k, density=0.3):
    mask = rng.random((m, k)) < density
    rows, cols = np.nonzero(mask)
    indptr = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=indptr[1:])
    return cols.astype(np.int32), indptr, rows


# ------------------------------------------------------------------------------------------------ model vs torch autograd
@pytest.mark.parametrize('transpose', [True, False])
@pytest.mark.parametrize('nb', [1, 3, 33])
def test_rows_model_matches_dense_autograd(transpose, nb):
    rng = np.random.default_rng(nb + 7 * transpose)
    m, k = 9, 13
    indices, indptr, rows = random_csr(rng, m, k)
    w = torch.tensor(rng.standard_normal(indices.size), dtype=torch.float64, requires_grad=True)
    dense = torch.zeros(m, k, dtype=torch.float64).index_put((torch.from_numpy(rows), torch.from_numpy(indices.astype(np.int64))), w)
    s = (rng.random((nb, m if transpose else k)) < 0.4).astype(np.float64)
    g = rng.standard_normal((nb, k if transpose else m))
    y = torch.from_numpy(s) @ dense if transpose else torch.from_numpy(s) @ dense.T
    y.backward(torch.from_numpy(g))
    got = model_rows_dw(indices, rows, transpose, active(s), g, torch.float64)
    np.testing.assert_allclose(got.numpy(), w.grad.numpy(), rtol=1e-12, atol=1e-12)
    homo = model_rows_homo(indices, rows, transpose, active(s), g)
    assert homo == pytest.approx(float(w.grad.sum()), rel=1e-12, abs=1e-12)


@pytest.mark.parametrize('transpose', [True, False])
def test_dense_model_matches_dense_autograd(transpose):
    rng = np.random.default_rng(3)
    R, C, nb = 7, 5, 4
    W = torch.tensor(rng.standard_normal((R, C)), requires_grad=True)
    s = (rng.random((nb, R if transpose else C)) < 0.5).astype(np.float64)
    g = rng.standard_normal((nb, C if transpose else R))
    y = torch.from_numpy(s) @ W if transpose else torch.from_numpy(s) @ W.T
    y.backward(torch.from_numpy(g))
    got = model_dense_dw(transpose, active(s), g, torch.float64)
    np.testing.assert_allclose(got.numpy(), W.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_non_binary_float_spikes_use_activity_not_values():
    """The documented divergence from the reference's transpose rule: a float spike of 0.5 counts as 1 (the forward product
    is linear in the weights with coefficient active(s)), a negative one as 0."""
    rng = np.random.default_rng(5)
    m, k = 6, 8
    indices, indptr, rows = random_csr(rng, m, k, 0.5)
    s = np.array([[0.5, -1.0, 2.0, 0.0, 0.25, 1.0]])
    g = rng.standard_normal((1, k))
    got = model_rows_dw(indices, rows, True, active(s), g, torch.float64).numpy()
    w = torch.tensor(rng.standard_normal(indices.size), requires_grad=True)
    dense = torch.zeros(m, k, dtype=torch.float64).index_put((torch.from_numpy(rows), torch.from_numpy(indices.astype(np.int64))), w)
    (torch.from_numpy(active(s).astype(np.float64)) @ dense).backward(torch.from_numpy(g))
    np.testing.assert_array_equal(got, w.grad.numpy())
    raw = g[0, indices] * s[0, rows]           # the reference's transpose rule (values, not activity)
    assert not np.allclose(got, raw)
    on = s[0, rows] == 1.0
    np.testing.assert_array_equal(got[on], raw[on])     # ... agrees where the spike is exactly 1


def test_model_sums_in_f32_ascending_and_rounds_once():
    g = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=np.float64)     # f32: 1 + 2^-24 + 2^-24 = 1 (ascending order)
    a = np.ones((3, 1), bool)
    got = model_rows_dw(np.array([0]), np.array([0]), True, a, g, torch.float32)
    assert got.item() == 1.0
    got16 = model_rows_dw(np.array([0]), np.array([0]), True, a, np.array([[1.0], [2.0 ** -11], [2.0 ** -11]]), torch.float16)
    assert got16.item() == 1.0 + 2.0 ** -10         # f32 accumulation, one rounding to f16


# ------------------------------------------------------------------------------------------------ validation without a device
def test_numpy_and_bool_spikes_never_need_a_gradient():
    assert not AG.needed(np.ones(3, np.float32), np.zeros(3, bool))
    with pytest.raises(RuntimeError):
        torch.zeros(3, dtype=torch.bool, requires_grad=True)         # bool spikes cannot require grad at all
    assert AG.diff_spikes(torch.zeros(3, dtype=torch.bool)) is None
    assert AG.diff_spikes(np.ones(3, np.float32)) is None


def test_needed_follows_grad_mode_and_operands():
    w = torch.ones(4, requires_grad=True)
    s = torch.ones(4, requires_grad=True)
    assert AG.needed(w, np.zeros(4))
    assert AG.needed(torch.ones(4), BinaryArray(s))
    assert AG.diff_spikes(BinaryArray(s)) is s
    assert not AG.needed(torch.ones(4), BinaryArray(torch.ones(4)))
    with torch.no_grad():
        assert not AG.needed(w, s)
    # a bit-packed container is not differentiable: only its weights can get a gradient
    assert AG.diff_spikes(BitPackedBinary(np.array([1, 0, 1], bool))) is None


def test_once_differentiable():
    assert getattr(AG.RowsProduct.backward, '__wrapped__', None) is not None
    assert getattr(AG.DenseProduct.backward, '__wrapped__', None) is not None
