"""Sampled dense-dense products (SDDMM): the values of ``A @ B`` at the positions of a sparsity pattern, without forming the
``(m, n)`` product — ``out[e] = sum_b A[r(e), b] * B[b, c(e)]``.  A three-factor / e-prop weight update is one
(``dw[j] = sum_t pre_trace[t, r(j)] * learning_signal[t, c(j)]``), and so is the weight gradient of ``csr @ X``
(``_autograd.FloatRowsProduct`` calls :func:`sddmm_rows`).

Reference surface (read as text): ``brainevent/_sddmm.py`` (``sddmm_indices``, ``sddmm_coo_indices``, ``sddmm_bcoo``).  Names and
argument checks follow it; two differences:

* this project has no BCOO container: the functions return the sampled **values** as a ``[nse]`` array in ``A``'s dtype, in the
  order of the given positions (the reference wraps the same values and ``indices`` in a ``BCOO``), and there is no
  ``sddmm_bcoo``.  On a stored matrix use ``M.sddmm(A, B)`` (CSR, CSC, ``FixedNumPerPre``, ``FixedNumPerPost``), which returns
  ``M.with_data(values)``: the structure arrays are shared, not copied;
* the result has ``A``'s dtype and ``B`` is cast to it (the float-operand rule, ``_float.py``).

All of it runs on one kernel (``csrc/be_sddmm.hip``, ``be_sddmm_rows``): per entry, f32 (f64) accumulation, one rounding, every
entry written once, no atomics; the order of an entry's sum depends on ``nb`` and the dtype only, so the CSR, fixed-number and
COO readings of one matrix agree bit for bit.  ``B`` is transposed to neuron-major (``[n, nb]``) once on the host side of the
call.  No autograd through these functions themselves (tensors that require grad are taken by value)."""
import numpy as np
import torch

from . import _array as A
from ._error import UnsupportedOperationError
from ._lib import call
from ._misc import _as_int32_indices
from ._op import OpKernel

__all__ = ['sddmm_indices', 'sddmm_coo_indices', 'sddmm_p', 'sddmm_p_call', 'sddmm_rows']


def sddmm_rows(indices, indptr, row_len: int, row_ids, n_rows: int, n_cols: int, P, Q) -> torch.Tensor:
    """``be_sddmm_rows``: ``out[e] = sum_b P[r(e), b] * Q[indices[e], b]`` as a flat ``[nse]`` tensor in ``P``'s dtype.  ``P
    [n_rows, nb]`` and ``Q [n_cols, nb]`` are neuron-major device tensors (made contiguous here; ``Q`` is cast to ``P``'s
    dtype); the row of an entry comes from ``row_ids`` (int32 ``[nse]``), else ``indptr`` (int32 / int64), else ``row_len``."""
    P = P.detach().contiguous()
    Q = Q.detach().to(P.dtype).contiguous()
    nb = int(P.shape[1])
    assert tuple(P.shape) == (n_rows, nb) and tuple(Q.shape) == (n_cols, nb), (
        f"sddmm operands {tuple(P.shape)} / {tuple(Q.shape)} do not match ({n_rows}, nb) / ({n_cols}, nb)")
    idx = indices.reshape(-1).contiguous()
    row_ids = None if row_ids is None else row_ids.contiguous()
    nse = int(idx.numel())
    out = torch.empty(nse, dtype=P.dtype, device=A.device())
    if nse == 0 or n_rows == 0:
        return out
    if nb == 0:                             # an empty sum per entry
        return out.zero_()
    is64 = int(indptr is not None and indptr.dtype == torch.int64)
    call('be_sddmm_rows', A.ptr(out), A.wcode(P), A.ptr(idx), A.ptr(indptr), is64, int(row_len), A.ptr(row_ids), int(n_rows),
         int(n_cols), nse, A.ptr(P), A.ptr(Q), nb, A.stream_ptr())
    return out


def _neuron_major(B_mat, dtype) -> torch.Tensor:
    """``B [nb, n]`` as the view ``[n, nb]`` on the device: :func:`sddmm_rows` makes it contiguous — the one transposing copy
    of the call (none when ``B`` already is the transpose of a contiguous ``[n, nb]`` array)."""
    t = B_mat if isinstance(B_mat, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(B_mat)))
    return t.detach().to(device=A.device(), dtype=dtype).T


def _sddmm_hip(A_mat, B_mat, pre_idx, post_idx):
    """``A [m, k]``, ``B [k, n]``, positions ``(pre_idx[e], post_idx[e])`` (int32 device tensors) -> ``[nse]``."""
    a = A.to_device(A_mat)
    b_nm = _neuron_major(B_mat, a.dtype)
    return sddmm_rows(post_idx, None, -1, pre_idx, int(a.shape[0]), int(b_nm.shape[0]), a, b_nm)


sddmm_p = OpKernel('sddmm')
sddmm_p.def_kernel('hip', 'gpu', _sddmm_hip, asdefault=True)
sddmm_p.def_tags('coo', 'float')


def _arr(x):
    return x if isinstance(x, torch.Tensor) else np.asarray(x)


def _is_floating(x) -> bool:
    return x.dtype.is_floating_point if isinstance(x, torch.Tensor) else np.issubdtype(x.dtype, np.floating)


def _check_dense(A_mat, B_mat) -> None:
    assert A_mat.ndim == 2, "A must be 2D (m, k)."
    assert B_mat.ndim == 2, "B must be 2D (k, n)."
    assert A_mat.shape[1] == B_mat.shape[0], f"A {tuple(A_mat.shape)} and B {tuple(B_mat.shape)} do not contract."
    assert _is_floating(A_mat) and _is_floating(B_mat), "A and B must be floating-point arrays."


def sddmm_p_call(A_mat, B_mat, pre_idx, post_idx, *, backend=None):
    """Validate (the reference's assertions, ``brainevent/_sddmm.py:67-71``, ``:116-119``; positions range-checked by the rules
    of the constructors, ``_as_int32_indices``), then dispatch.  Returns a 1-list."""
    A_mat, B_mat, pre_idx, post_idx = _arr(A_mat), _arr(B_mat), _arr(pre_idx), _arr(post_idx)
    assert pre_idx.ndim == 1, "pre_idx must be 1D."
    assert post_idx.ndim == 1, "post_idx must be 1D."
    _check_dense(A_mat, B_mat)
    assert tuple(pre_idx.shape) == tuple(post_idx.shape), "pre_idx and post_idx must have the same shape."
    pre = _as_int32_indices(A.to_device(pre_idx), int(A_mat.shape[0]), 'sddmm pre_idx')
    post = _as_int32_indices(A.to_device(post_idx), int(B_mat.shape[1]), 'sddmm post_idx')
    return [sddmm_p(A_mat, B_mat, pre, post, backend=backend)]


sddmm_p.def_call(sddmm_p_call)


def sddmm_coo_indices(A_mat, B_mat, pre_idx, post_idx, *, backend=None):
    """``(A @ B)[pre_idx[e], post_idx[e]]`` for every ``e`` (reference ``brainevent/_sddmm.py:83-121``): ``A (m, k)``, ``B (k,
    n)``, two 1-D integer arrays of one length.  Returns the values, ``(nse,)`` in ``A``'s dtype — the reference returns a BCOO
    holding them; this project has no BCOO container.  numpy in gives numpy out."""
    as_np = A.wants_numpy(A_mat, B_mat, pre_idx, post_idx)
    return A.to_result(sddmm_p_call(A_mat, B_mat, pre_idx, post_idx, backend=backend)[0], as_np)


def sddmm_indices(A_mat, B_mat, indices, *, backend=None):
    """``(A @ B)[indices[e, 0], indices[e, 1]]`` for every ``e`` (reference ``brainevent/_sddmm.py:31-79``): ``indices (nse,
    2)`` holds ``(row, col)`` pairs.  Returns the values, ``(nse,)`` in ``A``'s dtype (no BCOO container here, see the module
    docstring).  numpy in gives numpy out."""
    A_mat, B_mat, indices = _arr(A_mat), _arr(B_mat), _arr(indices)
    _check_dense(A_mat, B_mat)
    assert indices.ndim == 2, "indices must be 2D (nse, 2)."
    assert indices.shape[1] == 2, "indices must be (nse, 2)."
    return sddmm_coo_indices(A_mat, B_mat, indices[:, 0], indices[:, 1], backend=backend)


# ------------------------------------------------------------------------------------------------ containers
def container_sddmm(M, A_mat, B_mat):
    """``M.sddmm(A, B)``: ``A @ B`` sampled on ``M``'s pattern, as ``M.with_data(values)``.  ``A (M.shape[0], nb)``, ``B (nb,
    M.shape[1])``.  CSR / ``FixedNumPerPre`` store the rows (``P = A``, ``Q = B.T``); CSC / ``FixedNumPerPost`` store the
    transpose (``P = B.T``, ``Q = A``)."""
    A_mat, B_mat = _arr(A_mat), _arr(B_mat)
    _check_dense(A_mat, B_mat)
    assert int(A_mat.shape[0]) == int(M.shape[0]), f"A has {A_mat.shape[0]} rows, the matrix {M.shape[0]}."
    assert int(B_mat.shape[1]) == int(M.shape[1]), f"B has {B_mat.shape[1]} columns, the matrix {M.shape[1]}."
    if M.data.numel() == 1 and M.nse != 1:
        raise UnsupportedOperationError(
            f"{type(M).__name__}.sddmm: this matrix holds one shared weight, so it has no per-entry data to return. Build it "
            "with per-entry weights (data shaped like indices), or use sddmm_coo_indices for the bare values.")
    rows = M._stored_rows()
    a = A.to_device(A_mat, dtype=M.data.dtype)
    b_nm = _neuron_major(B_mat, M.data.dtype)
    P, Q = (b_nm, a) if M._stored_transposed else (a, b_nm)
    values = sddmm_rows(rows.indices, rows.indptr, rows.row_len, None, rows.m, rows.k, P, Q)
    return M.with_data(values.reshape(M.data.shape))
