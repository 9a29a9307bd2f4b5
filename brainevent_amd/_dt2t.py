"""The per-synapse products (the reference's *dt2t* family): one output per stored entry, ``out[j] = w[j] * y[row(j)]`` or
``w[j] * y[indices[j]]`` — the ``D^t e^{t-1}`` term of a D-RTRL eligibility-trace update, and the general way to scale a
per-synapse state (trace, conductance, short-term plasticity variable) kept beside ``csr.data`` by a per-neuron factor.

Reference surface (read as text): ``brainevent/_csr/dt2t.py:42-136`` (``csrmv_dt2t``), ``:139-234`` (``cscmv_dt2t``),
``:392-505`` (``csrmv_dt2t_p_call``), ``:545-648`` (``csrmm_dt2t``), ``:651-760`` (``cscmm_dt2t``), ``:902-1030``
(``csrmm_dt2t_p_call``); ``brainevent/_fcn/dt2t.py:33-175`` (``fcnmv_dt2t``), ``:179-344`` (``fcnmm_dt2t``); the container
methods ``_csr/main.py:1816-1886`` / ``:2736-2809`` and ``_fcn/main.py:359-418``.

  csr*_dt2t, transpose=False: ``y`` is indexed by the row of the entry     (``y`` has ``shape[0]`` elements per batch row)
  csr*_dt2t, transpose=True : ``y`` is indexed by the stored index         (``shape[1]`` elements)
  fcn*_dt2t: the same two senses (``transpose=False``: the row) — the reference's convention, the opposite of ``fcnmv``'s

All of it runs through one kernel file (``csrc/be_dt2t.hip``, ``be_dt2t``): a stream over the entries, balanced per entry
whatever the row lengths.  Deviations from the reference, both this project's rules:

* the result has the weights' dtype and ``y`` is cast to it (the float-operand rule, ``_float.py``); the CSR functions keep
  the reference's assertion that ``y`` and ``w`` already share a dtype, the ``fcn`` functions cast instead of promoting;
* ``out=``: a device tensor of the result's shape and dtype that is written and returned — ``out=w`` updates a trace in
  place, with no second array of the matrix's size.  A view that starts off a 16-byte boundary (``data[1:]``) is taken as
  it is: nothing is cloned.

No autograd: the reference defines forward-mode rules only ("the transpose rule is not yet implemented") and D-RTRL does not
back-propagate through the trace, so tensors that require grad are taken by value, as the float twins take them.  The
JIT-connectivity twins ``jit{s,u,n}mv_dt2t`` live in ``_jitc.py``."""
from typing import Optional

import numpy as np
import torch

from . import _array as A
from ._lib import call
from ._misc import _as_indptr, _as_int32_indices
from ._op import OpKernel

__all__ = ['csrmv_dt2t', 'csrmm_dt2t', 'cscmv_dt2t', 'cscmm_dt2t', 'fcnmv_dt2t', 'fcnmm_dt2t',
           'csrmv_dt2t_p', 'csrmm_dt2t_p', 'fcnmv_dt2t_p', 'fcnmm_dt2t_p',
           'csrmv_dt2t_p_call', 'csrmm_dt2t_p_call', 'fcnmv_dt2t_p_call', 'fcnmm_dt2t_p_call']


# ------------------------------------------------------------------------------------------------ operands, host or device
def _arr(x):
    """A tensor as it is, anything else as a numpy array: enough for the validators (``ndim`` / ``shape`` / ``dtype``)."""
    return x if isinstance(x, torch.Tensor) else np.asarray(x)


def _dtype_name(x) -> str:
    return str(x.dtype).replace('torch.', '')


def _is_floating(x) -> bool:
    return x.dtype.is_floating_point if isinstance(x, torch.Tensor) else np.issubdtype(x.dtype, np.floating)


def _is_integer(x) -> bool:
    if isinstance(x, torch.Tensor):
        return not (x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool)
    return np.issubdtype(x.dtype, np.integer)


def _size(x) -> int:
    return int(np.prod(tuple(x.shape))) if x.ndim else 1


def _check_out(out, shape, dtype_name: str) -> None:
    """``out=`` is written on the device, in place: a contiguous device tensor of exactly the result's shape and dtype."""
    if out is None:
        return
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"out must be a device tensor (it is written in place), got {type(out).__name__}.")
    if tuple(out.shape) != tuple(shape) or _dtype_name(out) != dtype_name:
        raise ValueError(f"out must have shape {tuple(shape)} and dtype {dtype_name}, got {tuple(out.shape)} and "
                         f"{_dtype_name(out)}.")
    if not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor on the device.")


def _launch(w, homo, y, indices, indptr, row_len, out, n_rows, n_cols, n_batch, nnz, by_col) -> None:
    is64 = int(indptr is not None and indptr.dtype == torch.int64)
    call('be_dt2t', A.ptr(w), int(homo), A.wcode(w), A.ptr(y), A.ptr(indices), A.ptr(indptr), is64, int(row_len), A.ptr(out),
         int(n_rows), int(n_cols), int(n_batch), int(nnz), int(by_col), A.stream_ptr())


def _product(w, y, indices, indptr, row_len, *, n_rows, n_cols, n_batch, nnz, by_col, result_shape, out):
    """``w`` (flat per batch row, or one shared value) times ``y [n_batch, n_rows | n_cols]`` into ``out`` or a new tensor."""
    w = A.to_device(w).detach()
    y = A.to_device(y, dtype=w.dtype).detach()
    homo = w.numel() == 1
    res = out if out is not None else torch.empty(result_shape, dtype=w.dtype, device=A.device())
    if nnz == 0 or n_batch == 0:
        return res
    _launch(w, homo, y, indices, indptr, row_len, res, n_rows, n_cols, n_batch, nnz, by_col)
    return res


# ------------------------------------------------------------------------------------------------ CSR / CSC
def _csr_dt2t_hip(y, w, indices, indptr, *, shape, transpose, out=None):
    """``y [m | k]``, ``w [nse]`` -> ``[nse]``; ``y [n_batch, m | k]``, ``w [n_batch, nse]`` -> ``[n_batch, nse]``."""
    idx = A.to_device(indices)
    if idx.dtype != torch.int32:
        idx = _as_int32_indices(idx, None, 'csr_dt2t', check_values=False)
    ptr_ = None
    if not transpose:                           # (by the stored index, the rows are not looked at)
        ptr_ = A.to_device(indptr)
        if ptr_.dtype not in (torch.int32, torch.int64):
            ptr_ = _as_indptr(ptr_, idx.shape[0], 'auto', 'csr_dt2t')
    n_batch = 1 if w.ndim == 1 else int(w.shape[0])
    return _product(w, y, idx, ptr_, -1, n_rows=int(shape[0]), n_cols=int(shape[1]), n_batch=n_batch, nnz=int(idx.shape[0]),
                    by_col=bool(transpose), result_shape=tuple(w.shape), out=out)


csrmv_dt2t_p = OpKernel('csrmv_dt2t')
csrmv_dt2t_p.def_kernel('hip', 'gpu', _csr_dt2t_hip, asdefault=True)
csrmv_dt2t_p.def_tags('csr', 'float')
csrmm_dt2t_p = OpKernel('csrmm_dt2t')
csrmm_dt2t_p.def_kernel('hip', 'gpu', _csr_dt2t_hip, asdefault=True)
csrmm_dt2t_p.def_tags('csr', 'float')


def _check_csr_dt2t(y, w, indices, indptr, shape, transpose, matrix: bool) -> None:
    """The reference's assertions (``_csr/dt2t.py:477-490``, ``:1000-1018``), on host or device arrays alike."""
    assert _dtype_name(y) == _dtype_name(w), f"y and w must have the same dtype, but got {y.dtype} and {w.dtype}."
    assert indptr.ndim == 1, "Indptr must be 1D."
    assert indices.ndim == 1, "Indices must be 1D."
    if matrix:
        assert y.ndim == 2, "y must be 2D (batch, vector)."
        assert w.ndim == 2, "w must be 2D (batch, nse)."
    else:
        assert y.ndim == w.ndim == 1, "y and w must have the same shape."
    assert _is_integer(indices), "Indices must be an integer type."
    assert _is_integer(indptr), "indptr must be an integer type."
    assert _is_floating(w), 'Weights must be a floating-point type.'
    if matrix:
        assert w.shape[0] == y.shape[0], f"Batch mismatch, y has batch {y.shape[0]} but w has batch {w.shape[0]}."
    assert tuple(w.shape[-1:]) == tuple(indices.shape), (
        f"Weights shape mismatch, expected {tuple(indices.shape)}, got {tuple(w.shape[-1:])}.")
    if transpose:
        assert shape[1] == y.shape[-1], "Shape mismatch for transpose operation."
    else:
        assert shape[0] == y.shape[-1], "Shape mismatch for non-transpose operation."
        assert indptr.shape[0] == shape[0] + 1, f"indptr must have shape[0] + 1 = {shape[0] + 1} entries, got {indptr.shape[0]}."


def csrmv_dt2t_p_call(y, w, indices, indptr, *, shape, transpose, backend=None, out=None):
    """Validate, then dispatch (reference ``brainevent/_csr/dt2t.py:392-505``).  Returns a 1-list."""
    y, w, indices, indptr = _arr(y), _arr(w), _arr(indices), _arr(indptr)
    _check_csr_dt2t(y, w, indices, indptr, shape, transpose, matrix=False)
    _check_out(out, w.shape, _dtype_name(w))
    return [csrmv_dt2t_p(y, w, indices, indptr, shape=tuple(shape), transpose=transpose, out=out, backend=backend)]


def csrmm_dt2t_p_call(y, w, indices, indptr, *, shape, transpose, backend=None, out=None):
    """Validate, then dispatch the batched op (reference ``brainevent/_csr/dt2t.py:902-1030``).  Returns a 1-list."""
    y, w, indices, indptr = _arr(y), _arr(w), _arr(indices), _arr(indptr)
    _check_csr_dt2t(y, w, indices, indptr, shape, transpose, matrix=True)
    _check_out(out, w.shape, _dtype_name(w))
    return [csrmm_dt2t_p(y, w, indices, indptr, shape=tuple(shape), transpose=transpose, out=out, backend=backend)]


csrmv_dt2t_p.def_call(csrmv_dt2t_p_call)
csrmm_dt2t_p.def_call(csrmm_dt2t_p_call)


def csrmv_dt2t(y, w, indices, indptr, *, shape, transpose: bool = False, backend: Optional[str] = None, out=None):
    """``out[j] = w[j] * y[row(j)]`` (``transpose=False``; ``y`` has ``shape[0]`` elements) or ``w[j] * y[indices[j]]``
    (``transpose=True``; ``shape[1]`` elements) for every stored entry ``j`` of a CSR matrix (reference
    ``brainevent/_csr/dt2t.py:42-136``).  ``y`` and ``w`` share a floating dtype; the result is ``(nse,)`` in that dtype.
    ``out=``: a device tensor to write and return instead of a new one — may be ``w`` itself."""
    as_np = out is None and A.wants_numpy(y, w, indices, indptr)
    res = csrmv_dt2t_p_call(y, w, indices, indptr, shape=tuple(shape), transpose=transpose, backend=backend, out=out)[0]
    return A.to_result(res, as_np)


def csrmm_dt2t(y, w, indices, indptr, *, shape, transpose: bool = False, backend: Optional[str] = None, out=None):
    """Batched :func:`csrmv_dt2t` (reference ``brainevent/_csr/dt2t.py:545-648``): ``y (n_batch, shape[0] | shape[1])``,
    ``w (n_batch, nse)`` -> ``(n_batch, nse)``, ``out[b, j] = w[b, j] * y[b, row(j) | indices[j]]``."""
    as_np = out is None and A.wants_numpy(y, w, indices, indptr)
    res = csrmm_dt2t_p_call(y, w, indices, indptr, shape=tuple(shape), transpose=transpose, backend=backend, out=out)[0]
    return A.to_result(res, as_np)


def cscmv_dt2t(y, w, indices, indptr, *, shape, transpose: bool = False, backend: Optional[str] = None, out=None):
    """The CSC counterpart (reference ``brainevent/_csr/dt2t.py:139-234``): the CSC arrays of ``W (m, k)`` are the CSR arrays of
    ``W.T``, so ``transpose=False`` (``y`` indexed by the row of ``W``, the stored index) forwards to :func:`csrmv_dt2t` with
    the shape reversed and the flag flipped."""
    return csrmv_dt2t(y, w, indices, indptr, shape=tuple(shape)[::-1], transpose=not transpose, backend=backend, out=out)


def cscmm_dt2t(y, w, indices, indptr, *, shape, transpose: bool = False, backend: Optional[str] = None, out=None):
    """Batched :func:`cscmv_dt2t` (reference ``brainevent/_csr/dt2t.py:651-760``)."""
    return csrmm_dt2t(y, w, indices, indptr, shape=tuple(shape)[::-1], transpose=not transpose, backend=backend, out=out)


# ------------------------------------------------------------------------------------------------ fixed-number connectivity
def _fcn_dt2t_hip(weights, indices, y, *, shape, transpose, out=None):
    """``indices [rows, n_conn]``; ``y [len]`` -> ``[rows, n_conn]``, ``y [n_batch, len]`` -> ``[n_batch, rows, n_conn]``."""
    idx = A.to_device(indices)
    if idx.dtype != torch.int32:
        idx = _as_int32_indices(idx.reshape(-1), None, 'fcn_dt2t', check_values=False).reshape(idx.shape)
    rows, n_conn = int(idx.shape[0]), int(idx.shape[1])
    batched = y.ndim == 2
    n_batch = int(y.shape[0]) if batched else 1
    return _product(weights, y, idx, None, n_conn, n_rows=int(shape[0]), n_cols=int(shape[1]), n_batch=n_batch,
                    nnz=rows * n_conn, by_col=bool(transpose), result_shape=((n_batch, rows, n_conn) if batched else (rows, n_conn)),
                    out=out)


fcnmv_dt2t_p = OpKernel('fcnmv_dt2t')
fcnmv_dt2t_p.def_kernel('hip', 'gpu', _fcn_dt2t_hip, asdefault=True)
fcnmv_dt2t_p.def_tags('fcn', 'float')
fcnmm_dt2t_p = OpKernel('fcnmm_dt2t')
fcnmm_dt2t_p.def_kernel('hip', 'gpu', _fcn_dt2t_hip, asdefault=True)
fcnmm_dt2t_p.def_tags('fcn', 'float')


def _check_fcn_dt2t(weights, indices, y, shape, transpose, matrix: bool) -> None:
    """The reference's errors, in its order (``_fcn/dt2t.py:149-171``, ``:314-338``) — plus the one this layout adds: the
    stored rows are the rows of ``shape``."""
    if indices.ndim != 2:
        raise ValueError(f"indices must be 2D, got {indices.ndim}D.")
    if len(shape) != 2:
        raise ValueError(f"shape must be length-2, got {shape!r}.")
    if not _is_floating(weights):
        raise ValueError(f"weights must be a floating-point type, got {weights.dtype}.")
    if not matrix:
        if _size(weights) != 1 and tuple(weights.shape) != tuple(indices.shape):
            raise ValueError(f"weights must be size-1 or match indices shape {tuple(indices.shape)}, got {tuple(weights.shape)}.")
        if y.ndim != 1:
            raise ValueError(f"y must be 1D, got {y.ndim}D.")
    elif y.ndim != 2:
        raise ValueError(f"y must be 2D (batch, vector), got {y.ndim}D.")
    expected_y = shape[1] if transpose else shape[0]
    if y.shape[-1] != expected_y:
        raise ValueError(f"y {'trailing dimension' if matrix else 'length'} {y.shape[-1]} does not match expected {expected_y} "
                         f"for transpose={transpose} and shape={tuple(shape)}.")
    if matrix:
        want = (int(y.shape[0]),) + tuple(indices.shape)
        if _size(weights) != 1 and tuple(weights.shape) != want:
            raise ValueError(f"weights must be size-1 or have shape {want}, got {tuple(weights.shape)}.")
    if int(indices.shape[0]) != int(shape[0]):
        raise ValueError(f"indices has {indices.shape[0]} rows, shape[0] is {shape[0]}.")
    if not _is_integer(indices):
        raise ValueError(f"indices must be an integer type, got {indices.dtype}.")


def fcnmv_dt2t_p_call(weights, indices, y, *, shape, transpose, backend=None, out=None):
    """Validate, then dispatch.  Returns a 1-list."""
    weights, indices, y = _arr(weights), _arr(indices), _arr(y)
    _check_fcn_dt2t(weights, indices, y, shape, transpose, matrix=False)
    _check_out(out, tuple(indices.shape), _dtype_name(weights))
    return [fcnmv_dt2t_p(weights, indices, y, shape=tuple(shape), transpose=transpose, out=out, backend=backend)]


def fcnmm_dt2t_p_call(weights, indices, y, *, shape, transpose, backend=None, out=None):
    """Validate, then dispatch the batched op.  Returns a 1-list."""
    weights, indices, y = _arr(weights), _arr(indices), _arr(y)
    _check_fcn_dt2t(weights, indices, y, shape, transpose, matrix=True)
    _check_out(out, (int(y.shape[0]),) + tuple(indices.shape), _dtype_name(weights))
    return [fcnmm_dt2t_p(weights, indices, y, shape=tuple(shape), transpose=transpose, out=out, backend=backend)]


fcnmv_dt2t_p.def_call(fcnmv_dt2t_p_call)
fcnmm_dt2t_p.def_call(fcnmm_dt2t_p_call)


def fcnmv_dt2t(weights, indices, y, *, shape, transpose: bool, backend: Optional[str] = None, out=None):
    """``out[i, c] = weights[i, c] * y[i]`` (``transpose=False``; ``y`` has ``shape[0]`` elements) or ``weights[i, c] *
    y[indices[i, c]]`` (``transpose=True``; ``shape[1]`` elements) for fixed-number connectivity ``indices (rows, n_conn)``
    (reference ``brainevent/_fcn/dt2t.py:33-175``).  ``weights`` match ``indices`` or hold one shared value; the result is
    shaped like ``indices`` either way.  Unlike the reference, which promotes, ``y`` is cast to the weights' dtype and the
    result has that dtype.  ``out=``: a device tensor to write and return — may be ``weights`` itself."""
    as_np = out is None and A.wants_numpy(weights, indices, y)
    res = fcnmv_dt2t_p_call(weights, indices, y, shape=tuple(shape), transpose=transpose, backend=backend, out=out)[0]
    return A.to_result(res, as_np)


def fcnmm_dt2t(weights, indices, y, *, shape, transpose: bool, backend: Optional[str] = None, out=None):
    """Batched :func:`fcnmv_dt2t` (reference ``brainevent/_fcn/dt2t.py:179-344``): ``y (n_batch, shape[0] | shape[1])``,
    ``weights (n_batch, rows, n_conn)`` or one shared value -> ``(n_batch, rows, n_conn)``; ``y`` is cast to the weights'
    dtype."""
    as_np = out is None and A.wants_numpy(weights, indices, y)
    res = fcnmm_dt2t_p_call(weights, indices, y, shape=tuple(shape), transpose=transpose, backend=backend, out=out)[0]
    return A.to_result(res, as_np)


# ------------------------------------------------------------------------------------------------ containers
def container_dt2t(M, y, w, pre_axis: bool, out=None):
    """``M.dt2t`` (``pre_axis``: ``y`` indexed by the row of the matrix ``M`` stands for) / ``M.dt2t_transposed`` (by its
    column) for the four stored-rows containers, with the reference's routing: CSR and ``FixedNumPerPre`` store the rows
    (the pre axis is the row of an entry), CSC and ``FixedNumPerPost`` store the transpose (it is the stored index)."""
    rows = M._stored_rows()
    by_index = bool(pre_axis) == bool(M._stored_transposed)
    as_np = out is None and A.wants_numpy(y, w)
    if rows.indptr is None:
        res = fcnmv_dt2t_p_call(w, rows.indices, y, shape=(rows.m, rows.k), transpose=by_index, backend=M.backend, out=out)[0]
    else:
        res = csrmv_dt2t_p_call(y, w, rows.indices, rows.indptr, shape=(rows.m, rows.k), transpose=by_index, backend=M.backend,
                                out=out)[0]
    return A.to_result(res, as_np)
