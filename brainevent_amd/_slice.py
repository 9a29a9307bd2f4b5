"""Row slicing: ``W[rows]`` as a dense block, the gradient of that read, and ``W.slice_rows(rows)`` as a sparse sub-matrix —
the way to look at a neuron's outgoing weights during or after learning, or to cut a sub-population out of a connectome, and
the only differentiable read of individual rows.

Reference surface (read as text): ``brainevent/_csr/slice.py:39-83`` (``csr_slice_rows``), ``:204-252``
(``csr_slice_rows_p_call``), ``:300-340`` (``csr_slice_rows_grad``), ``:436-479`` (``csr_slice_rows_grad_p_call``); the
container methods ``_csr/main.py:1458-1499`` / ``:2361-2415`` and ``_fcn/main.py:918-960`` / ``:1182-1240``; the helpers
``_misc.py:1156-1252``.

All of it runs through one kernel file (``csrc/be_slice.hip``): ``be_slice_rows`` writes every element of the dense result
(zeros included: no memset, nothing depends on what ``torch.empty`` handed over), ``be_slice_rows_grad`` is its transpose,
``be_slice_rows_copy`` moves the selected rows' segments for the sparse result.  A row index outside ``[0, shape[0])`` reaches
the functional ops as a zero row (the reference's kernel rule); the containers raise ``IndexError`` before
(``normalize_row_index``).  Deviations from the reference, both this project's rules (``csrc/be_grad.hip`` has the same):

* duplicates of a column inside a row are added in ascending storage order in f32 (f64 for f64) and rounded once — the
  reference accumulates f16 in f16;
* one shared weight: ``out = count * w``, an integer count and one product (``+0`` where the count is 0) — the reference
  adds ``w`` repeatedly.

Neither kernel uses float atomics: results are bit-reproducible.  Cost of the dense read: every (selected row, column tile)
workgroup scans its whole row, ``ceil(n_cols / tile) * row length`` entries per selected row."""
from typing import Optional

import torch

from . import _array as A
from . import _autograd as _ag
from ._dt2t import _arr, _is_floating, _is_integer
from ._error import UnsupportedOperationError
from ._lib import call, fn
from ._misc import _as_indptr, _as_int32_indices, build_sub_csr, normalize_row_index
from ._op import OpKernel

__all__ = ['csr_slice_rows', 'csr_slice_rows_p', 'csr_slice_rows_p_call', 'csr_slice_rows_grad', 'csr_slice_rows_grad_p',
           'csr_slice_rows_grad_p_call']


# ------------------------------------------------------------------------------------------------ device calls
def _structure(indices, indptr):
    idx = A.to_device(indices).reshape(-1)
    if idx.dtype != torch.int32:
        idx = _as_int32_indices(idx, None, 'csr_slice_rows', check_values=False)
    ptr_ = None
    if indptr is not None:
        ptr_ = A.to_device(indptr)
        if ptr_.dtype not in (torch.int32, torch.int64):
            ptr_ = _as_indptr(ptr_, idx.shape[0], 'auto', 'csr_slice_rows')
    return idx, ptr_


def _rows64(row_indices) -> torch.Tensor:
    return A.to_device(row_indices, dtype=torch.int64).reshape(-1)


def _slice_rows_hip(data, indices, indptr, row_indices, *, shape, row_len: int = -1):
    """``data [nse | 1]``, ``row_indices [n_sel]`` -> ``[n_sel, shape[1]]``.  ``indptr=None`` + ``row_len``: fixed-length rows."""
    w = A.to_device(data).detach().reshape(-1)
    idx, ptr_ = _structure(indices, indptr)
    rows = _rows64(row_indices)
    n_sel, n_rows, n_cols, nse = int(rows.numel()), int(shape[0]), int(shape[1]), int(idx.numel())
    out = torch.empty((n_sel, n_cols), dtype=w.dtype, device=A.device())
    code = A.wcode(w)
    if n_sel == 0 or n_cols == 0:
        return out
    call('be_slice_rows', A.ptr(w), int(w.numel() == 1), code, A.ptr(idx), A.ptr(ptr_),
         int(ptr_ is not None and ptr_.dtype == torch.int64), int(row_len), A.ptr(rows), n_sel, A.ptr(out), n_rows, n_cols, nse,
         A.stream_ptr())
    return out


def _slice_rows_grad_hip(ct, indices, indptr, row_indices, *, shape, row_len: int = -1, homo: bool = False):
    """``ct [n_sel, shape[1]]`` -> ``dw [nse]`` (``homo``: ``[1]``, the sum over everything).  The selection is grouped by row
    here — a stable sort keeps each row's ``k`` ascending — and the number of distinct rows is read back for the launch."""
    g = A.to_device(ct).detach()
    idx, ptr_ = _structure(indices, indptr)
    rows = _rows64(row_indices)
    n_sel, n_rows, n_cols, nse = int(rows.numel()), int(shape[0]), int(shape[1]), int(idx.numel())
    code = A.wcode(g)
    dw = torch.empty(1 if homo else nse, dtype=g.dtype, device=A.device())
    ks = torch.argsort(rows, stable=True)
    urows, counts = torch.unique_consecutive(rows[ks], return_counts=True)
    n_u = int(urows.numel())
    seg = torch.zeros(n_u + 1, dtype=torch.int64, device=rows.device)
    if n_u:
        torch.cumsum(counts, 0, out=seg[1:])
    ws = A.workspace(fn('be_slice_rows_grad_workspace_bytes')(n_sel, code)) if homo else None
    call('be_slice_rows_grad', A.ptr(g), code, A.ptr(idx), A.ptr(ptr_), int(ptr_ is not None and ptr_.dtype == torch.int64),
         int(row_len), A.ptr(urows), A.ptr(seg), A.ptr(ks), n_u, n_sel, A.ptr(dw), int(homo), n_rows, n_cols, nse, A.ptr(ws),
         0 if ws is None else ws.numel(), A.stream_ptr())
    return dw


csr_slice_rows_p = OpKernel('csr_slice_rows')
csr_slice_rows_p.def_kernel('hip', 'gpu', _slice_rows_hip, asdefault=True)
csr_slice_rows_p.def_tags('csr', 'slice')
csr_slice_rows_grad_p = OpKernel('csr_slice_rows_grad')
csr_slice_rows_grad_p.def_kernel('hip', 'gpu', _slice_rows_grad_hip, asdefault=True)
csr_slice_rows_grad_p.def_tags('csr', 'slice', 'grad')


# ------------------------------------------------------------------------------------------------ validators
def _atleast_1d(x):
    x = _arr(x)
    return x.reshape(1) if x.ndim == 0 else x


def _check_structure(indices, indptr, row_indices, shape) -> None:
    """The reference's assertions (``_csr/slice.py:232-238``, ``:463-466``) plus the two the kernels' bounds rest on."""
    assert indices.ndim == 1, "indices must be 1D"
    assert indptr.ndim == 1, "indptr must be 1D"
    assert row_indices.ndim == 1, "row_indices must be 1D"
    assert _is_integer(indices), "indices must be integer"
    assert _is_integer(indptr), "indptr must be integer"
    assert _is_integer(row_indices), "row_indices must be integer"
    assert len(shape) == 2, f"shape must be (n_rows, n_cols), got {shape!r}"
    assert indptr.shape[0] == shape[0] + 1, f"indptr must have shape[0] + 1 = {shape[0] + 1} entries, got {indptr.shape[0]}."


def _plain_slice(data, indices, indptr, rows, shape, backend, row_len=-1):
    return csr_slice_rows_p(data, indices, indptr, rows, shape=tuple(shape), row_len=row_len, backend=backend)


def _sliced(data, w, indices, indptr, rows, shape, backend, row_len=-1, perm=None):
    """The dense rows of the CSR reading ``(w, indices, indptr | row_len)``; ``data`` is the tensor the caller holds (``w`` is
    ``data`` flat, or — with ``perm`` — its weights moved into the reading's order: ``w = data.reshape(-1)[perm]``).  Wrapped
    for autograd only when grad mode is on and ``data`` requires grad."""
    if not (isinstance(data, torch.Tensor) and _ag.needed(data)):
        return _plain_slice(w, indices, indptr, rows, shape, backend, row_len)
    homo = data.numel() == 1

    def run():
        return _plain_slice(w, indices, indptr, rows, shape, backend, row_len)

    def grad(g):
        dw = csr_slice_rows_grad_p(g.to(data.dtype).contiguous(), indices, indptr, rows, shape=tuple(shape), row_len=row_len, homo=homo,
                                   backend=backend)
        if perm is not None and not homo:
            stored = torch.zeros_like(dw)
            stored[perm.long()] = dw
            dw = stored
        return dw.reshape(data.shape)

    return _ag.slice_rows(data, run, grad)


def csr_slice_rows_p_call(data, indices, indptr, row_indices, *, shape, backend=None):
    """Validate, then dispatch (reference ``brainevent/_csr/slice.py:204-252``).  Returns a 1-list holding
    ``(len(row_indices), shape[1])`` in ``data``'s dtype."""
    data, indices, indptr, row_indices = _atleast_1d(data), _arr(indices), _arr(indptr), _atleast_1d(row_indices)
    assert data.ndim == 1, "data must be 1D"
    _check_structure(indices, indptr, row_indices, shape)
    assert _is_floating(data), "data must be a floating-point type"
    assert data.shape[0] in (1, indices.shape[0]), f"data must have 1 or {indices.shape[0]} elements, got {data.shape[0]}."
    return [_sliced(data, data, indices, indptr, row_indices, shape, backend)]


def csr_slice_rows_grad_p_call(ct, indices, indptr, row_indices, *, shape, backend=None):
    """Validate, then dispatch the gradient (reference ``brainevent/_csr/slice.py:436-479``).  Returns a 1-list holding
    ``(nse,)`` in ``ct``'s dtype."""
    ct, indices, indptr, row_indices = _arr(ct), _arr(indices), _arr(indptr), _atleast_1d(row_indices)
    assert ct.ndim == 2, "ct must be 2D"
    _check_structure(indices, indptr, row_indices, shape)
    assert _is_floating(ct), "ct must be a floating-point type"
    assert tuple(ct.shape) == (row_indices.shape[0], shape[1]), (
        f"ct must have shape {(row_indices.shape[0], shape[1])}, got {tuple(ct.shape)}.")
    return [csr_slice_rows_grad_p(ct, indices, indptr, row_indices, shape=tuple(shape), backend=backend)]


csr_slice_rows_p.def_call(csr_slice_rows_p_call)
csr_slice_rows_grad_p.def_call(csr_slice_rows_grad_p_call)


def csr_slice_rows(data, indices, indptr, row_indices, *, shape, backend: Optional[str] = None):
    """Rows ``row_indices`` of the CSR matrix ``(data, indices, indptr)`` of ``shape`` as a dense ``(len(row_indices),
    shape[1])`` array in ``data``'s dtype; a 0-d ``row_indices`` gives the 1-D row (reference
    ``brainevent/_csr/slice.py:39-83``).  ``data`` holds one value per stored entry or one shared value.  A row index outside
    ``[0, shape[0])`` gives a zero row.  Duplicate column ids inside a row are summed — in ascending storage order, in f32
    (f64 for f64), rounded once (the reference sums f16 in f16); one shared weight gives ``count * w`` (the reference adds
    ``w`` repeatedly).  Differentiable in ``data`` under ``torch.autograd`` (:func:`csr_slice_rows_grad` is the backward)."""
    as_np = A.wants_numpy(data, indices, indptr, row_indices)
    scalar = _arr(row_indices).ndim == 0
    res = csr_slice_rows_p_call(data, indices, indptr, row_indices, shape=tuple(shape), backend=backend)[0]
    return A.to_result(res[0] if scalar else res, as_np)


def csr_slice_rows_grad(ct, indices, indptr, row_indices, *, shape, backend: Optional[str] = None):
    """The transpose of :func:`csr_slice_rows`: ``dw[j] = sum of ct[k, indices[j]] over the k with row_indices[k] == row(j)``,
    zero for the entries of rows that were not selected; ``(nse,)`` in ``ct``'s dtype (reference
    ``brainevent/_csr/slice.py:300-340``).  Each sum runs over ascending ``k`` in f32 (f64 for f64) and is rounded once; no
    atomics."""
    as_np = A.wants_numpy(ct, indices, indptr, row_indices)
    res = csr_slice_rows_grad_p_call(ct, indices, indptr, row_indices, shape=tuple(shape), backend=backend)[0]
    return A.to_result(res, as_np)


# ------------------------------------------------------------------------------------------------ containers
def _row_major_view(M, want_grad: bool):
    """``(w, indices, indptr, row_len, perm)``: a CSR reading of the matrix ``M`` stands for.  CSR and ``FixedNumPerPre`` store
    it.  CSC and ``FixedNumPerPost`` store the transpose: the reading is their transposed mirror with its raw arrays (the
    reference's ``_weight_indices`` route) — the cached one when it still holds them, a cached one built here when there is
    none, and a private one when the cached mirror was released or lacks the permutation a gradient needs; a cached mirror is
    never replaced here."""
    rows = M._stored_rows()
    homo = M.data.numel() == 1
    if not M._stored_transposed:
        return (M.data if homo else M.data.reshape(-1)), rows.indices.reshape(-1), rows.indptr, rows.row_len, None
    from ._csr import build_mirror_of
    need_perm = want_grad and not homo
    mr = M.buffers.get('mirror')
    if mr is None:
        mr = M.build_mirror(keep_raw=True, keep_perm=True)
    elif not mr.released:
        mr = M._fresh_mirror()
    if mr.released or (need_perm and mr.perm is None):
        mr = build_mirror_of(M.data, rows.indices, rows.indptr, rows.row_len, rows.m, rows.k, keep_raw=True, keep_perm=True)
        if mr.released or (need_perm and mr.perm is None):
            raise UnsupportedOperationError(f"{type(M).__name__}: the row-major arrays of this matrix do not fit beside it; rows "
                                            f"cannot be read (convert with tocsr() on a machine that holds both).")
    return mr.data, mr.indices, mr.indptr, -1, mr.perm


def _as_numpy(M, index) -> bool:
    return bool(M._numpy_result) and not isinstance(index, torch.Tensor)


def container_getitem(M, index):
    """``M[index]``: rows of the matrix ``M`` stands for (``shape[0]`` of them, whatever the storage axis) as a dense array —
    ``(shape[1],)`` for an ``int``, ``(len(rows), shape[1])`` otherwise."""
    rows = normalize_row_index(index, M.shape[0])
    want_grad = _ag.needed(M.data)
    w, indices, indptr, row_len, perm = _row_major_view(M, want_grad)
    out = _sliced(M.data, w, indices, indptr, rows.reshape(-1), M.shape, M.backend, row_len, perm)
    return A.to_result(out[0] if rows.ndim == 0 else out, _as_numpy(M, index))


def container_slice_rows(M, index):
    """``M.slice_rows(index)``: ``W[rows, :]`` as a sparse matrix of the reference's type — CSR -> CSR, CSC -> CSC,
    ``FixedNumPerPre`` -> ``FixedNumPerPre``, ``FixedNumPerPost`` -> CSR (selecting rows breaks the fixed number per column).
    An ``int`` gives a ``1 x shape[1]`` matrix."""
    from ._csr import CSR, CSC
    rows = normalize_row_index(index, M.shape[0]).reshape(-1)
    if not M._stored_transposed and M._stored_rows().indptr is None:          # FixedNumPerPre: plain indexing of [n_pre, K]
        sel = A.to_device(rows, dtype=torch.int64)
        data = M.data if M.data.numel() == 1 else M.data.detach()[sel]
        obj = type(M)((data, M.indices[sel]), shape=(int(sel.numel()), M.shape[1]), backend=M.backend, check_indices=False)
        obj._numpy_result = M._numpy_result
        return obj
    w, indices, indptr, row_len, _ = _row_major_view(M, False)
    sub = CSR._from_parts(*build_sub_csr(w.detach(), indices, indptr, rows, M.shape[1], row_len=row_len)[:3],
                          shape=(int(rows.shape[0]), M.shape[1]), backend=M.backend, numpy_result=M._numpy_result)
    return sub.tocsc() if isinstance(M, CSC) else sub
