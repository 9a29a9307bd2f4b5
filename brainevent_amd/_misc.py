"""Index dtype policy and structure validators for the hot path.

Restates the contracts of the reference's ``brainevent/_misc.py``:
``_resolve_indptr_dtype`` (:213-241), ``_as_int32_indices`` (:271-316), ``_as_indptr`` (:316-335),
``_check_compressed_structure`` (:335-378), ``check_fixed_conn_num_shape`` (:697-869),
``_normalize_chunk_size`` (:74-122) and the walk strides ``_MV_STRIDE`` / ``_MM_STRIDE`` (:37-38).
Validation that needs the values runs on the device (torch reductions) and reads back scalars only.
"""
from typing import Optional, Tuple

import numpy as np
import torch

_INT32_MAX = int(np.iinfo(np.int32).max)

#: residue-class stride of the light-RNG walk: part of the *drawn matrix* (mv and mm differ).
_MV_STRIDE = 32
_MM_STRIDE = 4


def _normalize_chunk_size(n_cols, chunk_size=None, target_chunks: int = 4) -> int:
    if chunk_size is None:
        target_chunks = int(target_chunks)
        if target_chunks <= 0:
            raise ValueError("target_chunks must be positive")
        chunk_size = max(1, (int(n_cols) + target_chunks - 1) // target_chunks)
    chunk_size = int(chunk_size)
    if chunk_size <= 0:
        raise ValueError("chunk_size must be positive")
    return chunk_size


def _is_int_dtype(dt: torch.dtype) -> bool:
    return dt in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def _resolve_indptr_dtype(nse: int, requested="auto") -> torch.dtype:
    nse = int(nse)
    if isinstance(requested, str):
        if requested != "auto":
            raise ValueError(f"indptr_dtype must be 'auto', int32, or int64; got {requested!r}.")
        return torch.int64 if nse > _INT32_MAX else torch.int32
    dt = np.dtype(requested) if not isinstance(requested, torch.dtype) else None
    if requested is torch.int32 or (dt is not None and dt == np.dtype(np.int32)):
        if nse > _INT32_MAX:
            raise OverflowError(f"nnz={nse} exceeds the int32 range ({_INT32_MAX}); request "
                                "indptr_dtype='auto' or int64.")
        return torch.int32
    if requested is torch.int64 or (dt is not None and dt == np.dtype(np.int64)):
        return torch.int64
    raise ValueError(f"indptr_dtype must be 'auto', int32, or int64; got {requested!r}.")


def _as_int32_indices(indices: torch.Tensor, secondary_dim: Optional[int], context: str,
                      check_values: bool = True) -> torch.Tensor:
    if not _is_int_dtype(indices.dtype):
        raise TypeError(f"{context}: indices must be an integer array; got dtype {indices.dtype}.")
    if secondary_dim is not None and int(secondary_dim) > _INT32_MAX + 1:
        raise OverflowError(f"{context}: secondary dimension {int(secondary_dim)} exceeds the "
                            "int32-representable coordinate range.")
    if check_values and indices.numel():
        min_v = int(indices.min())
        max_v = int(indices.max())
        if min_v < 0:
            raise ValueError(f"{context}: indices must be non-negative; got minimum {min_v}.")
        if secondary_dim is not None and max_v >= int(secondary_dim):
            raise ValueError(f"{context}: index {max_v} is out of bounds for secondary "
                             f"dimension {int(secondary_dim)}.")
        if max_v > _INT32_MAX:
            raise OverflowError(f"{context}: index {max_v} exceeds the int32 range; "
                                "secondary-axis coordinates must fit int32.")
    return indices if indices.dtype == torch.int32 else indices.to(torch.int32)


def _as_indptr(indptr: torch.Tensor, nse: int, indptr_dtype, context: str) -> torch.Tensor:
    if not _is_int_dtype(indptr.dtype):
        raise TypeError(f"{context}: indptr must be an integer array; got dtype {indptr.dtype}.")
    target = _resolve_indptr_dtype(nse, indptr_dtype)
    return indptr if indptr.dtype == target else indptr.to(target)


def _check_compressed_structure(indices: torch.Tensor, indptr: torch.Tensor, shape, format: str = "csr",
                                check_values: bool = True) -> None:
    fmt = format.lower()
    if fmt not in ("csr", "csc"):
        raise ValueError(f"format must be 'csr' or 'csc'; got {format!r}.")
    primary_dim = shape[0] if fmt == "csr" else shape[1]
    if indices.ndim != 1:
        raise ValueError(f"{fmt} indices must be a 1D array; got ndim {indices.ndim}.")
    if indptr.ndim != 1:
        raise ValueError(f"{fmt} indptr must be a 1D array; got ndim {indptr.ndim}.")
    if indices.dtype != torch.int32:
        raise TypeError(f"{fmt} indices must be int32; got {indices.dtype}.")
    if indptr.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{fmt} indptr must be int32 or int64; got {indptr.dtype}.")
    if indptr.shape[0] != int(primary_dim) + 1:
        raise ValueError(f"{fmt} indptr length must be primary dimension + 1 "
                         f"({int(primary_dim) + 1}); got {indptr.shape[0]}.")
    if not check_values:
        return
    if indptr.numel() and int(indptr[0]) != 0:
        raise ValueError(f"{fmt} indptr[0] must be 0; got {int(indptr[0])}.")
    if indptr.numel() > 1 and bool((indptr[1:] < indptr[:-1]).any()):
        raise ValueError(f"{fmt} indptr must be monotonically non-decreasing.")
    if int(indptr[-1]) != int(indices.shape[0]):
        raise ValueError(f"{fmt} indptr[-1] ({int(indptr[-1])}) must equal the number of "
                         f"stored elements ({int(indices.shape[0])}).")


def check_fixed_conn_num_shape(weights, indices, vector, shape: Tuple[int, int], transpose: bool,
                               require_scalar_weight: bool = False):
    """Shape contract of the fixed-number-connectivity ops (reference ``_misc.py:697-869``).

    ``indices`` is ``(n_pre, n_conn)``; ``weights`` has the same shape or one element; the
    vector has ``shape[0]`` entries when ``transpose`` (scatter) and ``shape[1]`` otherwise.
    Returns ``(out_len, n_pre, n_post)``.
    """
    if indices.ndim != 2:
        raise ValueError(f"indices must be 2D (n_pre, n_conn); got ndim {indices.ndim}.")
    n_pre, n_post = int(shape[0]), int(shape[1])
    assert indices.shape[0] == n_pre, (
        f"Pre size mismatch, got {indices.shape[0]} != {n_pre}")
    if weights.numel() != 1:
        assert tuple(weights.shape) == tuple(indices.shape), (
            f"The shape of weights {tuple(weights.shape)} and indices {tuple(indices.shape)} should be the same.")
    elif require_scalar_weight:
        pass
    if vector is not None:
        if transpose:
            assert vector.shape[0] == n_pre, f"vector length {vector.shape[0]} != shape[0] {n_pre}"
        else:
            assert vector.shape[0] == n_post, f"vector length {vector.shape[0]} != shape[1] {n_post}"
    return (n_post if transpose else n_pre), n_pre, n_post


# ------------------------------------------------------------------------------------------------ row slicing
def normalize_row_index(index, n_rows: int):
    """A row selector of ``W[index]`` / ``slice_rows(index)`` as int64 row numbers in ``[0, n_rows)``.

    Takes an ``int``, a ``list`` / ``tuple`` / numpy array / tensor of integers, or a ``slice`` (the reference's
    ``_misc.py:1156``, NumPy's rules: negative numbers count from the end, a slice is resolved against ``n_rows``).  An ``int``
    comes back 0-d — the mark of a scalar selection: its dense row is 1-D — everything else 1-D; a tensor stays a tensor on its
    device, anything else is a numpy array.  ``IndexError``: a dtype that is not an integer (``bool`` and floats included), or a
    number outside ``[-n_rows, n_rows)``."""
    n_rows = int(n_rows)
    if isinstance(index, slice):
        return np.arange(*index.indices(n_rows), dtype=np.int64)
    if isinstance(index, torch.Tensor):
        if not _is_int_dtype(index.dtype):
            raise IndexError(f"Row index must be integer, got dtype {index.dtype}.")
        if index.ndim > 1:
            raise IndexError(f"Row index must be a scalar or 1-D, got {index.ndim}-D.")
        rows = index.detach().to(torch.int64)
        rows = torch.where(rows < 0, rows + n_rows, rows)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n_rows):
            raise IndexError(f"Row index out of bounds for axis 0 with size {n_rows}.")
        return rows
    arr = np.asarray(index)
    if arr.size == 0 and arr.ndim == 1:           # ([] has no dtype of its own)
        return np.zeros(0, dtype=np.int64)
    if not np.issubdtype(arr.dtype, np.integer):
        raise IndexError(f"Row index must be integer, got dtype {arr.dtype}.")
    if arr.ndim > 1:
        raise IndexError(f"Row index must be a scalar or 1-D, got {arr.ndim}-D.")
    rows = arr.astype(np.int64)
    rows = np.where(rows < 0, rows + n_rows, rows)
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows):
        raise IndexError(f"Row index out of bounds for axis 0 with size {n_rows}.")
    return rows


def build_sub_csr(data, indices, indptr, rows, n_cols: int, *, row_len: int = -1):
    """The CSR arrays of ``W[rows, :]`` from the CSR arrays of ``W`` (the reference's ``_misc.py:1199``), built on the device:
    the new ``indptr`` is a prefix sum of the selected rows' lengths (torch), the segments are moved by ``be_slice_rows_copy``,
    balanced per entry.  ``indptr=None`` + ``row_len``: fixed-length rows.  One shared weight (size-1 ``data``) is returned as
    it is.  The number of stored entries of the result depends on values, so one scalar is read back.

    Returns ``(new_data, new_indices, new_indptr, (len(rows), n_cols))``; ``new_indptr`` is int32, or int64 when the source's
    is.  ``IndexError``: a row outside ``[0, n_rows)``."""
    from . import _array as A
    from ._lib import call
    idx = A.to_device(indices).reshape(-1)
    if idx.dtype != torch.int32:
        idx = _as_int32_indices(idx, None, 'build_sub_csr', check_values=False)
    nse = int(idx.numel())
    if indptr is None:
        ptr_, n_rows = None, (nse // int(row_len) if int(row_len) > 0 else 0)
    else:
        ptr_ = A.to_device(indptr)
        if ptr_.dtype not in (torch.int32, torch.int64):
            ptr_ = _as_indptr(ptr_, nse, 'auto', 'build_sub_csr')
        n_rows, row_len = int(ptr_.numel()) - 1, -1
    sel = A.to_device(rows, dtype=torch.int64).reshape(-1)
    n_sel = int(sel.numel())
    if n_sel and (int(sel.min()) < 0 or int(sel.max()) >= n_rows):
        raise IndexError(f"Row index out of bounds for axis 0 with size {n_rows}.")
    new_ptr = torch.zeros(n_sel + 1, dtype=torch.int64, device=idx.device)
    if n_sel:
        counts = (ptr_[sel + 1] - ptr_[sel]).to(torch.int64) if ptr_ is not None else torch.full_like(sel, int(row_len))
        torch.cumsum(counts, 0, out=new_ptr[1:])
    new_nse = int(new_ptr[-1]) if n_sel else 0
    w = A.to_device(data)
    homo = w.numel() == 1
    new_idx = torch.empty(new_nse, dtype=torch.int32, device=idx.device)
    new_w = w if homo else torch.empty(new_nse, dtype=w.dtype, device=idx.device)
    if new_nse:
        flat = None if homo else w.detach().reshape(-1)
        call('be_slice_rows_copy', A.ptr(idx), A.ptr(flat), 0 if homo else flat.element_size(), A.ptr(ptr_),
             int(ptr_ is not None and ptr_.dtype == torch.int64), int(row_len), A.ptr(sel), A.ptr(new_ptr), n_sel, n_rows, nse,
             new_nse, A.ptr(new_idx), A.ptr(None if homo else new_w), A.stream_ptr())
    if (ptr_ is None or ptr_.dtype == torch.int32) and new_nse <= _INT32_MAX:
        new_ptr = new_ptr.to(torch.int32)
    return new_w, new_idx, new_ptr, (n_sel, int(n_cols))
