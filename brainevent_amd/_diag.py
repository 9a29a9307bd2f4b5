"""``diag_add``: ``A + diag(d)`` for CSR / CSC with the missing diagonal entries INSERTED — the leak term of a recurrent
projection, a regulariser on a sparse Jacobian.

Reference surface (read as text): ``brainevent/_csr/diag_add.py`` (``csr_diag_position`` ``:36-242``, ``csr_diag_add``
``:245-330``) and the container method ``_csr/main.py:878-950``.  Semantics are the reference's (``diag_add.py:99-110``,
``:196-238``, ``:325-329``): a row ``i < min(shape)`` that lacks the stored index ``i`` gains one entry, placed before the first
stored entry with an index ``> i`` in storage order (at the row's end if there is none); where the diagonal is stored more than
once the LAST copy receives the addend; every other entry is copied; the result holds the full diagonal.

Differences, all this project's own:

* the plan is per ROW, not per entry (:class:`DiagPlan`): beside the new structure it keeps three int64 words per row — the
  shift, the old offset before which the diagonal goes, the old offset of an existing diagonal — and the kernels compute an
  entry's new position ``e + shift[r] + (inserted before e)`` from its row.  ``old_to_new`` (``nse`` integers) is only
  materialised for the callers of :func:`csr_diag_position`;
* planning runs on the device (``csrc/be_arith.hip``: ``be_diag_scan`` + one ``torch.cumsum``) and offsets are int64 wherever
  ``indptr`` is int64 or the new entry count exceeds int32 (:func:`offset_dtype`) — the reference plans on the host and raises
  ``NotImplementedError`` there;
* a shared weight (``data`` of size 1) is expanded: the result holds per-entry data.

The first ``diag_add`` of a structure reads the new entry count back (one ``.item()``: not capturable in a HIP graph); every
later call on the cached plan — and every call on a result, which carries its own plan — launches two kernels and nothing
else, and is capturable."""
from typing import Optional

import numpy as np
import torch

from . import _array as A
from ._dt2t import _arr, _is_floating, _is_integer
from ._lib import call
from ._misc import _INT32_MAX

__all__ = ['csr_diag_position', 'csr_diag_add', 'DiagPlan', 'offset_dtype', 'container_diag_add']

_I64_MAX = np.iinfo(np.int64).max


def offset_dtype(indptr_dtype, new_nse: int) -> torch.dtype:
    """The dtype of the new ``indptr`` and of the position maps: int64 wherever the old ``indptr`` is int64 or the new entry
    count does not fit int32."""
    if indptr_dtype == torch.int64 or int(new_nse) > _INT32_MAX:
        return torch.int64
    return torch.int32


class DiagPlan:
    """The value-independent plan of ``diag_add`` on one structure, cached under the buffer name ``diag_positions``.

    ``new_indptr`` / ``new_indices``: the structure with the full diagonal; ``diag_dest [n_diag]``: where element ``(i, i)``
    lives in it; per old row ``shift`` (entries inserted in the rows before it), ``ins`` (the old offset before which its
    diagonal goes, ``-1`` where none is inserted) and per diagonal ``exist`` (the old offset of the stored diagonal, ``-1``
    where it is missing) — all int64 on the device; ``result_plan`` is the identity plan of the result's own structure."""
    __slots__ = ('indices', 'indptr', 'n_rows', 'n_diag', 'nse', 'new_nse', 'new_indptr', 'new_indices', 'diag_dest', 'shift',
                 'ins', 'exist', 'old_to_new', 'result_plan')

    def positions(self):
        """The reference's 4-tuple ``(new_indptr, new_indices, old_to_new, diag_dest)``; ``old_to_new`` is written on first
        use by the move kernel in its index-only mode."""
        if self.old_to_new is None:
            dt = self.new_indptr.dtype
            o2n = torch.empty(self.nse, dtype=dt, device=A.device())
            if self.result_plan is self:              # an identity plan: nothing moves
                torch.arange(self.nse, dtype=dt, device=A.device(), out=o2n)
            else:
                call('be_diag_move', A.ptr(None), 0, 0, A.ptr(self.indices), A.ptr(self.indptr),
                     int(self.indptr.dtype == torch.int64), self.n_rows, self.nse, A.ptr(self.shift), A.ptr(self.ins),
                     self.new_nse, A.ptr(None), A.ptr(None), A.ptr(o2n), int(dt == torch.int64), A.stream_ptr())
            self.old_to_new = o2n
        return self.new_indptr, self.new_indices, self.old_to_new, self.diag_dest


def _identity_plan(indices, indptr, n_rows: int, n_diag: int, diag_dest) -> DiagPlan:
    """The plan of a structure that holds its full diagonal at ``diag_dest``: nothing is inserted, nothing moves."""
    p = DiagPlan()
    dev = A.device()
    p.indices, p.indptr, p.n_rows, p.n_diag = indices, indptr, n_rows, n_diag
    p.nse = p.new_nse = int(indices.numel())
    p.new_indptr, p.new_indices, p.diag_dest = indptr, indices, diag_dest
    p.shift = torch.zeros(n_rows, dtype=torch.int64, device=dev)
    p.ins = torch.full((n_rows,), -1, dtype=torch.int64, device=dev)
    p.exist = diag_dest.to(torch.int64)
    p.old_to_new = None
    p.result_plan = p
    return p


def plan_structure(indices: torch.Tensor, indptr: torch.Tensor, n_rows: int, n_diag: int) -> DiagPlan:
    """Scan the stored rows ``(indices, indptr)`` (int32 / int32-or-int64 device tensors, ``n_rows`` rows) and derive the
    plan.  The new structure is NOT written here: ``new_indices`` is allocated and filled by the first :func:`apply_plan`."""
    dev = A.device()
    nse = int(indices.numel())
    found = torch.empty((max(n_diag, 1), 2), dtype=torch.int64, device=dev)
    found[:, 0] = -1
    found[:, 1] = _I64_MAX
    call('be_diag_scan', A.ptr(indices), A.ptr(indptr), int(indptr.dtype == torch.int64), n_rows, n_diag, nse, A.ptr(found),
         A.stream_ptr())
    ptr64 = indptr.to(torch.int64)
    exist = found[:n_diag, 0].contiguous()
    missing = exist < 0
    ins = torch.full((n_rows,), -1, dtype=torch.int64, device=dev)
    ins[:n_diag] = torch.where(missing, torch.minimum(found[:n_diag, 1], ptr64[1:n_diag + 1]), ins[:n_diag])
    shift = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    if n_diag:
        torch.cumsum(missing.to(torch.int64), 0, out=shift[1:n_diag + 1])
        shift[n_diag + 1:] = shift[n_diag]
    new_nse = nse + int(shift[n_rows].item())          # the one host synchronisation, once per structure
    dt = offset_dtype(indptr.dtype, new_nse)
    p = DiagPlan()
    p.indices, p.indptr, p.n_rows, p.n_diag, p.nse, p.new_nse = indices, indptr, n_rows, n_diag, nse, new_nse
    p.new_indptr = (ptr64 + shift).to(dt)
    p.shift = shift[:n_rows].contiguous()
    p.ins, p.exist = ins, exist
    p.diag_dest = (torch.where(missing, ins[:n_diag], exist) + p.shift[:n_diag]).to(dt)
    p.new_indices = None
    p.old_to_new = None
    p.result_plan = None
    return p


def apply_plan(plan: DiagPlan, data: Optional[torch.Tensor], diag: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Move and fill on the current stream: the new values for ``data`` (flat, ``nse`` or 1 elements) and ``diag`` — and, on the
    first call of a plan, its ``new_indices`` in the same two launches.  ``data=None``: the structure alone."""
    dev = A.device()
    first = plan.new_indices is None
    new_indices = torch.empty(plan.new_nse, dtype=torch.int32, device=dev) if first else None
    nd = None if data is None else torch.empty(plan.new_nse, dtype=data.dtype, device=dev)
    code = 0 if data is None else A.wcode(data)
    homo = int(data is not None and data.numel() == 1 and plan.nse != 1)
    call('be_diag_move', A.ptr(data), homo, code, A.ptr(plan.indices), A.ptr(plan.indptr),
         int(plan.indptr.dtype == torch.int64), plan.n_rows, plan.nse, A.ptr(plan.shift), A.ptr(plan.ins), plan.new_nse,
         A.ptr(new_indices), A.ptr(nd), A.ptr(None), 0, A.stream_ptr())
    call('be_diag_fill', A.ptr(data), homo, code, plan.nse, plan.n_diag, A.ptr(plan.shift), A.ptr(plan.ins), A.ptr(plan.exist),
         A.ptr(diag), plan.new_nse, A.ptr(new_indices), A.ptr(nd), A.stream_ptr())
    if first:
        plan.new_indices = new_indices
        plan.result_plan = _identity_plan(new_indices, plan.new_indptr, plan.n_rows, plan.n_diag, plan.diag_dest)
    return nd


def _device_structure(indptr, indices):
    from ._misc import _as_indptr, _as_int32_indices
    idx = A.to_device(indices)
    if idx.dtype != torch.int32:
        idx = _as_int32_indices(idx, None, 'csr_diag_position', check_values=False)
    ptr_ = A.to_device(indptr)
    if ptr_.dtype not in (torch.int32, torch.int64):
        ptr_ = _as_indptr(ptr_, idx.shape[0], 'auto', 'csr_diag_position')
    return ptr_, idx


def csr_diag_position(indptr, indices, *, shape):
    """Plan ``A + diag(d)`` on the CSR structure ``(indptr, indices)`` of ``shape`` (for a CSC matrix pass its column pointers
    and row indices: the diagonals of a matrix and of its transpose coincide).  Returns the reference's four arrays
    ``(new_indptr, new_indices, old_to_new, diag_dest)`` (``brainevent/_csr/diag_add.py:36-242``): ``nd[old_to_new[p]] ==
    data[p]`` and element ``(i, i)`` lives at ``nd[diag_dest[i]]``.  ``new_indices`` is int32; the three offset arrays are int32,
    or int64 wherever ``indptr`` is int64 or the new entry count exceeds int32 (the reference raises there).  numpy in gives
    numpy out.  Reads one number back from the device."""
    assert isinstance(shape, (tuple, list)), "shape must be a tuple or list"
    indptr_a, indices_a = _arr(indptr), _arr(indices)
    assert indptr_a.ndim == 1, "indptr must be a 1D array"
    assert indices_a.ndim == 1, "indices must be a 1D array"
    assert len(shape) == 2, "shape must be a tuple or list of length 2"
    assert all(isinstance(s, (int, np.integer)) and s > 0 for s in shape), "shape must be a tuple or list of positive integers"
    assert _is_integer(indptr_a) and _is_integer(indices_a), "indptr and indices must be integer arrays"
    assert indptr_a.shape[0] >= min(shape) + 1, "indptr is shorter than the diagonal"
    as_np = A.wants_numpy(indptr, indices)
    ptr_, idx = _device_structure(indptr_a, indices_a)
    plan = plan_structure(idx, ptr_, int(ptr_.shape[0]) - 1, int(min(shape)))
    apply_plan(plan, None, None)
    return tuple(A.to_result(t, as_np) for t in plan.positions())


def csr_diag_add(csr_value, positions, diag_value):
    """The values of ``A + diag(diag_value)`` on the plan of :func:`csr_diag_position`: ``nd = zeros; nd[old_to_new] =
    csr_value; nd[diag_dest] += diag_value`` — three torch index operations, with the reference's assertions
    (``brainevent/_csr/diag_add.py:313-329``).  The containers' ``diag_add`` does the same from the per-row plan without the
    ``old_to_new`` array."""
    csr_value, diag_value = _arr(csr_value), _arr(diag_value)
    assert csr_value.ndim == 1, "csr_value must be a 1D array"
    assert diag_value.ndim == 1, "diag_value must be a 1D array"
    assert csr_value.dtype == diag_value.dtype, "csr_value and diag_value must have the same dtype"
    _, new_indices, old_to_new, diag_dest = (_arr(p) for p in positions)
    assert old_to_new.ndim == 1, "old_to_new must be a 1D array"
    assert diag_dest.ndim == 1, "diag_dest must be a 1D array"
    assert _is_integer(old_to_new), "old_to_new must be an integer array"
    assert _is_integer(diag_dest), "diag_dest must be an integer array"
    assert csr_value.shape[0] == old_to_new.shape[0], "csr_value length must match the original number of stored elements"
    assert diag_value.shape[0] == diag_dest.shape[0], "diag_value must have one entry per diagonal (min(shape))"
    as_np = A.wants_numpy(csr_value, diag_value)
    w, d = A.to_device(csr_value), A.to_device(diag_value)
    nd = torch.zeros(int(new_indices.shape[0]), dtype=w.dtype, device=A.device())
    nd[A.to_device(old_to_new, dtype=torch.int64)] = w
    nd.index_add_(0, A.to_device(diag_dest, dtype=torch.int64), d)
    return A.to_result(nd, as_np)


def container_diag_add(M, other):
    """``M.diag_add(other)`` of CSR / CSC: a new matrix of the same class and shape holding ``M + diag(other)`` on the
    structure with the full diagonal; it carries the identity plan of that structure."""
    from ._arith import is_matrix
    assert not is_matrix(other), "diag_add does not support sparse objects."
    n_diag = int(min(M.shape))
    d = _arr(other)
    if d.ndim != 1 or int(d.shape[0]) != n_diag:
        raise ValueError(f"{type(M).__name__}.diag_add: the diagonal must have shape ({n_diag},), got {tuple(d.shape)}.")
    assert _is_floating(d), "the diagonal must be a floating-point array"
    d = A.to_device(d).detach()
    assert d.dtype == M.data.dtype, f"the diagonal's dtype {d.dtype} must be data's dtype {M.data.dtype}"
    plan = M.buffers.get('diag_positions')
    if not isinstance(plan, DiagPlan) or plan.indices is not M.indices or plan.indptr is not M.indptr:
        rows = M._stored_rows()
        plan = plan_structure(M.indices, M.indptr, rows.m, n_diag)
        M.buffers['diag_positions'] = plan
    nd = apply_plan(plan, M.data.detach().reshape(-1), d)
    obj = object.__new__(type(M))
    obj.data, obj.indices, obj.indptr = nd, plan.new_indices, plan.new_indptr
    obj.shape, obj.backend, obj._numpy_result = M.shape, M.backend, M._numpy_result
    obj._init_buffers({'diag_positions': plan.result_plan})
    return obj
