"""Container arithmetic: ``2 * csr``, ``-csr``, ``abs(csr)``, ``csr * mask``, ``csr / norm``, ``csr + x``, ``M.apply(fn)``,
``M.apply2(other, fn)`` — one :class:`ArithmeticMixin` over three hooks, as the reference writes it (read as text:
``brainevent/_data.py:432-760``; the hooks of the families ``_csr/main.py:1288-1319``, ``:1501-1593``, ``:2417-2507``,
``_fcn/main.py:721-780``, ``_dense/main.py:231-320``, ``_jit_{scalar,uniform,normal}/main.py`` ``_unitary_op`` /
``_binary_op`` / ``_binary_rop``).

The stored-rows containers (CSR, CSC, ``FixedNumPerPre`` / ``FixedNumPerPost``) follow these rules:

* unary / ``apply``: a new container of the same class around ``fn(data)``; ``indices`` / ``indptr`` are shared by reference;
* a size-1 operand: ``fn(data, other)`` on the data tensor, in torch (differentiable wherever ``data`` requires grad);
* a 2-D operand of exactly ``shape``: the dense operand is sampled on the stored pattern by ``be_entries_dense_op``
  (``csrc/be_arith.hip``) — ``*`` and ``/`` (both sides) fused, any other callable through the kernel's ``take``;
* ``+`` / ``-`` with a dense or scalar operand: a DENSE result, ``fn(dense(self), other)``, as in the reference;
* a sparse operand: same class and the same structure arrays by identity -> ``fn(self.data, other.data)``; any other sparse
  operand raises ``NotImplementedError``.  This rule is this project's own: the reference's branch for it
  (``_csr/main.py:1508-1518``) passes the structure arrays to the operator and cannot run as written;
* any other dense shape raises ``NotImplementedError`` (per-row / per-column vectors are ``dt2t`` / ``dt2t_transposed``).

Only structure-only caches travel with a result (``STRUCTURE_BUFFERS``: the ``diag_positions`` plan of ``_diag``); scatter plans
and mirrors embed weights and are rebuilt on first use."""
import operator

import numpy as np
import torch

from . import _array as A
from . import _autograd as _ag
from ._error import UnsupportedOperationError
from ._lib import call
from ._op import OpKernel

__all__ = ['ArithmeticMixin', 'entries_dense_op', 'entries_dense_op_p', 'STRUCTURE_BUFFERS', 'OPS']

#: buffers that describe the structure alone: they stay valid for any data on the same ``indices`` / ``indptr``
STRUCTURE_BUFFERS = ('diag_positions',)
#: the kernel's op codes
OPS = {'take': 0, 'mul': 1, 'div': 2, 'rdiv': 3}


class ArithmeticMixin:
    """``apply`` / ``apply2`` and the operators, over ``_unitary_op(fn)``, ``_binary_op(other, fn)`` and
    ``_binary_rop(other, fn)`` (reference ``brainevent/_data.py:432-760``)."""

    def _unitary_op(self, fn):
        raise NotImplementedError(f"{type(self).__name__}: unitary operation not implemented.")

    def _binary_op(self, other, fn):
        raise NotImplementedError(f"{type(self).__name__}: binary operation not implemented.")

    def _binary_rop(self, other, fn):
        raise NotImplementedError(f"{type(self).__name__}: binary operation not implemented.")

    def apply(self, fn):
        """A new matrix with ``fn`` applied to the stored values; the structure is kept (and shared, not copied).  This
        allocates a new value array: for a per-step rescaling write in place instead (``M.data.mul_(x)``; with cached plans,
        ``prepare(plastic=...)`` or ``refresh_weights()`` keep them current)."""
        return self._unitary_op(fn)

    def apply2(self, other, fn, *, reverse: bool = False):
        """``fn(self, other)``, or ``fn(other, self)`` with ``reverse``, by the rules of the family (module docstring)."""
        if reverse:
            return self._binary_rop(other, fn)
        return self._binary_op(other, fn)

    def __abs__(self):
        return self.apply(operator.abs)

    def __neg__(self):
        return self.apply(operator.neg)

    def __pos__(self):
        return self.apply(operator.pos)

    def __mul__(self, other):
        return self.apply2(other, operator.mul)

    def __truediv__(self, other):
        return self.apply2(other, operator.truediv)

    def __add__(self, other):
        return self.apply2(other, operator.add)

    def __sub__(self, other):
        return self.apply2(other, operator.sub)

    def __rmul__(self, other):
        return self.apply2(other, operator.mul, reverse=True)

    def __rtruediv__(self, other):
        return self.apply2(other, operator.truediv, reverse=True)

    def __radd__(self, other):
        return self.apply2(other, operator.add, reverse=True)

    def __rsub__(self, other):
        return self.apply2(other, operator.sub, reverse=True)


# ------------------------------------------------------------------------------------------------ operands
def is_matrix(x) -> bool:
    """A weight-matrix container of this package (or one of the objects that stand for one)."""
    from ._data import DataRepresentation
    return isinstance(x, DataRepresentation) or type(x).__name__ in ('PlannedMatrix', 'Mirror', 'JITCScatterShard',
                                                                      'JITCGatherShard')


def as_operand(other):
    """A dense operand as a tensor (kept where it lives) or a numpy array."""
    return other if isinstance(other, torch.Tensor) else np.asarray(other)


def scalar_operand(x):
    """A size-1 operand as torch takes it beside a data tensor without changing its dtype: a 0-d tensor on the device (so a
    tensor that requires grad stays in the graph), else a python number."""
    if isinstance(x, torch.Tensor):
        t = x.reshape(())
        return t if t.device == A.device() else t.to(A.device())
    return x.reshape(-1)[0].item()


def broadcast_check(shape, other_shape, what: str) -> tuple:
    try:
        return tuple(np.broadcast_shapes(tuple(shape), tuple(other_shape)))
    except ValueError as exc:
        raise ValueError(f"{what}: operand shape {tuple(other_shape)} cannot broadcast with shape {tuple(shape)}.") from exc


# ------------------------------------------------------------------------------------------------ the sample kernel
def _entries_dense_op_hip(data, indices, indptr, dense, *, shape, op: str, row_len: int = -1, transposed: bool = False):
    """``out[e] = op(data[e or 0], dense[r(e), c(e)])`` over the stored rows ``(indices, indptr | row_len)`` of ``shape =
    (m, k)``; with ``transposed`` the stored rows are the COLUMNS of ``dense`` (its strides are swapped, nothing is moved).
    ``dense`` is read in place in ``data``'s dtype or as bool / uint8; any other dtype is converted once on the device.
    Returns a tensor shaped like ``indices`` in ``data``'s dtype."""
    w = A.to_device(data).detach().reshape(-1)
    idx = indices if indices.is_contiguous() else indices.contiguous()
    m, k = int(shape[0]), int(shape[1])
    D = dense.detach() if isinstance(dense, torch.Tensor) else torch.from_numpy(np.asarray(dense))
    if D.device != A.device():
        D = D.to(A.device())
    if D.dtype == torch.bool:
        D = D.view(torch.uint8)
    elif D.dtype != torch.uint8 and D.dtype != w.dtype:
        D = D.to(w.dtype)
    want = (k, m) if transposed else (m, k)
    assert D.ndim == 2 and tuple(D.shape) == want, f"dense operand {tuple(D.shape)} does not match the matrix {want}"
    s0, s1 = (int(D.stride(1)), int(D.stride(0))) if transposed else (int(D.stride(0)), int(D.stride(1)))
    out = torch.empty(tuple(idx.shape), dtype=w.dtype, device=A.device())
    nse = int(idx.numel())
    if nse == 0:
        return out
    call('be_entries_dense_op', A.ptr(out), A.ptr(w), int(w.numel() == 1), A.wcode(w), A.ptr(idx), A.ptr(indptr),
         int(indptr is not None and indptr.dtype == torch.int64), int(row_len), m, k, nse, A.ptr(D),
         int(D.dtype == torch.uint8), s0, s1, OPS[op], A.stream_ptr())
    return out


entries_dense_op_p = OpKernel('entries_dense_op')
entries_dense_op_p.def_kernel('hip', 'gpu', _entries_dense_op_hip, asdefault=True)
entries_dense_op_p.def_tags('csr', 'arith')


def entries_dense_op(M, dense, op: str, data=None) -> torch.Tensor:
    """The dense operand (of exactly ``M.shape``) sampled on the pattern of the stored-rows container ``M`` and combined with
    ``data`` (default ``M.data``) by ``op`` (``'take'``, ``'mul'``, ``'div'``, ``'rdiv'``): one value per stored entry, shaped
    like ``M.indices``, in ``data``'s dtype.  No autograd."""
    rows = M._stored_rows()
    return entries_dense_op_p(M.data if data is None else data, rows.indices, rows.indptr, dense, shape=(rows.m, rows.k), op=op,
                              row_len=rows.row_len, transposed=M._stored_transposed, backend=M.backend)


_FUSED = {(operator.mul, False): 'mul', (operator.mul, True): 'mul', (operator.truediv, False): 'div',
          (operator.truediv, True): 'rdiv'}


def _sampled(M, D, fn, reverse: bool) -> torch.Tensor:
    """The per-entry data of ``fn(M, D)`` (``fn(D, M)`` with ``reverse``) for a dense ``D`` of ``M.shape``.  Autograd covers
    ``data`` only: for ``mul`` / ``div`` the gradient is the same kernel applied to the incoming gradient, for the reflected
    ``div`` it is ``-g * out / w``; a shared weight receives the sum."""
    if isinstance(D, torch.Tensor) and D.requires_grad and torch.is_grad_enabled():
        raise UnsupportedOperationError(
            f"{type(M).__name__}: the dense operand of an elementwise product requires grad, and no gradient into it is "
            "computed here (it would be a silent zero). Detach it, or form the product on M.todense().")
    op = _FUSED.get((fn, reverse))
    if op is None:                  # any other callable: the operand's values on the pattern, then fn in torch
        vals = entries_dense_op(M, D, 'take')
        data = M.data if M.data.numel() == 1 else M.data.reshape(vals.shape)
        return fn(vals, data) if reverse else fn(data, vals)
    if not _ag.needed(M.data):
        return entries_dense_op(M, D, op)
    data = M.data
    kept = {}

    def run():
        kept['out'] = entries_dense_op(M, D, op)
        return kept['out']

    def grad(g):
        g = g.to(data.dtype).contiguous()
        if op == 'rdiv':
            w = data.detach()
            dw = -g * kept['out'] / (w.reshape(()) if w.numel() == 1 else w.reshape(g.shape))
        else:
            dw = entries_dense_op(M, D, op, data=g)
        if data.numel() == 1 and dw.numel() != 1:
            acc = torch.float64 if dw.dtype == torch.float64 else torch.float32
            dw = dw.to(acc).sum().to(data.dtype)
        return dw.reshape(data.shape)

    return _ag.slice_rows(data, run, grad)


# ------------------------------------------------------------------------------------------------ stored-rows containers
def share_structure(M, data):
    """A new container of ``M``'s class around ``data`` on ``M``'s own structure arrays (shared by reference, no validation,
    no conversion); of the buffers only the structure-only ones travel."""
    obj = object.__new__(type(M))
    for name in ('indices', 'indptr', 'shape', 'backend', '_numpy_result'):
        if hasattr(M, name):
            setattr(obj, name, getattr(M, name))
    obj.data = data if data.is_contiguous() else data.contiguous()
    obj._init_buffers({k: M.buffers[k] for k in STRUCTURE_BUFFERS if M.buffers.get(k) is not None})
    return obj


def _checked_data(M, data, what: str) -> torch.Tensor:
    if not isinstance(data, torch.Tensor):
        data = A.to_device(data)
    if tuple(data.shape) != tuple(M.data.shape) and tuple(data.shape) != tuple(M.indices.shape):
        raise ValueError(f"{type(M).__name__}.{what}: the function changed the shape of data from {tuple(M.data.shape)} to "
                         f"{tuple(data.shape)}; only the dtype may change.")
    return data


def rows_unitary(M, fn):
    return share_structure(M, _checked_data(M, fn(M.data), 'apply'))


def dense_of(M) -> torch.Tensor:
    """``M`` as a dense device tensor of ``M.shape``: the row-read kernel over all rows (``_slice``; deterministic,
    differentiable in ``data``)."""
    from ._misc import normalize_row_index
    from ._slice import _row_major_view, _sliced
    rows = normalize_row_index(slice(None), M.shape[0])
    w, indices, indptr, row_len, perm = _row_major_view(M, _ag.needed(M.data))
    return _sliced(M.data, w, indices, indptr, rows, M.shape, M.backend, row_len, perm)


def rows_binary(M, other, fn, reverse: bool):
    """``_binary_op`` / ``_binary_rop`` of the stored-rows containers (module docstring)."""
    name = type(M).__name__
    if is_matrix(other):
        same = (type(other) is type(M) and other.indices is M.indices
                and getattr(other, 'indptr', None) is getattr(M, 'indptr', None))
        if not same:
            raise NotImplementedError(f"{name}: binary operation {getattr(fn, '__name__', fn)} between two sparse objects is "
                                      "served only for the same class on the same structure arrays (by identity).")
        a, b = (other.data, M.data) if reverse else (M.data, other.data)
        if a.numel() != b.numel():          # a shared weight beside per-entry data: broadcast over the entries
            a, b = (x.reshape(()) if x.numel() == 1 else x for x in (a, b))
        return share_structure(M, _checked_data(M, fn(a, b), 'apply2'))
    x = as_operand(other)
    if fn in (operator.add, operator.sub):           # a dense result, as in the reference
        shape = broadcast_check(M.shape, x.shape, f"{name} {fn.__name__}")
        as_np = bool(M._numpy_result) and not isinstance(other, torch.Tensor)
        dense = dense_of(M)
        if int(np.prod(x.shape)) == 1:
            xt = scalar_operand(x)
        else:
            xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
            xt = xt if xt.device == dense.device else xt.to(dense.device)
        r = fn(xt, dense) if reverse else fn(dense, xt)
        return A.to_result(r.reshape(shape), as_np)
    if int(np.prod(x.shape)) == 1:
        s = scalar_operand(x)
        return share_structure(M, _checked_data(M, fn(s, M.data) if reverse else fn(M.data, s), 'apply2'))
    if x.ndim == 2 and tuple(x.shape) == tuple(M.shape):
        return share_structure(M, _checked_data(M, _sampled(M, x, fn, reverse), 'apply2'))
    raise NotImplementedError(
        f"{name}: elementwise operation with an operand of shape {tuple(x.shape)} (the matrix is {tuple(M.shape)}): only a "
        "size-1 operand or a 2-D operand of exactly the matrix's shape is served. For a per-row / per-column vector use "
        "dt2t / dt2t_transposed.")
