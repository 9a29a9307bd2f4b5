"""Fixed-number connectivity (ELL): ``FixedNumPerPre`` / ``FixedNumPerPost`` and ``binary_fcnmv`` / ``binary_fcnmm``.

Reference surface mirrored (read as text): ``brainevent/_fcn/main.py:199-460`` (``FixedNumConn`` dispatch),
``:781-854`` (``FixedNumPerPre``: ``indices (n_pre, n_conn)`` are post ids), ``:1042-1115`` (``FixedNumPerPost``:
``indices (n_post, n_conn)`` are pre ids), ``brainevent/_fcn/binary.py:43-143`` / ``:564-675`` (functional ops),
``:156-253`` / ``:677-766`` (CPU semantics), ``:450-509`` / ``:1077-1137`` (``*_p_call`` validation).

Semantics for ``indices[n_rows, n_conn]`` and ``shape = (n_rows, n_cols)`` as the functional ops see it:
  transpose=True  (scatter): ``out[indices[i, c]] += w[i, c]`` for every active ``i``      -> ``out[n_cols]``
  transpose=False (gather) : ``out[i] = sum_c w[i, c] * e(s[indices[i, c]])``              -> ``out[n_rows]``

An ELL matrix is a CSR matrix with an implicit ``indptr`` (``row r = [r*n_conn, (r+1)*n_conn)``), so the
kernels are the CSR ones (``csrc/be_csr.hip``), reached through the stored-rows step (``_csr.rows_step``) with
``indptr = None`` and ``row_len = n_conn``.  The
unfavourable direction (``FixedNumPerPre @ spk``, ``spk @ FixedNumPerPost``) runs event-driven through the CSC
mirror (reference ``_fcn/main.py:280-326``: ``_weight_indices`` + the perm-fused CSR kernel) — here a
:class:`brainevent_amd._csr.Mirror` built by the column-block kernels with the weights moved along, on first use for
matrices large enough for it to pay (``_csr.AUTO_MIRROR_MIN_NNZ``) or by ``prepare(mirror=True)`` — and the gather
kernel otherwise.
"""
from typing import Dict, Optional

import numpy as np
import torch

from . import _array as A
from ._csr import StoredRows, StoredRowsData, rows_step, _step_operand
from . import _csr as _csr_mod
from ._event import is_event, event_operand
from ._misc import _as_int32_indices, check_fixed_conn_num_shape
from ._op import OpKernel
from . import _autograd as _ag

__all__ = ['FixedNumConn', 'FixedNumPerPre', 'FixedNumPerPost', 'binary_fcnmv', 'binary_fcnmm',
           'binary_fcnmv_p', 'binary_fcnmm_p', 'binary_fcnmv_p_call', 'binary_fcnmm_p_call']


def _binary_fcn_hip(weights, indices, operand, *, shape, transpose, workspace=None):
    """An event vector ``[len]`` or a matrix operand ``[len, n_batch]`` through the stored-rows step: rows of ``n_conn`` entries
    each, no ``indptr``."""
    spikes_bm, sd = _step_operand(operand)
    out_bm = rows_step(weights, indices, None, int(indices.shape[1]), spikes_bm, sd, m=indices.shape[0], k=shape[1],
                       transpose=transpose, workspace=workspace)
    return out_bm[0] if operand.ndim == 1 else out_bm.T


binary_fcnmv_p = OpKernel('binary_fcnmv')
binary_fcnmv_p.def_kernel('hip', 'gpu', _binary_fcn_hip, asdefault=True)
binary_fcnmv_p.def_tags('fcn', 'binary')
binary_fcnmm_p = OpKernel('binary_fcnmm')
binary_fcnmm_p.def_kernel('hip', 'gpu', _binary_fcn_hip, asdefault=True)
binary_fcnmm_p.def_tags('fcn', 'binary')


def _fcn_p_call(op, weights, indices, operand, shape, transpose, backend, workspace):
    """Validation and dispatch shared by ``binary_fcnmv_p_call`` / ``binary_fcnmm_p_call`` (``op``: the operator object)."""
    if op is binary_fcnmm_p:
        assert operand.ndim == 2, "matrix must be 2D."
    check_fixed_conn_num_shape(weights, indices, operand, shape, transpose)
    assert weights.dtype.is_floating_point, 'Weights must be a floating-point type.'
    weights = weights.reshape(1) if weights.numel() == 1 else weights
    if _ag.needed(weights, operand):
        def run():
            return op(weights, indices, operand, shape=shape, transpose=transpose, workspace=workspace, backend=backend)
        rows = StoredRows(indices, None, int(indices.shape[1]), int(shape[0]), int(shape[1]))
        return (_ag.rows_product(run, weights, operand, operand, 'nm' if op is binary_fcnmm_p else 'vec', rows, transpose),)
    return (op(weights, indices, operand, shape=shape, transpose=transpose, workspace=workspace, backend=backend),)


def binary_fcnmv_p_call(weights, indices, spikes, *, shape, transpose, backend=None, workspace=None):
    """Validation + dispatch (reference ``brainevent/_fcn/binary.py:450-509``).  Returns a 1-tuple."""
    return _fcn_p_call(binary_fcnmv_p, weights, indices, spikes, shape, transpose, backend, workspace)


def binary_fcnmm_p_call(weights, indices, matrix, *, shape, transpose, backend=None, workspace=None):
    """Validation + dispatch of the matrix op (reference ``brainevent/_fcn/binary.py:1077-1137``)."""
    return _fcn_p_call(binary_fcnmm_p, weights, indices, matrix, shape, transpose, backend, workspace)


binary_fcnmv_p.def_call(binary_fcnmv_p_call)
binary_fcnmm_p.def_call(binary_fcnmm_p_call)


def _fcn_op(p_call, weights, indices, operand, shape, transpose, backend):
    as_np = A.wants_numpy(weights, indices, operand)
    w, idx = A.to_device(weights), A.to_device(indices)
    if idx.dtype != torch.int32:
        idx = _as_int32_indices(idx, None, 'binary_fcn', check_values=False)
    x = operand if isinstance(operand, torch.Tensor) else np.asarray(operand)
    return A.to_result(p_call(w, idx, x, shape=tuple(shape), transpose=transpose, backend=backend)[0], as_np)


def binary_fcnmv(weights, indices, spikes, *, shape, transpose: bool = False, backend: Optional[str] = None):
    """Event-driven product with a fixed-number-connectivity matrix (reference ``_fcn/binary.py:43-143``).

    ``transpose=False``: ``y[i] = sum_c w[i,c] * e(s[indices[i,c]])`` (``y`` has ``shape[0]`` entries);
    ``transpose=True`` : ``y[indices[i,c]] += w[i,c]`` for active ``s[i]`` (``y`` has ``shape[1]`` entries).
    """
    return _fcn_op(binary_fcnmv_p_call, weights, indices, spikes, shape, transpose, backend)


def binary_fcnmm(weights, indices, matrix, *, shape, transpose: bool = False, backend: Optional[str] = None):
    """Matrix-operand version (reference ``_fcn/binary.py:564-675``): ``matrix`` is ``(shape[1], n)`` for
    ``transpose=False`` -> ``(shape[0], n)``; ``(shape[0], n)`` for ``transpose=True`` -> ``(shape[1], n)``."""
    return _fcn_op(binary_fcnmm_p_call, weights, indices, matrix, shape, transpose, backend)


# =====================================================================================================
# containers
# =====================================================================================================
def _validate_fixed_conn_indices(indices, *, expected_rows: int, kind: str):
    if indices.ndim != 2:
        raise ValueError(f'{kind} indices must be 2D, got {indices.ndim}D.')
    if indices.shape[0] != expected_rows:
        raise ValueError(f'{kind} row number mismatch. {indices.shape[0]} != {expected_rows}')
    if indices.dtype.is_floating_point or indices.dtype == torch.bool:
        raise ValueError(f'{kind} indices must be integer type, got {indices.dtype}.')


def _contains_invalid_indices(indices, *, upper_bound: int):
    if indices.numel() == 0:
        return
    lo, hi = int(indices.min()), int(indices.max())
    if lo < 0 or hi >= upper_bound:
        raise ValueError('Found invalid indices in the connection matrix. '
                         f'All indices must be in the range [0, {upper_bound - 1}]. '
                         f'But found indices with min {lo} and max {hi}.')


class FixedNumConn(StoredRowsData):
    """Base of the two ELL containers (reference ``_fcn/main.py:199-460``)."""

    def __init__(self, data, indices=None, *, shape, backend: Optional[str] = None, buffers: Optional[Dict] = None,
                 check_indices: bool = True):
        args = data if indices is None else (data, indices)
        assert len(args) == 2, "Expected two arguments: data, indices."
        self._numpy_result = A.wants_numpy(*args)
        self.data = A.to_device(args[0])
        idx = A.to_device(args[1])
        self.shape = (int(shape[0]), int(shape[1]))
        rows, upper = self.shape[::-1] if self._stored_transposed else self.shape
        _validate_fixed_conn_indices(idx, expected_rows=rows, kind=self._kind)
        self.indices = _as_int32_indices(idx, upper, f'{type(self).__name__} indices', check_values=False)
        if self.data.numel() != 1 and tuple(self.data.shape) != tuple(self.indices.shape):
            raise ValueError(f"Data shape {tuple(self.data.shape)} must match indices shape "
                             f"{tuple(self.indices.shape)}. But got {tuple(self.data.shape)} != {tuple(self.indices.shape)}")
        self.backend = backend
        self._init_buffers(buffers)
        if check_indices:
            _contains_invalid_indices(self.indices, upper_bound=upper)

    _kind = 'Connection'

    # -- properties -------------------------------------------------------------------------------
    num_conn = property(lambda self: int(self.indices.shape[1]))
    nse = property(lambda self: int(self.indices.numel()))
    dtype = property(lambda self: self.data.dtype)
    ndim = property(lambda self: 2)

    def _stored_rows(self) -> StoredRows:
        m, k = self.shape[::-1] if self._stored_transposed else self.shape      # (FixedNumPerPost stores the transpose)
        return StoredRows(self.indices, None, int(self.indices.shape[1]), m, k)

    # -- dispatch (reference ``_binary_matvec`` / ``_binary_matmat`` / ``_dispatch``) -----------------
    def _binary_product(self, op, x, transpose_W: bool):
        rows = self._stored_rows()
        shape = (rows.m, rows.k)
        scatter = transpose_W != self._stored_transposed
        if not scatter:
            mr = self._fresh_mirror(auto=True)
            if mr is not None:           # unfavourable direction, event-driven (reference ``_fcn/main.py:317-326``)
                if op is binary_fcnmm_p:
                    assert x.ndim == 2, "matrix must be 2D."
                check_fixed_conn_num_shape(self.data, self.indices, x, shape, False)
                return mr.apply(x, backend=self.backend)
        return _fcn_p_call(op, self.data, self.indices, x, shape, scatter, self.backend,
                           self._scatter_workspace() if scatter else None)[0]

    def _binary_matvec(self, s, transpose_W: bool):
        return self._binary_product(binary_fcnmv_p, s, transpose_W)

    def _binary_matmat(self, matrix, transpose_W: bool):
        return self._binary_product(binary_fcnmm_p, matrix, transpose_W)

    def _dispatch(self, other, transpose_W: bool):
        if is_event(other) and _ag.needed(self.data, other):
            return _ag.container_product(self, other, transpose_W, lambda: self._dispatch(other, transpose_W))
        if not is_event(other) and _ag.float_needed(self.data, other):
            return _ag.container_float_product(self, other, transpose_W, lambda: self._dispatch(other, transpose_W))
        scatter = transpose_W != self._stored_transposed
        if not is_event(other):     # a dense operand: the float twins (reference ``_fcn/main.py:308-460`` dispatches them alike)
            from ._float import fcnmv_p_call, fcnmm_p_call
            x = other if isinstance(other, torch.Tensor) else np.asarray(other)
            # scatter direction: a gather over the mirror beats float atomics (built on first use only while it keeps its raw arrays)
            mr = self._fresh_mirror(auto=self.nse <= _csr_mod.MIRROR_KEEP_RAW_MAX_NNZ) if scatter else None
            if mr is not None and (mr.released or mr.indices is None):
                mr = None
            if x.ndim not in (1, 2):
                raise NotImplementedError(f"matmul with object of shape {tuple(x.shape)}")
            rows = self._stored_rows()
            if mr is not None:
                from ._float import csrmv_p_call, csrmm_p_call
                if x.ndim == 1:
                    r = csrmv_p_call(mr.data, mr.indices, mr.indptr, x, shape=tuple(mr.shape), transpose=False, backend=self.backend)[0]
                else:
                    r = csrmm_p_call(mr.data, mr.indices, mr.indptr, x.T if transpose_W else x, shape=tuple(mr.shape), transpose=False,
                                     backend=self.backend)[0]
                    r = r.T if transpose_W else r
            elif x.ndim == 1:
                r = fcnmv_p_call(self.data, self.indices, x, shape=(rows.m, rows.k), transpose=scatter, backend=self.backend)[0]
            else:
                r = fcnmm_p_call(self.data, self.indices, x.T if transpose_W else x, shape=(rows.m, rows.k), transpose=scatter,
                                 backend=self.backend)[0]
                r = r.T if transpose_W else r
            return self._res(r) if A.wants_numpy(x) else r
        # scatter kernels take compacted id lists as they are — the favourable direction, and the other one once its mirror exists
        ids = other.ndim == 1 and (scatter or self._fresh_mirror(auto=True) is not None)
        value = event_operand(other, scatter=ids)
        if value.ndim == 1:
            r = self._binary_product(binary_fcnmv_p, value, transpose_W)
        elif value.ndim == 2:
            # binary_fcnmm returns (out_len, n) for an operand (in_len, n): ``events @ M`` hands it the transposed events and
            # transposes the result back.  (The orientation is fixed here, not guessed from the shapes: a square result —
            # batch size equal to the output length — would make such a guess ambiguous.)
            if transpose_W:
                expected = (value.shape[0], self.shape[1])
                r = self._binary_product(binary_fcnmm_p, value.T, transpose_W).T
            else:
                expected = (self.shape[0], value.shape[1])
                r = self._binary_product(binary_fcnmm_p, value, transpose_W)
            if tuple(r.shape) != tuple(expected):
                raise ValueError(f'binary matmat output shape mismatch: got {tuple(r.shape)}, expected {expected}.')
        else:
            raise NotImplementedError(f"matmul with object of shape {value.shape}")
        return self._res(r) if A.wants_numpy(value) else r

    def __matmul__(self, other):
        return self._dispatch(other, transpose_W=False)

    def __rmatmul__(self, other):
        return self._dispatch(other, transpose_W=True)

    # -- conversions (reference ``_fcn/main.py:857-897`` / ``:1118-1160`` fromdense, ``tocsr`` / ``tocsc``) ---------------
    @classmethod
    def fromdense(cls, mat, *, num_conn=None, backend=None):
        """Encode a dense ``(num_pre, num_post)`` matrix: ``num_conn`` connections per pre row (``FixedNumPerPre``) or per
        post column (``FixedNumPerPost``); explicit zeros are absent; short rows are padded with a zero-weight entry at
        index 0; ``num_conn=None`` requires a uniform count.  Host-side helper."""
        dense = mat.cpu().numpy() if isinstance(mat, torch.Tensor) else np.asarray(mat)
        if dense.ndim != 2:
            raise ValueError(f"{cls.__name__}.fromdense expects a 2-D matrix; got {dense.ndim}-D.")
        view = dense.T if cls._stored_transposed else dense
        mask = view != 0
        nnz = mask.sum(axis=1)
        if num_conn is None:
            if view.shape[0] == 0:
                num_conn = 0
            elif not bool((nnz == nnz[0]).all()):
                raise ValueError(f"{cls.__name__}.fromdense: rows have a non-uniform number of connections (min {int(nnz.min())}, "
                                 f"max {int(nnz.max())}). Pass num_conn= to pad to a fixed count, or use CSR.fromdense / "
                                 f"CSC.fromdense for an irregular matrix.")
            else:
                num_conn = int(nnz[0])
        num_conn = int(num_conn)
        if view.shape[0] and bool((nnz > num_conn).any()):
            raise ValueError(f"{cls.__name__}.fromdense: num_conn={num_conn} is too small; a row has {int(nnz.max())} connections.")
        data = np.zeros((view.shape[0], num_conn), dtype=dense.dtype)
        indices = np.zeros((view.shape[0], num_conn), dtype=np.int32)
        for r in range(view.shape[0]):
            cols = np.flatnonzero(mask[r])
            data[r, :cols.size] = view[r, cols]
            indices[r, :cols.size] = cols
        obj = cls((data, indices), shape=dense.shape, backend=backend)
        obj._numpy_result = not isinstance(mat, torch.Tensor)
        return obj

    def _as_compressed(self):
        """(data, indices, indptr) of the stored rows: row ``r`` holds ``num_conn`` entries."""
        n_rows, n_conn = int(self.indices.shape[0]), int(self.indices.shape[1])
        indptr = torch.arange(n_rows + 1, dtype=torch.int64, device=self.indices.device) * n_conn
        if indptr[-1].item() <= np.iinfo(np.int32).max:
            indptr = indptr.to(torch.int32)
        data = self.data if self.data.numel() == 1 else self.data.reshape(-1)
        return data, self.indices.reshape(-1), indptr

    def tocsr(self):
        """The same matrix as a :class:`CSR` (``FixedNumPerPre`` rows are CSR rows; ``FixedNumPerPost`` is re-encoded)."""
        from ._csr import CSR, CSC
        data, idx, ptr = self._as_compressed()
        native = (CSC if self._stored_transposed else CSR)._from_parts(data, idx, ptr, shape=self.shape, backend=self.backend,
                                                                             numpy_result=self._numpy_result)
        return native.tocsr()

    def tocsc(self):
        """The same matrix as a :class:`CSC`."""
        from ._csr import CSR, CSC
        data, idx, ptr = self._as_compressed()
        native = (CSC if self._stored_transposed else CSR)._from_parts(data, idx, ptr, shape=self.shape, backend=self.backend,
                                                                             numpy_result=self._numpy_result)
        return native.tocsc()

    def with_data(self, data):
        data = A.to_device(data)
        assert data.shape == self.data.shape and data.dtype == self.data.dtype
        obj = type(self)((data, self.indices), shape=self.shape, backend=self.backend, check_indices=False)
        obj._numpy_result = self._numpy_result
        return obj

    def todense(self):
        idx = self.indices.cpu().numpy()
        w = (self.data.float() if self.data.dtype == torch.bfloat16 else self.data).cpu().numpy()
        vals = np.broadcast_to(w.reshape(-1), (idx.size,)) if w.size == 1 else w.reshape(-1)
        rows = np.repeat(np.arange(idx.shape[0]), idx.shape[1])
        dense = np.zeros(self.shape[::-1] if self._stored_transposed else self.shape, dtype=vals.dtype)
        np.add.at(dense, (rows, idx.reshape(-1)), vals)
        return dense.T if self._stored_transposed else dense


class FixedNumPerPre(FixedNumConn):
    """Each pre-synaptic neuron has ``n_conn`` post targets: ``indices (n_pre, n_conn)`` hold post ids
    (reference ``_fcn/main.py:781-854``).  ``spk @ M`` is the favourable (scatter) direction."""
    _kind = 'Post-synaptic'

    num_pre = property(lambda self: int(self.indices.shape[0]))
    num_post = property(lambda self: int(self.shape[1]))

    def with_delays(self, delays, depth: int):
        """This matrix with one conduction delay per stored entry (integer steps in ``[0, depth)``, shaped like ``indices``): a
        :class:`~brainevent_amd.DelayedCSR` (the stacked rows no longer have one length), multiplied from the left by a
        :class:`~brainevent_amd.SpikeRing`."""
        from ._delay import DelayedCSR
        return DelayedCSR.of_container(self, None, delays, depth)

    def transpose(self, axes=None):
        assert axes is None, "transpose does not support axes argument."
        obj = FixedNumPerPost((self.data, self.indices), shape=self.shape[::-1], backend=self.backend, check_indices=False)
        obj._numpy_result = self._numpy_result
        return obj

    T = property(lambda self: self.transpose())


class FixedNumPerPost(FixedNumConn):
    """Each post-synaptic neuron has ``n_conn`` pre sources: ``indices (n_post, n_conn)`` hold pre ids
    (reference ``_fcn/main.py:1042-1115``).  ``M @ spk`` is the favourable (scatter) direction."""
    _kind = 'Pre-synaptic'
    _stored_transposed = True

    num_post = property(lambda self: int(self.indices.shape[0]))
    num_pre = property(lambda self: int(self.shape[0]))

    def transpose(self, axes=None):
        assert axes is None, "transpose does not support axes argument."
        obj = FixedNumPerPre((self.data, self.indices), shape=self.shape[::-1], backend=self.backend, check_indices=False)
        obj._numpy_result = self._numpy_result
        return obj

    T = property(lambda self: self.transpose())
