"""Event-driven dense products: ``binary_densemv`` / ``binary_densemm`` (the ``BinaryArray @ ndarray`` path).

Reference surface (read as text): ``brainevent/_dense/binary.py:79-165`` (``binary_densemv``), ``:347-432``
(``binary_densemv_p_call``), ``:487-576`` (``binary_densemm``), ``:818-912`` (``binary_densemm_p_call``),
``:168-211`` / ``:579-632`` (CPU semantics).

  transpose=False: ``weights[m, k] @ spikes[k]      -> out[m]``     /  ``weights[m, k] @ spikes[k, n] -> out[m, n]``
  transpose=True : ``spikes[k] @ weights[k, n]      -> out[n]``     /  ``weights[k, m].T @ spikes[k, n] -> out[m, n]``

Non-bool, non-float spikes are cast to bool first (reference ``:162-163``); float spikes are active when
``> 0`` (the documented binary semantics; the reference's ``jax_raw`` multiply-by-value shortcut is not followed).
"""
from typing import Optional

import numpy as np
import torch

from . import _array as A
from ._data import DataRepresentation
from ._lib import call, fn
from ._op import OpKernel
from ._plasticity import PlasticityMixin
from ._arith import ArithmeticMixin, as_operand, broadcast_check, is_matrix
from . import _autograd as _ag
from . import _dense_f8 as _f8

__all__ = ['Dense', 'binary_densemv', 'binary_densemm', 'binary_densemv_p', 'binary_densemm_p', 'binary_densemv_p_call',
           'binary_densemm_p_call']


def _dense_batched(weights: torch.Tensor, spikes_bm: torch.Tensor, sd: int, transpose: bool) -> torch.Tensor:
    """``spikes_bm [nb, k]`` -> ``[nb, out_len]`` through ``be_binary_densemm_{transpose,no_transpose}_*``."""
    if _f8.is_fp8(weights):        # OCP FP8 codes: their own kernels (be_dense_f8.hip), scale 1, f32 out
        _f8.check_finite(weights)
        return _f8.dense_f8_batched(weights, 1.0, spikes_bm, sd, transpose)
    rows_w, cols_w = int(weights.shape[0]), int(weights.shape[1])
    nb = int(spikes_bm.shape[0])
    out_len = cols_w if transpose else rows_w
    out = torch.empty((nb, out_len), dtype=weights.dtype, device=weights.device)
    if out_len == 0 or nb == 0:
        return out
    ws = A.workspace(fn('be_binary_densemm_workspace_bytes')(rows_w, cols_w, nb, int(transpose), A.wcode(weights)))
    if sd == A.BE_SPIKE_BITS:      # bit-packed rows [nb, ceil(k / 32)] words: the generic entry point (the per-variant names cover bool / float)
        call('be_binary_densemm', A.ptr(weights), A.wcode(weights), A.ptr(spikes_bm), sd, A.ptr(out), rows_w, cols_w, nb,
             int(transpose), A.ptr(ws), ws.numel(), A.stream_ptr())
        return out
    name = (f"be_binary_densemm_{'transpose' if transpose else 'no_transpose'}_{A.wsuffix(weights)}_"
            f"{'bool' if sd == A.BE_SPIKE_BOOL else 'float'}")
    call(name, A.ptr(weights), A.ptr(spikes_bm), A.ptr(out), rows_w, cols_w, nb, A.ptr(ws), ws.numel(), A.stream_ptr())
    return out


def _binary_densemv_hip(weights, spikes, *, transpose):
    w = A.to_device(weights)
    s, sd = A.spikes_to_device(spikes)
    return _dense_batched(w, s.reshape(1, -1), sd, transpose)[0]


def _binary_densemm_hip(weights, spikes, *, transpose):
    w = A.to_device(weights)
    spikes_bm, sd = A.spikes_batch_major(spikes)
    return _dense_batched(w, spikes_bm, sd, transpose).T


binary_densemv_p = OpKernel('binary_densemv')
binary_densemv_p.def_kernel('hip', 'gpu', _binary_densemv_hip, asdefault=True)
binary_densemv_p.def_tags('dense', 'binary')
binary_densemm_p = OpKernel('binary_densemm')
binary_densemm_p.def_kernel('hip', 'gpu', _binary_densemm_hip, asdefault=True)
binary_densemm_p.def_tags('dense', 'binary')


def binary_densemv_p_call(weights, spikes, *, transpose, backend=None):
    assert weights.ndim == 2 and spikes.ndim == 1, "weights must be 2D and spikes 1D."
    if transpose:
        assert spikes.shape[0] == weights.shape[0], (
            f"shapes {tuple(spikes.shape)} and {tuple(weights.shape)} not aligned: "
            f"{spikes.shape[0]} (dim 0) != {weights.shape[0]} (dim 0)")
    else:
        assert spikes.shape[0] == weights.shape[1], (
            f"spikes shape {tuple(spikes.shape)} and weights shape {tuple(weights.shape)} are not compatible")
    _f8.refuse_grad(weights, spikes)
    if _ag.needed(weights, spikes):
        return [_ag.dense_product(lambda: binary_densemv_p(weights, spikes, transpose=transpose, backend=backend), weights, spikes,
                                  spikes, 'vec', transpose=transpose)]
    return [binary_densemv_p(weights, spikes, transpose=transpose, backend=backend)]


binary_densemv_p.def_call(binary_densemv_p_call)


def binary_densemm_p_call(weights, spikes, *, transpose, backend=None):
    assert weights.ndim == 2 and spikes.ndim == 2, "weights and spikes must be 2D."
    if transpose:
        assert weights.shape[0] == spikes.shape[0], (
            f"weights shape {tuple(weights.shape)} and spikes shape {tuple(spikes.shape)} do not match for event matrix "
            f"multiplication: weights dim 0 ({weights.shape[0]}) != spikes dim 0 ({spikes.shape[0]})")
    else:
        assert weights.shape[1] == spikes.shape[0], (
            f"weights.shape[1] ({weights.shape[1]}) != spikes.shape[0] ({spikes.shape[0]}), "
            f"weights: {tuple(weights.shape)}, spikes: {tuple(spikes.shape)}")
    _f8.refuse_grad(weights, spikes)
    if _ag.needed(weights, spikes):
        return [_ag.dense_product(lambda: binary_densemm_p(weights, spikes, transpose=transpose, backend=backend), weights, spikes,
                                  spikes, 'nm', transpose=transpose)]
    return [binary_densemm_p(weights, spikes, transpose=transpose, backend=backend)]


binary_densemm_p.def_call(binary_densemm_p_call)


def _as_arr(x):
    return x if isinstance(x, (torch.Tensor, A.PackedSpikes)) else np.asarray(x)


def _float_weights(w):
    dt = w.dtype
    ok = dt.is_floating_point if isinstance(w, torch.Tensor) else np.issubdtype(dt, np.floating)
    assert ok, 'Weights must be a floating-point type.'
    if _f8.is_fp8(w):              # non-finite codes are refused here, before any device call (once per tensor version)
        _f8.check_finite(w)


def binary_densemv(weights, spikes, *, transpose, backend: Optional[str] = None):
    """``weights[m,k] @ spikes[k]`` (``transpose=False``) or ``spikes[k] @ weights[k,n]`` (``transpose=True``)."""
    as_np = A.wants_numpy(weights, spikes)
    w, s = _as_arr(weights), _as_arr(spikes)
    _float_weights(w)
    return A.to_result(binary_densemv_p_call(w, s, transpose=transpose, backend=backend)[0], as_np)


def binary_densemm(weights, spikes, *, transpose, backend: Optional[str] = None):
    """``weights[m,k] @ spikes[k,n]`` (``transpose=False``) or ``weights[k,m].T @ spikes[k,n]`` (``transpose=True``)."""
    as_np = A.wants_numpy(weights, spikes)
    w, s = _as_arr(weights), _as_arr(spikes)
    _float_weights(w)
    return A.to_result(binary_densemm_p_call(w, s, transpose=transpose, backend=backend)[0], as_np)


class Dense(PlasticityMixin, ArithmeticMixin, DataRepresentation):
    """Explicit dense matrix with the representation contract of the sparse families (reference
    ``brainevent/_dense/main.py:60-510``, minus units and pytree plumbing): ``data``, ``shape``,
    ``backend``, ``buffers``, ``with_data``, ``todense``, ``T`` / ``transpose`` and event-driven ``@``.

    ``Dense @ events`` -> ``binary_densemv/mm(transpose=False)``; ``events @ Dense`` -> ``transpose=True``
    (``_dense/main.py:426-476``).  Non-event operands are outside the accelerated path."""

    def __init__(self, data, shape=None, backend: Optional[str] = None, buffers: Optional[dict] = None):
        self._numpy_result = not isinstance(data, torch.Tensor)
        self.data = A.to_device(data)
        if self.data.ndim != 2:
            raise ValueError(f"Dense data must be two-dimensional, got {self.data.ndim}D.")
        if shape is not None and tuple(shape) != tuple(self.data.shape):
            raise ValueError(f"shape {tuple(shape)} does not match the data shape {tuple(self.data.shape)}.")
        self.shape = (int(self.data.shape[0]), int(self.data.shape[1]))
        self.backend = backend
        self._init_buffers(buffers)

    dtype = property(lambda self: self.data.dtype)
    ndim = property(lambda self: 2)

    def with_data(self, data) -> 'Dense':
        d = A.to_device(data)
        assert tuple(d.shape) == tuple(self.data.shape) and d.dtype == self.data.dtype
        out = Dense(d, shape=self.shape, backend=self.backend, buffers=self.buffers)
        out._numpy_result = self._numpy_result
        return out

    def todense(self):
        return A.to_result(self.data, self._numpy_result)

    def transpose(self, axes=None) -> 'Dense':
        assert axes is None, f"axes must be None, got {axes}."
        out = Dense(self.data.T.contiguous(), shape=self.shape[::-1], backend=self.backend, buffers=self.buffers)
        out._numpy_result = self._numpy_result
        return out

    T = property(lambda self: self.transpose())

    def quantize(self, fmt: str = 'e4m3', scale=None):
        """``quantize_fp8(self.data, fmt, scale)``: the read-only ``Float8Dense`` twin of this matrix."""
        out = _f8.quantize_fp8(self.data, fmt=fmt, scale=scale)
        out._numpy_result = self._numpy_result
        return out

    def __getitem__(self, index):
        return self.todense()[index]

    # -- arithmetic: plain torch on ``data`` (reference ``_dense/main.py:231-320``, ``:391-406``) -------------------------
    def _wrap(self, data) -> 'Dense':
        out = Dense(data, backend=self.backend, buffers=self.buffers)
        out._numpy_result = self._numpy_result
        return out

    def _unitary_op(self, op) -> 'Dense':
        return self._wrap(op(self.data))

    def _binary_operand_data(self, other):
        """The operand as torch takes it beside ``data``; it has to broadcast to exactly ``shape`` (``ValueError``)."""
        if isinstance(other, Dense):
            if other.shape != self.shape:
                raise ValueError(f"Dense operand shape {other.shape} is not compatible with shape {self.shape}.")
            return other.data
        if is_matrix(other):
            raise NotImplementedError("binary operation between Dense and sparse objects.")
        x = as_operand(other)
        if broadcast_check(self.shape, x.shape, 'Dense') != tuple(self.shape):
            raise ValueError(f"operand shape {tuple(x.shape)} broadcasts beyond the Dense shape {self.shape}.")
        if x.ndim == 0 and not isinstance(x, torch.Tensor):
            return x.item()
        return A.to_device(x) if not isinstance(x, torch.Tensor) else (x if x.device == self.data.device else x.to(self.data.device))

    def _binary_op(self, other, op) -> 'Dense':
        return self._wrap(op(self.data, self._binary_operand_data(other)))

    def _binary_rop(self, other, op) -> 'Dense':
        return self._wrap(op(self._binary_operand_data(other), self.data))

    def diag_add(self, other) -> 'Dense':
        """``self + diag(other)``: a copy with ``other`` (length ``min(shape)``, ``ValueError`` otherwise) added on the
        diagonal."""
        d = as_operand(other)
        n = min(self.shape)
        if d.ndim != 1 or int(d.shape[0]) != n:
            raise ValueError(f"Dense.diag_add: the diagonal must have shape ({n},), got {tuple(d.shape)}.")
        out = self.data.clone()
        out.diagonal().add_(A.to_device(d, dtype=out.dtype))
        return self._wrap(out)

    def solve(self, b, tol=1e-6, reorder=1, *, rtol=None, maxiter=1000, x0=None, return_info=False):
        """Solve the dense system ``self @ x = b`` by ``torch.linalg.solve`` (reference ``_dense/main.py:408-424``, with its two
        assertions).  ``tol`` and ``reorder`` are accepted for parity with the sparse solvers and unused, as in the reference; so
        are ``rtol``, ``maxiter`` and ``x0`` of the iterative sparse method.  ``return_info=True`` adds the dict of a direct
        solve: zero iterations and restarts, ``residual`` the measured ``|b - A x|_2 / |b|_2`` (one dense product; 0 for
        ``b == 0``) and ``converged`` whether that figure is finite — a direct solve has no ``rtol`` to meet."""
        from ._solve import dense_solve
        return dense_solve(self, b, return_info=return_info)

    def _event(self, other):
        from ._event import is_event, event_operand
        if not is_event(other):
            raise NotImplementedError("only event operands are on the accelerated path (plain dense matmul is out of scope).")
        return event_operand(other)        # (1-D bit-packed containers hand their words over: BE_SPIKE_BITS)

    def __matmul__(self, other):          # dense @ events
        ev = self._event(other)
        if ev.ndim == 1:
            r = binary_densemv_p_call(self.data, ev, transpose=False, backend=self.backend)[0]
        elif ev.ndim == 2:
            r = binary_densemm_p_call(self.data, ev, transpose=False, backend=self.backend)[0]
        else:
            raise NotImplementedError(f"matmul with object of shape {ev.shape}")
        return A.to_result(r, self._numpy_result and A.wants_numpy(ev))

    def __rmatmul__(self, other):         # events @ dense
        ev = self._event(other)
        if ev.ndim == 1:
            r = binary_densemv_p_call(self.data, ev, transpose=True, backend=self.backend)[0]
        elif ev.ndim == 2:
            r = binary_densemm_p_call(self.data, ev.T, transpose=True, backend=self.backend)[0].T
        else:
            raise NotImplementedError(f"matmul with object of shape {ev.shape}")
        return A.to_result(r, self._numpy_result and A.wants_numpy(ev))

    def __repr__(self):
        return f"Dense(shape={self.shape}, dtype={self.dtype}, backend={self.backend})"
