"""FP8 weights for the event-driven dense products: ``Float8Dense``, ``quantize_fp8`` and the FP8 branch of
``binary_densemv`` / ``binary_densemm`` (``csrc/be_dense_f8.hip``, ``be_binary_densemm_f8``).

The formats are OCP: ``e4m3`` is ``torch.float8_e4m3fn`` and ``e5m2`` is ``torch.float8_e5m2`` (never the ``fnuz`` forms).
A product is ``fl32((sum of the decoded weights the active events select) * scale)``: the sum in f32, one f32 ``scale`` per
matrix applied once to the finished sum, the output always f32.  Quantised weights are read-only: no plasticity, arithmetic,
gradients or slicing; ``todense()`` is the way back.

Non-finite codes are refused (the MFMA kernel has no repair path for ``0 * inf``): a byte test on the ``uint8`` view, once per
``(tensor, version)`` — in the container's constructor and on the functional path — and never in a steady-state step.
"""
import weakref
from typing import Optional

import numpy as np
import torch

from . import _array as A
from ._lib import call, fn

__all__ = ['Float8Dense', 'quantize_fp8']

BE_F8_E4M3, BE_F8_E5M2 = 0, 1
_FMT_OF_DTYPE = {torch.float8_e4m3fn: 'e4m3', torch.float8_e5m2: 'e5m2'}
_DTYPE_OF_FMT = {'e4m3': torch.float8_e4m3fn, 'e5m2': torch.float8_e5m2}
_CODE_OF_FMT = {'e4m3': BE_F8_E4M3, 'e5m2': BE_F8_E5M2}
_NONFINITE_MASK = {'e4m3': 0x7f, 'e5m2': 0x7c}      # a code c is non-finite when (c & mask) == mask
FMT_MAX = {'e4m3': 448.0, 'e5m2': 57344.0}


def is_fp8(x) -> bool:
    return isinstance(x, torch.Tensor) and x.dtype in _FMT_OF_DTYPE


def fmt_of(t: torch.Tensor) -> str:
    return _FMT_OF_DTYPE[t.dtype]


def refuse_grad(weights, spikes) -> None:
    """``TypeError`` when a product with FP8 weights would have to be differentiated (grad mode on, an operand requires grad)."""
    if is_fp8(weights) and torch.is_grad_enabled() and any(
            isinstance(x, torch.Tensor) and x.requires_grad for x in (weights, getattr(spikes, 'value', spikes))):
        raise TypeError("FP8 weights are read-only quantised weights: no gradients flow through their products.")


_checked = {}      # id(tensor) -> (weak reference, version at the check)


def check_finite(t: torch.Tensor) -> None:
    """``ValueError`` if the FP8 tensor ``t`` holds an inf / NaN code.  Reads the tensor (on the device: a synchronising
    read) once per ``(tensor, version)``; later calls with the same unchanged tensor return at once."""
    e = _checked.get(id(t))
    if e is not None and e[0]() is t and e[1] == t._version:
        return
    fmt = fmt_of(t)
    m = _NONFINITE_MASK[fmt]
    if t.numel() and bool(((t.view(torch.uint8) & m) == m).any()):
        raise ValueError(f"FP8 ({fmt}) weights hold non-finite codes (inf / NaN): the event-driven products refuse them.")
    key = id(t)
    _checked[key] = (weakref.ref(t, lambda _, k=key: _checked.pop(k, None)), t._version)


def dense_f8_batched(codes: torch.Tensor, scale: float, spikes_bm, sd: int, transpose: bool) -> torch.Tensor:
    """``spikes_bm [nb, k]`` (or ``[nb, ceil(k / 32)]`` words for ``BE_SPIKE_BITS``) -> f32 ``[nb, out_len]`` through
    ``be_binary_densemm_f8``.  ``codes`` is a contiguous FP8 matrix on the device."""
    rows_w, cols_w = int(codes.shape[0]), int(codes.shape[1])
    nb = int(spikes_bm.shape[0])
    out_len = cols_w if transpose else rows_w
    out = torch.empty((nb, out_len), dtype=torch.float32, device=codes.device)
    if out_len == 0 or nb == 0:
        return out
    code = _CODE_OF_FMT[fmt_of(codes)]
    ws = A.workspace(fn('be_binary_densemm_f8_workspace_bytes')(rows_w, cols_w, nb, int(transpose), code))
    call('be_binary_densemm_f8', A.ptr(codes), code, float(scale), A.ptr(spikes_bm), sd, A.ptr(out), rows_w, cols_w, nb,
         int(transpose), A.ptr(ws), ws.numel(), A.stream_ptr())
    return out


def _as_codes(codes, fmt: Optional[str]) -> torch.Tensor:
    """The FP8 tensor of ``codes``: a torch FP8 tensor as it is, or ``uint8`` codes (array / tensor) viewed as ``fmt``."""
    if is_fp8(codes):
        if fmt is not None and fmt != fmt_of(codes):
            raise ValueError(f"fmt={fmt!r} does not match the codes' dtype {codes.dtype}.")
        return codes
    if fmt not in _DTYPE_OF_FMT:
        raise ValueError("uint8 codes need fmt='e4m3' or fmt='e5m2'." if fmt is None else
                         f"unknown FP8 format {fmt!r}: 'e4m3' or 'e5m2'.")
    t = codes if isinstance(codes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(codes)))
    if t.dtype != torch.uint8:
        raise TypeError(f"Float8Dense takes a torch FP8 tensor or uint8 codes, got {t.dtype}: quantize_fp8() makes the codes.")
    return t.view(_DTYPE_OF_FMT[fmt])


def _refuse(what: str):
    def method(self, *args, **kwargs):
        raise TypeError(f"Float8Dense is read-only quantised weights: {what} is not supported; todense() gives the f32 matrix "
                        f"back.")
    method.__name__ = what
    return method


class Float8Dense:
    """Dense matrix of OCP FP8 codes with one f32 ``scale``: the matrix it stands for is ``decode(codes) * scale``.

    ``codes`` is a torch FP8 tensor (``float8_e4m3fn`` / ``float8_e5m2``), or ``uint8`` codes (numpy or torch) together with
    ``fmt='e4m3' | 'e5m2'``.  ``Float8Dense @ events`` and ``events @ Float8Dense`` (``BinaryArray``, ``BitPackedBinary``,
    ``CompactBinary``; 1-D and 2-D) are the event-driven products, f32 out; numpy in -> numpy out as for ``Dense``.  Everything
    that would write or differentiate the weights raises: plain float operands, ``update_on_*``, arithmetic, ``solve``, slicing."""

    def __init__(self, codes, scale: float = 1.0, fmt: Optional[str] = None):
        self._numpy_result = not isinstance(codes, torch.Tensor)
        c = _as_codes(codes, fmt)
        if c.ndim != 2:
            raise ValueError(f"Float8Dense codes must be two-dimensional, got {c.ndim}D.")
        if c.requires_grad:
            raise TypeError("Float8Dense is read-only quantised weights: codes that require grad are not supported.")
        if isinstance(scale, torch.Tensor):
            if scale.requires_grad:
                raise TypeError("Float8Dense is read-only quantised weights: a scale that requires grad is not supported.")
            scale = float(scale)
        scale = float(np.float32(scale))
        if not np.isfinite(scale):
            raise ValueError(f"Float8Dense: scale must be finite, got {scale}.")
        check_finite(c)
        self.codes = c
        self.scale = scale
        self.fmt = fmt_of(c)
        self.shape = (int(c.shape[0]), int(c.shape[1]))
        self._dev = None

    dtype = property(lambda self: self.codes.dtype)
    ndim = property(lambda self: 2)

    def _device_codes(self) -> torch.Tensor:
        if self._dev is None:
            self._dev = A.to_device(self.codes)
        return self._dev

    def todense(self, dtype=torch.float32):
        """``decode(codes) * scale`` (the multiply in f32), as ``dtype``; numpy if the codes came as numpy."""
        w = (self.codes.to(torch.float32) * torch.tensor(self.scale, dtype=torch.float32, device=self.codes.device)).to(dtype)
        return A.to_result(w, self._numpy_result) if self._numpy_result else w

    def transpose(self, axes=None) -> 'Float8Dense':
        assert axes is None, f"axes must be None, got {axes}."
        out = Float8Dense(self.codes.view(torch.uint8).T.contiguous().view(self.codes.dtype), scale=self.scale)
        out._numpy_result = self._numpy_result
        return out

    T = property(lambda self: self.transpose())

    def _event(self, other):
        from ._event import is_event, event_operand
        if not is_event(other):
            raise TypeError("Float8Dense multiplies event operands only (BinaryArray, BitPackedBinary, CompactBinary); for a "
                            "plain float operand use todense().")
        ev = event_operand(other)
        if isinstance(ev, torch.Tensor) and ev.requires_grad:
            raise TypeError("Float8Dense is read-only quantised weights: no gradients flow through its products.")
        if ev.ndim not in (1, 2):
            raise NotImplementedError(f"matmul with object of shape {tuple(ev.shape)}")
        return ev

    def _product(self, ev, transpose: bool):
        k = self.shape[0] if transpose else self.shape[1]
        if ev.ndim == 1:
            if int(ev.shape[0]) != k:
                raise ValueError(f"shapes {tuple(ev.shape)} and {self.shape} are not aligned for the product.")
            s, sd = A.spikes_to_device(ev)
            r = dense_f8_batched(self._device_codes(), self.scale, s.reshape(1, -1), sd, transpose)[0]
        else:              # ``ev`` is [k, nb] here (the operand convention of binary_densemm)
            if int(ev.shape[0]) != k:
                raise ValueError(f"shapes {tuple(ev.shape)} and {self.shape} are not aligned for the product.")
            spikes_bm, sd = A.spikes_batch_major(ev)
            r = dense_f8_batched(self._device_codes(), self.scale, spikes_bm, sd, transpose).T
        return r

    def __matmul__(self, other):          # W8 @ events
        ev = self._event(other)
        return A.to_result(self._product(ev, False), self._numpy_result and A.wants_numpy(ev))

    def __rmatmul__(self, other):         # events @ W8
        ev = self._event(other)
        r = self._product(ev, True) if ev.ndim == 1 else self._product(ev.T, True).T
        return A.to_result(r, self._numpy_result and A.wants_numpy(ev))

    def __repr__(self):
        return f"Float8Dense(shape={self.shape}, fmt={self.fmt}, scale={self.scale!r})"

    __getitem__ = _refuse('slicing')
    solve = _refuse('solve')
    with_data = _refuse('with_data')
    diag_add = _refuse('diag_add')
    update_on_pre = _refuse('update_on_pre')
    update_on_post = _refuse('update_on_post')
    update_on_binary_pre = _refuse('update_on_binary_pre')
    update_on_binary_post = _refuse('update_on_binary_post')


for _n in ('add', 'radd', 'iadd', 'sub', 'rsub', 'isub', 'mul', 'rmul', 'imul', 'truediv', 'rtruediv', 'itruediv', 'pow', 'neg',
           'pos', 'abs', 'imatmul'):
    setattr(Float8Dense, f'__{_n}__', _refuse(f'arithmetic (__{_n}__)'))


def quantize_fp8(W, fmt: str = 'e4m3', scale: Optional[float] = None) -> Float8Dense:
    """``Float8Dense`` of the float matrix ``W``: codes ``= cast(clamp(W / scale, ±FMT_MAX))`` with torch's round-to-nearest-even,
    ``scale = amax(|W|) / FMT_MAX`` (1 for an all-zero matrix) unless given; ``FMT_MAX`` is 448 (e4m3) / 57344 (e5m2).  The
    clamp is what keeps an out-of-range value from becoming NaN (e4m3fn) or inf (e5m2) in the cast.  Plain torch, not a hot path."""
    if fmt not in _DTYPE_OF_FMT:
        raise ValueError(f"unknown FP8 format {fmt!r}: 'e4m3' or 'e5m2'.")
    as_np = not isinstance(W, torch.Tensor)
    w = torch.from_numpy(np.ascontiguousarray(np.asarray(W))) if as_np else W.detach()
    if not w.dtype.is_floating_point or w.dtype in _FMT_OF_DTYPE:
        raise TypeError(f"quantize_fp8 takes a float matrix, got {w.dtype}.")
    if w.ndim != 2:
        raise ValueError(f"quantize_fp8 takes a two-dimensional matrix, got {w.ndim}D.")
    w = w.to(torch.float32)
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_fp8: the matrix holds non-finite values.")
    fmax = FMT_MAX[fmt]
    if scale is None:
        amax = float(w.abs().max()) if w.numel() else 0.0
        scale = float(np.float32(amax) / np.float32(fmax)) if amax > 0 else 1.0
    scale = float(np.float32(scale))
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"quantize_fp8: scale must be a positive finite number, got {scale}.")
    codes = (w / torch.tensor(scale, dtype=torch.float32, device=w.device)).clamp(-fmax, fmax).to(_DTYPE_OF_FMT[fmt])
    out = Float8Dense(codes, scale=scale)
    out._numpy_result = as_np
    return out
