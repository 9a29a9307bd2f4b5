"""FP8 weights for the event-driven CSR products: ``Float8CSR``, ``CSR.quantize_fp8`` and the q8 scatter plan
(``csrc/be_csr_f8.hip``, the q8 layout of ``csrc/be_csr_plan.hip``).

A stored entry is one OCP FP8 code (``e4m3`` = ``torch.float8_e4m3fn``, ``e5m2`` = ``torch.float8_e5m2``; never the ``fnuz`` forms)
and the matrix is ``decode(codes) * scale`` with one f32 ``scale``.  Every finite code is an integer multiple of ``2^-E`` (``E`` = 9 /
16), so ``events @ W8`` sums exact 64-bit integers and rounds once: ``out[j] = f32(f64(R_j) * ldexp(f64(f32(scale)), -E))`` — the same
bits on the planned route (2 bytes per synapse) and on the direct route (global integer atomics), whatever the geometry.  The
semantics are stated in ``include/brainevent_amd.h``.  Quantised weights are read-only, as ``Float8Dense``'s are.
"""
import ctypes
from typing import Optional

import numpy as np
import torch

from . import _array as A
from . import _csr as C
from . import _dense_f8 as F8
from ._lib import call, fn
from ._misc import _as_indptr, _as_int32_indices, _check_compressed_structure

__all__ = ['Float8CSR', 'Q8Plan', 'csr_quantize_fp8']

F8_EXP = {'e4m3': 9, 'e5m2': 16}      # Q(c) = decode(c) * 2^E is an integer for every finite code
_QUANT_SLAB = 1 << 27                 # entries quantised at a time by csr_quantize_fp8


class Q8Plan:
    """The q8 scatter plan of a ``Float8CSR``: ``seg`` / ``blob`` as ``ScatterPlan``'s, blocks of ``[uint8 code][uint8 delta]``
    (sorted columns, d8's delta / escape / pad rules).  It takes rows of at most 16384 entries and at most 1024 slices;
    :meth:`applies` says whether a matrix fits, and the direct route serves the rest.  Geometry comes from ``ScatterPlan``'s helpers
    with the d8 limits (64-bit accumulators, 20000 columns per slice).  One workspace per ``(parts, n_batch)``, never evicted (a
    captured graph keeps its pointer); calls on one plan must be ordered on a stream."""
    MAX_ROW, MAX_SLICES, CAP = C.ScatterPlan.D8_MAX_ROW, C.ScatterPlan.D8_MAX_SLICES, C.ScatterPlan.D8_CAP

    def __init__(self, m, k, nnz, slice_shift, slice_width, seg, blob, block_hint):
        self.m, self.k, self.nnz = int(m), int(k), int(nnz)
        self.slice_shift, self.slice_width = int(slice_shift), int(slice_width)
        self.n_slices = (self.k + self.slice_width - 1) // self.slice_width
        self.seg, self.blob = seg, blob
        self.block_hint = int(block_hint)
        self._ws = {}

    @classmethod
    def geometry(cls, m: int, k: int, nnz: int, slice_shift: Optional[int] = None, slice_width: Optional[int] = None):
        """``(slice_shift, slice_width)``: the capacity of 64-bit sums and ``ScatterPlan.auto_geometry``'s pass-sized delta width."""
        if slice_shift is None:
            slice_shift = C.ScatterPlan.default_shift(k, False)
        if slice_width is None:
            slice_width = C.ScatterPlan.auto_geometry(m, k, nnz, False, slice_shift, delta_ok=True, force='delta')[1]
        return int(slice_shift), int(slice_width)

    @classmethod
    def applies(cls, m: int, k: int, nnz: int, max_row: int) -> bool:
        if m <= 0 or k <= 0 or nnz <= 0 or max_row > cls.MAX_ROW:
            return False
        _, w = cls.geometry(m, k, nnz)
        return -(-k // w) <= cls.MAX_SLICES

    @classmethod
    def build(cls, codes: torch.Tensor, indices: torch.Tensor, indptr: torch.Tensor, *, shape, slice_shift: Optional[int] = None,
              slice_width: Optional[int] = None) -> 'Q8Plan':
        """Count -> scan -> fill on the device (``be_scatter_plan_q8_count`` / ``_fill``); the rows' column order written by the
        count pass is read back by the fill and then freed (the weights are read-only: there is no refresh)."""
        m, k = int(shape[0]), int(shape[1])
        codes = A.to_device(codes).view(torch.uint8).reshape(-1)
        indices, indptr = A.to_device(indices).reshape(-1), A.to_device(indptr)
        assert indices.dtype == torch.int32 and indptr.dtype in (torch.int32, torch.int64)
        nnz = int(indices.numel())
        slice_shift, slice_width = cls.geometry(m, k, nnz, slice_shift, slice_width)
        n_slices = -(-k // slice_width)
        dev, st = A.device(), A.stream_ptr()
        is64 = int(indptr.dtype == torch.int64)
        seg = torch.empty(n_slices * m * 2, dtype=torch.int32, device=dev)
        scratch = A.workspace(fn('be_scatter_plan_q8_scratch_bytes')(m, k, slice_shift, slice_width))
        order = torch.empty(max(nnz, 1), dtype=torch.int16, device=dev)
        blob_bytes = ctypes.c_int64(0)
        call('be_scatter_plan_q8_count', A.ptr(indices), A.ptr(indptr), is64, -1, m, k, slice_shift, slice_width, A.ptr(seg),
             A.ptr(scratch), scratch.numel(), ctypes.byref(blob_bytes), A.ptr(order), st)
        blob = torch.empty(int(blob_bytes.value) + 128, dtype=torch.uint8, device=dev)
        call('be_scatter_plan_q8_fill', A.ptr(codes), A.ptr(indices), A.ptr(indptr), is64, -1, m, k, slice_shift, slice_width,
             A.ptr(seg), A.ptr(blob), A.ptr(order), st)
        # average stored items (entries + escapes) per block, from a strided sample of the table's lane-group counts
        n_blk = m * n_slices
        ng = seg.view(n_blk, 2)[::max(1, n_blk >> 22), 1] & 0xffff
        hint = max(1, min(1 << 20, int(round(4.0 * ng.double().mean().item())))) if nnz else 0
        return cls(m, k, nnz, slice_shift, slice_width, seg, blob, hint)

    def nbytes(self) -> int:
        return self.seg.numel() * 4 + self.blob.numel()

    def default_parts(self) -> int:
        return C.ScatterPlan.parts_for(self.n_slices, self.nnz)

    def workspace(self, parts: int, n_batch: int = 1) -> torch.Tensor:
        key = (parts, n_batch)
        ws = self._ws.get(key)
        if ws is None:
            ws = A.workspace(fn('be_binary_csrmm_t_plan_f8_workspace_bytes')(self.m, self.k, n_batch, self.slice_shift,
                                                                             self.slice_width, parts, self.block_hint))
            ws[:4 * max(n_batch, 64)].zero_()      # spike counters: zero on entry, re-armed by every call
            self._ws[key] = ws
        return ws

    def step(self, fmt_code: int, scale: float, spikes_bm, sd: int, out_bm: torch.Tensor, parts: Optional[int] = None) -> None:
        nb = int(out_bm.shape[0])
        parts = self.default_parts() if parts is None else int(parts)
        if nb > 1:
            parts = max(1, min(parts, 512 // (self.n_slices * nb)))
        ws = self.workspace(parts, nb)
        call('be_binary_csrmm_t_plan_f8', A.ptr(self.blob), A.ptr(self.seg), fmt_code, float(scale), A.ptr(spikes_bm), sd,
             A.ptr(out_bm), self.m, self.k, nb, self.slice_shift, self.slice_width, self.block_hint, parts, A.ptr(ws), ws.numel(),
             A.stream_ptr())


def f8_direct(codes: torch.Tensor, fmt_code: int, scale: float, indices, indptr, spikes_bm, sd: int, out_bm: torch.Tensor,
              m: int, k: int) -> None:
    """``be_binary_csrmm_t_f8``: batch-major spikes ``[nb, m]`` -> f32 ``out_bm [nb, k]``, any spike encoding."""
    nb = int(out_bm.shape[0])
    ws = A.workspace(fn('be_binary_csrmm_t_f8_workspace_bytes')(m, k, nb))
    call('be_binary_csrmm_t_f8', A.ptr(codes), fmt_code, float(scale), A.ptr(indices), A.ptr(indptr),
         int(indptr.dtype == torch.int64), -1, int(indices.numel()), A.ptr(spikes_bm), sd, A.ptr(out_bm), m, k, nb, A.ptr(ws),
         ws.numel(), A.stream_ptr())


def _refuse(what: str):
    def method(self, *args, **kwargs):
        raise TypeError(f"Float8CSR is read-only quantised weights: {what} is not supported; tocsr() gives the f32 CSR back.")
    method.__name__ = what
    return method


def _as_host_or_device(x) -> torch.Tensor:
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))


class Float8CSR:
    """CSR matrix of OCP FP8 codes with one f32 ``scale``: the matrix it stands for is ``decode(codes) * scale`` at the stored
    positions (duplicates add).

    ``Float8CSR((codes, indices, indptr), shape=(m, k), scale=1.0, fmt=None)``: ``codes`` is a torch FP8 tensor, or ``uint8`` codes
    (numpy or torch) together with ``fmt='e4m3' | 'e5m2'``; ``indptr`` int32 or int64.  ``events @ W8`` (``BinaryArray``,
    ``BitPackedBinary``, ``CompactBinary``; 1-D and batched ``[nb, m]``) is the event-driven product, f32 out, numpy in -> numpy
    out; it is exact (see the module docstring) and takes the q8 plan — built by :meth:`prepare` or the first product — when the
    matrix has at least ``PLAN_MIN_NNZ`` entries and the sorted layout holds it, else the direct route: same bits.  Everything
    that would write or differentiate the weights raises, a plain float operand gets ``TypeError`` (use :meth:`tocsr`), and the
    gather direction ``W8 @ events`` is not built (``NotImplementedError``)."""

    def __init__(self, args, *, shape, scale: float = 1.0, fmt: Optional[str] = None):
        assert len(args) == 3, "Expected three arguments: codes, indices, indptr."
        codes_arg, indices_arg, indptr_arg = args
        self._numpy_result = A.wants_numpy(codes_arg, indices_arg, indptr_arg)
        if not (F8.is_fp8(codes_arg) or _is_u8(codes_arg)):
            dt = codes_arg.dtype if hasattr(codes_arg, 'dtype') else type(codes_arg).__name__
            raise TypeError(f"Float8CSR takes a torch FP8 tensor or uint8 codes, got {dt}: CSR.quantize_fp8() makes the codes.")
        c = F8._as_codes(codes_arg, fmt)
        if c.ndim != 1:
            raise ValueError(f"Float8CSR codes must be one-dimensional (one per stored entry), got {c.ndim}D.")
        if c.requires_grad:
            raise TypeError("Float8CSR is read-only quantised weights: codes that require grad are not supported.")
        if isinstance(scale, torch.Tensor):
            if scale.requires_grad:
                raise TypeError("Float8CSR is read-only quantised weights: a scale that requires grad is not supported.")
            scale = float(scale)
        scale = float(np.float32(scale))
        if not np.isfinite(scale):
            raise ValueError(f"Float8CSR: scale must be finite, got {scale}.")
        shape = (int(shape[0]), int(shape[1]))
        context = "Float8CSR constructor"
        indices = _as_int32_indices(_as_host_or_device(indices_arg), shape[1], context, check_values=True)
        indptr = _as_indptr(_as_host_or_device(indptr_arg), int(indices.shape[0]), "auto", context)
        _check_compressed_structure(indices, indptr, shape, format='csr', check_values=True)
        if int(c.shape[0]) != int(indices.shape[0]):
            raise ValueError(f"Float8CSR: {int(c.shape[0])} codes for {int(indices.shape[0])} indices.")
        F8.check_finite(c)
        self.codes, self.indices, self.indptr = c, indices, indptr
        self.scale = scale
        self.fmt = F8.fmt_of(c)
        self.shape = shape
        self._dev = None
        self._plan: Optional[Q8Plan] = None
        self._max_row: Optional[int] = None

    dtype = property(lambda self: self.codes.dtype)
    ndim = property(lambda self: 2)
    nse = property(lambda self: int(self.indices.shape[0]))

    def _device_arrays(self):
        if self._dev is None:
            self._dev = (A.to_device(self.codes), A.to_device(self.indices), A.to_device(self.indptr))
        return self._dev

    def _dequantised(self) -> torch.Tensor:
        return self.codes.to(torch.float32) * torch.tensor(self.scale, dtype=torch.float32, device=self.codes.device)

    def todense(self, dtype=torch.float32):
        """``decode(codes) * scale`` (the multiply in f32) scattered to ``shape``, duplicates summed in f32, as ``dtype``; numpy if
        the arrays came as numpy.  Host-side helper for tests and small matrices."""
        w = self._dequantised().cpu()
        ptr = self.indptr.cpu().to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(self.shape[0], dtype=torch.int64), ptr[1:] - ptr[:-1])
        out = torch.zeros(self.shape, dtype=torch.float32)
        out.index_put_((rows, self.indices.cpu().to(torch.int64)), w, accumulate=True)
        out = out.to(dtype)
        return out.numpy() if self._numpy_result else out

    def tocsr(self, dtype=torch.float32):
        """The dequantised ``CSR`` (``decode(codes) * scale`` as ``dtype``) over the same ``indices`` / ``indptr``."""
        out = C.CSR._from_parts(A.to_device(self._dequantised().to(dtype)), A.to_device(self.indices), A.to_device(self.indptr),
                                shape=self.shape, numpy_result=self._numpy_result)
        return out

    # -- route --------------------------------------------------------------------------------------
    def _planned(self) -> bool:
        m, k = self.shape
        if self.nse < C.PLAN_MIN_NNZ:
            return False
        if self._max_row is None:
            self._max_row = int((self.indptr[1:] - self.indptr[:-1]).max()) if m > 0 else 0
        return Q8Plan.applies(m, k, self.nse, self._max_row)

    def _scatter_plan(self) -> Optional[Q8Plan]:
        if self._plan is None and self._planned():
            codes, indices, indptr = self._device_arrays()
            self._plan = Q8Plan.build(codes, indices, indptr, shape=self.shape)
        return self._plan

    def prepare(self) -> 'Float8CSR':
        """Build the q8 plan now (otherwise the first product builds it).  A matrix the plan does not take — fewer than
        ``PLAN_MIN_NNZ`` entries, a row above 16384 entries, more than 1024 slices — has nothing to prepare: its products run
        on the direct route."""
        self._device_arrays()
        self._scatter_plan()
        return self

    # -- products -----------------------------------------------------------------------------------
    def _event(self, other):
        from ._event import is_event, event_operand
        if not is_event(other):
            raise TypeError("Float8CSR multiplies event operands only (BinaryArray, BitPackedBinary, CompactBinary); for a plain "
                            "float operand use tocsr().")
        ev = event_operand(other, scatter=True)
        if isinstance(ev, torch.Tensor) and ev.requires_grad:
            raise TypeError("Float8CSR is read-only quantised weights: no gradients flow through its products.")
        if ev.ndim not in (1, 2):
            raise NotImplementedError(f"matmul with object of shape {tuple(ev.shape)}")
        return ev

    def __rmatmul__(self, other):          # events @ W8: the scatter over the active rows
        ev = self._event(other)
        m, k = self.shape
        if int(ev.shape[-1]) != m:
            raise ValueError(f"shapes {tuple(ev.shape)} and {self.shape} are not aligned for the product.")
        if ev.ndim == 1:
            s, sd = A.spikes_to_device(ev)
            spikes_bm = s.reshape(1, -1)
        else:
            spikes_bm, sd = A.spikes_batch_major(ev.T)
        nb = int(spikes_bm.shape[0])
        out = torch.empty((nb, k), dtype=torch.float32, device=A.device())
        if k and nb:
            if m == 0 or self.nse == 0:
                out.zero_()
            else:
                plan = self._scatter_plan()
                code = F8._CODE_OF_FMT[self.fmt]
                if plan is not None:
                    plan.step(code, self.scale, spikes_bm, sd, out)
                else:
                    codes, indices, indptr = self._device_arrays()
                    f8_direct(codes, code, self.scale, indices, indptr, spikes_bm, sd, out, m, k)
        r = out[0] if ev.ndim == 1 else out
        return A.to_result(r, self._numpy_result and A.wants_numpy(ev))

    def __matmul__(self, other):           # W8 @ events: the gather direction
        from ._event import is_event
        if not is_event(other):
            raise TypeError("Float8CSR multiplies event operands only (BinaryArray, BitPackedBinary, CompactBinary); for a plain "
                            "float operand use tocsr().")
        raise NotImplementedError("Float8CSR @ events (the gather direction, W8 @ events) is not built: only events @ Float8CSR "
                                  "is; tocsr() gives a CSR that serves both.")

    def __repr__(self):
        return f"Float8CSR(shape={self.shape}, nse={self.nse}, fmt={self.fmt}, scale={self.scale!r})"

    __getitem__ = _refuse('slicing')
    slice_rows = _refuse('slice_rows')
    solve = _refuse('solve')
    with_data = _refuse('with_data')
    diag_add = _refuse('diag_add')
    update_on_pre = _refuse('update_on_pre')
    update_on_post = _refuse('update_on_post')
    update_on_binary_pre = _refuse('update_on_binary_pre')
    update_on_binary_post = _refuse('update_on_binary_post')


for _n in ('add', 'radd', 'iadd', 'sub', 'rsub', 'isub', 'mul', 'rmul', 'imul', 'truediv', 'rtruediv', 'itruediv', 'pow', 'neg',
           'pos', 'abs', 'imatmul'):
    setattr(Float8CSR, f'__{_n}__', _refuse(f'arithmetic (__{_n}__)'))


def _is_u8(x) -> bool:
    return (isinstance(x, torch.Tensor) and x.dtype == torch.uint8) or (isinstance(x, np.ndarray) and x.dtype == np.uint8)


def csr_quantize_fp8(csr, fmt: str = 'e4m3', scale: Optional[float] = None) -> Float8CSR:
    """``Float8CSR`` of a ``CSR``: ``quantize_fp8``'s formula applied to ``csr.data`` — ``scale = f32(amax) / f32(FMT_MAX)`` (1 for
    an all-zero matrix) unless given, ``codes = cast(clamp(data / scale, ±FMT_MAX))`` — over the source's own ``indices`` /
    ``indptr`` (shared, not copied).  Non-finite values are refused; so is a CSR of one shared weight, which the ``h8`` plan already
    stores in 1 byte per synapse."""
    if fmt not in F8._DTYPE_OF_FMT:
        raise ValueError(f"unknown FP8 format {fmt!r}: 'e4m3' or 'e5m2'.")
    data = csr.data.detach()
    if data.numel() == 1 and csr.nse != 1:
        raise TypeError("quantize_fp8: this CSR has one shared weight, which the h8 plan already stores in 1 byte per synapse; "
                        "FP8 codes would save nothing.")
    if not data.dtype.is_floating_point:
        raise TypeError(f"quantize_fp8 takes float weights, got {data.dtype}.")
    w = data.reshape(-1).to(torch.float32)
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_fp8: the matrix holds non-finite values.")
    fmax = F8.FMT_MAX[fmt]
    if scale is None:
        amax = float(w.abs().max()) if w.numel() else 0.0
        scale = float(np.float32(amax) / np.float32(fmax)) if amax > 0 else 1.0
    scale = float(np.float32(scale))
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"quantize_fp8: scale must be a positive finite number, got {scale}.")
    s = torch.tensor(scale, dtype=torch.float32, device=w.device)
    codes = torch.empty(w.numel(), dtype=F8._DTYPE_OF_FMT[fmt], device=w.device)
    for e0 in range(0, int(w.numel()), _QUANT_SLAB):       # in slabs: the f32 temporaries of 1e10 entries would be 80 GB
        codes[e0:e0 + _QUANT_SLAB] = (w[e0:e0 + _QUANT_SLAB] / s).clamp(-fmax, fmax).to(F8._DTYPE_OF_FMT[fmt])
    out = Float8CSR((codes, csr.indices, csr.indptr), shape=csr.shape, scale=scale)
    out._numpy_result = csr._numpy_result
    return out
