"""FP8 weights for the event-driven CSR products: ``Float8CSR`` / ``Float8CSC``, ``CSR.quantize_fp8`` / ``CSC.quantize_fp8`` and
the q8 scatter plan (``csrc/be_csr_f8.hip``, the q8 layout of ``csrc/be_csr_plan.hip``; the gather: ``csrc/be_csr_f8_gather.hip``).

A stored entry is one OCP FP8 code (``e4m3`` = ``torch.float8_e4m3fn``, ``e5m2`` = ``torch.float8_e5m2``; never the ``fnuz`` forms)
and the matrix is ``decode(codes) * scale`` with one f32 ``scale``.  Every finite code is an integer multiple of ``2^-E`` (``E`` = 9 /
16), so ``events @ W8`` sums exact 64-bit integers and rounds once: ``out[j] = f32(f64(R_j) * ldexp(f64(f32(scale)), -E))`` — the same
bits on the planned route (2 bytes per synapse) and on the direct route (global integer atomics), whatever the geometry.  The
semantics are stated in ``include/brainevent_amd.h``.  Quantised weights are read-only, as ``Float8Dense``'s are.

The gather direction sums a stored row's entries whose input fired, with the same finish, so it too is exact: the streaming
kernel, the mirror on the q8 plan and the mirror on the direct scatter give the same bits.  ``Float8CSR`` and ``Float8CSC`` are two
views of one shared stored-rows state (``W8.T``): the arrays, the plan and the mirror exist once.
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

__all__ = ['Float8CSR', 'Float8CSC', 'Q8Plan', 'csr_quantize_fp8', 'csc_quantize_fp8']

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


def f8_gather(codes: torch.Tensor, fmt_code: int, scale: float, indices, indptr, spikes_bm, sd: int, out_bm: torch.Tensor,
              m: int, k: int) -> None:
    """``be_binary_csrmm_nt_f8``: batch-major spikes ``[nb, k]`` (bool, float or packed words) -> f32 ``out_bm [nb, m]``."""
    nb = int(out_bm.shape[0])
    ws = A.workspace(fn('be_binary_csrmm_nt_f8_workspace_bytes')(m, k, nb))
    call('be_binary_csrmm_nt_f8', A.ptr(codes), fmt_code, float(scale), A.ptr(indices), A.ptr(indptr),
         int(indptr.dtype == torch.int64), -1, int(indices.numel()), A.ptr(spikes_bm), sd, A.ptr(out_bm), m, k, nb, A.ptr(ws),
         ws.numel(), A.stream_ptr())


class F8Mirror:
    """The transposed structure of FP8 stored rows ``(m, k)``, for the gather as a scatter over the active inputs: the q8 plan
    over ``(k, m)`` when it takes the matrix (the raw mirror arrays are then released: the weights are read-only, there is no
    refresh), else the raw arrays ``codes`` / ``indices`` (row ids) / ``indptr`` (``k + 1``) for the direct scatter."""

    def __init__(self, m, k, plan, codes, indices, indptr):
        self.m, self.k = int(m), int(k)
        self.plan, self.codes, self.indices, self.indptr = plan, codes, indices, indptr

    @classmethod
    def build(cls, codes, indices, indptr, *, shape) -> 'F8Mirror':
        from ._convert import CscBuilder
        m, k = int(shape[0]), int(shape[1])
        b = CscBuilder(indptr, indices, shape=(m, k))
        rows, codes_t, _ = b.block(0, k, data=A.to_device(codes).view(torch.uint8).reshape(-1))
        ptr_t, nnz = b.offsets(), int(indices.numel())
        if nnz >= C.PLAN_MIN_NNZ and Q8Plan.applies(k, m, nnz, b.max_col_count):
            return cls(m, k, Q8Plan.build(codes_t, rows, ptr_t, shape=(k, m)), None, None, None)
        return cls(m, k, None, codes_t, rows, ptr_t)

    def nbytes(self) -> int:
        if self.plan is not None:
            return self.plan.nbytes()
        return sum(t.numel() * t.element_size() for t in (self.codes, self.indices, self.indptr))

    def step(self, fmt_code: int, scale: float, spikes_bm, sd: int, out_bm: torch.Tensor) -> None:
        if self.plan is not None:
            self.plan.step(fmt_code, scale, spikes_bm, sd, out_bm)
        else:
            f8_direct(self.codes, fmt_code, scale, self.indices, self.indptr, spikes_bm, sd, out_bm, self.k, self.m)


class _F8Rows:
    """The state the two views share: ``m`` stored rows over ``k`` ids as codes / indices / indptr, one scale, the format, and
    what was built over them — the device copies, the q8 scatter plan and the mirror."""

    def __init__(self, codes, indices, indptr, scale, fmt, m, k, numpy_result):
        self.codes, self.indices, self.indptr = codes, indices, indptr
        self.scale, self.fmt, self.m, self.k = scale, fmt, int(m), int(k)
        self.numpy_result = numpy_result
        self.dev = None
        self.plan: Optional[Q8Plan] = None
        self.max_row: Optional[int] = None
        self.mirror: Optional[F8Mirror] = None

    nse = property(lambda self: int(self.indices.shape[0]))

    def device_arrays(self):
        if self.dev is None:
            self.dev = (A.to_device(self.codes), A.to_device(self.indices), A.to_device(self.indptr))
        return self.dev

    def planned(self) -> bool:
        if self.nse < C.PLAN_MIN_NNZ:
            return False
        if self.max_row is None:
            self.max_row = int((self.indptr[1:] - self.indptr[:-1]).max()) if self.m > 0 else 0
        return Q8Plan.applies(self.m, self.k, self.nse, self.max_row)

    def scatter_plan(self) -> Optional[Q8Plan]:
        if self.plan is None and self.planned():
            codes, indices, indptr = self.device_arrays()
            self.plan = Q8Plan.build(codes, indices, indptr, shape=(self.m, self.k))
        return self.plan

    def build_mirror(self) -> F8Mirror:
        if self.mirror is None:
            codes, indices, indptr = self.device_arrays()
            self.mirror = F8Mirror.build(codes, indices, indptr, shape=(self.m, self.k))
        return self.mirror

    def scatter(self, spikes_bm, sd: int) -> torch.Tensor:
        """Spikes ``[nb, m]`` over the stored rows -> f32 ``[nb, k]``."""
        nb = int(spikes_bm.shape[0])
        out = torch.empty((nb, self.k), dtype=torch.float32, device=A.device())
        if self.k and nb:
            if self.m == 0 or self.nse == 0:
                out.zero_()
            else:
                plan = self.scatter_plan()
                code = F8._CODE_OF_FMT[self.fmt]
                if plan is not None:
                    plan.step(code, self.scale, spikes_bm, sd, out)
                else:
                    codes, indices, indptr = self.device_arrays()
                    f8_direct(codes, code, self.scale, indices, indptr, spikes_bm, sd, out, self.m, self.k)
        return out

    def gather(self, spikes_bm, sd: int) -> torch.Tensor:
        """Spikes ``[nb, k]`` over the stored ids -> f32 ``[nb, m]``: through the mirror if one was built, else streamed."""
        nb = int(spikes_bm.shape[0])
        out = torch.empty((nb, self.m), dtype=torch.float32, device=A.device())
        if self.m and nb:
            if self.k == 0 or self.nse == 0:
                out.zero_()
            elif self.mirror is not None:
                self.mirror.step(F8._CODE_OF_FMT[self.fmt], self.scale, spikes_bm, sd, out)
            else:
                codes, indices, indptr = self.device_arrays()
                f8_gather(codes, F8._CODE_OF_FMT[self.fmt], self.scale, indices, indptr, spikes_bm, sd, out, self.m, self.k)
        return out


def _refuse(what: str):
    def method(self, *args, **kwargs):
        raise TypeError(f"{type(self).__name__} is read-only quantised weights: {what} is not supported; {self._BACK}() gives the "
                        f"f32 {self._BACK[2:].upper()} back.")
    method.__name__ = what
    return method


def _as_host_or_device(x) -> torch.Tensor:
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))


class _Float8Stored:
    """What ``Float8CSR`` and ``Float8CSC`` share: a view (``shape``) of one :class:`_F8Rows` state."""
    _FORMAT = 'csr'
    _BACK = 'tocsr'

    def __init__(self, args, *, shape, scale: float = 1.0, fmt: Optional[str] = None):
        name = type(self).__name__
        assert len(args) == 3, "Expected three arguments: codes, indices, indptr."
        codes_arg, indices_arg, indptr_arg = args
        numpy_result = A.wants_numpy(codes_arg, indices_arg, indptr_arg)
        if not (F8.is_fp8(codes_arg) or _is_u8(codes_arg)):
            dt = codes_arg.dtype if hasattr(codes_arg, 'dtype') else type(codes_arg).__name__
            raise TypeError(f"{name} takes a torch FP8 tensor or uint8 codes, got {dt}: {self._FORMAT.upper()}.quantize_fp8() makes "
                            "the codes.")
        c = F8._as_codes(codes_arg, fmt)
        if c.ndim != 1:
            raise ValueError(f"{name} codes must be one-dimensional (one per stored entry), got {c.ndim}D.")
        if c.requires_grad:
            raise TypeError(f"{name} is read-only quantised weights: codes that require grad are not supported.")
        if isinstance(scale, torch.Tensor):
            if scale.requires_grad:
                raise TypeError(f"{name} is read-only quantised weights: a scale that requires grad is not supported.")
            scale = float(scale)
        scale = float(np.float32(scale))
        if not np.isfinite(scale):
            raise ValueError(f"{name}: scale must be finite, got {scale}.")
        shape = (int(shape[0]), int(shape[1]))
        m, k = shape if self._FORMAT == 'csr' else shape[::-1]          # stored rows x stored ids
        context = f"{name} constructor"
        indices = _as_int32_indices(_as_host_or_device(indices_arg), k, context, check_values=True)
        indptr = _as_indptr(_as_host_or_device(indptr_arg), int(indices.shape[0]), "auto", context)
        _check_compressed_structure(indices, indptr, shape, format=self._FORMAT, check_values=True)
        if int(c.shape[0]) != int(indices.shape[0]):
            raise ValueError(f"{name}: {int(c.shape[0])} codes for {int(indices.shape[0])} indices.")
        F8.check_finite(c)
        self._rows = _F8Rows(c, indices, indptr, scale, F8.fmt_of(c), m, k, numpy_result)
        self.shape = shape

    @classmethod
    def _view(cls, rows: _F8Rows):
        obj = cls.__new__(cls)
        obj._rows = rows
        obj.shape = (rows.m, rows.k) if cls._FORMAT == 'csr' else (rows.k, rows.m)
        return obj

    codes = property(lambda self: self._rows.codes)
    indices = property(lambda self: self._rows.indices)
    indptr = property(lambda self: self._rows.indptr)
    scale = property(lambda self: self._rows.scale)
    fmt = property(lambda self: self._rows.fmt)
    dtype = property(lambda self: self._rows.codes.dtype)
    ndim = property(lambda self: 2)
    nse = property(lambda self: self._rows.nse)
    _plan = property(lambda self: self._rows.plan)
    _mirror = property(lambda self: self._rows.mirror)

    @property
    def _numpy_result(self):
        return self._rows.numpy_result

    @_numpy_result.setter
    def _numpy_result(self, value):
        self._rows.numpy_result = bool(value)

    def transpose(self, axes=None):
        """The other view of the same stored rows (``shape[::-1]``): nothing is copied, and a plan or a mirror built through
        either view serves both."""
        assert axes is None, "transpose does not support axes argument."
        return (Float8CSC if self._FORMAT == 'csr' else Float8CSR)._view(self._rows)

    T = property(lambda self: self.transpose())

    def _dequantised(self) -> torch.Tensor:
        return self.codes.to(torch.float32) * torch.tensor(self.scale, dtype=torch.float32, device=self.codes.device)

    def todense(self, dtype=torch.float32):
        """``decode(codes) * scale`` (the multiply in f32) scattered to ``shape``, duplicates summed in f32, as ``dtype``; numpy if
        the arrays came as numpy.  Host-side helper for tests and small matrices."""
        r = self._rows
        w = self._dequantised().cpu()
        ptr = self.indptr.cpu().to(torch.int64)
        major = torch.repeat_interleave(torch.arange(r.m, dtype=torch.int64), ptr[1:] - ptr[:-1])
        minor = self.indices.cpu().to(torch.int64)
        out = torch.zeros(self.shape, dtype=torch.float32)
        out.index_put_((major, minor) if self._FORMAT == 'csr' else (minor, major), w, accumulate=True)
        out = out.to(dtype)
        return out.numpy() if self._numpy_result else out

    def _tof32(self, cls, dtype):
        return cls._from_parts(A.to_device(self._dequantised().to(dtype)), A.to_device(self.indices), A.to_device(self.indptr),
                               shape=self.shape, numpy_result=self._numpy_result)

    # -- route --------------------------------------------------------------------------------------
    def prepare(self, mirror: bool = False):
        """Without arguments: build the q8 plan of the scatter over the stored rows now (otherwise the first such product builds
        it).  A matrix the plan does not take — fewer than ``PLAN_MIN_NNZ`` entries, a row above 16384 entries, more than 1024
        slices — has nothing to prepare: its products run on the direct route.  ``mirror=True``: build the mirror instead
        (:meth:`build_mirror`), for the gather direction."""
        self._rows.device_arrays()
        if mirror:
            self._rows.build_mirror()
        else:
            self._rows.scatter_plan()
        return self

    def build_mirror(self):
        """Build the mirror — the transposed structure with the codes moved along, one byte each — after which the gather
        products are the scatter over the active inputs: on a q8 plan over the mirror when the plan takes it (the raw mirror
        arrays are then released), else on the direct route.  Same bits as the streaming gather kernel, which serves the
        gather until a mirror is asked for; the mirror is never built on its own.  Shared by both views."""
        self._rows.build_mirror()
        return self

    # -- products -----------------------------------------------------------------------------------
    def _event(self, other, scatter: bool):
        from ._event import is_event, event_operand
        if not is_event(other):
            raise TypeError(f"{type(self).__name__} multiplies event operands only (BinaryArray, BitPackedBinary, CompactBinary); "
                            f"for a plain float operand use {self._BACK}().")
        ev = event_operand(other, scatter=scatter)
        if isinstance(ev, torch.Tensor) and ev.requires_grad:
            raise TypeError(f"{type(self).__name__} is read-only quantised weights: no gradients flow through its products.")
        if ev.ndim not in (1, 2):
            raise NotImplementedError(f"matmul with object of shape {tuple(ev.shape)}")
        return ev

    def _product(self, other, gather: bool, events_first: bool):
        """``events @ self`` (``events_first``; batches ``[nb, n]`` -> ``[nb, out]``) or ``self @ events`` (``[n, nb]`` ->
        ``[out, nb]``) as the scatter over the stored rows or the gather over them."""
        r = self._rows
        ev = self._event(other, scatter=not gather or r.mirror is not None)
        n = r.k if gather else r.m
        if int(ev.shape[-1 if events_first or ev.ndim == 1 else 0]) != n:
            a, b = (tuple(ev.shape), self.shape) if events_first else (self.shape, tuple(ev.shape))
            raise ValueError(f"shapes {a} and {b} are not aligned for the product.")
        if ev.ndim == 1:
            s, sd = A.spikes_to_device(ev)
            spikes_bm = s.reshape(1, -1)
        else:
            spikes_bm, sd = A.spikes_batch_major(ev.T if events_first else ev)
        out = r.gather(spikes_bm, sd) if gather else r.scatter(spikes_bm, sd)
        res = out[0] if ev.ndim == 1 else (out if events_first else out.T)
        return A.to_result(res, self._numpy_result and A.wants_numpy(ev))

    def __repr__(self):
        return f"{type(self).__name__}(shape={self.shape}, nse={self.nse}, fmt={self.fmt}, scale={self.scale!r})"

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
    setattr(_Float8Stored, f'__{_n}__', _refuse(f'arithmetic (__{_n}__)'))


class Float8CSR(_Float8Stored):
    """CSR matrix of OCP FP8 codes with one f32 ``scale``: the matrix it stands for is ``decode(codes) * scale`` at the stored
    positions (duplicates add).

    ``Float8CSR((codes, indices, indptr), shape=(m, k), scale=1.0, fmt=None)``: ``codes`` is a torch FP8 tensor, or ``uint8`` codes
    (numpy or torch) together with ``fmt='e4m3' | 'e5m2'``; ``indptr`` int32 or int64.  ``events @ W8`` (``BinaryArray``,
    ``BitPackedBinary``, ``CompactBinary``; 1-D and batched ``[nb, m]``) is the event-driven product, f32 out, numpy in -> numpy
    out; it is exact (see the module docstring) and takes the q8 plan — built by :meth:`prepare` or the first product — when the
    matrix has at least ``PLAN_MIN_NNZ`` entries and the sorted layout holds it, else the direct route: same bits.  Everything
    that would write or differentiate the weights raises, and a plain float operand gets ``TypeError`` (use :meth:`tocsr`).  The
    gather direction is spelled through the transpose view, ``events @ W8.T`` (:class:`Float8CSC` over the same arrays; the
    streaming gather kernel, or the mirror after :meth:`build_mirror`): ``W8 @ events`` itself still raises
    ``NotImplementedError``."""
    _FORMAT, _BACK = 'csr', 'tocsr'

    def tocsr(self, dtype=torch.float32):
        """The dequantised ``CSR`` (``decode(codes) * scale`` as ``dtype``) over the same ``indices`` / ``indptr``."""
        return self._tof32(C.CSR, dtype)

    def __rmatmul__(self, other):          # events @ W8: the scatter over the active rows
        return self._product(other, gather=False, events_first=True)

    def __matmul__(self, other):           # W8 @ events: the gather direction, spelled events @ W8.T
        from ._event import is_event
        if not is_event(other):
            raise TypeError("Float8CSR multiplies event operands only (BinaryArray, BitPackedBinary, CompactBinary); for a plain "
                            "float operand use tocsr().")
        raise NotImplementedError("Float8CSR @ events (the gather direction, W8 @ events) is not built under this spelling: "
                                  "events @ W8.T is the same product (W8.T is the Float8CSC view of the same arrays); tocsr() "
                                  "gives a CSR that serves both.")


class Float8CSC(_Float8Stored):
    """CSC matrix of OCP FP8 codes with one f32 ``scale``: :class:`Float8CSR`'s arrays read as columns.

    ``Float8CSC((codes, indices, indptr), shape=(m, k), scale=1.0, fmt=None)``: ``indices`` are row ids and ``indptr`` has
    ``k + 1`` entries; everything else — the codes, the validation, the refusals — as :class:`Float8CSR`, whose ``.T`` is this
    class over the same arrays (and back).  ``W8 @ events[k]`` -> ``[m]`` (``[k, nb]`` -> ``[m, nb]``) is the scatter over the
    stored columns (q8 plan or direct route); ``events[m] @ W8`` -> ``[k]`` (``[nb, m]`` -> ``[nb, k]``) is the gather: the
    streaming kernel, or after :meth:`build_mirror` / ``prepare(mirror=True)`` the scatter over the mirror.  Every route gives the
    same bits."""
    _FORMAT, _BACK = 'csc', 'tocsc'

    def tocsc(self, dtype=torch.float32):
        """The dequantised ``CSC`` (``decode(codes) * scale`` as ``dtype``) over the same ``indices`` / ``indptr``."""
        return self._tof32(C.CSC, dtype)

    def __matmul__(self, other):           # W8 @ events: the scatter over the active columns
        return self._product(other, gather=False, events_first=False)

    def __rmatmul__(self, other):          # events @ W8: the gather over the stored columns
        return self._product(other, gather=True, events_first=True)


def _is_u8(x) -> bool:
    return (isinstance(x, torch.Tensor) and x.dtype == torch.uint8) or (isinstance(x, np.ndarray) and x.dtype == np.uint8)


def csr_quantize_fp8(csr, fmt: str = 'e4m3', scale: Optional[float] = None, cls=Float8CSR):
    """``Float8CSR`` of a ``CSR``: ``quantize_fp8``'s formula applied to ``csr.data`` — ``scale = f32(amax) / f32(FMT_MAX)`` (1 for
    an all-zero matrix) unless given, ``codes = cast(clamp(data / scale, ±FMT_MAX))`` — over the source's own ``indices`` /
    ``indptr`` (shared, not copied).  Non-finite values are refused; so is a CSR of one shared weight, which the ``h8`` plan already
    stores in 1 byte per synapse.  ``cls=Float8CSC`` with a ``CSC`` source: the same over its columns."""
    if fmt not in F8._DTYPE_OF_FMT:
        raise ValueError(f"unknown FP8 format {fmt!r}: 'e4m3' or 'e5m2'.")
    data = csr.data.detach()
    if data.numel() == 1 and csr.nse != 1:
        raise TypeError(f"quantize_fp8: this {type(csr).__name__} has one shared weight, which the h8 plan already stores in 1 byte per synapse; "
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
    out = cls((codes, csr.indices, csr.indptr), shape=csr.shape, scale=scale)
    out._numpy_result = csr._numpy_result
    return out


def csc_quantize_fp8(csc, fmt: str = 'e4m3', scale: Optional[float] = None) -> Float8CSC:
    """``Float8CSC`` of a ``CSC``: :func:`csr_quantize_fp8`'s formula over the source's own ``indices`` / ``indptr``."""
    return csr_quantize_fp8(csc, fmt, scale, cls=Float8CSC)
