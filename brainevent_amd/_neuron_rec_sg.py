"""The fused recurrent spiking layer: :func:`~brainevent_amd.synaptic_lif_sequence`'s neuron with a sparse
recurrent projection INSIDE the time loop, a whole sequence as ONE launch forwards and one backwards (``be_lif_rec_sg_forward`` /
``be_lif_rec_sg_backward``, ``csrc/be_neuron_sg_rec.hip``) under ``torch.autograd``.

    xin[t] = x[t] + s[t-1] @ rec          (s[-1] = s0, or no spike)
    then synaptic_lif_step on xin[t]:  c' = syn_decay * c + xin;  h = beta * v + c';  th = v_th + kappa * a;  s = h >= th;  ...

``rec`` is a :class:`~brainevent_amd.CSR` ``[N, N]`` whose rows are the presynaptic neurons, with one f32 weight per stored entry.
One workgroup owns one sample and keeps its spikes on the chip between steps; the recurrent sums are 64-bit fixed-point integers
(order independent), so the forward pass is a function of its inputs bit for bit and equals the per-step loop
``synaptic_lif_step(state, x[t] + BinaryArray(s) @ rec)`` wherever that loop's own sums are exact.  The backward pass is that
loop's: straight-through in the spikes for the recurrent product, the surrogate for the neuron; the weight gradient is the
existing per-entry kernel (``be_grad_rows``) over all ``T * B`` spike rows at once.

``recurrent_lif_sequence`` takes Python numbers.  :func:`parametric_recurrent_lif_sequence` (DESIGN.md §2.25;
``be_lif_rec_sg_forward_params`` / ``be_lif_rec_sg_backward_params``, the same kernels) takes each of ``syn_decay``, ``beta``, ``v_th``,
``rho`` and ``kappa`` as a number or an f32 device tensor — one element, or ``[N]`` for a value per neuron — read on the device and,
where it requires grad, differentiated: per-(sample, neuron) sums over time from the backward launch, then
``be_lif_sg_reduce_slots`` over the batch.

SYNAPTIC DELAYS (``be_lif_rec_delay_sg_forward`` / ``be_lif_rec_delay_sg_backward``,
``csrc/be_neuron_sg_rec_delay.hip``): ``rec`` may be a :class:`~brainevent_amd.DelayedCSR` (``csr.with_delays(delays, depth)``).
Every stored entry then acts ``delay`` steps later,

    xin[t] = x[t] + sum over the delays d < depth of sp(t - 1 - d) @ W_d,    sp(tau) = s[tau], or the history ``s0`` before step 0,

the kernels keep a sample's last ``depth`` spike vectors on the chip and walk the stacked matrix ``rec.stacked`` (row ``d * N + i``:
neuron ``i``'s synapses of delay ``d``); ``s0`` may hold up to ``depth`` past steps, and the leaf of the weight gradient is
``rec.stacked.data``, as for ``ring @ D``.  Delay 0 everywhere is the layer without delays.

A DENSE RECURRENCE (``be_lif_rec_dense_sg_forward`` / ``be_lif_rec_dense_sg_backward``,
``csrc/be_neuron_sg_rec_dense.hip``): ``rec`` may be a :class:`~brainevent_amd.Dense` ``[N, N]`` (f32, rows = presynaptic neurons).
The function is the one above on the CSR that stores all ``N * N`` entries — the same fixed-point sums, so the same forward bits —
but the kernels walk the matrix itself: forwards the active rows are streamed into register sums from a spike mask in LDS,
backwards the gather is a row-times-vector product.  The leaf of the weight gradient is ``rec.data`` (``be_grad_dense``).
``rec.data`` may also be f16 or bf16 (``be_lif_rec_dense_half_sg_forward`` / ``_backward``,
``csrc/be_neuron_sg_rec_dense_half.hip``): the layer is then the f32 layer on ``rec.data.float()`` — the up-conversion is exact, the
forward outputs equal the f32 call's bit for bit — through kernels that load two weights in 4 bytes forwards and eight in 16 bytes
backwards; the weight gradient is summed in f32 and rounded to the weights' dtype once.

FP8 WEIGHTS (``be_lif_rec_dense_f8_sg_forward`` / ``_backward``, ``csrc/be_neuron_sg_rec_dense_f8.hip``): ``rec`` may be
a :class:`~brainevent_amd.Float8Dense` ``[N, N]`` (e4m3 or e5m2 codes, one f32 scale, rows = presynaptic neurons).  Every finite
FP8 value is a multiple of 2^-9 / 2^-16, so the recurrent sum of the decoded weights is an exact integer in that unit, rounded to
f32 once and multiplied by the scale in f32 — ``Float8Dense``'s product contract with an exact sum; there is no exponent and no
host synchronisation.  The weights are read-only and get no gradient; ``x``, the state and ``s0`` do.

FP8 WEIGHTS FOR THE SPARSE RECURRENCE (``be_lif_rec_f8_sg_forward`` / ``_backward``, ``csrc/be_neuron_sg_rec_f8.hip``):
``rec`` may be a :class:`~brainevent_amd.Float8CSR` ``[N, N]`` (one e4m3 or e5m2 code per stored entry, one f32 scale, an int32
``indptr``).  The recurrent sums are ``Float8CSR``'s own — exact 64-bit integers in the format's unit, finished as ``events @ W8``
finishes them — so the layer equals the per-step loop ``x[t] + BinaryArray(s) @ W8`` bit for bit, with no exponent and no host
synchronisation.  The kernels are the CSR layer's split of work with a row walk made for one byte per weight: forwards four codes
in one 4-byte load and their columns in one 16-byte load, decoded in the integer ALU.  Read-only weights, as ``Float8Dense``'s.

Not built: CSC / fixed-number / JITC recurrences, a Dense, Float8Dense or Float8CSR recurrence with tensor parameters, a Dense or
FP8 recurrence with delays (FP8 weights for a DelayedCSR), a (straight-through) gradient of FP8 weights, per-row or per-block FP8 scales, one shared
(homogeneous) weight, learnable ``v_reset`` / ``alpha``,
per-sample (``[B, N]``) parameters, learnable delays, learnable neuron parameters together with delays, more than 8192 neurons (one
sample's sums and spike ids live in one workgroup's LDS; with delays also its spike history: see :func:`delay_fits`), a sample split
over several workgroups.  A cached scatter plan or mirror of ``rec`` is neither used nor needed: the kernels read the raw CSR arrays.
"""
import numbers
from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _array as A
from . import _autograd
from ._lib import call, fn
from ._neuron_sg import _check_device, _check_tensor, _grad_in, _reduce_slots
from ._neuron_syn_sg import FIVE_TENSORS, _Params, _check_state, _device_params, _new_grads, _new_outputs, _split_params

__all__ = ['recurrent_lif_sequence', 'parametric_recurrent_lif_sequence']

#: kRecMaxN of csrc/be_neuron_sg_rec.hip (and kDelMaxN of csrc/be_neuron_sg_rec_delay.hip)
MAX_N = 8192
#: the exponents ``be_fixed_point_exponent`` returns
SCALE_EXP_RANGE = (-90, 150)
#: kDelMaxDepth, kDelLdsBytes and kDelMinIds of csrc/be_neuron_sg_rec_delay.hip
MAX_DEPTH = 256
DELAY_LDS_BYTES = 160 * 1024 - 1024
DELAY_MIN_IDS = 4096


def delay_fits(n: int, depth: int) -> bool:
    """The limit rule of the delayed kernels: one sample's sums (8 B per neuron), its bit-packed spike history (``depth`` times
    ``ceil(n / 64)`` 8-byte words) and a list of at least ``DELAY_MIN_IDS`` active stacked rows fit one workgroup's LDS.  Every
    ``n <= 8192`` with ``depth <= 16`` and every ``n <= 2048`` with ``depth <= 256`` does."""
    return n <= MAX_N and 1 <= depth <= MAX_DEPTH and 8 * n + 8 * depth * ((n + 63) // 64) + 4 * DELAY_MIN_IDS <= DELAY_LDS_BYTES


def _limit(who, n: int, why: str):
    if n > MAX_N:
        raise ValueError(f"{who}: {n} neurons; the limit is {MAX_N} ({why}).")


class _Rec:
    """A :class:`~brainevent_amd.CSR` recurrence as the host path takes it — and the shape of every family's adapter (DESIGN.md
    §2.32): the family's checks (the constructor), its entry points, the arguments that stand for the matrix in the C calls, how
    ``s0`` goes in, the exponent, the leaf of the weight gradient and that gradient.  A matrix without entries hands over one unused
    element: no NULL pointer."""
    forward = 'be_lif_rec_sg_forward'
    backward = 'be_lif_rec_sg_backward'
    takes_exp = True                          # the C calls take scale_exp
    no_tensors = None                         # or: why parametric_recurrent_lif_sequence refuses the family tensor parameters
    ages = None                               # with delays: the past steps s0 holds

    def __init__(self, who, m, n: int, like=None, int64_hint='.'):
        if m.data.dtype != torch.float32:
            raise TypeError(f"{who}: the weights of rec must be float32, not {m.data.dtype}.")
        self.nse = int(m.indices.numel())
        if m.data.numel() != self.nse:
            raise ValueError(f"{who}: rec must hold one weight per stored entry ({self.nse}), not {m.data.numel()} (one shared weight "
                             f"is not built).")
        if m.indptr.dtype != torch.int32:
            raise TypeError(f"{who}: the indptr of rec must be int32, not {m.indptr.dtype}" + int64_hint)
        _limit(who, n, "one sample's sums and spike ids live in one workgroup's LDS")
        self.m, self.leaf = m, m.data
        self.w = m.data.detach().reshape(-1) if self.nse else torch.zeros(1, dtype=torch.float32, device=m.indptr.device)
        self.indices = m.indices if self.nse else torch.zeros(1, dtype=torch.int32, device=m.indptr.device)
        self.indptr = m.indptr
        self.matrix = (A.ptr(self.w), A.ptr(self.indices), A.ptr(self.indptr))

    def check_s0(self, who, s0, slots):
        if tuple(s0.shape) != slots:
            raise ValueError(f"{who}: s0 {tuple(s0.shape)} must have the shape of a step of x, {slots}.")

    def s0_shape(self, B: int, N: int):
        """``s0`` — and its gradient — as the kernels take it."""
        return (B, N) if self.ages is None else (self.ages, B, N)

    def s0_args(self, t):
        """Forwards ``s0``, backwards its gradient: a pointer, with delays a pointer and the ages."""
        return (A.ptr(t),) if self.ages is None else (A.ptr(t), self.ages)

    def exponent(self, who, scale_exp, n: int) -> int:
        if scale_exp is None:
            return self.own_exponent(n)
        if isinstance(scale_exp, bool) or not isinstance(scale_exp, numbers.Integral):
            raise TypeError(f"{who}: scale_exp must be None or an int, not {type(scale_exp).__name__}.")
        if not SCALE_EXP_RANGE[0] <= scale_exp <= SCALE_EXP_RANGE[1]:
            raise ValueError(f"{who}: scale_exp {scale_exp} is outside {SCALE_EXP_RANGE[0]} .. {SCALE_EXP_RANGE[1]}, the exponents "
                             f"fixed_point_exponent returns.")
        return int(scale_exp)

    def own_exponent(self, n: int) -> int:    # (a stacked matrix has the same columns: every stacked row active)
        if self.nse == 0 or n == 0:
            return 0
        from ._csr import fixed_point_exponent
        return fixed_point_exponent(self.m.data.detach(), self.m.indices, n)

    def weight_grad(self, s, w, s0, g_x, T: int, B: int, N: int) -> torch.Tensor:
        """``g_w[k] = sum over t, b of sp[t][b][row k] * g_x[t][b][col k]`` with ``sp = cat(s0, s[:-1])``: ``be_grad_rows`` (the
        ``transpose=True`` side) over ``T * B`` batch rows — ``(T - 1) * B`` without ``s0`` — in ascending order; ``g_x`` is read
        batch-major through the stride arguments, nothing is transposed."""
        if T == 0 or self.nse == 0:
            return torch.zeros_like(w)
        if s0 is None:
            sp, g = s[:T - 1], g_x[1:]
        else:
            sp, g = torch.cat(((s0 != 0).to(s.dtype)[None], s[:T - 1])), g_x
        nb = int(sp.shape[0]) * B
        if nb == 0:
            return torch.zeros_like(w)
        mask, _ = _autograd.activity(sp.reshape(nb, N), 'bm')
        dw = torch.empty(self.nse, dtype=w.dtype, device=w.device)
        g = g.contiguous()
        call('be_grad_rows', 1, A.ptr(dw), 0, A.wcode(dw), A.ptr(self.indices), A.ptr(self.indptr), 0, -1, N, self.nse, A.ptr(mask),
             nb, A.ptr(g), 1, N, A.ptr(None), 0, A.stream_ptr())
        return dw.reshape(w.shape)


class _DelayedRec(_Rec):
    """A :class:`~brainevent_amd.DelayedCSR`: the stacked arrays, the row mask and the depth; ``s0`` is a history ``[ages, B, N]``
    and the leaf ``rec.stacked.data``."""
    forward = 'be_lif_rec_delay_sg_forward'
    backward = 'be_lif_rec_delay_sg_backward'
    no_tensors = ('synaptic delays', 'DelayedCSR')

    def __init__(self, who, rec, n: int, like=None):
        super().__init__(who, rec.stacked, n, like,  # with delays the kernels read the stacked arrays
                         " (a DelayedCSR built from an int64 indptr, or with 2^31 entries or more, is not built).")
        self.row_mask, self.depth, self.ages = rec.row_mask, int(rec.depth), 0
        self.matrix += (A.ptr(self.row_mask), self.depth)
        if not delay_fits(n, self.depth):
            raise ValueError(f"{who}: {n} neurons at depth {self.depth} do not fit: with delays 8 * N + 8 * depth * ceil(N / 64) + "
                             f"{4 * DELAY_MIN_IDS} must stay within {DELAY_LDS_BYTES} bytes (one sample's sums, its spike history and a "
                             f"list of active rows live in one workgroup's LDS; every N <= 8192 fits at depth <= 16, every N <= 2048 at "
                             f"depth <= {MAX_DEPTH}); a sample split over several workgroups is not built.")

    def check_s0(self, who, s0, slots):
        if tuple(s0.shape) == slots:
            self.ages = 1
        elif s0.ndim == len(slots) + 1 and tuple(s0.shape[1:]) == slots and 1 <= s0.shape[0] <= self.depth:
            self.ages = int(s0.shape[0])
        else:
            raise ValueError(f"{who}: s0 {tuple(s0.shape)} must have the shape of a step of x, {slots}, or hold A past steps, "
                             f"(A,) + {slots} with 1 <= A <= depth = {self.depth} (s0[a]: the spikes a + 1 steps before step 0).")

    def weight_grad(self, s, w, s_hist, g_x, T: int, B: int, N: int) -> torch.Tensor:
        """``g_w[k] = sum over t, b of sp(t - 1 - d)[b][i] * g_x[t][b][col k]`` for ``k`` in stacked row ``d * N + i``: one launch packs
        the aged activity of all ``depth * N`` stacked rows over the ``T * B`` batch rows (``be_grad_pack_activity_aged``), then
        ``be_grad_rows`` (``transpose=True``) over the stacked matrix, in ascending ``(t, b)``."""
        nb = T * B
        if nb == 0 or N == 0 or self.nse == 0:
            return torch.zeros_like(w)
        rows = self.depth * N
        mask = torch.empty(max(fn('be_grad_mask_bytes')(rows, nb), 4) // 4, dtype=torch.int32, device=w.device)
        call('be_grad_pack_activity_aged', A.ptr(s), A.ptr(s_hist), N, B, T, self.depth, 0 if s_hist is None else int(s_hist.shape[0]),
             A.ptr(mask), A.stream_ptr())
        dw = torch.empty(self.nse, dtype=w.dtype, device=w.device)
        call('be_grad_rows', 1, A.ptr(dw), 0, A.wcode(dw), A.ptr(self.indices), A.ptr(self.indptr), 0, -1, rows, self.nse,
             A.ptr(mask), nb, A.ptr(g_x), 1, N, A.ptr(None), 0, A.stream_ptr())
        return dw.reshape(w.shape)


class _DenseRec(_Rec):
    """A :class:`~brainevent_amd.Dense`: the matrix itself, contiguous ``[N, N]`` (no neuron: one unused element), and for two-byte
    weights — the ``_half_`` entry points — its dtype code; the leaf is ``rec.data``."""
    no_tensors = ('a Dense recurrence', 'Dense rec')

    def __init__(self, who, rec, n: int, like=None):
        w = rec.data
        if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"{who}: the weights of rec must be float32, float16 or bfloat16, not {w.dtype}.")
        if w.ndim != 2:
            raise ValueError(f"{who}: the data of a Dense rec must be two-dimensional, not {w.ndim}-dimensional.")
        _limit(who, n, "one workgroup holds a sample's neurons")
        self.leaf = w
        self.w = w.detach().contiguous() if w.numel() else torch.zeros(1, dtype=w.dtype, device=w.device)
        self.half = w.dtype != torch.float32
        self.forward = 'be_lif_rec_dense_half_sg_forward' if self.half else 'be_lif_rec_dense_sg_forward'
        self.backward = 'be_lif_rec_dense_half_sg_backward' if self.half else 'be_lif_rec_dense_sg_backward'
        self.matrix = (A.ptr(self.w), A.wcode(self.w)) if self.half else (A.ptr(self.w),)

    def own_exponent(self, n: int) -> int:    # the exponent of the CSR that stores all N * N entries
        if n == 0:
            return 0
        from ._csr import fixed_point_exponent
        cols = torch.arange(n, dtype=torch.int32, device=self.leaf.device).repeat(n)
        return fixed_point_exponent(self.leaf.detach().float().reshape(-1), cols, n)    # (f16 / bf16: the up-converted matrix)

    def weight_grad(self, s, w, s0, g_x, T: int, B: int, N: int) -> torch.Tensor:
        """``g_W[i, :] = sum over (t, b) with sp[t][b][i] of g_x[t][b][:]``, ``sp = cat(s0, s[:-1])``: ``be_grad_dense`` (the
        ``transpose=True`` side) over ``T * B`` batch rows — ``(T - 1) * B`` without ``s0``.  For f16 / bf16 weights the sum is the
        same f32 sum of the f32 ``g_x`` into an f32 ``[N, N]`` temporary, rounded to ``w.dtype`` ONCE: the gradient has the leaf's
        dtype, as torch requires, and carries one rounding, not ``T * B`` of them."""
        if s0 is None:
            sp, g = s[:max(T - 1, 0)], g_x[1:]
        else:
            sp, g = torch.cat(((s0 != 0).to(s.dtype)[None], s[:max(T - 1, 0)])), g_x
        nb = int(sp.shape[0]) * B
        if T == 0 or N == 0 or nb == 0:
            return torch.zeros_like(w)
        mask, _ = _autograd.activity(sp.reshape(nb, N), 'bm')
        if w.dtype != torch.float32:
            return _autograd.dense_weight_grad(((N, N), torch.float32), True, mask, nb, g.reshape(nb, N).T).to(w.dtype)
        return _autograd.dense_weight_grad(w, True, mask, nb, g.reshape(nb, N).T)


class _Float8Rec(_Rec):
    """A :class:`~brainevent_amd.Float8Dense`: the codes, contiguous ``[N, N]`` bytes on the device (no neuron: one unused byte), the
    format's code and the scale.  The sums are exact integers in the format's own unit, so there is no exponent; the weights are
    read-only, so there is no leaf (a Float8Dense's codes are not written in place) and no weight gradient."""
    forward = 'be_lif_rec_dense_f8_sg_forward'
    backward = 'be_lif_rec_dense_f8_sg_backward'
    takes_exp, leaf = False, None
    no_tensors = ('a Float8Dense recurrence', 'Float8Dense rec')
    kind = 'Float8Dense'

    def __init__(self, who, rec, n: int, like=None):      # codes [N, N] and one scale; the constructor has refused non-finite codes
        from ._dense_f8 import _CODE_OF_FMT
        _limit(who, n, "one workgroup holds a sample's neurons")
        c = rec._device_codes()
        if like is not None and c.device != like.device:
            raise ValueError(f"{who}: the codes of rec are on {c.device}, x is on {like.device}: they must share a device.")
        self.codes = c.contiguous() if c.numel() else torch.zeros(1, dtype=torch.uint8, device=c.device)
        self.matrix = (A.ptr(self.codes), _CODE_OF_FMT[rec.fmt], float(rec.scale))

    def exponent(self, who, scale_exp, n: int) -> int:    # nothing to ask for, nothing to give
        if scale_exp is not None:
            raise ValueError(f"{who}: scale_exp must be None with a {self.kind} rec: its recurrent sums are exact integers in the "
                             f"format's own unit (2^-9 for e4m3, 2^-16 for e5m2) and take no exponent.")
        return 0


class _Float8CSRRec(_Float8Rec):
    """A :class:`~brainevent_amd.Float8CSR`: the device arrays of its stored rows — one code per entry, the columns, an int32
    ``indptr`` — as they are (no plan, no mirror, no repacking), the format's code, the scale and the entry count.  The sums are
    ``Float8CSR``'s own exact 64-bit integers, so there is no exponent; the weights are read-only: no leaf, no weight gradient."""
    forward = 'be_lif_rec_f8_sg_forward'
    backward = 'be_lif_rec_f8_sg_backward'
    no_tensors = ('a Float8CSR recurrence', 'Float8CSR rec')
    kind = 'Float8CSR'

    def __init__(self, who, rec, n: int, like=None):      # the constructor has checked the structure and refused non-finite codes
        from ._dense_f8 import _CODE_OF_FMT
        codes, indices, indptr = rec._rows.device_arrays()
        if indptr.dtype != torch.int32:
            raise TypeError(f"{who}: the indptr of rec must be int32, not {indptr.dtype} (a Float8CSR built from an int64 indptr, or "
                            f"with 2^31 entries or more, is not built).")
        _limit(who, n, "one sample's sums and spike ids live in one workgroup's LDS")
        if like is not None and codes.device != like.device:
            raise ValueError(f"{who}: the codes of rec are on {codes.device}, x is on {like.device}: they must share a device.")
        self.nse = int(indices.numel())
        self.codes = codes.view(torch.uint8).reshape(-1) if self.nse else torch.zeros(1, dtype=torch.uint8, device=indptr.device)
        self.indices = indices if self.nse else torch.zeros(1, dtype=torch.int32, device=indptr.device)
        self.indptr = indptr
        self.matrix = (A.ptr(self.codes), _CODE_OF_FMT[rec.fmt], float(rec.scale), A.ptr(self.indices), A.ptr(self.indptr), self.nse)


def _family(rec):
    """The adapter class of ``rec``'s family, or None."""
    from ._csr import CSR
    from ._csr_f8 import Float8CSR
    from ._delay import DelayedCSR
    from ._dense import Dense
    from ._dense_f8 import Float8Dense
    for container, adapter in ((Float8Dense, _Float8Rec), (Float8CSR, _Float8CSRRec), (DelayedCSR, _DelayedRec), (Dense, _DenseRec),
                               (CSR, _Rec)):
        if isinstance(rec, container):
            return adapter
    return None


def _recurrence(who, rec, n: int, like=None) -> _Rec:
    """``rec`` classified, once, and checked: its family's adapter."""
    adapter = _family(rec)
    if adapter is None:
        raise TypeError(f"{who}: rec must be a CSR matrix (rows = presynaptic neurons), a DelayedCSR, a Dense, a Float8Dense or a "
                        f"Float8CSR, not {type(rec).__name__}; CSC (Float8CSC), fixed-number, JITC and planned matrices are not "
                        f"built.")
    if rec.shape[0] != rec.shape[1]:
        raise ValueError(f"{who}: rec {tuple(rec.shape)} must be square (a recurrent projection).")
    if rec.shape[0] != n:
        raise ValueError(f"{who}: rec {tuple(rec.shape)} must have the size of x's last axis, {n}.")
    return adapter(who, rec, n, like)


def _scale_exp(who, scale_exp, rec, n: int) -> int:
    """The exponent the calls on ``rec`` take: ``scale_exp`` checked, or for None the family's own."""
    return _recurrence(who, rec, n).exponent(who, scale_exp, n)


def _forward(x, r: _Rec, s0, c0, v0, a0, T: int, B: int, N: int, p: _Params, e: int, want_v: bool, want_h: bool):
    """The family's forward entry point on contiguous ``x [T, B, N]``: ``(s, v_seq, h, th, c_last, v_last, a_last)``; what was not
    asked for (and, without adaptation, ``th`` / ``a_last``) is None and neither allocated nor written.  ``s0`` is ``[B, N]``, with
    delays ``[ages, B, N]``, or None."""
    outs = _new_outputs(x, (B, N), (c0, v0, a0), T, p, (want_v, want_h, want_h and p.adaptive))
    if T != 0:
        s, v_seq, h, th, c_last, v_last, a_last = outs
        call(r.forward, A.ptr(x), *r.matrix, *r.s0_args(s0), A.ptr(c0), A.ptr(v0), A.ptr(a0), A.ptr(s), A.ptr(v_seq), A.ptr(h),
             A.ptr(th), A.ptr(c_last), A.ptr(v_last), A.ptr(a_last), T, B, N, p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa,
             p.reset, p.adaptive, *((e,) if r.takes_exp else ()), A.stream_ptr())
    return outs


def _backward(h, th, r: _Rec, g_s, g_vseq, g_last, T: int, B: int, N: int, p: _Params, want):
    """The family's backward entry point: ``(g_x, g_c0, g_v0, g_a0, g_s0)``, the last in ``s0``'s shape.  A gradient that is None
    goes in as NULL; a state or ``s0`` gradient is None unless ``want`` asks for it."""
    shapes = [(B, N) if k else None for k in want[:3]] + [r.s0_shape(B, N) if want[3] else None]
    g_x, g_c0, g_v0, g_a0, g_s0 = grads = _new_grads(h, shapes, g_last, T == 0)
    if T != 0:
        call(r.backward, A.ptr(h), A.ptr(th), *r.matrix, A.ptr(g_s), A.ptr(g_vseq), A.ptr(g_last[0]), A.ptr(g_last[1]),
             A.ptr(g_last[2]), A.ptr(g_x), A.ptr(g_c0), A.ptr(g_v0), A.ptr(g_a0), *r.s0_args(g_s0), T, B, N, p.syn_decay, p.beta,
             p.v_th, p.v_reset, p.rho, p.kappa, p.reset, p.surrogate, p.alpha, p.adaptive, p.detach_reset, A.stream_ptr())
    return grads


def _grads_in(ctx, g_s, rest):
    """The prologue both Functions' ``backward`` share: None if no output's gradient arrived; else what was saved, ``needs_input_grad``,
    which state and ``s0`` gradients are wanted, and the arrived gradients contiguous — ``g_s``, ``g_vseq``, ``g_last`` (three entries)."""
    p, return_v = ctx.meta[2:]
    g_vseq = rest[0] if return_v else None
    g_last = list(rest[1:] if return_v else rest) + [None] * (3 - p.entries)
    if g_s is None and g_vseq is None and all(g is None for g in g_last):
        return None
    saved, need = ctx.saved_tensors, ctx.needs_input_grad
    want = [need[1], need[2], bool(p.adaptive) and need[3], need[4]]
    return saved, need, want, _grad_in(g_s), _grad_in(g_vseq), [_grad_in(g) for g in g_last]


class RecurrentLifSequence(torch.autograd.Function):
    """Every family's Function.  Outputs ``s, [v_seq,] c_last, v_last [, a_last]``; ``w`` is the adapter's leaf and ``s0`` as the
    kernels take it.  Saved: ``h``, ``th`` when adaptive and, where there is a leaf (all but FP8 weights, dense or sparse), ``s`` (the weight
    gradient's activity), the weights and ``s0``.  The gradient of an output nobody used arrives as None
    (``set_materialize_grads(False)``) and goes in as NULL; the weight gradient is computed only if the weights need one."""

    @staticmethod
    def forward(ctx, x, c0, v0, a0, s0, w, r: _Rec, dims, p: _Params, e: int, return_v: bool):
        ctx.set_materialize_grads(False)
        T, B, N = dims
        s, v_seq, h, th, c_last, v_last, a_last = _forward(x, r, s0, c0, v0, a0, T, B, N, p, e, return_v, True)
        ctx.save_for_backward(*((h, th) if w is None else (h, th, s, w, s0)))
        ctx.meta = (r, dims, p, return_v)
        return tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, *rest):
        grads = _grads_in(ctx, g_s, rest)
        if grads is None:
            return (None,) * 11
        (h, th, *kept), need, want, g_s, g_vseq, g_last = grads
        r, (T, B, N), p, _ = ctx.meta
        g_x, g_c0, g_v0, g_a0, g_s0 = _backward(h, th, r, g_s, g_vseq, g_last, T, B, N, p, want)
        g_w = r.weight_grad(*kept, g_x, T, B, N) if need[5] else None
        return (g_x if need[0] else None), g_c0, g_v0, g_a0, g_s0, g_w, None, None, None, None, None


def recurrent_lif_sequence(x: torch.Tensor, rec, state0: Optional[Sequence[Optional[torch.Tensor]]] = None,
                           s0: Optional[torch.Tensor] = None, *, syn_decay: float = 0.0, beta: float, v_th: float = 1.0,
                           v_reset: float = 0.0, reset: str = 'hard', surrogate: str = 'fast_sigmoid', alpha: float = 10.0,
                           detach_reset: bool = False, adapt: Optional[Tuple[float, float]] = None, return_v: bool = False,
                           scale_exp: Optional[int] = None):
    """A recurrent layer of current-based leaky integrate-and-fire neurons over a whole input sequence, one launch forwards and
    one backwards: at every step the input of :func:`synaptic_lif_step` is ``x[t] + s[t-1] @ rec`` — the previous step's spikes
    through the sparse recurrent projection ``rec`` (a :class:`CSR` ``[N, N]``, rows = presynaptic neurons, one f32 weight per
    stored entry; duplicate columns, self-loops and empty rows are allowed).  ``x`` is ``[T, B, N]`` (or ``[T, N]``: one sample);
    ``state0`` (None, or a None entry: zeros) and the returned state are ``(c, v)``, or ``(c, v, a)`` with ``adapt=(rho, kappa)``,
    each ``[B, N]``; ``s0 [B, N]`` (f32, active where ``!= 0``; None: no spike) are the spikes before step 0.  Returns
    ``(s [T, B, N], state_last)``, or ``(s, v_seq, state_last)`` with ``return_v``.  ``syn_decay=0`` is the plain LIF.  The neuron's
    parameters, surrogates and ``detach_reset`` are :func:`synaptic_lif_sequence`'s; ``detach_reset`` does not cut the recurrent path.

    The recurrent sums are 64-bit fixed-point integers at the exponent ``scale_exp``, so the forward pass is a function of its
    inputs bit for bit.  ``scale_exp=None`` asks :func:`~brainevent_amd._csr.fixed_point_exponent` for it on every call — its
    bound, every row active, is exactly this kernel's worst case — which costs ONE HOST SYNCHRONISATION per call and cannot run
    under graph capture.  An ``int`` (for instance that function's answer, computed once; still valid while no column's sum of
    ``|w|`` grows past the next power of two) is used as given: no synchronisation, usable under ``capture_step``.

    Differentiable, once, in ``x``, every given state entry, ``s0`` and ``rec.data`` through ``s``, ``v_seq`` and the returned
    state: straight-through in the spikes for the recurrent product (as ``BinaryArray(s) @ rec``), the surrogate for the neuron.
    ``rec.data`` is read from device memory on every call: an in-place update is seen by the next call.

    The neuron's parameters are Python numbers here; :func:`parametric_recurrent_lif_sequence` takes them as device tensors, shared
    or per neuron, and differentiates them.

    **Synaptic delays.**  ``rec`` may be a :class:`DelayedCSR` ``[N, N]`` (``csr.with_delays(delays, depth)``; f32 weights, one
    per entry, an int32 ``stacked.indptr``): the entry ``e`` then delivers the spike its row emitted ``delays[e]`` steps before the
    previous step, ``xin[t][j] = x[t][j] + sum of w_e over the entries e of column j with sp(t - 1 - delays[e])[row(e)] != 0``, where
    ``sp(tau)`` is ``s[tau]`` for ``tau >= 0`` and the history ``s0`` before step 0 — delay 0 everywhere is the layer without delays.
    ``s0`` is then ``[B, N]`` (the previous step alone, as above) or ``[A, B, N]`` with ``1 <= A <= depth``: ``s0[a]`` are the spikes
    emitted ``a + 1`` steps before step 0, older steps were silent (with ``x [T, N]``: ``[N]`` or ``[A, N]``).  Everything else is as
    above, still one launch each way (``be_lif_rec_delay_sg_forward`` / ``_backward``); the forward contract is the same, the sums
    running over the active stacked rows; ``scale_exp=None`` asks for the exponent of ``rec.stacked``.  Differentiable in ``x``, the
    state, ``s0`` (in its own shape) and ``rec.stacked.data`` — the leaf, as for ``ring @ D``; ``rec.stacked_to_original`` moves its
    gradient to the order the synapses were given in.  The limit is ``N <= 8192`` with ``8 * N + 8 * depth * ceil(N / 64) + 16384 <=
    162816`` (every ``N <= 8192`` at ``depth <= 16``, every ``N <= 2048`` at ``depth <= 256``).

    **A dense recurrence.**  ``rec`` may be a :class:`Dense` ``[N, N]`` (f32 — or f16 / bf16, below —, rows = presynaptic neurons; ``rec.data`` may be a
    ``torch.nn.Parameter``): the same function as on the :class:`CSR` that stores all ``N * N`` entries of the matrix at the same
    exponent — the forward outputs are equal bit for bit, a zero entry adds the integer 0 — through kernels that walk the matrix
    itself (``be_lif_rec_dense_sg_forward`` / ``_backward``), still one launch each way.  ``scale_exp=None`` asks for the exponent of
    that fully stored CSR (one host synchronisation).  Differentiable in ``x``, the state, ``s0`` and ``rec.data``; the backward
    row products are f32 sums in an order ``N`` alone fixes (not the CSR kernel's).  ``N <= 8192``.

    **f16 / bf16 dense weights.**  ``rec.data`` of a :class:`Dense` may be ``torch.float16`` or ``torch.bfloat16`` (row-major, possibly
    a ``Parameter``): the layer is the f32 layer on ``rec.data.float()``.  The up-conversion is exact and the recurrent sums are the
    same 64-bit integers, so every forward output equals the f32 call's on ``rec.data.float()`` at the same exponent, bit for bit
    (``be_lif_rec_dense_half_sg_forward`` / ``_backward``: kernels of their own, one launch each way, no f32 copy of the matrix).
    ``scale_exp=None`` asks for the exponent of the up-converted matrix: one host synchronisation AND an f32 ``[N, N]`` temporary
    per call; an ``int`` is used as given and runs under ``capture_step``.  The backward row products up-convert in registers, round
    every product and add in f32 in an order ``N`` alone fixes (the half kernel's own).  The gradient of ``rec.data`` has its dtype:
    it is summed in f32 from the f32 ``g_x`` (``be_grad_dense`` into an f32 ``[N, N]`` temporary) and rounded to the dtype once.

    **FP8 dense weights.**  ``rec`` may be a :class:`Float8Dense` ``[N, N]`` (``quantize_fp8(W, fmt)``: e4m3 or e5m2 codes and one f32
    ``scale``; rows = presynaptic neurons): ``xin[t][j] = x[t][j] + fl32(fl32(sum of decode(codes[i, j]) over the spiking i) * scale)``.
    Every finite e4m3 / e5m2 value is a multiple of 2^-9 / 2^-16, so the inner sum is an exact integer in that unit — rounded to f32
    once, then multiplied by ``scale`` in f32: ``Float8Dense``'s own product contract with the sum exact, equal to the per-step loop
    ``x[t] + BinaryArray(s) @ rec`` wherever that loop's f32 sums are exact, and a function of the inputs bit for bit
    (``be_lif_rec_dense_f8_sg_forward`` / ``_backward``, one launch each way, ``N <= 8192``).  ``scale_exp`` must stay ``None`` (an
    int raises ``ValueError``: there is no exponent); the call never synchronises the host and always runs under ``capture_step``.
    The weights are read-only and get no gradient.  Unlike the ``events @ Float8Dense`` products, which refuse an operand that
    requires grad, this layer ACCEPTS a grad-requiring ``x`` / state / ``s0`` and differentiates them, once — a frozen, quantised
    recurrence inside a trained network passes ``g_x`` to the layers below; backwards ``g_rec[i] = fl32((sum_j decode(codes[i, j]) *
    G[j]) * scale)``, f32 products and sums in an order ``N`` alone fixes, the scale applied once per row.

    **FP8 sparse weights.**  ``rec`` may be a :class:`Float8CSR` ``[N, N]`` (``csr.quantize_fp8(fmt)``: one e4m3 or e5m2 code per stored
    entry and one f32 ``scale``; rows = presynaptic neurons, an int32 ``indptr``; duplicate columns, self-loops and empty rows are
    allowed): ``xin[t][j] = x[t][j] + f32(f64(R[j]) * ldexp(f64(scale), -E))`` with ``R[j]`` the sum of ``decode(code) * 2^E`` (``E`` = 9 /
    16: an integer for every finite code) over the entries of column ``j`` in the rows that spiked — an exact 64-bit integer whatever
    the order, finished as ``events @ W8`` finishes it.  So the layer equals the per-step loop ``x[t] + BinaryArray(s) @ rec`` bit for
    bit, unconditionally, and is a function of its inputs bit for bit (``be_lif_rec_f8_sg_forward`` / ``_backward``, one launch each
    way, ``N <= 8192``; the kernels read the container's arrays as they are: no plan, no mirror, no repacking).  ``scale_exp`` must
    stay ``None`` (an int raises ``ValueError``: there is no exponent); the call never synchronises the host and always runs under
    ``capture_step``.  The weights are read-only and get no gradient.  Unlike the ``events @ Float8CSR`` products, which refuse an
    operand that requires grad, this layer ACCEPTS a grad-requiring ``x`` / state / ``s0`` and differentiates them, once, as with a
    :class:`Float8Dense`: backwards ``g_rec[i] = fl32((sum over row i of decode(code_k) * G[col_k]) * scale)``, f32 products and sums
    in an order the row's length alone fixes, the scale applied once per row.  A :class:`Float8CSC` (``W8.T``) is refused.

    Not built: CSC / fixed-number / JITC recurrences, a Dense, Float8Dense or Float8CSR recurrence with tensor parameters, a Dense or
    FP8 recurrence with delays (FP8 weights for a DelayedCSR), a (straight-through) gradient of FP8 weights, per-row or per-block FP8 scales,
    one shared weight, learnable delays, ``N > 8192``, a sample split over several workgroups (only ``B`` of the chip's compute units
    work)."""
    who = 'recurrent_lif_sequence'
    p = _Params(who, syn_decay, beta, v_th, v_reset, reset, surrogate, alpha, detach_reset, adapt)
    r, (T, B, N), slots, x3, (c0, v0, a0, sp), e = _prepare(who, x, rec, state0, s0, p, scale_exp)
    return_v = bool(return_v)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x3, c0, v0, a0, sp, r.leaf)):
        outs = RecurrentLifSequence.apply(x3, c0, v0, a0, sp, r.leaf, r, (T, B, N), p, e, return_v)
    else:                                     # no backward pass: h / th are not kept
        s, v_seq, _, _, c_last, v_last, a_last = _forward(x3, r, sp, c0, v0, a0, T, B, N, p, e, return_v, False)
        outs = tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)
    return _shaped(outs, x, slots, return_v)


def _prepare(who, x, rec, state0, s0, p: _Params, scale_exp):
    """The checks and layouts both functions share: the adapter of ``rec``, ``(T, B, N)``, the shape of a step, contiguous
    ``x [T, B, N]``, the state entries and ``s0`` as the kernels take them (``[B, N]``, with delays ``[ages, B, N]``; or None), and the
    exponent."""
    _check_tensor(who, 'x', x)
    if x.ndim not in (2, 3):
        raise ValueError(f"{who}: x must be [T, B, N] or [T, N], not {x.ndim}-dimensional.")
    slots = tuple(x.shape[1:])
    T, N = int(x.shape[0]), int(x.shape[-1])
    B = int(x.shape[1]) if x.ndim == 3 else 1
    r = _recurrence(who, rec, N, x)
    state = _check_state(who, 'state0', state0, p, slots, allow_none=True)
    if s0 is not None:
        _check_tensor(who, 's0', s0)
        r.check_s0(who, s0, slots)
    _check_device(who, x=x, s0=s0, **{f'state0 entry {k}': t for k, t in zip('cva', state)})
    e = r.exponent(who, scale_exp, N)
    x3 = x.contiguous().reshape(T, B, N)
    start = tuple(None if t is None else t.contiguous().reshape(B, N) for t in state)
    if s0 is not None:
        s0 = s0.contiguous().reshape(r.s0_shape(B, N))
    return r, (T, B, N), slots, x3, start + (s0,), e


def _shaped(outs, x, slots, return_v: bool):
    k = 2 if return_v else 1
    return tuple(o.reshape(x.shape) for o in outs[:k]) + (tuple(o.reshape(slots) for o in outs[k:]),)


# ------------------------------------------------------------------------------------------------ the five parameters on the device
def _forward_params(x, r: _Rec, s0, c0, v0, a0, params, T: int, B: int, N: int, p: _Params, e: int, want_v: bool, want_h: bool,
                    want_c: bool):
    """``be_lif_rec_sg_forward_params``: :func:`_forward` with the five parameters contiguous f32 device tensors (``rho`` / ``kappa``
    None without adaptation; a period is the element count): ``(s, v_seq, h, c_save, a_save, c_last, v_last, a_last)``.  ``a_save`` —
    the trace every step started from — is kept beside ``h`` when adaptive, ``c_save`` only when asked for."""
    outs = _new_outputs(x, (B, N), (c0, v0, a0), T, p, (want_v, want_h, want_c, want_h and p.adaptive))
    if T != 0 and B * N > 0:
        s, v_seq, h, c_save, a_save, c_last, v_last, a_last = outs
        call('be_lif_rec_sg_forward_params', A.ptr(x), *r.matrix, A.ptr(s0), A.ptr(c0), A.ptr(v0), A.ptr(a0),
             *(v for t in params for v in (A.ptr(t), 1 if t is None else t.numel())), A.ptr(s), A.ptr(v_seq), A.ptr(h),
             A.ptr(c_save), A.ptr(a_save), A.ptr(c_last), A.ptr(v_last), A.ptr(a_last), T, B, N, p.v_reset, p.reset, p.adaptive, e,
             A.stream_ptr())
    return outs


class RecurrentLifSequenceParams(torch.autograd.Function):
    """:class:`RecurrentLifSequence` over a CSR with the five parameters as device tensors that may require grad.  Saved: ``h``,
    ``a_save`` in ``th``'s place when adaptive, ``s``, the weights, ``s0``, the parameters, ``c_save`` only if ``syn_decay`` needs a
    gradient, and ``c0`` / ``v0`` only for the gradient of ``syn_decay`` / ``beta`` (what the first step started from).  A parameter
    that does not need a gradient has its ``[B, N]`` accumulator go in as NULL."""

    @staticmethod
    def forward(ctx, x, c0, v0, a0, s0, w, syn_decay, beta, v_th, rho, kappa, r: _Rec, dims, p: _Params, e: int, return_v: bool):
        ctx.set_materialize_grads(False)
        T, B, N = dims
        params = (syn_decay, beta, v_th, rho, kappa)
        need_sd, need_b = ctx.needs_input_grad[6], ctx.needs_input_grad[7]
        s, v_seq, h, c_save, a_save, c_last, v_last, a_last = _forward_params(x, r, s0, c0, v0, a0, params, T, B, N, p, e, return_v,
                                                                              True, need_sd)
        ctx.save_for_backward(h, a_save, s, w, s0, c_save, *params, c0 if need_sd else None, v0 if need_b else None)
        ctx.meta = (r, dims, p, return_v)
        return tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, *rest):
        grads = _grads_in(ctx, g_s, rest)
        if grads is None:
            return (None,) * 16
        (h, a_save, s, w, s0, c_save, *params, c0, v0), need, want, g_s, g_vseq, g_last = grads
        r, (T, B, N), p, _ = ctx.meta
        need_p = [need[6 + k] and params[k] is not None for k in range(5)]
        no_step = T == 0 or B * N == 0        # the state's gradient passes through, the parameters were not used
        g_x, *g_state = _new_grads(h, [(B, N) if k else None for k in want], g_last, no_step)
        if no_step:
            g_params = [torch.zeros_like(t) if k else None for t, k in zip(params, need_p)]
        else:
            slot = [torch.empty((B, N), dtype=h.dtype, device=h.device) if k else None for k in need_p]
            call('be_lif_rec_sg_backward_params', A.ptr(h), A.ptr(c_save), A.ptr(a_save), A.ptr(c0), A.ptr(v0), *r.matrix, A.ptr(g_s),
                 A.ptr(g_vseq), A.ptr(g_last[0]), A.ptr(g_last[1]), A.ptr(g_last[2]),
                 *(v for t in params for v in (A.ptr(t), 1 if t is None else t.numel())), A.ptr(g_x), *(A.ptr(g) for g in g_state),
                 *(A.ptr(t) for t in slot), T, B, N, p.v_reset, p.reset, p.surrogate, p.alpha, p.adaptive, p.detach_reset,
                 A.stream_ptr())
            g_params = [_reduce_slots(sl.reshape(-1), t) if k else None for sl, t, k in zip(slot, params, need_p)]
        g_w = r.weight_grad(s, w, s0, g_x, T, B, N) if need[5] else None
        return ((g_x if need[0] else None), *g_state, g_w, *g_params, None, None, None, None, None)


def _layer_params(who, given, like, N: int, adaptive):
    """The five parameters as contiguous device tensors (a number: one element).  The rule of this layer, beyond
    :func:`~brainevent_amd._neuron_syn_sg._device_params`': a tensor has one element or is ``[N]`` — the shape of a step is
    ``[B, N]``, but a value per sample and neuron is refused: the layer's neurons are the same neurons in every sample, as the rows
    of ``rec`` are."""
    labels = ('syn_decay', 'beta', 'v_th', 'adapt[0] (rho)', 'adapt[1] (kappa)')
    for label, v in zip(labels, given):
        if isinstance(v, torch.Tensor) and v.ndim >= 2 and v.numel() != 1:
            raise ValueError(f"{who}: {label} {tuple(v.shape)} must have one element or be [N] = ({N},): the layer's neurons are the "
                             f"same neurons in every sample, as rec is, so a parameter has no batch dimension ([B, N] parameters "
                             f"are not built).")
    return _device_params(who, given, like, (N,), adaptive)


def parametric_recurrent_lif_sequence(x: torch.Tensor, rec, state0: Optional[Sequence[Optional[torch.Tensor]]] = None,
                                      s0: Optional[torch.Tensor] = None, *, syn_decay=0.0, beta, v_th=1.0, v_reset: float = 0.0,
                                      reset: str = 'hard', surrogate: str = 'fast_sigmoid', alpha: float = 10.0,
                                      detach_reset: bool = False, adapt=None, return_v: bool = False,
                                      scale_exp: Optional[int] = None):
    """:func:`recurrent_lif_sequence` with each of ``syn_decay``, ``beta``, ``v_th`` and the two entries of ``adapt = (rho, kappa)``
    independently a Python number or an f32 device tensor: one element (0-d or ``[1]``) for a value the layer shares, or ``[N]`` for a
    value per neuron, shared by the samples of the batch (a ``[B, N]`` tensor is refused: the layer's neurons are the same neurons in
    every sample, as ``rec`` is).  The LSNN with heterogeneous, learned time constants and thresholds as two launches.

    A tensor is read on the device (never copied to the host: an optimiser's in-place update is seen by the next call and the next
    replay of a captured graph — with ``scale_exp`` given the function runs under ``capture_step``) and, if it requires grad, gets
    its gradient in its own shape: per (sample, neuron) the sum over time from the backward launch, in f32 in descending ``t``, then
    the sum over the samples — and, for one element, the neurons — in f64 in a fixed order (``be_lif_sg_reduce_slots``).  A number
    beside a tensor becomes a one-element device tensor; all numbers is :func:`recurrent_lif_sequence` itself.  ``v_reset`` and
    ``alpha`` stay numbers.  ``x``, ``rec``, ``state0``, ``s0``, ``scale_exp``, the outputs, the limit ``N <= 8192``, the refusals and
    the bit-for-bit forward contract are :func:`recurrent_lif_sequence`'s (``be_lif_rec_sg_forward_params``); differentiable, once,
    in ``x``, the state entries, ``s0``, ``rec.data`` and the five parameters.

    A :class:`DelayedCSR`, a :class:`Dense` (f32, f16 or bf16 weights), a :class:`Float8Dense` or a :class:`Float8CSR` is taken with
    all-number parameters only (that is :func:`recurrent_lif_sequence`); with a tensor parameter it raises ``NotImplementedError``.

    Not built: learnable ``v_reset`` / ``alpha``, ``[B, N]`` parameters, tensor parameters with synaptic delays, a dense (Dense,
    Float8Dense) or an FP8 (Float8Dense, Float8CSR) recurrence, and what
    :func:`recurrent_lif_sequence` does not build."""
    who = 'parametric_recurrent_lif_sequence'
    given, stand_in, any_tensor = _split_params(who, syn_decay, beta, v_th, adapt)
    if not any_tensor:
        return recurrent_lif_sequence(x, rec, state0, s0, syn_decay=syn_decay, beta=beta, v_th=v_th, v_reset=v_reset, reset=reset,
                                      surrogate=surrogate, alpha=alpha, detach_reset=detach_reset, adapt=adapt, return_v=return_v,
                                      scale_exp=scale_exp)
    adapter = _family(rec)
    if adapter is not None and adapter.no_tensors is not None:
        what, which = adapter.no_tensors
        raise NotImplementedError(f"{who}: learnable (tensor) neuron parameters together with {what} are not built: a {which} "
                                  f"takes syn_decay, beta, v_th and adapt as Python numbers (recurrent_lif_sequence).")
    p = _Params(who, stand_in[0], stand_in[1], stand_in[2], v_reset, reset, surrogate, alpha, detach_reset,
                None if adapt is None else (stand_in[3], stand_in[4]), FIVE_TENSORS)
    r, (T, B, N), slots, x3, (c0, v0, a0, sp), e = _prepare(who, x, rec, state0, s0, p, scale_exp)
    params = _layer_params(who, given, x, N, p.adaptive)
    return_v = bool(return_v)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x3, c0, v0, a0, sp, r.leaf, *params)):
        outs = RecurrentLifSequenceParams.apply(x3, c0, v0, a0, sp, r.leaf, *params, r, (T, B, N), p, e, return_v)
    else:                                     # no backward pass: nothing is kept
        s, v_seq, _, _, _, c_last, v_last, a_last = _forward_params(x3, r, sp, c0, v0, a0, params, T, B, N, p, e, return_v, False,
                                                                    False)
        outs = tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)
    return _shaped(outs, x, slots, return_v)
