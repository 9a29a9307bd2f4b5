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

Not built: CSC / fixed-number / dense / JITC recurrences, one shared (homogeneous) weight, learnable ``v_reset`` / ``alpha``,
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
from ._neuron_syn_sg import FIVE_TENSORS, _Params, _check_state, _device_params, _split_params

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


class _Rec:
    """The CSR arrays as the kernels take them (a matrix without entries hands over one unused element: no NULL pointer)."""
    __slots__ = ('w', 'indices', 'indptr', 'nse')

    def __init__(self, w, indices, indptr):
        self.nse = int(indices.numel())
        self.w = w.reshape(-1) if self.nse else torch.zeros(1, dtype=torch.float32, device=indptr.device)
        self.indices = indices if self.nse else torch.zeros(1, dtype=torch.int32, device=indptr.device)
        self.indptr = indptr


def _forward(x, r: _Rec, s0, c0, v0, a0, T: int, B: int, N: int, p: _Params, e: int, want_v: bool, want_h: bool):
    """``be_lif_rec_sg_forward`` on contiguous ``x [T, B, N]``: ``(s, v_seq, h, th, c_last, v_last, a_last)``; what was not asked
    for (and, without adaptation, ``th`` / ``a_last``) is None and neither allocated nor written."""
    new = lambda: torch.empty((B, N), dtype=x.dtype, device=x.device)
    s = torch.empty_like(x)
    v_seq = torch.empty_like(x) if want_v else None
    h = torch.empty_like(x) if want_h else None
    th = torch.empty_like(x) if want_h and p.adaptive else None
    c_last, v_last, a_last = new(), new(), (new() if p.adaptive else None)
    if T == 0:                                # no step: the state passes through
        for out, start in ((c_last, c0), (v_last, v0), (a_last, a0)):
            if out is not None:
                out.zero_() if start is None else out.copy_(start)
    else:
        call('be_lif_rec_sg_forward', A.ptr(x), A.ptr(r.w), A.ptr(r.indices), A.ptr(r.indptr), A.ptr(s0), A.ptr(c0), A.ptr(v0),
             A.ptr(a0), A.ptr(s), A.ptr(v_seq), A.ptr(h), A.ptr(th), A.ptr(c_last), A.ptr(v_last), A.ptr(a_last), T, B, N,
             p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa, p.reset, p.adaptive, e, A.stream_ptr())
    return s, v_seq, h, th, c_last, v_last, a_last


def _backward(h, th, r: _Rec, g_s, g_vseq, g_last, T: int, B: int, N: int, p: _Params, want):
    """``be_lif_rec_sg_backward``: ``(g_x, g_c0, g_v0, g_a0, g_s0)``.  A gradient that is None goes in as NULL; a state or ``s0``
    gradient is None unless ``want`` asks for it."""
    g_x = torch.empty_like(h)
    g_state = [torch.empty((B, N), dtype=h.dtype, device=h.device) if k else None for k in want]
    if T == 0:
        for out, g in zip(g_state[:3], g_last):
            if out is not None:
                out.zero_() if g is None else out.copy_(g)
        if g_state[3] is not None:
            g_state[3].zero_()
    else:
        call('be_lif_rec_sg_backward', A.ptr(h), A.ptr(th), A.ptr(r.w), A.ptr(r.indices), A.ptr(r.indptr), A.ptr(g_s), A.ptr(g_vseq),
             A.ptr(g_last[0]), A.ptr(g_last[1]), A.ptr(g_last[2]), A.ptr(g_x), A.ptr(g_state[0]), A.ptr(g_state[1]), A.ptr(g_state[2]),
             A.ptr(g_state[3]), T, B, N, p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa, p.reset, p.surrogate, p.alpha,
             p.adaptive, p.detach_reset, A.stream_ptr())
    return (g_x,) + tuple(g_state)


def _weight_grad(w, r: _Rec, s, s0, g_x, T: int, B: int, N: int) -> torch.Tensor:
    """``g_w[k] = sum over t, b of sp[t][b][row k] * g_x[t][b][col k]`` with ``sp = cat(s0, s[:-1])``: ``be_grad_rows`` (the
    ``transpose=True`` side) over ``T * B`` batch rows — ``(T - 1) * B`` without ``s0`` — in ascending order; ``g_x`` is read
    batch-major through the stride arguments, nothing is transposed."""
    if T == 0 or r.nse == 0:
        return torch.zeros_like(w)
    if s0 is None:
        sp, g = s[:T - 1], g_x[1:]
    else:
        sp, g = torch.cat(((s0 != 0).to(s.dtype)[None], s[:T - 1])), g_x
    nb = int(sp.shape[0]) * B
    if nb == 0:
        return torch.zeros_like(w)
    mask, _ = _autograd.activity(sp.reshape(nb, N), 'bm')
    dw = torch.empty(r.nse, dtype=w.dtype, device=w.device)
    g = g.contiguous()
    call('be_grad_rows', 1, A.ptr(dw), 0, A.wcode(dw), A.ptr(r.indices), A.ptr(r.indptr), 0, -1, N, r.nse, A.ptr(mask), nb, A.ptr(g),
         1, N, A.ptr(None), 0, A.stream_ptr())
    return dw.reshape(w.shape)


class RecurrentLifSequence(torch.autograd.Function):
    """Outputs ``s, [v_seq,] c_last, v_last [, a_last]``.  Saved: ``h``, ``th`` when adaptive, ``s`` (the weight gradient's
    activity), the weights and ``s0``.  The gradient of an output nobody used arrives as None (``set_materialize_grads(False)``)
    and goes in as NULL."""

    @staticmethod
    def forward(ctx, x, c0, v0, a0, s0, w, r: _Rec, dims, p: _Params, e: int, return_v: bool):
        ctx.set_materialize_grads(False)
        T, B, N = dims
        s, v_seq, h, th, c_last, v_last, a_last = _forward(x, r, s0, c0, v0, a0, T, B, N, p, e, return_v, True)
        ctx.save_for_backward(h, th, s, w, s0)
        ctx.meta = (r, dims, p, return_v)
        return tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, *rest):
        r, (T, B, N), p, return_v = ctx.meta
        g_vseq = rest[0] if return_v else None
        g_last = list(rest[1:] if return_v else rest) + [None] * (3 - p.entries)
        if g_s is None and g_vseq is None and all(g is None for g in g_last):
            return (None,) * 11
        h, th, s, w, s0 = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = [need[1], need[2], bool(p.adaptive) and need[3], need[4]]
        g_x, g_c0, g_v0, g_a0, g_s0 = _backward(h, th, r, _grad_in(g_s), _grad_in(g_vseq), [_grad_in(g) for g in g_last], T, B, N, p,
                                                want)
        g_w = _weight_grad(w, r, s, s0, g_x, T, B, N) if need[5] else None
        return (g_x if need[0] else None), g_c0, g_v0, g_a0, g_s0, g_w, None, None, None, None, None


class _DelayedRec:
    """The stacked arrays of a :class:`~brainevent_amd.DelayedCSR` as the delayed kernels take them (as :class:`_Rec`: a matrix
    without entries hands over one unused element)."""
    __slots__ = ('w', 'indices', 'indptr', 'row_mask', 'depth', 'nse')

    def __init__(self, w, rec):
        st = rec.stacked
        self.nse = int(st.indices.numel())
        self.w = w.reshape(-1) if self.nse else torch.zeros(1, dtype=torch.float32, device=st.indptr.device)
        self.indices = st.indices if self.nse else torch.zeros(1, dtype=torch.int32, device=st.indptr.device)
        self.indptr, self.row_mask, self.depth = st.indptr, rec.row_mask, int(rec.depth)


def _forward_delay(x, r: _DelayedRec, s_hist, c0, v0, a0, T: int, B: int, N: int, p: _Params, e: int, want_v: bool, want_h: bool):
    """``be_lif_rec_delay_sg_forward``: :func:`_forward` with the stacked arrays and ``s_hist [A, B, N]`` (or None: ``A = 0``)."""
    new = lambda: torch.empty((B, N), dtype=x.dtype, device=x.device)
    s = torch.empty_like(x)
    v_seq = torch.empty_like(x) if want_v else None
    h = torch.empty_like(x) if want_h else None
    th = torch.empty_like(x) if want_h and p.adaptive else None
    c_last, v_last, a_last = new(), new(), (new() if p.adaptive else None)
    if T == 0:                                # no step: the state passes through
        for out, start in ((c_last, c0), (v_last, v0), (a_last, a0)):
            if out is not None:
                out.zero_() if start is None else out.copy_(start)
    else:
        call('be_lif_rec_delay_sg_forward', A.ptr(x), A.ptr(r.w), A.ptr(r.indices), A.ptr(r.indptr), A.ptr(r.row_mask), r.depth,
             A.ptr(s_hist), 0 if s_hist is None else int(s_hist.shape[0]), A.ptr(c0), A.ptr(v0), A.ptr(a0), A.ptr(s), A.ptr(v_seq),
             A.ptr(h), A.ptr(th), A.ptr(c_last), A.ptr(v_last), A.ptr(a_last), T, B, N, p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho,
             p.kappa, p.reset, p.adaptive, e, A.stream_ptr())
    return s, v_seq, h, th, c_last, v_last, a_last


def _backward_delay(h, th, r: _DelayedRec, g_s, g_vseq, g_last, ages: int, T: int, B: int, N: int, p: _Params, want):
    """``be_lif_rec_delay_sg_backward``: ``(g_x, g_c0, g_v0, g_a0, g_s_hist)``, the last ``[ages, B, N]``; None as in
    :func:`_backward`."""
    g_x = torch.empty_like(h)
    g_state = [torch.empty((B, N), dtype=h.dtype, device=h.device) if k else None for k in want[:3]]
    g_hist = torch.empty((ages, B, N), dtype=h.dtype, device=h.device) if want[3] else None
    if T == 0:
        for out, g in zip(g_state, g_last):
            if out is not None:
                out.zero_() if g is None else out.copy_(g)
        if g_hist is not None:
            g_hist.zero_()
    else:
        call('be_lif_rec_delay_sg_backward', A.ptr(h), A.ptr(th), A.ptr(r.w), A.ptr(r.indices), A.ptr(r.indptr), A.ptr(r.row_mask),
             r.depth, A.ptr(g_s), A.ptr(g_vseq), A.ptr(g_last[0]), A.ptr(g_last[1]), A.ptr(g_last[2]), A.ptr(g_x), A.ptr(g_state[0]),
             A.ptr(g_state[1]), A.ptr(g_state[2]), A.ptr(g_hist), ages, T, B, N, p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa,
             p.reset, p.surrogate, p.alpha, p.adaptive, p.detach_reset, A.stream_ptr())
    return (g_x,) + tuple(g_state) + (g_hist,)


def _weight_grad_delay(w, r: _DelayedRec, s, s_hist, g_x, T: int, B: int, N: int) -> torch.Tensor:
    """``g_w[k] = sum over t, b of sp(t - 1 - d)[b][i] * g_x[t][b][col k]`` for ``k`` in stacked row ``d * N + i``: one launch packs the
    aged activity of all ``depth * N`` stacked rows over the ``T * B`` batch rows (``be_grad_pack_activity_aged``), then
    ``be_grad_rows`` (``transpose=True``) over the stacked matrix, in ascending ``(t, b)``."""
    nb = T * B
    if nb == 0 or N == 0 or r.nse == 0:
        return torch.zeros_like(w)
    rows = r.depth * N
    mask = torch.empty(max(fn('be_grad_mask_bytes')(rows, nb), 4) // 4, dtype=torch.int32, device=w.device)
    call('be_grad_pack_activity_aged', A.ptr(s), A.ptr(s_hist), N, B, T, r.depth, 0 if s_hist is None else int(s_hist.shape[0]),
         A.ptr(mask), A.stream_ptr())
    dw = torch.empty(r.nse, dtype=w.dtype, device=w.device)
    call('be_grad_rows', 1, A.ptr(dw), 0, A.wcode(dw), A.ptr(r.indices), A.ptr(r.indptr), 0, -1, rows, r.nse, A.ptr(mask), nb,
         A.ptr(g_x), 1, N, A.ptr(None), 0, A.stream_ptr())
    return dw.reshape(w.shape)


class DelayedRecurrentLifSequence(torch.autograd.Function):
    """:class:`RecurrentLifSequence` over a :class:`~brainevent_amd.DelayedCSR`: ``w`` is ``rec.stacked.data`` and ``s0`` the
    history ``[A, B, N]`` (or None).  Saved: ``h``, ``th`` when adaptive, ``s``, the weights and ``s0``; a None gradient goes in as
    NULL; the weight gradient is computed only if the weights need one."""

    @staticmethod
    def forward(ctx, x, c0, v0, a0, s0, w, r: _DelayedRec, dims, p: _Params, e: int, return_v: bool):
        ctx.set_materialize_grads(False)
        T, B, N = dims
        s, v_seq, h, th, c_last, v_last, a_last = _forward_delay(x, r, s0, c0, v0, a0, T, B, N, p, e, return_v, True)
        ctx.save_for_backward(h, th, s, w, s0)
        ctx.meta = (r, dims, p, return_v)
        return tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, *rest):
        r, (T, B, N), p, return_v = ctx.meta
        g_vseq = rest[0] if return_v else None
        g_last = list(rest[1:] if return_v else rest) + [None] * (3 - p.entries)
        if g_s is None and g_vseq is None and all(g is None for g in g_last):
            return (None,) * 11
        h, th, s, w, s0 = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = [need[1], need[2], bool(p.adaptive) and need[3], need[4]]
        ages = 0 if s0 is None else int(s0.shape[0])
        g_x, g_c0, g_v0, g_a0, g_s0 = _backward_delay(h, th, r, _grad_in(g_s), _grad_in(g_vseq), [_grad_in(g) for g in g_last], ages,
                                                      T, B, N, p, want)
        g_w = _weight_grad_delay(w, r, s, s0, g_x, T, B, N) if need[5] else None
        return (g_x if need[0] else None), g_c0, g_v0, g_a0, g_s0, g_w, None, None, None, None, None


def _is_delayed(rec) -> bool:
    from ._delay import DelayedCSR
    return isinstance(rec, DelayedCSR)


def _check_rec(who, rec, n: int):
    from ._csr import CSR
    delayed = _is_delayed(rec)
    if not delayed and not isinstance(rec, CSR):
        raise TypeError(f"{who}: rec must be a CSR matrix (rows = presynaptic neurons) or a DelayedCSR, not {type(rec).__name__}; "
                        f"CSC, fixed-number, dense, JITC and planned matrices are not built.")
    if rec.shape[0] != rec.shape[1]:
        raise ValueError(f"{who}: rec {tuple(rec.shape)} must be square (a recurrent projection).")
    if rec.shape[0] != n:
        raise ValueError(f"{who}: rec {tuple(rec.shape)} must have the size of x's last axis, {n}.")
    m = rec.stacked if delayed else rec       # with delays the kernels read the stacked arrays
    if m.data.dtype != torch.float32:
        raise TypeError(f"{who}: the weights of rec must be float32, not {m.data.dtype}.")
    nse = int(m.indices.numel())
    if m.data.numel() != nse:
        raise ValueError(f"{who}: rec must hold one weight per stored entry ({nse}), not {m.data.numel()} (one shared weight is not "
                         f"built).")
    if m.indptr.dtype != torch.int32:
        raise TypeError(f"{who}: the indptr of rec must be int32, not {m.indptr.dtype}" +
                        (" (a DelayedCSR built from an int64 indptr, or with 2^31 entries or more, is not built)." if delayed else "."))
    if n > MAX_N:
        raise ValueError(f"{who}: {n} neurons; the limit is {MAX_N} (one sample's sums and spike ids live in one workgroup's LDS).")
    if delayed and not delay_fits(n, int(rec.depth)):
        raise ValueError(f"{who}: {n} neurons at depth {int(rec.depth)} do not fit: with delays 8 * N + 8 * depth * ceil(N / 64) + "
                         f"{4 * DELAY_MIN_IDS} must stay within {DELAY_LDS_BYTES} bytes (one sample's sums, its spike history and a "
                         f"list of active rows live in one workgroup's LDS; every N <= 8192 fits at depth <= 16, every N <= 2048 at "
                         f"depth <= {MAX_DEPTH}); a sample split over several workgroups is not built.")


def _scale_exp(who, scale_exp, rec, n: int) -> int:
    if scale_exp is None:
        m = rec.stacked if _is_delayed(rec) else rec      # (the stacked matrix has the same columns: every stacked row active)
        if m.indices.numel() == 0 or n == 0:
            return 0
        from ._csr import fixed_point_exponent
        return fixed_point_exponent(m.data.detach(), m.indices, n)
    if isinstance(scale_exp, bool) or not isinstance(scale_exp, numbers.Integral):
        raise TypeError(f"{who}: scale_exp must be None or an int, not {type(scale_exp).__name__}.")
    if not SCALE_EXP_RANGE[0] <= scale_exp <= SCALE_EXP_RANGE[1]:
        raise ValueError(f"{who}: scale_exp {scale_exp} is outside {SCALE_EXP_RANGE[0]} .. {SCALE_EXP_RANGE[1]}, the exponents "
                         f"fixed_point_exponent returns.")
    return int(scale_exp)


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

    Not built: CSC / fixed-number / dense / JITC recurrences, one shared weight, learnable delays, ``N > 8192``, a sample split over
    several workgroups (only ``B`` of the chip's compute units work)."""
    who = 'recurrent_lif_sequence'
    p = _Params(who, syn_decay, beta, v_th, v_reset, reset, surrogate, alpha, detach_reset, adapt)
    (T, B, N), slots, x3, (c0, v0, a0, sp), e = _prepare(who, x, rec, state0, s0, p, scale_exp)
    return_v = bool(return_v)
    if _is_delayed(rec):                      # the stacked matrix, a history [A, B, N]
        w = rec.stacked.data
        r = _DelayedRec(w.detach(), rec)
        function, forward = DelayedRecurrentLifSequence, _forward_delay
    else:
        w = rec.data
        r = _Rec(w.detach(), rec.indices, rec.indptr)
        function, forward = RecurrentLifSequence, _forward
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x3, c0, v0, a0, sp, w)):
        outs = function.apply(x3, c0, v0, a0, sp, w, r, (T, B, N), p, e, return_v)
    else:                                     # no backward pass: h / th are not kept
        s, v_seq, _, _, c_last, v_last, a_last = forward(x3, r, sp, c0, v0, a0, T, B, N, p, e, return_v, False)
        outs = tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)
    return _shaped(outs, x, slots, return_v)


def _prepare(who, x, rec, state0, s0, p: _Params, scale_exp):
    """The checks and layouts both functions share: ``(T, B, N)``, the shape of a step, contiguous ``x [T, B, N]``, the state entries
    and ``s0`` as ``[B, N]`` (or None), and the exponent."""
    _check_tensor(who, 'x', x)
    if x.ndim not in (2, 3):
        raise ValueError(f"{who}: x must be [T, B, N] or [T, N], not {x.ndim}-dimensional.")
    slots = tuple(x.shape[1:])
    T, N = int(x.shape[0]), int(x.shape[-1])
    B = int(x.shape[1]) if x.ndim == 3 else 1
    _check_rec(who, rec, N)
    state = _check_state(who, 'state0', state0, p, slots, allow_none=True)
    ages = None                               # with delays: the past steps s0 holds
    if s0 is not None:
        _check_tensor(who, 's0', s0)
        if _is_delayed(rec):
            depth = int(rec.depth)
            if tuple(s0.shape) == slots:
                ages = 1
            elif s0.ndim == len(slots) + 1 and tuple(s0.shape[1:]) == slots and 1 <= s0.shape[0] <= depth:
                ages = int(s0.shape[0])
            else:
                raise ValueError(f"{who}: s0 {tuple(s0.shape)} must have the shape of a step of x, {slots}, or hold A past steps, "
                                 f"(A,) + {slots} with 1 <= A <= depth = {depth} (s0[a]: the spikes a + 1 steps before step 0).")
        elif tuple(s0.shape) != slots:
            raise ValueError(f"{who}: s0 {tuple(s0.shape)} must have the shape of a step of x, {slots}.")
    _check_device(who, x=x, s0=s0, **{f'state0 entry {k}': t for k, t in zip('cva', state)})
    e = _scale_exp(who, scale_exp, rec, N)
    x3 = x.contiguous().reshape(T, B, N)
    start = tuple(None if t is None else t.contiguous().reshape(B, N) for t in state)
    if s0 is not None:
        s0 = s0.contiguous().reshape((B, N) if ages is None else (ages, B, N))
    return (T, B, N), slots, x3, start + (s0,), e


def _shaped(outs, x, slots, return_v: bool):
    k = 2 if return_v else 1
    return tuple(o.reshape(x.shape) for o in outs[:k]) + (tuple(o.reshape(slots) for o in outs[k:]),)


# ------------------------------------------------------------------------------------------------ the five parameters on the device
def _forward_params(x, r: _Rec, s0, c0, v0, a0, params, T: int, B: int, N: int, p: _Params, e: int, want_v: bool, want_h: bool,
                    want_c: bool):
    """``be_lif_rec_sg_forward_params``: :func:`_forward` with the five parameters contiguous f32 device tensors (``rho`` / ``kappa``
    None without adaptation; a period is the element count): ``(s, v_seq, h, c_save, a_save, c_last, v_last, a_last)``.  ``a_save`` —
    the trace every step started from — is kept beside ``h`` when adaptive, ``c_save`` only when asked for."""
    new = lambda: torch.empty((B, N), dtype=x.dtype, device=x.device)
    s = torch.empty_like(x)
    v_seq = torch.empty_like(x) if want_v else None
    h = torch.empty_like(x) if want_h else None
    c_save = torch.empty_like(x) if want_c else None
    a_save = torch.empty_like(x) if want_h and p.adaptive else None
    c_last, v_last, a_last = new(), new(), (new() if p.adaptive else None)
    if T == 0:                                # no step: the state passes through
        for out, start in ((c_last, c0), (v_last, v0), (a_last, a0)):
            if out is not None:
                out.zero_() if start is None else out.copy_(start)
    elif B * N > 0:
        call('be_lif_rec_sg_forward_params', A.ptr(x), A.ptr(r.w), A.ptr(r.indices), A.ptr(r.indptr), A.ptr(s0), A.ptr(c0), A.ptr(v0),
             A.ptr(a0), *(v for t in params for v in (A.ptr(t), 1 if t is None else t.numel())), A.ptr(s), A.ptr(v_seq), A.ptr(h),
             A.ptr(c_save), A.ptr(a_save), A.ptr(c_last), A.ptr(v_last), A.ptr(a_last), T, B, N, p.v_reset, p.reset, p.adaptive, e,
             A.stream_ptr())
    return s, v_seq, h, c_save, a_save, c_last, v_last, a_last


class RecurrentLifSequenceParams(torch.autograd.Function):
    """:class:`RecurrentLifSequence` with the five parameters as device tensors that may require grad.  Saved: ``h``, ``a_save``
    in ``th``'s place when adaptive, ``s``, the weights, ``s0``, the parameters, ``c_save`` only if ``syn_decay`` needs a gradient,
    and ``c0`` / ``v0`` only for the gradient of ``syn_decay`` / ``beta`` (what the first step started from).  A parameter that does
    not need a gradient has its ``[B, N]`` accumulator go in as NULL."""

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
        r, (T, B, N), p, return_v = ctx.meta
        g_vseq = rest[0] if return_v else None
        g_last = list(rest[1:] if return_v else rest) + [None] * (3 - p.entries)
        if g_s is None and g_vseq is None and all(g is None for g in g_last):
            return (None,) * 16
        h, a_save, s, w, s0, c_save, *params, c0, v0 = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = [need[1], need[2], bool(p.adaptive) and need[3], need[4]]
        need_p = [need[6 + k] and params[k] is not None for k in range(5)]
        g_s, g_vseq, g_last = _grad_in(g_s), _grad_in(g_vseq), [_grad_in(g) for g in g_last]
        g_x = torch.empty_like(h)
        g_state = [torch.empty((B, N), dtype=h.dtype, device=h.device) if k else None for k in want]
        if T == 0 or B * N == 0:              # no step: the state's gradient passes through, the parameters were not used
            for out, g in zip(g_state[:3], g_last):
                if out is not None:
                    out.zero_() if g is None else out.copy_(g)
            if g_state[3] is not None:
                g_state[3].zero_()
            g_params = [torch.zeros_like(t) if k else None for t, k in zip(params, need_p)]
        else:
            slot = [torch.empty((B, N), dtype=h.dtype, device=h.device) if k else None for k in need_p]
            call('be_lif_rec_sg_backward_params', A.ptr(h), A.ptr(c_save), A.ptr(a_save), A.ptr(c0), A.ptr(v0), A.ptr(r.w),
                 A.ptr(r.indices), A.ptr(r.indptr), A.ptr(g_s), A.ptr(g_vseq), A.ptr(g_last[0]), A.ptr(g_last[1]), A.ptr(g_last[2]),
                 *(v for t in params for v in (A.ptr(t), 1 if t is None else t.numel())), A.ptr(g_x), A.ptr(g_state[0]),
                 A.ptr(g_state[1]), A.ptr(g_state[2]), A.ptr(g_state[3]), *(A.ptr(t) for t in slot), T, B, N, p.v_reset, p.reset,
                 p.surrogate, p.alpha, p.adaptive, p.detach_reset, A.stream_ptr())
            g_params = [_reduce_slots(sl.reshape(-1), t) if k else None for sl, t, k in zip(slot, params, need_p)]
        g_w = _weight_grad(w, r, s, s0, g_x, T, B, N) if need[5] else None
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

    A :class:`DelayedCSR` is taken with all-number parameters only (that is :func:`recurrent_lif_sequence`); with a tensor parameter
    it raises ``NotImplementedError``.

    Not built: learnable ``v_reset`` / ``alpha``, ``[B, N]`` parameters, tensor parameters with synaptic delays, and what
    :func:`recurrent_lif_sequence` does not build."""
    who = 'parametric_recurrent_lif_sequence'
    given, stand_in, any_tensor = _split_params(who, syn_decay, beta, v_th, adapt)
    if not any_tensor:
        return recurrent_lif_sequence(x, rec, state0, s0, syn_decay=syn_decay, beta=beta, v_th=v_th, v_reset=v_reset, reset=reset,
                                      surrogate=surrogate, alpha=alpha, detach_reset=detach_reset, adapt=adapt, return_v=return_v,
                                      scale_exp=scale_exp)
    if _is_delayed(rec):
        raise NotImplementedError(f"{who}: learnable (tensor) neuron parameters together with synaptic delays are not built: a "
                                  f"DelayedCSR takes syn_decay, beta, v_th and adapt as Python numbers (recurrent_lif_sequence).")
    p = _Params(who, stand_in[0], stand_in[1], stand_in[2], v_reset, reset, surrogate, alpha, detach_reset,
                None if adapt is None else (stand_in[3], stand_in[4]), FIVE_TENSORS)
    (T, B, N), slots, x3, (c0, v0, a0, sp), e = _prepare(who, x, rec, state0, s0, p, scale_exp)
    params = _layer_params(who, given, x, N, p.adaptive)
    w = rec.data
    r = _Rec(w.detach(), rec.indices, rec.indptr)
    return_v = bool(return_v)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x3, c0, v0, a0, sp, w, *params)):
        outs = RecurrentLifSequenceParams.apply(x3, c0, v0, a0, sp, w, *params, r, (T, B, N), p, e, return_v)
    else:                                     # no backward pass: nothing is kept
        s, v_seq, _, _, _, c_last, v_last, a_last = _forward_params(x3, r, sp, c0, v0, a0, params, T, B, N, p, e, return_v, False,
                                                                    False)
        outs = tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)
    return _shaped(outs, x, slots, return_v)
