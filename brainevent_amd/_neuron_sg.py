"""The differentiable neuron between two products: a leaky integrate-and-fire step, and a whole input
sequence of them, as ONE launch forwards and one backwards (``be_lif_sg_forward`` / ``be_lif_sg_backward``,
``csrc/be_neuron_sg.hip``), under ``torch.autograd`` with a surrogate gradient for the spike.

    h = beta * v + x;   s = h >= v_th;   v' = v_reset if s else h   (reset='soft': h - v_th if s else h)

``s`` is an f32 0/1 tensor: ``BinaryArray(s) @ csr`` takes it as float spikes and hands back its straight-through gradient,
which the backward pass here multiplies by the surrogate's derivative at ``u = h - v_th`` (``fast_sigmoid``:
``1 / (1 + alpha |u|)^2``; ``atan``: ``(alpha / 2) / (1 + (pi / 2 alpha u)^2)``; ``triangle``: ``alpha max(0, 1 - alpha |u|)``).
The reset carries a gradient through the spike too unless ``detach_reset``.  Every operation of both passes is an individually
rounded f32 operation in the order the header states, so the results equal the elementwise formulation bit for bit.

``beta`` and ``v_th`` are Python numbers (one constant for the population: the entry points above) or f32 device tensors
(``be_lif_sg_forward_params`` / ``be_lif_sg_backward_params``, the same ``csrc/be_neuron_sg.hip``): one element for a
shared value, or the shape of the last dimensions of a step for a value per neuron, broadcast over the leading (batch)
dimensions.  The kernels read them from device memory — no value crosses to the host, so an optimiser's in-place update is seen
by the next call and by the next replay of a captured graph — and a tensor that requires grad gets its gradient: per-slot sums
over time from the backward launch, then a deterministic f64 reduction over the batch (``be_lif_sg_reduce_slots``).

Not here: learnable ``v_reset`` / ``alpha``, refractory periods and conductances (:func:`lif_coba_step`), f16 / bf16 state or
parameters, double backward, a bit-packed spike output (the differentiable path needs the float tensor).
"""
from typing import Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from . import _array as A
from ._lib import call, fn

__all__ = ['lif_step', 'lif_sequence', 'RESETS', 'SURROGATES']

#: ``reset=`` / ``surrogate=`` -> the header's BE_LIF_RESET_* / BE_LIF_SG_* codes
RESETS = {'hard': 0, 'soft': 1}
SURROGATES = {'fast_sigmoid': 0, 'atan': 1, 'triangle': 2}


class _Params:
    __slots__ = ('beta', 'v_th', 'v_reset', 'reset', 'surrogate', 'alpha', 'detach_reset')

    def __init__(self, who, beta, v_th, v_reset, reset, surrogate, alpha, detach_reset):
        if reset not in RESETS:
            raise ValueError(f"{who}: reset must be one of {sorted(RESETS)}, not {reset!r}.")
        if surrogate not in SURROGATES:
            raise ValueError(f"{who}: surrogate must be one of {sorted(SURROGATES)}, not {surrogate!r}.")
        if not float(alpha) > 0.0:
            raise ValueError(f"{who}: alpha must be positive, not {alpha!r}.")
        # a tensor stays on the device (no float(tensor): that would be a copy to the host and a sync); the params path has it
        self.beta = None if isinstance(beta, torch.Tensor) else float(beta)
        self.v_th = None if isinstance(v_th, torch.Tensor) else float(v_th)
        self.v_reset, self.alpha = float(v_reset), float(alpha)
        self.reset, self.surrogate, self.detach_reset = RESETS[reset], SURROGATES[surrogate], int(bool(detach_reset))


def _check_tensor(who, name, t) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor, not {type(t).__name__}.")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be float32, not {t.dtype} (f16 / bf16 state is not built).")


def _check_device(who, **tensors) -> None:
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise ValueError(f"{who}: {name} must be a device tensor (there is no CPU implementation).")


def _check_param(who, name, value, slots) -> None:
    """A tensor ``beta`` / ``v_th``: f32, on the device, one element (0-d or ``[1]``) or the last ``k >= 1`` dimensions of a step."""
    if not isinstance(value, torch.Tensor):
        return
    if value.dtype != torch.float32:
        raise TypeError(f"{who}: a tensor {name} must be float32, not {value.dtype}.")
    if not value.is_cuda:
        raise ValueError(f"{who}: a tensor {name} must be a device tensor (the kernels read it from device memory).")
    shape = tuple(value.shape)
    if shape in ((), (1,)):
        return
    if not (1 <= len(shape) <= len(slots) and shape == tuple(slots[len(slots) - len(shape):])):
        raise ValueError(f"{who}: {name} {shape} must have one element or the shape of the last dimensions of a step, "
                         f"{tuple(slots)}.")


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _forward(x, v0, T: int, slots: Tuple[int, ...], p: _Params, want_v: bool, want_h: bool):
    """``be_lif_sg_forward`` on contiguous ``x`` (``T`` rows of ``slots``) and ``v0`` (``slots`` or None): ``(s, v_seq, h,
    v_last)``; ``v_seq`` / ``h`` are None unless asked for, and are then neither allocated nor written."""
    s = torch.empty_like(x)
    v_seq = torch.empty_like(x) if want_v else None
    h = torch.empty_like(x) if want_h else None
    v_last = torch.empty(slots, dtype=x.dtype, device=x.device)
    if T == 0:                                # no step: the state passes through
        v_last.zero_() if v0 is None else v_last.copy_(v0)
    else:
        call('be_lif_sg_forward', A.ptr(x), A.ptr(v0), A.ptr(s), A.ptr(v_seq), A.ptr(h), A.ptr(v_last), T, _numel(slots), p.beta,
             p.v_th, p.v_reset, p.reset, A.stream_ptr())
    return s, v_seq, h, v_last


def _backward(h, g_s, g_vseq, g_vlast, T: int, slots: Tuple[int, ...], p: _Params, want_v0: bool):
    """``be_lif_sg_backward``: ``(g_x, g_v0)``.  A gradient that is None goes in as NULL; ``g_v0`` is None unless asked for."""
    g_x = torch.empty_like(h)
    g_v0 = torch.empty(slots, dtype=h.dtype, device=h.device) if want_v0 else None
    if T == 0:
        if want_v0:
            g_v0.zero_() if g_vlast is None else g_v0.copy_(g_vlast)
    else:
        call('be_lif_sg_backward', A.ptr(h), A.ptr(g_s), A.ptr(g_vseq), A.ptr(g_vlast), A.ptr(g_x), A.ptr(g_v0), T, _numel(slots),
             p.beta, p.v_th, p.v_reset, p.reset, p.surrogate, p.alpha, p.detach_reset, A.stream_ptr())
    return g_x, g_v0


def _grad_in(g) -> Optional[torch.Tensor]:
    return None if g is None else g.contiguous()


class LifSequence(torch.autograd.Function):
    """``T`` steps (``lif_step``: ``T = 1``).  Saved: ``h`` alone — the spike and the surrogate's argument are recomputed from
    it.  The gradient of an output nobody used arrives as None (``set_materialize_grads(False)``) and goes in as NULL."""

    @staticmethod
    def forward(ctx, x, v0, T: int, slots, p: _Params, return_v: bool):
        ctx.set_materialize_grads(False)
        s, v_seq, h, v_last = _forward(x, v0, T, slots, p, return_v, True)
        ctx.save_for_backward(h)
        ctx.meta = (T, slots, p, return_v)
        return (s, v_seq, v_last) if return_v else (s, v_last)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, *rest):
        T, slots, p, return_v = ctx.meta
        g_vseq, g_vlast = rest if return_v else (None, rest[0])
        if g_s is None and g_vseq is None and g_vlast is None:
            return None, None, None, None, None, None
        h, = ctx.saved_tensors
        g_x, g_v0 = _backward(h, _grad_in(g_s), _grad_in(g_vseq), _grad_in(g_vlast), T, slots, p,
                              want_v0=ctx.needs_input_grad[1])
        return (g_x if ctx.needs_input_grad[0] else None), g_v0, None, None, None, None


# ------------------------------------------------------------------------------------------------ beta, v_th on the device
def _forward_params(x, v0, beta, v_th, T: int, slots, p: _Params, want_v: bool, want_h: bool):
    """``be_lif_sg_forward_params``: :func:`_forward` with ``beta`` / ``v_th`` contiguous f32 device tensors (the period is the
    element count)."""
    s = torch.empty_like(x)
    v_seq = torch.empty_like(x) if want_v else None
    h = torch.empty_like(x) if want_h else None
    v_last = torch.empty(slots, dtype=x.dtype, device=x.device)
    n = _numel(slots)
    if T == 0:
        v_last.zero_() if v0 is None else v_last.copy_(v0)
    elif n > 0:
        call('be_lif_sg_forward_params', A.ptr(x), A.ptr(v0), A.ptr(beta), beta.numel(), A.ptr(v_th), v_th.numel(), A.ptr(s),
             A.ptr(v_seq), A.ptr(h), A.ptr(v_last), T, n, p.v_reset, p.reset, A.stream_ptr())
    return s, v_seq, h, v_last


def _reduce_slots(slot, like) -> torch.Tensor:
    """``be_lif_sg_reduce_slots``: the per-slot sums ``[N]`` -> the gradient of the parameter ``like`` (period = its element
    count), in its shape.  One slot per element: the slots are the gradient.  The workspace comes from torch's allocator, so the
    call can be captured."""
    n, period = slot.numel(), like.numel()
    if period == n:
        return slot.reshape(like.shape)
    out = torch.empty(like.shape, dtype=slot.dtype, device=slot.device)
    nbytes = fn('be_lif_sg_reduce_slots_workspace_bytes')(n, period)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=slot.device) if nbytes else None
    call('be_lif_sg_reduce_slots', A.ptr(slot), n, period, A.ptr(out), A.ptr(ws), nbytes, A.stream_ptr())
    return out


class LifSequenceParams(torch.autograd.Function):
    """:class:`LifSequence` with ``beta`` / ``v_th`` as device tensors that may require grad.  Saved: ``h``, the two parameters, and
    ``v0`` when ``beta`` needs a gradient (the membrane the first step started from).  A parameter that does not need a gradient
    has its per-slot output go in as NULL."""

    @staticmethod
    def forward(ctx, x, v0, beta, v_th, T: int, slots, p: _Params, return_v: bool):
        ctx.set_materialize_grads(False)
        s, v_seq, h, v_last = _forward_params(x, v0, beta, v_th, T, slots, p, return_v, True)
        ctx.save_for_backward(h, beta, v_th, v0 if ctx.needs_input_grad[2] else None)
        ctx.meta = (T, slots, p, return_v)
        return (s, v_seq, v_last) if return_v else (s, v_last)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, *rest):
        T, slots, p, return_v = ctx.meta
        g_vseq, g_vlast = rest if return_v else (None, rest[0])
        if g_s is None and g_vseq is None and g_vlast is None:
            return (None,) * 8
        h, beta, v_th, v0 = ctx.saved_tensors
        need_x, need_v0, need_b, need_t = ctx.needs_input_grad[:4]
        g_s, g_vseq, g_vlast = _grad_in(g_s), _grad_in(g_vseq), _grad_in(g_vlast)
        n = _numel(slots)
        g_x = torch.empty_like(h)
        g_v0 = torch.empty(slots, dtype=h.dtype, device=h.device) if need_v0 else None
        slot_b = torch.empty(n, dtype=h.dtype, device=h.device) if need_b else None
        slot_t = torch.empty(n, dtype=h.dtype, device=h.device) if need_t else None
        if T == 0:                            # no step: the state's gradient passes through, the parameters were not used
            if need_v0:
                g_v0.zero_() if g_vlast is None else g_v0.copy_(g_vlast)
            return (g_x if need_x else None), g_v0, (torch.zeros_like(beta) if need_b else None), (torch.zeros_like(v_th) if need_t else None), \
                None, None, None, None
        if n > 0:
            call('be_lif_sg_backward_params', A.ptr(h), A.ptr(v0), A.ptr(g_s), A.ptr(g_vseq), A.ptr(g_vlast), A.ptr(beta),
                 beta.numel(), A.ptr(v_th), v_th.numel(), A.ptr(g_x), A.ptr(g_v0), A.ptr(slot_b), A.ptr(slot_t), T, n, p.v_reset,
                 p.reset, p.surrogate, p.alpha, p.detach_reset, A.stream_ptr())
        g_beta = _reduce_slots(slot_b, beta) if need_b else None
        g_vth = _reduce_slots(slot_t, v_th) if need_t else None
        return (g_x if need_x else None), g_v0, g_beta, g_vth, None, None, None, None


def _as_param(value, like) -> torch.Tensor:
    """A number next to a tensor parameter: a one-element device tensor holding its f32 value."""
    if isinstance(value, torch.Tensor):
        return value.contiguous()
    return torch.full((1,), float(value), dtype=torch.float32, device=like.device)


def _run(x, v0, T: int, slots, p: _Params, return_v: bool, beta=None, v_th=None):
    x = x.contiguous()
    if v0 is not None:
        v0 = v0.contiguous()
    if isinstance(beta, torch.Tensor) or isinstance(v_th, torch.Tensor):
        beta, v_th = _as_param(beta, x), _as_param(v_th, x)
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, v0, beta, v_th)):
            return LifSequenceParams.apply(x, v0, beta, v_th, T, slots, p, return_v)
        s, v_seq, _, v_last = _forward_params(x, v0, beta, v_th, T, slots, p, return_v, False)
        return (s, v_seq, v_last) if return_v else (s, v_last)
    if torch.is_grad_enabled() and (x.requires_grad or (v0 is not None and v0.requires_grad)):
        return LifSequence.apply(x, v0, T, slots, p, return_v)
    s, v_seq, _, v_last = _forward(x, v0, T, slots, p, return_v, False)        # no backward pass: h is not kept
    return (s, v_seq, v_last) if return_v else (s, v_last)


def lif_step(v: torch.Tensor, x: torch.Tensor, *, beta: Union[float, torch.Tensor], v_th: Union[float, torch.Tensor] = 1.0,
             v_reset: float = 0.0, reset: str = 'hard', surrogate: str = 'fast_sigmoid', alpha: float = 10.0,
             detach_reset: bool = False):
    """One step of a leaky integrate-and-fire population: ``(s, v_new)`` from the membrane ``v`` and this step's input ``x`` (f32
    device tensors of one shape; a batch is more neurons).  ``h = beta * v + x``, ``s = h >= v_th`` as an f32 0/1 tensor,
    ``v_new = v_reset where s else h`` (``reset='soft'``: ``h - v_th where s``).  Differentiable in ``v`` and ``x`` through both
    outputs; the spike's derivative is ``surrogate`` (``'fast_sigmoid'``, ``'atan'``, ``'triangle'``) with sharpness ``alpha``, and
    ``detach_reset`` cuts the gradient the reset carries through the spike.  One launch forwards, one backwards; bit for bit the
    elementwise f32 formulation (``be_lif_sg_forward``).

    ``beta`` and ``v_th`` are each a Python number or an f32 device tensor: one element (0-d or ``[1]``) for a shared value, or the
    shape of the last ``k >= 1`` dimensions of ``x`` for a value per neuron, broadcast over the leading dimensions.  A tensor is
    read on the device (never copied to the host) and, if it requires grad, gets its gradient in its own shape: the sum over the
    slots that share an element, accumulated in f64 in a fixed order (``be_lif_sg_reduce_slots``)."""
    p = _Params('lif_step', beta, v_th, v_reset, reset, surrogate, alpha, detach_reset)
    _check_tensor('lif_step', 'v', v)
    _check_tensor('lif_step', 'x', x)
    if v.shape != x.shape:
        raise ValueError(f"lif_step: v {tuple(v.shape)} and x {tuple(x.shape)} must have one shape.")
    _check_device('lif_step', v=v, x=x)
    _check_param('lif_step', 'beta', beta, tuple(x.shape))
    _check_param('lif_step', 'v_th', v_th, tuple(x.shape))
    return _run(x, v, 1, tuple(x.shape), p, False, beta, v_th)


def lif_sequence(x: torch.Tensor, v0: Optional[torch.Tensor] = None, *, beta: Union[float, torch.Tensor],
                 v_th: Union[float, torch.Tensor] = 1.0, v_reset: float = 0.0, reset: str = 'hard', surrogate: str = 'fast_sigmoid',
                 alpha: float = 10.0, detach_reset: bool = False, return_v: bool = False):
    """:func:`lif_step` over a whole input sequence ``x [T, ...]`` in one launch, starting from ``v0 [...]`` (None: zeros):
    ``(s [T, ...], v_last [...])``, or ``(s, v_seq [T, ...], v_last)`` with ``return_v`` (the membrane after every step).  Equal,
    bit for bit and in every gradient, to ``T`` calls of :func:`lif_step`; differentiable in ``x`` and ``v0`` through every
    output.  ``beta`` / ``v_th`` as in :func:`lif_step` (a tensor: one element, or the last dimensions of a STEP of ``x``); a
    tensor's gradient is the sum over time and batch, which ``T`` calls of ``lif_step`` add up in another order."""
    p = _Params('lif_sequence', beta, v_th, v_reset, reset, surrogate, alpha, detach_reset)
    _check_tensor('lif_sequence', 'x', x)
    if x.ndim < 1:
        raise ValueError('lif_sequence: x must be [T, ...].')
    if v0 is not None:
        _check_tensor('lif_sequence', 'v0', v0)
        if v0.shape != x.shape[1:]:
            raise ValueError(f"lif_sequence: v0 {tuple(v0.shape)} must have the shape of a step of x, {tuple(x.shape[1:])}.")
    _check_device('lif_sequence', x=x, v0=v0)
    _check_param('lif_sequence', 'beta', beta, tuple(x.shape[1:]))
    _check_param('lif_sequence', 'v_th', v_th, tuple(x.shape[1:]))
    return _run(x, v0, int(x.shape[0]), tuple(x.shape[1:]), p, bool(return_v), beta, v_th)
