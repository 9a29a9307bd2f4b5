"""The differentiable neuron with a synaptic current and an optional adaptive threshold: a current-based leaky
integrate-and-fire step, and a whole input sequence of them, as ONE launch forwards and one backwards (``be_lif_syn_sg_forward`` /
``be_lif_syn_sg_backward``, ``csrc/be_neuron_sg.hip``), under ``torch.autograd`` with a surrogate gradient for the spike.

    c' = syn_decay * c + x;   h = beta * v + c';   th = v_th + kappa * a  (no adaptation: v_th);   s = h >= th
    v' = v_reset if s else h   (reset='soft': h - v_th if s else h — the BASE threshold);   a' = rho * a + s

The state is the tuple ``(c, v)``, or ``(c, v, a)`` with ``adapt=(rho, kappa)`` (ALIF / LSNN: the trace ``a`` of the neuron's own
spikes raises its threshold and feeds back through the spike in the backward pass).  ``s`` is an f32 0/1 tensor, as
:func:`~brainevent_amd.lif_step`'s; the surrogates, ``alpha`` and ``detach_reset`` are the same (``detach_reset`` cuts the reset's
path through the spike only, never the adaptation's).  Every operation of both passes is an individually rounded f32 operation
in the order the header states, so the results equal the elementwise formulation bit for bit.

A non-spiking leaky-integrator readout is ``v_th=float('inf')`` (with the hard reset): ``s`` is all zero, ``v_seq`` is the input
filtered twice (by ``syn_decay``, then by ``beta``), and every surrogate is 0 at ``u = -inf``, so the gradients stay finite.

``synaptic_lif_step`` / ``synaptic_lif_sequence`` take Python numbers.  :func:`parametric_synaptic_lif_step` /
:func:`parametric_synaptic_lif_sequence` (``be_lif_syn_sg_forward_params`` / ``be_lif_syn_sg_backward_params``, the same
kernels) take each of ``syn_decay``, ``beta``, ``v_th``, ``rho`` and ``kappa`` as a number or an f32 device tensor — one element, or the
last dimensions of a step for a value per neuron — read on the device and, where it requires grad, differentiated: per-slot sums
over time from the backward launch, then ``be_lif_sg_reduce_slots`` over the batch, as :func:`~brainevent_amd.lif_step` does.

Not here: learnable ``v_reset`` / ``alpha``, refractory periods and conductances, f16 / bf16, double backward, a bit-packed spike
output.
"""
import numbers
from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _array as A
from ._lib import call
from ._neuron_sg import (RESETS, SURROGATES, _as_param, _check_device, _check_param, _check_tensor, _grad_in, _numel,
                         _reduce_slots)

__all__ = ['synaptic_lif_step', 'synaptic_lif_sequence', 'parametric_synaptic_lif_step', 'parametric_synaptic_lif_sequence']


#: what a tensor in a number's place is told: by default, by the two float functions here, and by the parametric ones
NO_TENSORS = 'learnable parameters exist for lif_step only'
SEE_PARAMETRIC = NO_TENSORS + '; for this neuron: parametric_synaptic_lif_step / parametric_synaptic_lif_sequence'
FIVE_TENSORS = 'syn_decay, beta, v_th, rho and kappa may be tensors'


def _number(who, name, value, hint=NO_TENSORS) -> float:
    if isinstance(value, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a Python number, not a tensor ({hint}).")
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise TypeError(f"{who}: {name} must be a Python number, not {type(value).__name__}.")
    return float(value)


class _Params:
    __slots__ = ('syn_decay', 'beta', 'v_th', 'v_reset', 'rho', 'kappa', 'adaptive', 'reset', 'surrogate', 'alpha', 'detach_reset')

    def __init__(self, who, syn_decay, beta, v_th, v_reset, reset, surrogate, alpha, detach_reset, adapt, hint=NO_TENSORS):
        if reset not in RESETS:
            raise ValueError(f"{who}: reset must be one of {sorted(RESETS)}, not {reset!r}.")
        if surrogate not in SURROGATES:
            raise ValueError(f"{who}: surrogate must be one of {sorted(SURROGATES)}, not {surrogate!r}.")
        self.syn_decay, self.beta = _number(who, 'syn_decay', syn_decay, hint), _number(who, 'beta', beta, hint)
        self.v_th, self.v_reset = _number(who, 'v_th', v_th, hint), _number(who, 'v_reset', v_reset, hint)
        self.alpha = _number(who, 'alpha', alpha, hint)
        if not self.alpha > 0.0:
            raise ValueError(f"{who}: alpha must be positive, not {alpha!r}.")
        self.rho = self.kappa = 0.0
        self.adaptive = int(adapt is not None)
        if adapt is not None:
            if not isinstance(adapt, (tuple, list)):
                raise TypeError(f"{who}: adapt must be None or a pair of numbers (rho, kappa), not {type(adapt).__name__}.")
            if len(adapt) != 2:
                raise ValueError(f"{who}: adapt must be a pair (rho, kappa), not {len(adapt)} values.")
            self.rho, self.kappa = _number(who, 'adapt[0] (rho)', adapt[0], hint), _number(who, 'adapt[1] (kappa)', adapt[1], hint)
        self.reset, self.surrogate, self.detach_reset = RESETS[reset], SURROGATES[surrogate], int(bool(detach_reset))

    @property
    def entries(self) -> int:
        return 3 if self.adaptive else 2


def _forward(x, c0, v0, a0, T: int, slots: Tuple[int, ...], p: _Params, want_v: bool, want_h: bool):
    """``be_lif_syn_sg_forward`` on contiguous ``x`` (``T`` rows of ``slots``) and a state whose entries are ``slots`` or None:
    ``(s, v_seq, h, th, c_last, v_last, a_last)``; what was not asked for (and, without adaptation, ``th`` / ``a_last``) is None
    and neither allocated nor written."""
    new = lambda: torch.empty(slots, dtype=x.dtype, device=x.device)
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
        call('be_lif_syn_sg_forward', A.ptr(x), A.ptr(c0), A.ptr(v0), A.ptr(a0), A.ptr(s), A.ptr(v_seq), A.ptr(h), A.ptr(th),
             A.ptr(c_last), A.ptr(v_last), A.ptr(a_last), T, _numel(slots), p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa,
             p.reset, p.adaptive, A.stream_ptr())
    return s, v_seq, h, th, c_last, v_last, a_last


def _backward(h, th, g_s, g_vseq, g_last, T: int, slots: Tuple[int, ...], p: _Params, want):
    """``be_lif_syn_sg_backward``: ``(g_x, g_c0, g_v0, g_a0)``.  A gradient that is None goes in as NULL; a state gradient is None
    unless ``want`` asks for it."""
    g_x = torch.empty_like(h)
    g_state = [torch.empty(slots, dtype=h.dtype, device=h.device) if w else None for w in want]
    if T == 0:
        for out, g in zip(g_state, g_last):
            if out is not None:
                out.zero_() if g is None else out.copy_(g)
    else:
        call('be_lif_syn_sg_backward', A.ptr(h), A.ptr(th), A.ptr(g_s), A.ptr(g_vseq), A.ptr(g_last[0]), A.ptr(g_last[1]),
             A.ptr(g_last[2]), A.ptr(g_x), A.ptr(g_state[0]), A.ptr(g_state[1]), A.ptr(g_state[2]), T, _numel(slots), p.syn_decay,
             p.beta, p.v_th, p.v_reset, p.rho, p.kappa, p.reset, p.surrogate, p.alpha, p.adaptive, p.detach_reset, A.stream_ptr())
    return (g_x,) + tuple(g_state)


class SynapticLifSequence(torch.autograd.Function):
    """``T`` steps (``synaptic_lif_step``: ``T = 1``).  Outputs ``s, [v_seq,] c_last, v_last [, a_last]``.  Saved: ``h``, and ``th``
    when adaptive — the spike and the surrogate's argument are recomputed from them.  The gradient of an output nobody used
    arrives as None (``set_materialize_grads(False)``) and goes in as NULL."""

    @staticmethod
    def forward(ctx, x, c0, v0, a0, T: int, slots, p: _Params, return_v: bool):
        ctx.set_materialize_grads(False)
        s, v_seq, h, th, c_last, v_last, a_last = _forward(x, c0, v0, a0, T, slots, p, return_v, True)
        ctx.save_for_backward(h, th)
        ctx.meta = (T, slots, p, return_v)
        return tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, *rest):
        T, slots, p, return_v = ctx.meta
        g_vseq = rest[0] if return_v else None
        g_last = list(rest[1:] if return_v else rest) + [None] * (3 - p.entries)
        if g_s is None and g_vseq is None and all(g is None for g in g_last):
            return (None,) * 8
        h, th = ctx.saved_tensors
        want = [ctx.needs_input_grad[1], ctx.needs_input_grad[2], bool(p.adaptive) and ctx.needs_input_grad[3]]
        g_x, g_c0, g_v0, g_a0 = _backward(h, th, _grad_in(g_s), _grad_in(g_vseq), [_grad_in(g) for g in g_last], T, slots, p, want)
        return (g_x if ctx.needs_input_grad[0] else None), g_c0, g_v0, g_a0, None, None, None, None


def _run(x, state, T: int, slots, p: _Params, return_v: bool):
    """``state``: three entries (tensor or None; the third is None without adaptation).  ``(s, [v_seq,] state_last)``."""
    x = x.contiguous()
    c0, v0, a0 = (None if t is None else t.contiguous() for t in state)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, c0, v0, a0)):
        outs = SynapticLifSequence.apply(x, c0, v0, a0, T, slots, p, return_v)
    else:                                     # no backward pass: h / th are not kept
        s, v_seq, _, _, c_last, v_last, a_last = _forward(x, c0, v0, a0, T, slots, p, return_v, False)
        outs = tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)
    k = 2 if return_v else 1
    return outs[:k] + (tuple(outs[k:]),)


def _check_state(who, name, state, p: _Params, shape, allow_none: bool):
    if state is None and allow_none:
        return (None, None, None)
    if not isinstance(state, (tuple, list)):
        raise TypeError(f"{who}: {name} must be a tuple of {p.entries} tensors, not {type(state).__name__}.")
    if len(state) != p.entries:
        raise ValueError(f"{who}: {name} has {len(state)} entries; " +
                         ("adapt=(rho, kappa) takes (c, v, a)." if p.adaptive else "without adapt it is (c, v)."))
    for label, t in zip('cva', state):
        if t is None and allow_none:
            continue
        _check_tensor(who, f'{name} entry {label}', t)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}: {name} entry {label} {tuple(t.shape)} must have the shape of a step of x, {tuple(shape)}.")
    return tuple(state) + (None,) * (3 - len(state))


def synaptic_lif_step(state: Sequence[torch.Tensor], x: torch.Tensor, *, syn_decay: float, beta: float, v_th: float = 1.0,
                      v_reset: float = 0.0, reset: str = 'hard', surrogate: str = 'fast_sigmoid', alpha: float = 10.0,
                      detach_reset: bool = False, adapt: Optional[Tuple[float, float]] = None):
    """One step of a current-based leaky integrate-and-fire population: ``(s, new_state)`` from ``state = (c, v)`` — the synaptic
    current and the membrane — and this step's input ``x`` (f32 device tensors of one shape; a batch is more neurons).
    ``c' = syn_decay * c + x``, ``h = beta * v + c'``, ``s = h >= th`` as an f32 0/1 tensor, ``v' = v_reset where s else h``
    (``reset='soft'``: ``h - v_th where s``).  With ``adapt=(rho, kappa)`` the state is ``(c, v, a)``: the threshold is
    ``th = v_th + kappa * a`` and the trace follows the spikes, ``a' = rho * a + s``; without it ``th = v_th``.

    Differentiable in ``x`` and every state entry through ``s`` and every entry of ``new_state``; the spike's derivative is
    ``surrogate`` (``'fast_sigmoid'``, ``'atan'``, ``'triangle'``) with sharpness ``alpha`` at ``u = h - th``, and ``detach_reset``
    cuts the gradient the reset carries through the spike (the adaptation's stays).  All parameters are Python numbers.  One launch
    forwards, one backwards; bit for bit the elementwise f32 formulation (``be_lif_syn_sg_forward``)."""
    who = 'synaptic_lif_step'
    p = _Params(who, syn_decay, beta, v_th, v_reset, reset, surrogate, alpha, detach_reset, adapt, SEE_PARAMETRIC)
    _check_tensor(who, 'x', x)
    state = _check_state(who, 'state', state, p, x.shape, allow_none=False)
    _check_device(who, x=x, **{f'state entry {k}': t for k, t in zip('cva', state)})
    s, new_state = _run(x, state, 1, tuple(x.shape), p, False)
    return s, new_state


def synaptic_lif_sequence(x: torch.Tensor, state0: Optional[Sequence[Optional[torch.Tensor]]] = None, *, syn_decay: float,
                          beta: float, v_th: float = 1.0, v_reset: float = 0.0, reset: str = 'hard',
                          surrogate: str = 'fast_sigmoid', alpha: float = 10.0, detach_reset: bool = False,
                          adapt: Optional[Tuple[float, float]] = None, return_v: bool = False):
    """:func:`synaptic_lif_step` over a whole input sequence ``x [T, ...]`` in one launch, starting from ``state0`` (None, or a
    None entry of the tuple: zeros): ``(s [T, ...], state_last)``, or ``(s, v_seq [T, ...], state_last)`` with ``return_v`` (the
    membrane after every step).  ``state_last`` is ``(c, v)``, or ``(c, v, a)`` with ``adapt``.  Equal, bit for bit and in every
    gradient, to ``T`` calls of :func:`synaptic_lif_step`; differentiable in ``x`` and every given state entry through every
    output.

    A leaky-integrator readout that never spikes: ``v_th=float('inf')`` with the hard reset — ``s`` is all zero, ``v_seq`` is the
    filtered membrane, and every surrogate is 0 at ``u = -inf``, so the gradients through ``v_seq`` stay finite::

        _, v_seq, _ = be.synaptic_lif_sequence(x, syn_decay=0.8, beta=0.9, v_th=float('inf'), return_v=True)
    """
    who = 'synaptic_lif_sequence'
    p = _Params(who, syn_decay, beta, v_th, v_reset, reset, surrogate, alpha, detach_reset, adapt, SEE_PARAMETRIC)
    _check_tensor(who, 'x', x)
    if x.ndim < 1:
        raise ValueError(f'{who}: x must be [T, ...].')
    state = _check_state(who, 'state0', state0, p, x.shape[1:], allow_none=True)
    _check_device(who, x=x, **{f'state0 entry {k}': t for k, t in zip('cva', state)})
    return _run(x, state, int(x.shape[0]), tuple(x.shape[1:]), p, bool(return_v))


# ------------------------------------------------------------------------------------------------ the five parameters on the device
#: the parameters a tensor may stand for, in the order of the entry points' arguments
PARAM_NAMES = ('syn_decay', 'beta', 'v_th', 'rho', 'kappa')


def _forward_params(x, c0, v0, a0, params, T: int, slots, p: _Params, want_v: bool, want_h: bool, want_c: bool):
    """``be_lif_syn_sg_forward_params``: :func:`_forward` with the five parameters contiguous f32 device tensors (``rho`` / ``kappa``
    None without adaptation; a period is the element count): ``(s, v_seq, h, c_save, a_save, c_last, v_last, a_last)``.  ``a_save`` —
    the trace every step started from — is kept beside ``h`` when adaptive, ``c_save`` only when asked for."""
    new = lambda: torch.empty(slots, dtype=x.dtype, device=x.device)
    s = torch.empty_like(x)
    v_seq = torch.empty_like(x) if want_v else None
    h = torch.empty_like(x) if want_h else None
    c_save = torch.empty_like(x) if want_c else None
    a_save = torch.empty_like(x) if want_h and p.adaptive else None
    c_last, v_last, a_last = new(), new(), (new() if p.adaptive else None)
    n = _numel(slots)
    if T == 0:
        for out, start in ((c_last, c0), (v_last, v0), (a_last, a0)):
            if out is not None:
                out.zero_() if start is None else out.copy_(start)
    elif n > 0:
        call('be_lif_syn_sg_forward_params', A.ptr(x), A.ptr(c0), A.ptr(v0), A.ptr(a0),
             *(v for t in params for v in (A.ptr(t), 1 if t is None else t.numel())), A.ptr(s), A.ptr(v_seq), A.ptr(h),
             A.ptr(c_save), A.ptr(a_save),
             A.ptr(c_last), A.ptr(v_last), A.ptr(a_last), T, n, p.v_reset, p.reset, p.adaptive, A.stream_ptr())
    return s, v_seq, h, c_save, a_save, c_last, v_last, a_last


class SynapticLifSequenceParams(torch.autograd.Function):
    """:class:`SynapticLifSequence` with the five parameters as device tensors that may require grad.  Saved: ``h``, ``a_save`` when
    adaptive, ``c_save`` only if ``syn_decay`` needs a gradient, the parameters, and ``c0`` / ``v0`` only for the gradient of
    ``syn_decay`` / ``beta`` (what the first step started from).  A parameter that does not need a gradient has its per-slot output
    go in as NULL."""

    @staticmethod
    def forward(ctx, x, c0, v0, a0, syn_decay, beta, v_th, rho, kappa, T: int, slots, p: _Params, return_v: bool):
        ctx.set_materialize_grads(False)
        params = (syn_decay, beta, v_th, rho, kappa)
        need_sd, need_b = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        s, v_seq, h, c_save, a_save, c_last, v_last, a_last = _forward_params(x, c0, v0, a0, params, T, slots, p, return_v, True, need_sd)
        ctx.save_for_backward(h, c_save, a_save, *params, c0 if need_sd else None, v0 if need_b else None)
        ctx.meta = (T, slots, p, return_v)
        return tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, *rest):
        T, slots, p, return_v = ctx.meta
        g_vseq = rest[0] if return_v else None
        g_last = list(rest[1:] if return_v else rest) + [None] * (3 - p.entries)
        if g_s is None and g_vseq is None and all(g is None for g in g_last):
            return (None,) * 13
        h, c_save, a_save, *params, c0, v0 = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = [need[1], need[2], bool(p.adaptive) and need[3]]
        need_p = [need[4 + k] and params[k] is not None for k in range(5)]
        g_s, g_vseq, g_last = _grad_in(g_s), _grad_in(g_vseq), [_grad_in(g) for g in g_last]
        n = _numel(slots)
        g_x = torch.empty_like(h)
        g_state = [torch.empty(slots, dtype=h.dtype, device=h.device) if w else None for w in want]
        if T == 0 or n == 0:                  # no step: the state's gradient passes through, the parameters were not used
            for out, g in zip(g_state, g_last):
                if out is not None:
                    out.zero_() if g is None else out.copy_(g)
            g_params = [torch.zeros_like(t) if w else None for t, w in zip(params, need_p)]
            return ((g_x if need[0] else None), *g_state, *g_params, None, None, None, None)
        slot = [torch.empty(n, dtype=h.dtype, device=h.device) if w else None for w in need_p]
        call('be_lif_syn_sg_backward_params', A.ptr(h), A.ptr(c_save), A.ptr(a_save), A.ptr(c0), A.ptr(v0), A.ptr(g_s), A.ptr(g_vseq),
             A.ptr(g_last[0]), A.ptr(g_last[1]), A.ptr(g_last[2]),
             *(v for t in params for v in (A.ptr(t), 1 if t is None else t.numel())), A.ptr(g_x), A.ptr(g_state[0]),
             A.ptr(g_state[1]), A.ptr(g_state[2]), *(A.ptr(t) for t in slot), T, n, p.v_reset, p.reset, p.surrogate, p.alpha,
             p.adaptive, p.detach_reset, A.stream_ptr())
        g_params = [_reduce_slots(sl, t) if w else None for sl, t, w in zip(slot, params, need_p)]
        return ((g_x if need[0] else None), *g_state, *g_params, None, None, None, None)


def _run_params(x, state, params, T: int, slots, p: _Params, return_v: bool):
    x = x.contiguous()
    c0, v0, a0 = (None if t is None else t.contiguous() for t in state)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, c0, v0, a0, *params)):
        outs = SynapticLifSequenceParams.apply(x, c0, v0, a0, *params, T, slots, p, return_v)
    else:                                     # no backward pass: nothing is kept
        s, v_seq, _, _, _, c_last, v_last, a_last = _forward_params(x, c0, v0, a0, params, T, slots, p, return_v, False, False)
        outs = tuple(o for o in (s, v_seq, c_last, v_last, a_last) if o is not None)
    k = 2 if return_v else 1
    return outs[:k] + (tuple(outs[k:]),)


def _split_params(who, syn_decay, beta, v_th, adapt):
    """The five parameters as given (``rho`` / ``kappa`` None without ``adapt``), the stand-ins :class:`_Params` checks in their
    place — a tensor's is 0.0: the kernels read the tensor — and whether any is a tensor."""
    rho = kappa = None
    if adapt is not None:
        if not isinstance(adapt, (tuple, list)):
            raise TypeError(f"{who}: adapt must be None or a pair (rho, kappa), not {type(adapt).__name__}.")
        if len(adapt) != 2:
            raise ValueError(f"{who}: adapt must be a pair (rho, kappa), not {len(adapt)} values.")
        rho, kappa = adapt
    given = (syn_decay, beta, v_th, rho, kappa)
    stand_in = [0.0 if isinstance(v, torch.Tensor) else v for v in given]
    return given, stand_in, any(isinstance(v, torch.Tensor) for v in given)


def _device_params(who, given, like, slots, adaptive):
    labels = ('syn_decay', 'beta', 'v_th', 'adapt[0] (rho)', 'adapt[1] (kappa)')
    for label, v in zip(labels, given):
        _check_param(who, label, v, slots)
    return tuple(_as_param(v, like) if k < 3 or adaptive else None for k, v in enumerate(given))


def parametric_synaptic_lif_step(state: Sequence[torch.Tensor], x: torch.Tensor, *, syn_decay, beta, v_th=1.0, v_reset: float = 0.0,
                                 reset: str = 'hard', surrogate: str = 'fast_sigmoid', alpha: float = 10.0,
                                 detach_reset: bool = False, adapt=None):
    """:func:`synaptic_lif_step` with each of ``syn_decay``, ``beta``, ``v_th`` and the two entries of ``adapt = (rho, kappa)``
    independently a Python number or an f32 device tensor: one element (0-d or ``[1]``) for a shared value, or the shape of the last
    ``k >= 1`` dimensions of ``x`` for a value per neuron, broadcast over the leading dimensions.  A tensor is read on the device
    (never copied to the host: an optimiser's in-place update is seen by the next call and the next replay of a captured graph)
    and, if it requires grad, gets its gradient in its own shape — the sum over the slots that share an element, accumulated in
    f64 in a fixed order (``be_lif_sg_reduce_slots``).  A number beside a tensor becomes a one-element device tensor; all numbers
    is :func:`synaptic_lif_step` itself.  ``v_reset`` and ``alpha`` stay numbers.  Same state handling, outputs and bit-for-bit
    contract (``be_lif_syn_sg_forward_params``)."""
    who = 'parametric_synaptic_lif_step'
    given, stand_in, any_tensor = _split_params(who, syn_decay, beta, v_th, adapt)
    if not any_tensor:
        return synaptic_lif_step(state, x, syn_decay=syn_decay, beta=beta, v_th=v_th, v_reset=v_reset, reset=reset,
                                 surrogate=surrogate, alpha=alpha, detach_reset=detach_reset, adapt=adapt)
    p = _Params(who, stand_in[0], stand_in[1], stand_in[2], v_reset, reset, surrogate, alpha, detach_reset,
                None if adapt is None else (stand_in[3], stand_in[4]), FIVE_TENSORS)
    _check_tensor(who, 'x', x)
    state = _check_state(who, 'state', state, p, x.shape, allow_none=False)
    _check_device(who, x=x, **{f'state entry {k}': t for k, t in zip('cva', state)})
    params = _device_params(who, given, x, tuple(x.shape), p.adaptive)
    s, new_state = _run_params(x, state, params, 1, tuple(x.shape), p, False)
    return s, new_state


def parametric_synaptic_lif_sequence(x: torch.Tensor, state0: Optional[Sequence[Optional[torch.Tensor]]] = None, *, syn_decay, beta,
                                     v_th=1.0, v_reset: float = 0.0, reset: str = 'hard', surrogate: str = 'fast_sigmoid',
                                     alpha: float = 10.0, detach_reset: bool = False, adapt=None, return_v: bool = False):
    """:func:`parametric_synaptic_lif_step` over a whole input sequence ``x [T, ...]`` in one launch: :func:`synaptic_lif_sequence`
    with the five parameters as in the step (a tensor: one element, or the last dimensions of a STEP of ``x``).  Outputs and state
    gradients equal ``T`` calls of the step bit for bit; a parameter's gradient is the sum over time and batch, which ``T`` calls
    add up in another order."""
    who = 'parametric_synaptic_lif_sequence'
    given, stand_in, any_tensor = _split_params(who, syn_decay, beta, v_th, adapt)
    if not any_tensor:
        return synaptic_lif_sequence(x, state0, syn_decay=syn_decay, beta=beta, v_th=v_th, v_reset=v_reset, reset=reset,
                                     surrogate=surrogate, alpha=alpha, detach_reset=detach_reset, adapt=adapt, return_v=return_v)
    p = _Params(who, stand_in[0], stand_in[1], stand_in[2], v_reset, reset, surrogate, alpha, detach_reset,
                None if adapt is None else (stand_in[3], stand_in[4]), FIVE_TENSORS)
    _check_tensor(who, 'x', x)
    if x.ndim < 1:
        raise ValueError(f'{who}: x must be [T, ...].')
    state = _check_state(who, 'state0', state0, p, x.shape[1:], allow_none=True)
    _check_device(who, x=x, **{f'state0 entry {k}': t for k, t in zip('cva', state)})
    params = _device_params(who, given, x, tuple(x.shape[1:]), p.adaptive)
    return _run_params(x, state, params, int(x.shape[0]), tuple(x.shape[1:]), p, bool(return_v))
