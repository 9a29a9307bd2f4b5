"""Shared by tests/test_lif_sg_cpu.py and tests/test_lif_sg_gpu.py: a numpy restatement of the two passes of the differentiable
LIF neuron (include/brainevent_amd.h, be_lif_sg_forward / be_lif_sg_backward; csrc/be_neuron_sg.hip), the CONSTS table the GPU
sizes are taken from (the CPU test holds it against the source text), and the case lists.

The restatement works on ``np.float32`` arrays with ``np.float32`` constants, one operation per statement in the header's order:
every one of them (add, subtract, multiply, divide, abs, compare, select) is correctly rounded in IEEE 754 binary32 on the host
and on the device, so the device results are compared with it as equalities.  NaN payloads are the one thing IEEE 754 leaves
open: :func:`same_bits` asks for a NaN where the reference has one and for equal bits everywhere else (signed zeros included)."""
import itertools
import math

import numpy as np

F = np.float32

#: the constants of csrc/be_neuron_sg.hip that the GPU sizes below are derived from
CONSTS = {'kSgThreads': 256, 'kSgGridCap': 2048, 'kSgVec': 4, 'kSgPrefetch': 4}
RESETS = ('hard', 'soft')
SURROGATES = ('fast_sigmoid', 'atan', 'triangle')
#: every reset x surrogate x detach_reset
MODES = list(itertools.product(RESETS, SURROGATES, (False, True)))
#: which output gradients a backward pass receives (the others go in as NULL)
GRAD_SETS = {'g_s': (True, False, False), 'g_vlast': (False, False, True), 'g_vseq': (False, True, False),
             'all': (True, True, True)}

#: one slot more than a full pass of the capped grid: of the 4-byte kernel, and (one lane more: N % 4 stays 0) of the 16-byte one
FULL_PASS_SCALAR = CONSTS['kSgThreads'] * CONSTS['kSgGridCap']
FULL_PASS_VECTOR = FULL_PASS_SCALAR * CONSTS['kSgVec']
N_SIZES = (1, 63, 64, 65)
N_PAST_ONE_PASS = (FULL_PASS_SCALAR + 1, FULL_PASS_VECTOR + CONSTS['kSgVec'])
T_SIZES = (1, 2, 25, CONSTS['kSgPrefetch'] - 1, CONSTS['kSgPrefetch'], CONSTS['kSgPrefetch'] + 1)
SHAPES = ((65,), (3, 65), (2, 3, 5))


class Params:
    """The scalar arguments of a call; the f32 constants are rounded once from doubles, as the host side of the library does."""

    def __init__(self, beta=0.9, v_th=1.0, v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=10.0, detach_reset=False):
        self.beta, self.v_th, self.v_reset, self.alpha = float(beta), float(v_th), float(v_reset), float(alpha)
        self.reset, self.surrogate, self.detach_reset = reset, surrogate, bool(detach_reset)

    def kwargs(self):
        return dict(beta=self.beta, v_th=self.v_th, v_reset=self.v_reset, reset=self.reset, surrogate=self.surrogate,
                    alpha=self.alpha, detach_reset=self.detach_reset)

    def __repr__(self):
        return f'Params({self.kwargs()})'


def forward(x, v0, p):
    """``x [T, N]``, ``v0 [N]`` or None -> ``(s_out, v_seq, h_save, v_last)``."""
    assert x.dtype == F and x.ndim == 2 and (v0 is None or (v0.dtype == F and v0.shape == x.shape[1:]))
    beta, v_th, v_reset = F(p.beta), F(p.v_th), F(p.v_reset)
    T, N = x.shape
    v = np.zeros(N, F) if v0 is None else v0.copy()
    s_out, v_seq, h_save = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    with np.errstate(all='ignore'):
        for t in range(T):
            bv = beta * v
            h = bv + x[t]
            s = h >= v_th
            if p.reset == 'hard':
                v = np.where(s, v_reset, h).astype(F)
            else:
                hm = h - v_th
                v = np.where(s, hm, h).astype(F)
            s_out[t] = np.where(s, F(1), F(0))
            v_seq[t] = v
            h_save[t] = h
            assert bv.dtype == h.dtype == v.dtype == F
    return s_out, v_seq, h_save, v


def surrogate(u, p):
    """The surrogate's derivative at ``u`` (f32 array)."""
    alpha = F(p.alpha)
    one = F(1)
    with np.errstate(all='ignore'):
        if p.surrogate == 'fast_sigmoid':
            a = np.abs(u)
            m = alpha * a
            d = one + m
            dd = d * d
            sg = one / dd
        elif p.surrogate == 'atan':
            c = F(math.pi / 2 * p.alpha)
            half = F(p.alpha / 2)
            q = c * u
            qq = q * q
            den = one + qq
            sg = half / den
        else:
            a = np.abs(u)
            m = alpha * a
            r = one - m
            r = np.where(r > F(0), r, F(0)).astype(F)        # a NaN compares false: 0
            sg = alpha * r
    assert sg.dtype == F
    return sg


def backward(h_save, g_s, g_vseq, g_vlast, p, with_bound=False):
    """``h_save [T, N]``; ``g_s`` / ``g_vseq [T, N]`` and ``g_vlast [N]`` or None -> ``(g_x, g_v0)``.

    ``with_bound``: also the per-element bound ``[T, N]`` (f64) within which another evaluation order of the same derivative may
    differ from ``g_x``, and the one of ``g_v0``: per step ``4 * 2**-24 * (sum of the absolute values of the terms g_h is the sum
    of)`` — the terms as the plain formula's autograd forms them: ``g_s * sg``, the reset's ``g_vo * h * sg`` and
    ``g_vo * v_reset * sg`` (soft: ``g_vo * v_th * sg``) and the pass-through ``g_vo`` — plus what the difference already carried
    by ``g_vo`` becomes at this step (times ``|d g_h / d g_vo|``), and ``beta`` times the sum is carried on."""
    assert h_save.dtype == F and h_save.ndim == 2
    beta, v_th, v_reset = F(p.beta), F(p.v_th), F(p.v_reset)
    T, N = h_save.shape
    hard = p.reset == 'hard'
    carry = np.zeros(N, F) if g_vlast is None else g_vlast.copy()
    g_x = np.empty_like(h_save)
    bound = np.zeros((T, N), np.float64)
    carried = np.zeros(N, np.float64)
    eps4 = 4.0 * 2.0 ** -24
    with np.errstate(all='ignore'):
        for t in range(T - 1, -1, -1):
            h = h_save[t]
            u = h - v_th
            s = h >= v_th
            g_vo = carry
            if g_vseq is not None:
                g_vo = carry + g_vseq[t]
            sg = surrogate(u, p)
            g_sp = np.zeros(N, F) if g_s is None else g_s[t]
            if not p.detach_reset:
                if hard:
                    r = v_reset - h
                    gr = g_vo * r
                    g_sp = g_sp + gr
                else:
                    gr = g_vo * v_th
                    g_sp = g_sp - gr
            through = np.where(s, F(0), g_vo).astype(F) if hard else g_vo
            gs = g_sp * sg
            g_h = gs + through
            g_x[t] = g_h
            carry = beta * g_h
            assert g_vo.dtype == g_sp.dtype == g_h.dtype == carry.dtype == F
            if with_bound:
                a = lambda z: np.abs(np.asarray(z, np.float64))
                terms = a(0 if g_s is None else g_s[t]) * a(sg) + a(through)
                coef = np.where(s, 0.0, 1.0) if hard else np.ones(N)
                if not p.detach_reset:
                    if hard:
                        terms = terms + (a(g_vo) * a(h) + a(g_vo) * a(v_reset)) * a(sg)
                        coef = coef + (a(h) + a(v_reset)) * a(sg)
                    else:
                        terms = terms + a(g_vo) * a(v_th) * a(sg)
                        coef = coef + a(v_th) * a(sg)
                bound[t] = eps4 * terms + carried * coef
                carried = a(beta) * bound[t]
    if with_bound:
        return g_x, carry, bound, carried
    return g_x, carry


def same_bits(got, ref):
    """Equal as bit patterns, except that any NaN stands for any NaN."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.dtype != F or ref.dtype != F or got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return bool(np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]))


def inputs(T, N, seed, p=None):
    """Seeded ``x [T, N]``, ``v0 [N]`` and the three output gradients: a drive that makes roughly a third of the steps spike at the
    default parameters, membranes on both sides of the threshold, a few values exactly on it."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(0.45, 0.6, (T, N))).astype(F)
    v0 = rng.normal(0.3, 0.5, N).astype(F)
    x[rng.random((T, N)) < 0.02] = F(1.0)                                  # with v = 0 after a reset: h == v_th exactly
    g_s = rng.normal(0, 1, (T, N)).astype(F)
    g_vseq = rng.normal(0, 1, (T, N)).astype(F)
    g_vlast = rng.normal(0, 1, N).astype(F)
    return x, v0, g_s, g_vseq, g_vlast
