"""Shared by tests/test_lif_syn_sg_cpu.py and tests/test_lif_syn_sg_gpu.py: a numpy restatement of the two passes of the
differentiable LIF neuron with a synaptic current and an optional adaptive threshold (include/brainevent_amd.h,
be_lif_syn_sg_forward / be_lif_syn_sg_backward; csrc/be_neuron_sg.hip), the CONSTS table the GPU sizes are taken from (the CPU
test holds it against the source text), seeded inputs, the crafted on-threshold cases and the mode list.

As tests/lif_sg_cases.py: ``np.float32`` arrays and constants, one operation per statement in the header's order, each of them
correctly rounded in IEEE 754 binary32 on the host and on the device, so the device results are compared as equalities
(:func:`lif_sg_cases.same_bits`)."""
import collections
import itertools

import numpy as np

from lif_sg_cases import F, same_bits, surrogate  # noqa: F401  (same_bits, F: for the tests that import this module)

#: the constants of csrc/be_neuron_sg.hip that the GPU sizes below are derived from
CONSTS = {'kSgThreads': 256, 'kSgGridCap': 2048, 'kSgVec': 4, 'kSgPrefetch': 4}
#: every ring depth a kernel of the file has (one: the adaptive 16-byte backward kernel stays within 128 VGPRs at it)
PREFETCH_DEPTHS = (CONSTS['kSgPrefetch'],)
RESETS = ('hard', 'soft')
SURROGATES = ('fast_sigmoid', 'atan', 'triangle')
#: every reset x surrogate x detach_reset x adaptive
MODES = list(itertools.product(RESETS, SURROGATES, (False, True), (False, True)))
#: the output gradients of a backward pass, in the order of the entry point's arguments
GRADS = ('g_s', 'g_vseq', 'g_clast', 'g_vlast', 'g_alast')
#: which of them a backward pass receives (the others go in as NULL): each alone, and all
GRAD_SETS = {**{name: tuple(g == name for g in GRADS) for name in GRADS}, 'all': (True,) * 5}

#: one slot more than a full pass of the capped grid: of the 4-byte kernel, and (one lane more: N % 4 stays 0) of the 16-byte one
FULL_PASS_SCALAR = CONSTS['kSgThreads'] * CONSTS['kSgGridCap']
FULL_PASS_VECTOR = FULL_PASS_SCALAR * CONSTS['kSgVec']
N_SIZES = (1, 63, 64, 65)
N_PAST_ONE_PASS = (FULL_PASS_SCALAR + 1, FULL_PASS_VECTOR + CONSTS['kSgVec'])
T_SIZES = tuple(sorted({1, 2, 25} | {d + k for d in PREFETCH_DEPTHS for k in (-1, 0, 1)}))
SHAPES = ((65,), (3, 65), (2, 3, 5))

Forward = collections.namedtuple('Forward', 's_out v_seq h_save th_save c_last v_last a_last')
Backward = collections.namedtuple('Backward', 'g_x g_c0 g_v0 g_a0')
#: per-element bounds (f64) of the four gradients, and the sum of the absolute terms of g_x they are relative to
Bound = collections.namedtuple('Bound', 'g_x g_c0 g_v0 g_a0 terms')


class Params:
    """The scalar arguments of a call; the f32 constants are rounded once from doubles, as the host side of the library does."""

    def __init__(self, syn_decay=0.8, beta=0.9, v_th=1.0, v_reset=0.0, rho=0.95, kappa=0.3, adaptive=False, reset='hard',
                 surrogate='fast_sigmoid', alpha=10.0, detach_reset=False):
        self.syn_decay, self.beta, self.v_th, self.v_reset = float(syn_decay), float(beta), float(v_th), float(v_reset)
        self.rho, self.kappa, self.alpha = float(rho), float(kappa), float(alpha)
        self.adaptive, self.reset, self.surrogate, self.detach_reset = bool(adaptive), reset, surrogate, bool(detach_reset)

    def kwargs(self):
        """The keyword arguments of ``be.synaptic_lif_step`` / ``be.synaptic_lif_sequence``."""
        return dict(syn_decay=self.syn_decay, beta=self.beta, v_th=self.v_th, v_reset=self.v_reset, reset=self.reset,
                    surrogate=self.surrogate, alpha=self.alpha, detach_reset=self.detach_reset,
                    adapt=(self.rho, self.kappa) if self.adaptive else None)

    def __repr__(self):
        return f'Params({self.kwargs()})'


def mode_params(reset, surrogate_name, detach, adaptive, **kw):
    """The parameters a mode is tested at: a reset value off zero, and a triangle wide enough to be hit."""
    kw.setdefault('v_reset', -0.25)
    return Params(reset=reset, surrogate=surrogate_name, detach_reset=detach, adaptive=adaptive,
                  alpha=2.0 if surrogate_name == 'triangle' else 10.0, **kw)


def _start(a, N):
    return np.zeros(N, F) if a is None else a.copy()


def forward(x, c0, v0, a0, p):
    """``x [T, N]``; ``c0`` / ``v0`` / ``a0 [N]`` or None (zeros) -> :class:`Forward` (``th_save`` / ``a_last`` None unless
    adaptive)."""
    assert x.dtype == F and x.ndim == 2 and all(a is None or (a.dtype == F and a.shape == x.shape[1:]) for a in (c0, v0, a0))
    syn_decay, beta, v_th, v_reset, rho, kappa = (F(c) for c in (p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa))
    T, N = x.shape
    c, v, a = _start(c0, N), _start(v0, N), _start(a0, N)
    s_out, v_seq, h_save, th_save = (np.empty_like(x) for _ in range(4))
    with np.errstate(all='ignore'):
        for t in range(T):
            dc = syn_decay * c
            c = dc + x[t]
            bv = beta * v
            h = bv + c
            if p.adaptive:
                ka = kappa * a
                th = v_th + ka
            else:
                th = np.full(N, v_th, F)
            s = h >= th
            if p.reset == 'hard':
                v = np.where(s, v_reset, h).astype(F)
            else:
                hm = h - v_th
                v = np.where(s, hm, h).astype(F)
            if p.adaptive:
                ra = rho * a
                a = ra + np.where(s, F(1), F(0))
            s_out[t] = np.where(s, F(1), F(0))
            v_seq[t] = v
            h_save[t] = h
            th_save[t] = th
            assert c.dtype == h.dtype == th.dtype == v.dtype == a.dtype == F
    return Forward(s_out, v_seq, h_save, th_save if p.adaptive else None, c, v, a if p.adaptive else None)


def backward(h_save, th_save, g_s, g_vseq, g_clast, g_vlast, g_alast, p, with_bound=False):
    """``h_save [T, N]``, ``th_save [T, N]`` (adaptive; else ignored); ``g_s`` / ``g_vseq [T, N]`` and ``g_clast`` / ``g_vlast`` /
    ``g_alast [N]`` or None -> :class:`Backward` (``g_a0`` None unless adaptive).

    ``with_bound``: also a :class:`Bound` — per element, how far another evaluation order of the same derivative may be from the
    result.  Per step ``4 * 2**-24 * (sum of the absolute values of the terms g_c is the sum of)`` — the terms as the plain
    formula's autograd forms them: ``g_s * sg``, the adaptation's ``ca * sg``, the reset's ``g_vo * h * sg`` and
    ``g_vo * v_reset * sg`` (soft: ``g_vo * v_th * sg``), the pass-through ``g_vo`` and the current's carry ``cc`` — plus what
    the differences already carried by ``cv``, ``cc`` and ``ca`` become at this step (times the absolute derivative of the
    step's results in them); the three carries take their bounds on with their coefficients ``beta``, ``syn_decay`` and
    ``rho`` / ``kappa`` (``ca`` adds the two terms of its own sum)."""
    assert h_save.dtype == F and h_save.ndim == 2
    syn_decay, beta, v_th, v_reset, rho, kappa = (F(c) for c in (p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa))
    T, N = h_save.shape
    hard = p.reset == 'hard'
    cc, cv, ca = _start(g_clast, N), _start(g_vlast, N), _start(g_alast, N)
    g_x = np.empty_like(h_save)
    bound, terms_x = np.zeros((T, N), np.float64), np.zeros((T, N), np.float64)
    e_c, e_v, e_a = np.zeros(N, np.float64), np.zeros(N, np.float64), np.zeros(N, np.float64)
    eps4 = 4.0 * 2.0 ** -24
    with np.errstate(all='ignore'):
        for t in range(T - 1, -1, -1):
            h = h_save[t]
            th = th_save[t] if p.adaptive else np.full(N, v_th, F)
            s = h >= th
            u = h - th
            g_vo = cv
            if g_vseq is not None:
                g_vo = cv + g_vseq[t]
            sg = surrogate(u, p)
            g_sp = np.zeros(N, F) if g_s is None else g_s[t]
            ca_in = ca
            if p.adaptive:
                g_sp = g_sp + ca
            if not p.detach_reset:
                if hard:
                    r = v_reset - h
                    gr = g_vo * r
                    g_sp = g_sp + gr
                else:
                    gr = g_vo * v_th
                    g_sp = g_sp - gr
            g_u = g_sp * sg
            through = np.where(s, F(0), g_vo).astype(F) if hard else g_vo
            g_h = g_u + through
            g_c = cc + g_h
            g_x[t] = g_c
            cc_in = cc
            cc = syn_decay * g_c
            cv = beta * g_h
            if p.adaptive:
                ra = rho * ca
                kg = kappa * g_u
                ca = ra - kg
            assert g_vo.dtype == g_sp.dtype == g_u.dtype == g_h.dtype == g_c.dtype == cc.dtype == cv.dtype == ca.dtype == F
            if with_bound:
                a = lambda z: np.abs(np.asarray(z, np.float64))
                reach = np.zeros(N) if p.detach_reset else (a(h) + a(v_reset) if hard else np.full(N, a(v_th)))
                terms_u = (a(0 if g_s is None else g_s[t]) + (a(ca_in) if p.adaptive else 0.0) + a(g_vo) * reach) * a(sg)
                err_u = eps4 * terms_u + (e_a + e_v * reach) * a(sg)
                coef = np.where(s, 0.0, 1.0) if hard else np.ones(N)
                terms_h = terms_u + a(through)
                err_h = eps4 * terms_h + (e_a + e_v * reach) * a(sg) + e_v * coef
                terms_x[t] = terms_h + a(cc_in)
                bound[t] = eps4 * terms_x[t] + (err_h - eps4 * terms_h) + e_c
                e_c = a(syn_decay) * bound[t]
                e_v = a(beta) * err_h
                if p.adaptive:
                    e_a = a(rho) * e_a + a(kappa) * err_u + eps4 * (a(rho) * a(ca_in) + a(kappa) * a(g_u))
    out = Backward(g_x, cc, cv, ca if p.adaptive else None)
    if with_bound:
        return out, Bound(bound, e_c, e_v, e_a if p.adaptive else None, terms_x)
    return out


def inputs(T, N, seed):
    """Seeded ``x [T, N]``, the start state ``c0`` / ``v0`` / ``a0 [N]`` and the five output gradients, in :data:`GRADS`' order:
    at the default parameters between a fifth and 0.45 of the steps spike in every mode."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.12, 0.25, (T, N)).astype(F)
    c0 = rng.normal(0.2, 0.3, N).astype(F)
    v0 = rng.normal(0.3, 0.5, N).astype(F)
    a0 = np.abs(rng.normal(0.5, 0.5, N)).astype(F)
    g_s, g_vseq = rng.normal(0, 1, (T, N)).astype(F), rng.normal(0, 1, (T, N)).astype(F)
    g_clast, g_vlast, g_alast = (rng.normal(0, 1, N).astype(F) for _ in range(3))
    return x, (c0, v0, a0), (g_s, g_vseq, g_clast, g_vlast, g_alast)


def pick(grads, use, p):
    """The five gradients with those not in ``use`` — and, without adaptation, ``g_alast`` — replaced by None."""
    return tuple(g if u and (p.adaptive or name != 'g_alast') else None for g, u, name in zip(grads, use, GRADS))


# ------------------------------------------------------------------------------------------------ crafted on-threshold cases
def threshold_case(adaptive):
    """Two slots and two steps from a zero current and membrane: slot 0 meets its threshold exactly at step 0 and spikes, slot 1
    is one f32 below it and does not.  Not adaptive: ``v_th = 1``, ``x[0] = 1`` and ``1 - 2**-24``.  Adaptive: ``kappa = 0.25``,
    ``a0 = 2``, so ``th = 1.5`` exactly, ``x[0] = 1.5`` and ``nextafter(1.5, 0)``; at step 1 slot 0's trace is ``2 * rho + 1``.
    -> ``(p, x [2, 2], state0, expected)`` with the expected ``s_out[0]`` and (adaptive) ``th_save[1]``."""
    if not adaptive:
        p = Params(syn_decay=0.5, beta=0.5, v_th=1.0)
        x = np.array([[1.0, 1.0 - 2.0 ** -24], [0.0, 0.0]], F)
        assert x[0, 1] < 1.0
        return p, x, (np.zeros(2, F), np.zeros(2, F), None), dict(s0=[1.0, 0.0])
    p = Params(syn_decay=0.5, beta=0.5, v_th=1.0, kappa=0.25, rho=0.75, adaptive=True)
    x = np.array([[1.5, np.nextafter(F(1.5), F(0))], [0.0, 0.0]], F)
    a0 = np.array([2.0, 2.0], F)
    rho, kappa = F(p.rho), F(p.kappa)
    a1 = np.array([F(2.0) * rho + F(1.0), F(2.0) * rho], F)                # 2.5 and 1.5: exact
    return p, x, (np.zeros(2, F), np.zeros(2, F), a0), dict(s0=[1.0, 0.0], th0=[1.5, 1.5], th1=(F(p.v_th) + kappa * a1).tolist())
