"""Shared by tests/test_lif_syn_sg_param_cpu.py and tests/test_lif_syn_sg_param_gpu.py: the numpy restatement of the differentiable
synaptic / adaptive LIF neuron with ``syn_decay``, ``beta``, ``v_th``, ``rho`` and ``kappa`` as periodic per-slot arrays
(include/brainevent_amd.h, be_lif_syn_sg_forward_params / be_lif_syn_sg_backward_params; csrc/be_neuron_sg.hip), seeded inputs and
the bounds the comparisons use.

It builds on tests/lif_syn_sg_cases.py (``Params`` for the host scalars and the modes, ``inputs``, the constants) and on
tests/lif_sg_param_cases.py (``expand``, the reduce's reference and bounds).  As there, every constant is an ``np.float32`` and every
operation a statement of its own on ``np.float32`` arrays in the header's order, so the device results are compared as equalities;
the bounds are for other evaluation orders of the same derivative (torch autograd on the CPU, f64)."""
import collections

import numpy as np

import lif_sg_param_cases as PC
import lif_syn_sg_cases as S
from lif_sg_cases import F, same_bits, surrogate  # noqa: F401
from lif_sg_param_cases import any_order_bound, expand, reduce_ref, within_reduce_bound  # noqa: F401

CONSTS = S.CONSTS
MODES = S.MODES
GRADS = S.GRADS
GRAD_SETS = S.GRAD_SETS
N_PAST_ONE_PASS = S.N_PAST_ONE_PASS
#: the issue's sizes: 84 = 2 * 42 and 96 = 3 * 32 — N / 2 = 42 is no multiple of kSgVec (the 4-byte kernel), N / 3 = 32 is
N_SIZES = (1, 63, 64, 65, 84, 96)
T_SIZES = S.T_SIZES
#: the five parameters, in the order of the entry points' arguments
NAMES = ('syn_decay', 'beta', 'v_th', 'rho', 'kappa')
#: the wrong versions of the backward pass the CPU test holds against the bound (``backward(..., variant=)``)
WRONG = ('rho_outgoing_carry', 'kappa_without_a', 'sd_with_c_t', 'v_prev_base_threshold', 'vth_without_direct')

Forward = collections.namedtuple('Forward', 's_out v_seq h_save c_save a_save c_last v_last a_last')
Backward = collections.namedtuple('Backward', 'g_x g_c0 g_v0 g_a0 g_sd_slot g_beta_slot g_vth_slot g_rho_slot g_kappa_slot')
SLOTS = Backward._fields[4:]


def periods_of(N, which):
    """The period a size is tested at: ``'1'``, ``'N'``, ``'N/2'``, ``'N/3'`` (None where it does not divide)."""
    d = {'1': 1, 'N': N, 'N/2': N // 2 if N % 2 == 0 else None, 'N/3': N // 3 if N % 3 == 0 else None}[which]
    return d if d else None


def param_inputs(periods, seed):
    """Seeded ``syn_decay`` in (0.6, 0.9), ``beta`` in (0.5, 0.95), ``v_th`` in (0.8, 1.2), ``rho`` in (0.85, 0.98), ``kappa`` in
    (0.1, 0.5), each with its period from ``periods`` (five); a few thresholds exactly 1."""
    rng = np.random.default_rng(2000 + seed)
    lo_hi = ((0.6, 0.9), (0.5, 0.95), (0.8, 1.2), (0.85, 0.98), (0.1, 0.5))
    q = [rng.uniform(lo, hi, P).astype(F) for (lo, hi), P in zip(lo_hi, periods)]
    q[2][rng.random(periods[2]) < 0.25] = F(1.0)
    return tuple(q)


def shared_params(p):
    """One-element arrays holding the f32 values of a ``lif_syn_sg_cases.Params``."""
    return tuple(np.array([c], F) for c in (p.syn_decay, p.beta, p.v_th, p.rho, p.kappa))


def membrane_after(h, th, v_th, p):
    s = h >= th
    if p.reset == 'hard':
        return np.where(s, F(p.v_reset), h).astype(F)
    hm = h - v_th
    return np.where(s, hm, h).astype(F)


def _start(a, N):
    return np.zeros(N, F) if a is None else a.copy()


def forward(x, c0, v0, a0, q, p):
    """``x [T, N]``; ``c0`` / ``v0`` / ``a0 [N]`` or None; ``q``: the five arrays (``rho`` / ``kappa`` unused unless adaptive);
    ``p``: ``lif_syn_sg_cases.Params`` for ``v_reset``, the reset and ``adaptive`` -> :class:`Forward` (``a_save`` / ``a_last`` None
    unless adaptive)."""
    assert x.dtype == F and x.ndim == 2
    T, N = x.shape
    sd, b, vth = (expand(a, N) for a in q[:3])
    rho, kap = (expand(a, N) for a in q[3:]) if p.adaptive else (None, None)
    c, v, a = _start(c0, N), _start(v0, N), _start(a0, N)
    s_out, v_seq, h_save, c_save, a_save = (np.empty_like(x) for _ in range(5))
    with np.errstate(all='ignore'):
        for t in range(T):
            a_in = a
            dc = sd * c
            c = dc + x[t]
            bv = b * v
            h = bv + c
            if p.adaptive:
                ka = kap * a_in
                th = vth + ka
            else:
                th = vth
            s = h >= th
            v = membrane_after(h, th, vth, p)
            if p.adaptive:
                ra = rho * a_in
                a = ra + np.where(s, F(1), F(0))
            s_out[t] = np.where(s, F(1), F(0))
            v_seq[t] = v
            h_save[t] = h
            c_save[t] = c
            a_save[t] = a_in
            assert c.dtype == h.dtype == th.dtype == v.dtype == a.dtype == F
    return Forward(s_out, v_seq, h_save, c_save, a_save if p.adaptive else None, c, v, a if p.adaptive else None)


def backward(h_save, c_save, a_save, c0, v0, g_s, g_vseq, g_clast, g_vlast, g_alast, q, p, with_bound=False, variant=None):
    """-> :class:`Backward` with all five per-slot accumulators (``g_rho_slot`` / ``g_kappa_slot`` / ``g_a0`` None unless adaptive).

    ``with_bound``: also a dict of f64 arrays.  ``g_x [T, N]``, ``g_c0`` / ``g_v0`` / ``g_a0 [N]``: the bound of
    ``lif_syn_sg_cases.backward`` with the slot's own coefficients.  Per parameter ``name``: ``name + '_terms' [T, N]`` — the terms
    the accumulator is the sum of — and ``name + '_carried' [T, N]`` — what the difference already carried by a term's factors
    becomes in it: the bound of ``g_c`` times ``|c_prev|``, of ``g_h`` times ``|v_prev|``, of ``g_u`` (plus, soft, of ``g_vo`` where
    the slot spiked), of ``g_u`` times ``|a_in|``, of ``ca_in`` times ``|a_in|`` (the forward factors are exact: every evaluation
    order computes them with the same operations).  A gradient's bound is the sum of its ``carried`` plus
    ``any_order_bound(terms)``.

    ``variant``: one of :data:`WRONG` — a plausible mistake, for the CPU test to show the bound tells it apart."""
    assert h_save.dtype == F and h_save.ndim == 2 and variant in (None,) + WRONG
    T, N = h_save.shape
    sd, b, vth = (expand(a, N) for a in q[:3])
    rho, kap = (expand(a, N) for a in q[3:]) if p.adaptive else (None, None)
    v_reset = F(p.v_reset)
    hard = p.reset == 'hard'
    cc, cv, ca = _start(g_clast, N), _start(g_vlast, N), _start(g_alast, N)
    acc = {k: np.zeros(N, F) for k in NAMES}
    g_x = np.empty_like(h_save)
    info = {f'{k}_{w}': np.zeros((T, N), np.float64) for k in NAMES for w in ('terms', 'carried')}
    bound = np.zeros((T, N), np.float64)
    e_c, e_v, e_a = np.zeros(N, np.float64), np.zeros(N, np.float64), np.zeros(N, np.float64)
    eps4 = 4.0 * 2.0 ** -24
    ab = lambda z: np.abs(np.asarray(z, np.float64))

    def threshold(t):
        if not p.adaptive:
            return vth
        ka = kap * a_save[t]
        return vth + ka

    with np.errstate(all='ignore'):
        for t in range(T - 1, -1, -1):
            h = h_save[t]
            th = threshold(t)
            a_in = a_save[t] if p.adaptive else None
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
                    gr = g_vo * vth
                    g_sp = g_sp - gr
            g_u = g_sp * sg
            through = np.where(s, F(0), g_vo).astype(F) if hard else g_vo
            g_h = g_u + through
            g_c = cc + g_h
            g_x[t] = g_c
            cc_in = cc
            cc = sd * g_c
            cv = b * g_h
            if p.adaptive:
                ra = rho * ca
                kg = kap * g_u
                ca = ra - kg
            # what the step started from
            if t > 0:
                th_prev = vth if variant == 'v_prev_base_threshold' else threshold(t - 1)
                v_prev = membrane_after(h_save[t - 1], th_prev, vth, p)
                c_prev = c_save[t - 1]
            else:
                v_prev = np.zeros(N, F) if v0 is None else v0
                c_prev = np.zeros(N, F) if c0 is None else c0
            if variant == 'sd_with_c_t':
                c_prev = c_save[t]
            # the accumulators
            term_sd = g_c * c_prev
            acc['syn_decay'] = acc['syn_decay'] + term_sd
            term_b = g_h * v_prev
            acc['beta'] = acc['beta'] + term_b
            d = g_u
            if not hard and variant != 'vth_without_direct':
                direct = np.where(s, g_vo, F(0)).astype(F)
                d = g_u + direct
            acc['v_th'] = acc['v_th'] - d
            if p.adaptive:
                term_k = g_u if variant == 'kappa_without_a' else g_u * a_in
                acc['kappa'] = acc['kappa'] - term_k
                term_r = (ca if variant == 'rho_outgoing_carry' else ca_in) * a_in
                acc['rho'] = acc['rho'] + term_r
            assert all(v.dtype == F for v in acc.values()) and g_c.dtype == cc.dtype == cv.dtype == ca.dtype == F
            if with_bound:
                reach = np.zeros(N) if p.detach_reset else (ab(h) + ab(v_reset) if hard else ab(vth))
                terms_u = (ab(0 if g_s is None else g_s[t]) + (ab(ca_in) if p.adaptive else 0.0) + ab(g_vo) * reach) * ab(sg)
                err_u = eps4 * terms_u + (e_a + e_v * reach) * ab(sg)
                coef = np.where(s, 0.0, 1.0) if hard else np.ones(N)
                terms_h = terms_u + ab(through)
                err_h = eps4 * terms_h + (e_a + e_v * reach) * ab(sg) + e_v * coef
                terms_x = terms_h + ab(cc_in)
                bound[t] = eps4 * terms_x + (err_h - eps4 * terms_h) + e_c
                info['syn_decay_terms'][t], info['syn_decay_carried'][t] = term_sd, bound[t] * ab(c_prev)
                info['beta_terms'][t], info['beta_carried'][t] = term_b, err_h * ab(v_prev)
                info['v_th_terms'][t] = d
                info['v_th_carried'][t] = err_u + (0.0 if hard else np.where(s, e_v + 2.0 ** -24 * ab(g_vo), 0.0))
                if p.adaptive:
                    info['kappa_terms'][t], info['kappa_carried'][t] = term_k, err_u * ab(a_in)
                    info['rho_terms'][t], info['rho_carried'][t] = term_r, e_a * ab(a_in)
                e_c = ab(sd) * bound[t]
                e_v = ab(b) * err_h
                if p.adaptive:
                    e_a = ab(rho) * e_a + ab(kap) * err_u + eps4 * (ab(rho) * ab(ca_in) + ab(kap) * ab(g_u))
    out = Backward(g_x, cc, cv, ca if p.adaptive else None, acc['syn_decay'], acc['beta'], acc['v_th'],
                   acc['rho'] if p.adaptive else None, acc['kappa'] if p.adaptive else None)
    if with_bound:
        info['g_x'], info['g_c0'], info['g_v0'], info['g_a0'] = bound, e_c, e_v, (e_a if p.adaptive else None)
        return out, info
    return out


def param_bound(info, name, P):
    """Per element of a parameter with period ``P``: the sum of what its terms carry plus the any-order bound of their sum."""
    carried = info[f'{name}_carried'].reshape(-1, P).sum(axis=0)
    return carried + any_order_bound(info[f'{name}_terms'], P)


def param_exact(info, name, P):
    """The f64 sum of the f32 terms (the sign of ``v_th`` / ``kappa``: their accumulators subtract)."""
    sign = -1.0 if name in ('v_th', 'kappa') else 1.0
    return sign * np.asarray(info[f'{name}_terms'], np.float64).reshape(-1, P).sum(axis=0)


def inputs(T, N, seed):
    """Seeded ``x [T, N]``, the start state ``(c0, v0, a0)`` and the five output gradients, as ``lif_syn_sg_cases.inputs`` but with
    a stronger start (c0, v0): the per-neuron thresholds reach 1.2 and ``kappa`` 0.5, and between 0.05 and 0.6 of the steps must spike in
    every mode from the first step on (tests/test_lif_syn_sg_param_cpu.py asserts it)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.14, 0.25, (T, N)).astype(F)
    c0 = rng.normal(0.45, 0.3, N).astype(F)
    v0 = rng.normal(0.5, 0.5, N).astype(F)
    a0 = np.abs(rng.normal(0.5, 0.5, N)).astype(F)
    g_s, g_vseq = rng.normal(0, 1, (T, N)).astype(F), rng.normal(0, 1, (T, N)).astype(F)
    g_clast, g_vlast, g_alast = (rng.normal(0, 1, N).astype(F) for _ in range(3))
    return x, (c0, v0, a0), (g_s, g_vseq, g_clast, g_vlast, g_alast)
