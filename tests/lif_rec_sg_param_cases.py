"""Shared by tests/test_lif_rec_sg_param_cpu.py and tests/test_lif_rec_sg_param_gpu.py: the numpy restatement of the fused recurrent
spiking layer with ``syn_decay``, ``beta``, ``v_th``, ``rho`` and ``kappa`` as device arrays with a period of 1 or ``N``
(include/brainevent_amd.h, be_lif_rec_sg_forward_params / be_lif_rec_sg_backward_params; csrc/be_neuron_sg_rec.hip).

Nothing is restated twice.  The recurrence — the fixed-point sums, the gather, their bound — is tests/lif_rec_sg_cases.py's (``R``);
the neuron's step with per-slot parameters and its five accumulators are tests/lif_syn_sg_param_cases.py's (``P``), called one time
step at a time on the ``B * N`` slots of a step, where a period of ``N`` is the period ``P`` already knows:

* forward: ``xin = x[t] + r`` with ``R.recurrent_input``, then ``P.forward`` on that one step;
* backward, values: ``g_sp = g_s[t] + g_rec`` with ``R.gather`` of the ``g_x[t + 1]`` just computed, then ``P.backward`` on that one
  step, started from the carries the step before left and from ``c_prev`` / ``v_prev`` as its ``c0`` / ``v0``.  One step's accumulator is
  ``+0 + term`` (``+0 - d``); adding it to the running sum is the kernel's ``acc + term`` (``acc - d``) bit for bit, because a
  running sum that started from ``+0`` is never ``-0``;
* backward, bounds: ``R.backward`` run once on the same arrays with a ``Params`` whose five values are ``[B, N]`` arrays gives the bound
  of ``g_x``, the state and ``s0`` through the carries and the gathers (its formulas are elementwise in the coefficients); its ``g_x``
  must equal the step-by-step one bit for bit, which :func:`backward` asserts.  A parameter's bound is ``P.param_bound``'s: what the
  factors of its terms carry plus the any-order bound of their sum.  The factors' own bounds come from that run: ``g_c``'s is its
  ``g_x``; ``g_u``'s and ``g_h``'s follow ``R.backward``'s rule for them from what arrives at the step — the gather's bound
  (``R.gather``), the bound of the carry ``cv`` (``|beta|`` times the bound of ``g_x[t + 1]``, which contains ``g_h``'s) and the bound of
  the carry ``ca``, which is the bound of ``g_a0`` of the same pass over the steps ``t + 1 .. T - 1`` alone."""
import collections
import copy

import numpy as np

import lif_rec_sg_cases as R
import lif_syn_sg_param_cases as P
from lif_rec_sg_cases import (F, Matrix, crafted_matrix, dense, dyadic_matrix, empty_matrix, exponent, random_matrix,  # noqa: F401
                              rows_of, same_bits, weight_grad)
from lif_syn_sg_param_cases import (NAMES, SLOTS, any_order_bound, expand, param_inputs, reduce_ref, shared_params,  # noqa: F401
                                    within_reduce_bound)
from lif_syn_sg_cases import Params, mode_params  # noqa: F401

CONSTS = R.CONSTS
N_SIZES, B_SIZES, T_SIZES = R.N_SIZES, R.B_SIZES, R.T_SIZES
MODES = R.MODES
GRADS, GRAD_SETS = P.GRADS, P.GRAD_SETS
EPS = R.EPS
#: five period patterns, one letter per parameter in NAMES' order: ``1`` shared, ``N`` per neuron
PATTERNS = ('11111', 'NNNNN', 'N1N1N', '1N1N1', 'NN11N')
#: the wrong versions of the backward pass the CPU test holds against the bound (``backward(..., variant=)``)
WRONG = ('no_recurrent_term', 'v_prev_from_step_t', 'vth_without_direct', 'rho_outgoing_carry', 'neighbour_parameters')

Forward = collections.namedtuple('Forward', 's_out v_seq h_save c_save a_save c_last v_last a_last r')
Backward = collections.namedtuple('Backward', 'g_x g_c0 g_v0 g_a0 g_s0 g_sd_slot g_beta_slot g_vth_slot g_rho_slot g_kappa_slot')


def periods(pattern, N):
    return tuple(1 if c == '1' else N for c in pattern)


def one_entry_matrix(n, seed):
    """Every row holds exactly one entry: a gather of one product has no order, so the backward pass is the kernel's bit for bit
    through the recurrence as well."""
    rng = np.random.default_rng(seed)
    return R._matrix(rng.normal(0.0, 0.3, n), rng.integers(0, n, n), np.ones(n, np.int64), n)


def inputs(T, B, N, seed):
    """``lif_rec_sg_cases.inputs`` with the stronger start of ``lif_syn_sg_param_cases.inputs`` (the per-neuron thresholds reach 1.2
    and ``kappa`` 0.5): ``x``, ``s0``, ``(c0, v0, a0)`` and the five output gradients."""
    x, s0, (c0, v0, a0), grads = R.inputs(T, B, N, seed)
    return (x + F(0.04)).astype(F), s0, ((c0 + F(0.25)).astype(F), (v0 + F(0.2)).astype(F), a0), grads


def array_params(q, p, B, N):
    """A ``Params`` whose five values are the ``[B, N]`` arrays every slot reads (for ``R.backward``, whose formulas are elementwise)."""
    pa = copy.copy(p)
    full = lambda a: expand(a, B * N).reshape(B, N)
    pa.syn_decay, pa.beta, pa.v_th = full(q[0]), full(q[1]), full(q[2])
    if p.adaptive:
        pa.rho, pa.kappa = full(q[3]), full(q[4])
    return pa


def thresholds(a_save, q, p):
    """``th_save`` from ``a_save``, with the forward pass's two operations."""
    T, B, N = a_save.shape
    vth, kap = expand(q[2], B * N).reshape(B, N), expand(q[4], B * N).reshape(B, N)
    ka = kap[None] * a_save
    th = vth[None] + ka
    assert th.dtype == F
    return th


# ------------------------------------------------------------------------------------------------ the forward pass
def forward(x, m, s0, c0, v0, a0, q, p, e):
    """``x [T, B, N]``; ``s0`` / ``c0`` / ``v0`` / ``a0 [B, N]`` or None; ``q``: the five arrays, each of 1 or ``N`` elements -> :class:`Forward`
    (``a_save`` / ``a_last`` None unless adaptive; ``r [T, B, N]``: the recurrent input of every step)."""
    assert x.dtype == F and x.ndim == 3 and x.shape[2] == m.n
    T, B, N = x.shape
    assert all(a is None or a.size in (1, N) for a in q)
    fixed = R.fixed_from_f32(m.w, e)
    flat = lambda a: None if a is None else a.reshape(-1)
    c, v, a = flat(c0), flat(v0), flat(a0) if p.adaptive else None
    sp = np.zeros((B, N), bool) if s0 is None else (s0 != 0)
    s_out, v_seq, h_save, c_save, a_save, r_all = (np.empty_like(x) for _ in range(6))
    for t in range(T):
        r = np.stack([R.recurrent_input(m, fixed, sp[b], e) for b in range(B)]) if B else np.zeros((0, N), F)
        xin = x[t] + r
        assert xin.dtype == F
        f = P.forward(xin.reshape(1, -1), c, v, a, q, p)
        c, v, a = f.c_last, f.v_last, f.a_last
        for out, got in ((s_out, f.s_out), (v_seq, f.v_seq), (h_save, f.h_save), (c_save, f.c_save)):
            out[t] = got.reshape(B, N)
        if p.adaptive:
            a_save[t] = f.a_save.reshape(B, N)
        r_all[t] = r
        sp = s_out[t] != 0
    z = np.zeros(B * N, F)
    c, v, a = (z if c is None else c), (z if v is None else v), ((z if a is None else a) if p.adaptive else None)
    shape = lambda g: None if g is None else g.reshape(B, N)
    return Forward(s_out, v_seq, h_save, c_save, a_save if p.adaptive else None, shape(c), shape(v), shape(a), r_all)


# ------------------------------------------------------------------------------------------------ the backward pass
def _neighbour(q, N):
    """The parameters of neuron ``i + 1`` in neuron ``i``'s place (a planted mistake)."""
    return tuple(a if a is None or a.size == 1 else np.roll(a, -1) for a in q)


def backward(h_save, c_save, a_save, m, c0, v0, g_s, g_vseq, g_clast, g_vlast, g_alast, q, p, with_bound=False, variant=None):
    """``h_save`` / ``c_save`` / ``a_save`` / ``g_s`` / ``g_vseq [T, B, N]``, the others ``[B, N]`` (gradients, ``c0`` and ``v0`` may be None)
    -> :class:`Backward` with all five ``[B, N]`` accumulators (``g_rho_slot`` / ``g_kappa_slot`` / ``g_a0`` None unless adaptive).

    ``with_bound``: also a dict of f64 arrays — ``g_x [T, B, N]``, ``g_c0`` / ``g_v0`` / ``g_a0`` / ``g_s0 [B, N]`` (``R.backward``'s
    bound), and per parameter ``name + '_terms'`` / ``name + '_carried' [T, B * N]`` as ``lif_syn_sg_param_cases.backward`` returns
    them, for ``P.param_bound`` / ``P.param_exact`` with a period of ``B * N`` (the accumulators), ``N`` or 1.

    ``variant``: one of :data:`WRONG`."""
    assert h_save.dtype == F and h_save.ndim == 3 and variant in (None,) + WRONG
    T, B, N = h_save.shape
    n = B * N
    if variant == 'neighbour_parameters':
        q = _neighbour(q, N)
    mg = empty_matrix(N) if variant == 'no_recurrent_term' else m
    p_variant = variant if variant in P.WRONG else None
    th_save = thresholds(a_save, q, p) if p.adaptive else None
    flat = lambda g: None if g is None else g.reshape(-1)
    cc, cv, ca = flat(g_clast), flat(g_vlast), flat(g_alast) if p.adaptive else None
    vth = expand(q[2], n)
    g_x = np.empty_like(h_save)
    acc = [None] * 5
    info = {f'{k}_{w}': np.zeros((T, n)) for k in NAMES for w in ('terms', 'carried')}
    prev = {}
    for t in range(T - 1, -1, -1):
        g_sp = None if g_s is None else g_s[t]
        if t < T - 1:
            g_rec = R.gather(mg, g_x[t + 1])
            g_sp = (np.zeros((B, N), F) if g_sp is None else g_sp) + g_rec
            assert g_sp.dtype == F
        if t > 0:
            k = t if variant == 'v_prev_from_step_t' else t - 1
            th_prev = th_save[k].reshape(-1) if p.adaptive else vth
            v_prev, c_prev = P.membrane_after(h_save[k].reshape(-1), th_prev, vth, p), c_save[t - 1].reshape(-1)
        else:
            v_prev, c_prev = flat(v0), flat(c0)
        one = lambda a: None if a is None else a[t].reshape(1, n)
        out = P.backward(one(h_save), one(c_save), one(a_save) if p.adaptive else None, c_prev, v_prev,
                         None if g_sp is None else g_sp.reshape(1, n), one(g_vseq), cc, cv, ca, q, p,
                         with_bound=with_bound, variant=p_variant)
        b, step_info = out if with_bound else (out, None)
        g_x[t] = b.g_x.reshape(B, N)
        g_vo = np.zeros(n, F) if cv is None else cv
        if g_vseq is not None:
            g_vo = g_vo + g_vseq[t].reshape(-1)
        prev[t] = (np.zeros(n, F) if c_prev is None else c_prev, np.zeros(n, F) if v_prev is None else v_prev, g_vo,
                   np.zeros(n, F) if ca is None else ca)
        cc, cv, ca = b.g_c0, b.g_v0, b.g_a0
        for j, part in enumerate(b[4:]):
            if part is not None:
                acc[j] = part if acc[j] is None else acc[j] + part
                assert acc[j].dtype == F
        if with_bound:
            for name in NAMES:
                info[f'{name}_terms'][t] = step_info[f'{name}_terms'][0]
    zero = np.zeros((B, N), F)
    g_s0 = R.gather(mg, g_x[0]) if T > 0 else zero
    shape = lambda g, given=True: None if not given else (zero.copy() if g is None else g.reshape(B, N))
    out = Backward(g_x, shape(cc), shape(cv), shape(ca, p.adaptive), g_s0, *(shape(acc[j], j < 3 or p.adaptive) for j in range(5)))
    if not with_bound:
        return out
    # the bounds of what the terms are made of: R's run on the same arrays with the slots' own coefficients
    pa = array_params(q, p, B, N)
    ref, bound = R.backward(h_save, th_save, mg, g_s, g_vseq, g_clast, g_vlast, g_alast, pa, with_bound=True)
    assert same_bits(ref.g_x, g_x) and same_bits(ref.g_s0, g_s0) and same_bits(ref.g_c0, out.g_c0) and same_bits(ref.g_v0, out.g_v0)
    ab = lambda z: np.abs(np.asarray(z, np.float64))
    eps4, hard = 4.0 * EPS, p.reset == 'hard'
    beta_a = ab(pa.beta).reshape(-1)
    for t in range(T):
        c_prev, v_prev, g_vo, ca_in = prev[t]
        h = h_save[t].reshape(-1)
        th = th_save[t].reshape(-1) if p.adaptive else vth
        s, sg = h >= th, ab(R.surrogate((h - th).astype(F), p))
        a_in = ab(a_save[t].reshape(-1)) if p.adaptive else np.zeros(n)
        # what arrives at the step: the carries' bounds (cv's from the bound of g_x[t + 1], which contains g_h's; ca's from the same
        # pass over the later steps alone) and the gather's
        e_v = beta_a * bound.g_x[t + 1].reshape(-1) if t < T - 1 else np.zeros(n)
        e_a, e_r, mag_r = np.zeros(n), np.zeros(n), np.zeros(n)
        if t < T - 1:
            _, e_r, mag_r = (z.reshape(-1) for z in R.gather(mg, g_x[t + 1], bound.g_x[t + 1]))
            if p.adaptive:
                later = lambda g: None if g is None else g[t + 1:]
                _, tail = R.backward(h_save[t + 1:], th_save[t + 1:], mg, later(g_s), later(g_vseq), g_clast, g_vlast, g_alast, pa,
                                     with_bound=True)
                e_a = tail.g_a0.reshape(-1)
        # g_u's and g_h's own bounds, by R.backward's rule for them
        reach = np.zeros(n) if p.detach_reset else (ab(h) + ab(F(p.v_reset)) if hard else ab(vth))
        terms_u = (ab(0 if g_s is None else g_s[t].reshape(-1)) + mag_r + ab(ca_in) + ab(g_vo) * reach) * sg
        err_u = eps4 * terms_u + (e_r + e_a + e_v * reach) * sg
        through = np.where(s, 0.0, ab(g_vo)) if hard else ab(g_vo)
        err_h = err_u + eps4 * through + e_v * (np.where(s, 0.0, 1.0) if hard else 1.0)
        info['syn_decay_carried'][t] = bound.g_x[t].reshape(-1) * ab(c_prev)
        info['beta_carried'][t] = err_h * ab(v_prev)
        info['v_th_carried'][t] = err_u + (0.0 if hard else np.where(s, e_v + EPS * ab(g_vo), 0.0))
        if p.adaptive:
            info['kappa_carried'][t] = err_u * a_in
            info['rho_carried'][t] = e_a * a_in
    info.update(g_x=bound.g_x, g_c0=bound.g_c0, g_v0=bound.g_v0, g_a0=bound.g_a0, g_s0=bound.g_s0)
    return out, info


def param_bound(info, name, period):
    return P.param_bound(info, name, period)


def param_exact(info, name, period):
    return P.param_exact(info, name, period)
