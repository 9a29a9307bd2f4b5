"""Shared by tests/test_lif_sg_param_cpu.py and tests/test_lif_sg_param_gpu.py: the numpy restatement of the differentiable LIF
neuron with ``beta`` and ``v_th`` as periodic per-slot arrays (include/brainevent_amd.h, be_lif_sg_forward_params /
be_lif_sg_backward_params / be_lif_sg_reduce_slots; csrc/be_neuron_sg.hip, be_neuron_sg_reduce.hip), the CONSTS table the GPU sizes
are taken from (the CPU test holds it against the source text), and the bounds the comparisons use.

It builds on tests/lif_sg_cases.py (``Params`` for the host scalars, ``surrogate``, ``same_bits``, ``inputs``) and adds the periods,
the two per-slot accumulators of the parameters' gradients and the reduce's reference.  As there, every constant is an
``np.float32`` and every operation a statement of its own on ``np.float32`` arrays, so the device results are compared with it as
equalities."""
import math

import numpy as np

import lif_sg_cases as C
from lif_sg_cases import F

#: the constants of csrc/be_neuron_sg.hip (the lane's) and csrc/be_neuron_sg_reduce.hip (kSgpRed*) the GPU sizes are derived from
CONSTS = {'kSgThreads': 256, 'kSgGridCap': 2048, 'kSgVec': 4, 'kSgPrefetch': 4,
          'kSgpRedThreads': 256, 'kSgpRedTile': 4096, 'kSgpRedGridCap': 256, 'kSgpRedCols': 64}

FULL_PASS_SCALAR = CONSTS['kSgThreads'] * CONSTS['kSgGridCap']
FULL_PASS_VECTOR = FULL_PASS_SCALAR * CONSTS['kSgVec']
N_SIZES = (1, 63, 64, 65)
#: one slot past a full pass of the capped grid of the 4-byte kernel, one lane past it of the 16-byte kernel
N_PAST_ONE_PASS = (FULL_PASS_SCALAR + 1, FULL_PASS_VECTOR + CONSTS['kSgVec'])
T_SIZES = (1, 2, 25, CONSTS['kSgPrefetch'] - 1, CONSTS['kSgPrefetch'], CONSTS['kSgPrefetch'] + 1)
#: the reduce with period 1: past one block's tile, and past one pass of the first stage's capped grid
REDUCE_N_SHARED = (1, CONSTS['kSgpRedThreads'] + 1, CONSTS['kSgpRedTile'] + 1, CONSTS['kSgpRedTile'] * CONSTS['kSgpRedGridCap'] + 1)
#: the reduce with a longer period: under, at and past one block's columns; rows under, at and past the row lanes of a block
REDUCE_PERIODS = (3, CONSTS['kSgpRedCols'], CONSTS['kSgpRedCols'] + 1)
REDUCE_ROWS = (1, 2, 33)


def expand(param, N):
    """The ``[N]`` array slot ``i`` reads: ``param[i % P]``."""
    param = np.ascontiguousarray(param, F).reshape(-1)
    assert param.size >= 1 and N % param.size == 0
    return np.tile(param, N // param.size)


def reset(h, th, p):
    """The membrane a step leaves behind, from its ``h``."""
    s = h >= th
    if p.reset == 'hard':
        return np.where(s, F(p.v_reset), h).astype(F)
    hm = h - th
    return np.where(s, hm, h).astype(F)


def forward(x, v0, beta, v_th, p):
    """``x [T, N]``, ``v0 [N]`` or None, ``beta [Pb]``, ``v_th [Pt]`` -> ``(s_out, v_seq, h_save, v_last)`` (``p.beta`` / ``p.v_th``
    are not used)."""
    assert x.dtype == F and x.ndim == 2 and (v0 is None or (v0.dtype == F and v0.shape == x.shape[1:]))
    T, N = x.shape
    b, th = expand(beta, N), expand(v_th, N)
    v = np.zeros(N, F) if v0 is None else v0.copy()
    s_out, v_seq, h_save = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    with np.errstate(all='ignore'):
        for t in range(T):
            bv = b * v
            h = bv + x[t]
            s = h >= th
            v = reset(h, th, p)
            s_out[t] = np.where(s, F(1), F(0))
            v_seq[t] = v
            h_save[t] = h
            assert bv.dtype == h.dtype == v.dtype == F
    return s_out, v_seq, h_save, v


def backward(h_save, v0, g_s, g_vseq, g_vlast, beta, v_th, p, with_bound=False):
    """``h_save [T, N]``, ``v0 [N]`` or None; ``g_s`` / ``g_vseq [T, N]`` and ``g_vlast [N]`` or None ->
    ``(g_x, g_v0, g_beta_slot, g_vth_slot)``.

    ``with_bound``: a dict too, with f64 arrays: ``g_x [T, N]`` and ``g_v0 [N]`` — the bound of ``lif_sg_cases.backward`` with the
    per-slot parameters; ``beta_terms`` / ``vth_terms [T, N]`` — the terms the two accumulators are the sums of; ``beta_carried`` /
    ``vth_carried [T, N]`` — what the difference carried by the quantities a term is built from becomes in it: ``bound[t] * |v_prev|``
    for ``g_h * v_prev``, and for ``d`` the bound of ``g_sp * sg`` formed as that of ``g_h`` is (without the pass-through) plus, soft,
    the difference carried by ``g_vo`` where the slot spiked."""
    assert h_save.dtype == F and h_save.ndim == 2
    T, N = h_save.shape
    b, th = expand(beta, N), expand(v_th, N)
    v_reset = F(p.v_reset)
    hard = p.reset == 'hard'
    carry = np.zeros(N, F) if g_vlast is None else g_vlast.copy()
    a_b, a_th = np.zeros(N, F), np.zeros(N, F)
    g_x = np.empty_like(h_save)
    bound = np.zeros((T, N), np.float64)
    carried = np.zeros(N, np.float64)
    info = {k: np.zeros((T, N), np.float64) for k in ('beta_terms', 'vth_terms', 'beta_carried', 'vth_carried')}
    eps4 = 4.0 * 2.0 ** -24
    a = lambda z: np.abs(np.asarray(z, np.float64))
    with np.errstate(all='ignore'):
        for t in range(T - 1, -1, -1):
            h = h_save[t]
            u = h - th
            s = h >= th
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
                    gr = g_vo * th
                    g_sp = g_sp - gr
            through = np.where(s, F(0), g_vo).astype(F) if hard else g_vo
            gs = g_sp * sg
            g_h = gs + through
            g_x[t] = g_h
            carry = b * g_h
            # the parameters' accumulators
            if t > 0:
                v_prev = reset(h_save[t - 1], th, p)
            else:
                v_prev = np.zeros(N, F) if v0 is None else v0
            term_b = g_h * v_prev
            a_b = a_b + term_b
            d = gs
            if not hard:
                direct = np.where(s, g_vo, F(0)).astype(F)
                d = gs + direct
            a_th = a_th - d
            assert g_vo.dtype == g_sp.dtype == g_h.dtype == carry.dtype == term_b.dtype == d.dtype == a_b.dtype == a_th.dtype == F
            if with_bound:
                terms_d = a(0 if g_s is None else g_s[t]) * a(sg)
                coef_d = np.zeros(N)
                if not p.detach_reset:
                    if hard:
                        terms_d = terms_d + (a(g_vo) * a(h) + a(g_vo) * a(v_reset)) * a(sg)
                        coef_d = coef_d + (a(h) + a(v_reset)) * a(sg)
                    else:
                        terms_d = terms_d + a(g_vo) * a(th) * a(sg)
                        coef_d = coef_d + a(th) * a(sg)
                terms = terms_d + a(through)
                coef = coef_d + (np.where(s, 0.0, 1.0) if hard else np.ones(N))
                bound[t] = eps4 * terms + carried * coef
                if not hard:
                    terms_d = terms_d + np.where(s, a(g_vo), 0.0)
                    coef_d = coef_d + np.where(s, 1.0, 0.0)
                info['beta_terms'][t] = term_b
                info['vth_terms'][t] = d
                info['beta_carried'][t] = bound[t] * a(v_prev)
                info['vth_carried'][t] = eps4 * terms_d + carried * coef_d
                carried = a(b) * bound[t]
    if with_bound:
        info['g_x'], info['g_v0'] = bound, carried
        return g_x, carry, a_b, a_th, info
    return g_x, carry, a_b, a_th


def surrogate(u, p):
    return C.surrogate(u, p)


# ------------------------------------------------------------------------------------------------ the reduce
def reduce_exact(slot, P):
    """``E[p]``: the sum of the slots ``r * P + p`` as exact f64 sums, rounded once (``math.fsum``)."""
    slot = np.asarray(slot).reshape(-1, P).astype(np.float64)
    return np.array([math.fsum(slot[:, p].tolist()) for p in range(P)], np.float64)


def reduce_bound(slot, P):
    """``2**-24 |E| + R 2**-52 A + 2**-149``: the final rounding to f32, and twice the first-order error of an R-term f64 sum in any
    order (``A`` the sum of the absolute values)."""
    slot = np.asarray(slot).reshape(-1, P).astype(np.float64)
    R = slot.shape[0]
    A = np.array([math.fsum(np.abs(slot[:, p]).tolist()) for p in range(P)], np.float64)
    return 2.0 ** -24 * np.abs(reduce_exact(slot, P)) + R * 2.0 ** -52 * A + 2.0 ** -149


def reduce_ref(slot, P):
    """The gradient the restatement gives: the exact sum rounded to f32."""
    return reduce_exact(slot, P).astype(F)


def within_reduce_bound(out, slot, P):
    out = np.asarray(out).reshape(-1)
    if out.dtype != F or out.size != P:
        return False
    err = np.abs(out.astype(np.float64) - reduce_exact(slot, P))
    return bool((err <= reduce_bound(slot, P)).all())


def any_order_bound(terms, P):
    """``(n + 1) 2**-23 sum |terms|`` per output element, over the ``n`` terms ``[T, N] -> [T * N / P]`` of each: twice the
    first-order bound of an n-term f32 sum of rounded products in any order."""
    terms = np.abs(np.asarray(terms, np.float64)).reshape(-1, P)
    return (terms.shape[0] + 1) * 2.0 ** -23 * terms.sum(axis=0)


def cancelling(R, P, seed):
    """``[R * P]`` f32 slots whose columns cancel heavily: large values of both signs in pairs that almost cancel, small ones
    between them (a running f32 sum loses the small ones)."""
    rng = np.random.default_rng(seed)
    slot = rng.normal(0, 1e-3, (R, P)).astype(F)
    big = (rng.normal(0, 1e4, (R, P))).astype(F)
    k = R // 2
    slot[:k] += big[:k]
    slot[k:2 * k] -= big[:k][::-1]
    return np.ascontiguousarray(rng.permutation(slot, axis=0) if R > 2 else slot).reshape(-1)


def param_inputs(Pb, Pt, seed):
    """Seeded ``beta [Pb]`` in (0.5, 0.95) and ``v_th [Pt]`` in (0.8, 1.2); a few thresholds exactly 1 (where ``inputs`` puts h)."""
    rng = np.random.default_rng(1000 + seed)
    beta = rng.uniform(0.5, 0.95, Pb).astype(F)
    v_th = rng.uniform(0.8, 1.2, Pt).astype(F)
    v_th[rng.random(Pt) < 0.25] = F(1.0)
    return beta, v_th
