"""Shared by tests/test_lif_rec_delay_cpu.py and tests/test_lif_rec_delay_gpu.py: a numpy restatement of the recurrent spiking
layer with synaptic delays (include/brainevent_amd.h, be_lif_rec_delay_sg_forward / _backward and be_grad_pack_activity_aged;
csrc/be_neuron_sg_rec_delay.hip).  It builds on tests/lif_rec_sg_cases.py (the fixed-point encoding, the
exponent's rule, the matrices, the inputs, the row gather and its bound), tests/lif_syn_sg_cases.py (the neuron's step) and
tests/delay_cases.py (the delay split) and restates only what the delays add.

Forward: stacked row ``d * N + i`` is active at step ``t`` when ``sp(t - 1 - d)[b][i]``; the sums are 64-bit wrapping integers
over the entries of the active stacked rows, so the device's forward outputs are compared as equalities.  Backward: f32; the
gather of one stacked row is ``lif_rec_sg_cases.gather`` on the rows of one delay (a plain ascending sum; the device's order is its
own), ``g_rec`` the sum over the delays in ascending order from +0.  The bound extends that module's: every stacked-row gather
adds ``(len + 1) * 2**-24 * sum |w * G|`` plus ``sum |w|`` times the bound of ``G``, and the sum over the ages adds one rounding
per term, each relative to at most the sum of all ``|w * G|``: ``(number of ages) * 2**-24 * sum over the ages of sum |w * G|``."""
import collections

import numpy as np

import lif_rec_sg_cases as R
import lif_syn_sg_cases as S
from delay_cases import split_by_delay_np
from lif_rec_sg_cases import EPS, F, Matrix, exponent, fixed_from_f32, inputs, same_bits  # noqa: F401  (for the tests)

#: the constants of csrc/be_neuron_sg_rec_delay.hip the GPU sizes and the limit rule are derived from
CONSTS = {'kDelThreads': 1024, 'kDelMaxN': 8192, 'kDelMaxDepth': 256, 'kDelRowLanes': 2, 'kDelUnroll': 4, 'kDelMinIds': 4096}
LDS_BYTES = 160 * 1024 - 1024
N_SIZES = R.N_SIZES
B_SIZES = R.B_SIZES
#: (T, depth): one step; as many steps as delays; more delays than steps; more steps than delays; both odd; the deepest split
T_DEPTHS = ((1, 1), (2, 2), (3, 7), (5, 2), (5, 7), (2, 256))
DELAY_KINDS = ('random', 'equal', 'ends')

Delayed = collections.namedtuple('Delayed', 'm delays depth stacked perm row_mask')
Forward = R.Forward
Backward = collections.namedtuple('Backward', 'g_x g_c0 g_v0 g_a0 g_s_hist')
Bound = collections.namedtuple('Bound', 'g_x g_c0 g_v0 g_a0 g_s_hist terms')


def fits(n, depth):
    """The limit rule of the kernels (the text of the source is held to it by tests/test_lif_rec_delay_cpu.py)."""
    return (n <= CONSTS['kDelMaxN'] and 1 <= depth <= CONSTS['kDelMaxDepth']
            and 8 * n + 8 * depth * ((n + 63) // 64) + 4 * CONSTS['kDelMinIds'] <= LDS_BYTES)


# ------------------------------------------------------------------------------------------------ the delay split
def split(m, delays, depth):
    """``m`` (a ``lif_rec_sg_cases.Matrix``) with one delay per stored entry -> :class:`Delayed`: ``stacked`` is a ``Matrix`` whose
    ``indptr`` has ``depth * n + 1`` elements (``n`` stays the number of columns), ``perm`` maps a stacked position to the original
    one, ``row_mask`` is uint32 ``[depth, ceil(n / 32)]``."""
    delays = np.asarray(delays, np.int32).reshape(-1)
    assert len(delays) == len(m.w) and (len(delays) == 0 or (0 <= delays.min() and delays.max() < depth))
    indptr_s, perm, row_mask = split_by_delay_np(m.indptr, delays, m.n, depth)
    stacked = Matrix(m.w[perm], m.indices[perm], indptr_s.astype(np.int32), m.n)
    return Delayed(m, delays, depth, stacked, perm, np.ascontiguousarray(row_mask))


def delays_for(kind, m, depth, seed):
    """One delay per entry: ``random``, ``equal`` (all ``depth // 2``) or ``ends`` (only 0 and ``depth - 1``)."""
    rng = np.random.default_rng(seed)
    nse = len(m.w)
    if kind == 'equal':
        return np.full(nse, depth // 2, np.int32)
    if kind == 'ends':
        return (rng.integers(0, 2, nse) * (depth - 1)).astype(np.int32)
    assert kind == 'random'
    return rng.integers(0, depth, nse).astype(np.int32)


def parallel_matrix(n, seed, dyadic=False):
    """Every synapse stored twice or three times — the same ``(row, col)``, to be given different delays — and every third row
    empty."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 4, n)
    counts[::3] = 0
    cols = [np.repeat(rng.integers(0, n, c), rng.integers(2, 4, c)) for c in counts]
    indices = np.concatenate(cols) if n else np.zeros(0, np.int64)
    nse = len(indices)
    w = rng.integers(-16, 17, nse) / 64.0 if dyadic else rng.normal(0.0, 0.05, nse)
    indptr = np.zeros(n + 1, np.int32)
    np.cumsum([len(c) for c in cols], out=indptr[1:])
    return Matrix(np.asarray(w, F), indices.astype(np.int32), indptr, n)


def stacked_rows(D):
    return np.repeat(np.arange(D.depth * D.m.n), np.diff(D.stacked.indptr))


def of_delay(D, d):
    """The rows of delay ``d`` as a square ``Matrix`` of their own."""
    n, st = D.m.n, D.stacked
    ptr = st.indptr[d * n:(d + 1) * n + 1]
    return Matrix(st.w[ptr[0]:ptr[-1]], st.indices[ptr[0]:ptr[-1]], (ptr - ptr[0]).astype(np.int32), n)


def to_original(D, per_stacked_entry):
    out = np.empty_like(per_stacked_entry)
    out[D.perm] = per_stacked_entry
    return out


# ------------------------------------------------------------------------------------------------ the spikes of any step
def spikes_at(s_out, s_hist, tau):
    """``sp(tau) [B, N]`` as booleans: the layer's output for ``tau >= 0``, the history before step 0 (``s_hist [A, B, N]`` or
    None), silence before the history."""
    if tau >= 0:
        return s_out[tau] != 0
    age = -1 - tau
    if s_hist is not None and age < s_hist.shape[0]:
        return s_hist[age] != 0
    return np.zeros(s_out.shape[1:], bool)


def active_rows(s_out, s_hist, t, depth, late=0):
    """``[B, depth * N]``: stacked row ``d * N + i`` is active at step ``t`` when ``sp(t - 1 - d)[b][i]`` (``late``: a deliberately
    wrong shift for the tests that must fail)."""
    return np.concatenate([spikes_at(s_out, s_hist, t - 1 - d - late) for d in range(depth)], axis=1)


# ------------------------------------------------------------------------------------------------ the forward pass
def recurrent_input(D, fixed, active, e):
    """``r [N]`` of one sample from the active stacked rows ``[depth * N]``: the 64-bit wrapping sum, scaled back in f64 and rounded
    to f32 once — ``lif_rec_sg_cases.recurrent_input`` over the stacked rows."""
    R_ = np.zeros(D.m.n, np.int64)
    on = active[stacked_rows(D)]
    np.add.at(R_, D.stacked.indices[on], fixed[on])
    return (R_.astype(np.float64) * np.ldexp(1.0, -e)).astype(F)


def forward(x, D, s_hist, c0, v0, a0, p, e):
    """``x [T, B, N]``; ``s_hist [A, B, N]`` (``0 <= A <= depth``) or None; ``c0`` / ``v0`` / ``a0 [B, N]`` or None ->
    ``lif_rec_sg_cases.Forward`` (``r [T, B, N]``: the recurrent input of every step)."""
    assert x.dtype == F and x.ndim == 3 and x.shape[2] == D.m.n
    assert s_hist is None or (s_hist.ndim == 3 and s_hist.shape[0] <= D.depth and s_hist.shape[1:] == x.shape[1:])
    T, B, N = x.shape
    fixed = fixed_from_f32(D.stacked.w, e)
    flat = lambda a: None if a is None else a.reshape(-1)
    c, v, a = flat(c0), flat(v0), flat(a0) if p.adaptive else None
    s_out, v_seq, h_save, th_save, r_all = (np.zeros_like(x) for _ in range(5))
    for t in range(T):
        act = active_rows(s_out, s_hist, t, D.depth)
        r = np.stack([recurrent_input(D, fixed, act[b], e) for b in range(B)]) if B else np.zeros((0, N), F)
        xin = x[t] + r
        assert xin.dtype == F
        f = S.forward(xin.reshape(1, -1), c, v, a, p)
        c, v, a = f.c_last, f.v_last, f.a_last
        s_out[t], v_seq[t], h_save[t], r_all[t] = f.s_out.reshape(B, N), f.v_seq.reshape(B, N), f.h_save.reshape(B, N), r
        if p.adaptive:
            th_save[t] = f.th_save.reshape(B, N)
    if T == 0:
        z = np.zeros(B * N, F)
        c, v, a = (z if c is None else c), (z if v is None else v), ((z if a is None else a) if p.adaptive else None)
    shape = lambda q: None if q is None else q.reshape(B, N)
    return Forward(s_out, v_seq, h_save, th_save if p.adaptive else None, shape(c), shape(v), shape(a), r_all)


# ------------------------------------------------------------------------------------------------ the backward pass
def aged_gather(D, g_x, bound, t, only=None):
    """``sum over d (ascending, from +0) with 0 <= t + 1 + d <= T - 1 of gather(rows of delay d, g_x[t + 1 + d])`` in f32 ->
    ``(out [B, N], its bound, sum |w * G|, the number of terms)``; ``t = -1 - a`` gives ``g_s_hist[a]``.  ``only``: a deliberately
    wrong variant that keeps the one delay given."""
    T, B, N = g_x.shape
    out = np.zeros((B, N), F)
    err, mag, terms = np.zeros((B, N)), np.zeros((B, N)), 0
    for d in range(max(0, -1 - t), min(D.depth - 1, T - 2 - t) + 1):
        if only is not None and d != only:
            continue
        g, e, m = R.gather(of_delay(D, d), g_x[t + 1 + d], bound[t + 1 + d])
        out = out + g
        err, mag, terms = err + e, mag + m, terms + 1
    assert out.dtype == F
    return out, err + terms * EPS * mag, mag, terms


def backward(h_save, th_save, D, g_s, g_vseq, g_clast, g_vlast, g_alast, p, hist_ages=0, with_bound=False, own_age_only=False):
    """``lif_rec_sg_cases.backward`` with ``g_rec`` the gather over the ages and ``g_s_hist [hist_ages, B, N]`` in the place of
    ``g_s0`` -> :class:`Backward`, and with ``with_bound`` a :class:`Bound`.  Per step the operations and their order are
    tests/lif_syn_sg_cases.py's ``backward``.  ``own_age_only``: the deliberately wrong ``g_s_hist`` without its ``d > a`` terms."""
    assert h_save.dtype == F and h_save.ndim == 3
    syn_decay, beta, v_th, v_reset, rho, kappa = (F(c) for c in (p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa))
    T, B, N = h_save.shape
    hard = p.reset == 'hard'
    start = lambda g: np.zeros((B, N), F) if g is None else g.copy()
    cc, cv, ca = start(g_clast), start(g_vlast), start(g_alast)
    g_x = np.zeros_like(h_save)
    bound, terms_x = np.zeros((T, B, N)), np.zeros((T, B, N))
    e_c, e_v, e_a = np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N))
    eps4 = 4.0 * EPS
    a = lambda z: np.abs(np.asarray(z, np.float64))
    with np.errstate(all='ignore'):
        for t in range(T - 1, -1, -1):
            h = h_save[t]
            th = th_save[t] if p.adaptive else np.full((B, N), v_th, F)
            s = h >= th
            u = h - th
            g_vo = cv
            if g_vseq is not None:
                g_vo = cv + g_vseq[t]
            sg = S.surrogate(u, p)
            g_sp = np.zeros((B, N), F) if g_s is None else g_s[t]
            e_r, mag_r = np.zeros((B, N)), np.zeros((B, N))
            if t < T - 1:
                g_rec, e_r, mag_r, _ = aged_gather(D, g_x, bound, t)
                g_sp = g_sp + g_rec
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
                reach = np.zeros((B, N)) if p.detach_reset else (a(h) + a(v_reset) if hard else np.full((B, N), a(v_th)))
                terms_u = (a(0 if g_s is None else g_s[t]) + mag_r + (a(ca_in) if p.adaptive else 0.0) + a(g_vo) * reach) * a(sg)
                carried = (e_r + e_a + e_v * reach) * a(sg)
                err_u = eps4 * terms_u + carried
                coef = np.where(s, 0.0, 1.0) if hard else np.ones((B, N))
                terms_h = terms_u + a(through)
                err_h = eps4 * terms_h + carried + e_v * coef
                terms_x[t] = terms_h + a(cc_in)
                bound[t] = eps4 * terms_x[t] + (err_h - eps4 * terms_h) + e_c
                e_c = a(syn_decay) * bound[t]
                e_v = a(beta) * err_h
                if p.adaptive:
                    e_a = a(rho) * e_a + a(kappa) * err_u + eps4 * (a(rho) * a(ca_in) + a(kappa) * a(g_u))
    g_hist, e_hist = np.zeros((hist_ages, B, N), F), np.zeros((hist_ages, B, N))
    for age in range(hist_ages):
        g_hist[age], e_hist[age], _, _ = aged_gather(D, g_x, bound, -1 - age, only=age if own_age_only else None)
    out = Backward(g_x, cc, cv, ca if p.adaptive else None, g_hist)
    if with_bound:
        # the three carries come out as rounded products of results that may differ by their bounds: one more rounding each (ca:
        # two products and a difference) — inside the loop the next step's own 4 * 2**-24 covers it, after the last step nothing does
        e_c, e_v, e_a = e_c + EPS * a(cc), e_v + EPS * a(cv), e_a + 3 * EPS * (a(ca) if T else 0.0)
        return out, Bound(bound, e_c, e_v, e_a if p.adaptive else None, e_hist, terms_x)
    return out


# ------------------------------------------------------------------------------------------------ the weight gradient
def weight_grad(D, s_out, s_hist, g_x, g_x_bound=None, late=0):
    """In the order of ``stacked.w``: ``g_w[k] = sum over t, b of sp(t - 1 - d)[b][i] * g_x[t][b][col k]`` for ``k`` in stacked row
    ``d * N + i``, in f32 over the active ``(t, b)`` in ascending order — ``be_grad_rows``' order.  With ``g_x_bound`` also its bound:
    ``(number of active rows) * 2**-24 * sum |terms| + sum (bound of the terms)``.  ``late``: see :func:`active_rows`."""
    T, B, N = s_out.shape
    rows, st = stacked_rows(D), D.stacked
    nse = len(st.w)
    g_w = np.zeros(nse, F)
    mag, carried, count = np.zeros(nse), np.zeros(nse), np.zeros(nse)
    for t in range(T):
        act = active_rows(s_out, s_hist, t, D.depth, late)
        for b in range(B):
            on = act[b][rows]
            term = g_x[t, b][st.indices]
            g_w = np.where(on, g_w + term, g_w).astype(F)
            mag += np.where(on, np.abs(term.astype(np.float64)), 0.0)
            count += on
            if g_x_bound is not None:
                carried += np.where(on, g_x_bound[t, b][st.indices], 0.0)
    if g_x_bound is None:
        return g_w
    return g_w, count * EPS * mag + carried


def aged_mask(s_out, s_hist, depth):
    """``be_grad_pack_activity_aged``: uint32 ``[depth * N, ceil(T * B / 32)]``, bit ``p % 32`` of word ``p // 32`` of row
    ``d * N + i``, ``p = t * B + b``, is ``sp(t - 1 - d)[b][i]``."""
    T, B, N = s_out.shape
    nb = T * B
    bits = np.zeros((depth * N, (nb + 31) // 32 * 32), np.uint64)
    for t in range(T):
        act = active_rows(s_out, s_hist, t, depth)
        for b in range(B):
            bits[:, t * B + b] = act[b]
    return (bits.reshape(depth * N, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def history(A, B, N, seed, rate=0.2):
    """``s_hist [A, B, N]`` (f32 zeros and ones) or None for ``A = 0``."""
    if A == 0:
        return None
    return (np.random.default_rng(seed).random((A, B, N)) < rate).astype(F)
