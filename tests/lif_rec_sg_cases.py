"""Shared by tests/test_lif_rec_sg_cpu.py and tests/test_lif_rec_sg_gpu.py: a numpy restatement of the two passes of the fused
recurrent spiking layer (include/brainevent_amd.h, be_lif_rec_sg_forward / be_lif_rec_sg_backward; csrc/be_neuron_sg_rec.hip;
DESIGN.md §2.22), seeded inputs and the matrices the tests use.

Forward: the recurrent sums are 64-bit wrapping integers (``np.int64`` with ``np.add.at``: order independent) of the fixed-point
encoding restated operation by operation in f32 (:func:`fixed_from_f32`), and the neuron's step is tests/lif_syn_sg_cases.py's
``forward`` on one step — so the device's forward outputs are compared as equalities.  Backward: f32, the gather as a plain
ascending sum (the device's order is its own), with a propagated bound in the manner of ``lif_syn_sg_cases.backward(with_bound=
True)``: the gather of row ``i`` adds ``(len(row i) + 1) * 2**-24 * sum_k |w[k] * G[col k]|`` — a sum of ``len`` rounded products
in any order — plus ``sum_k |w[k]| * (the bound of G[col k])`` to the bound of ``g_sp``, which then travels through the three
carries and through the earlier steps' gathers; ``sum_k |w[k] * G[col k]|`` also joins the terms the step's own ``4 * 2**-24``
is relative to (``g_rec`` is one more addend of ``g_sp``)."""
import collections

import numpy as np

import lif_syn_sg_cases as S
from lif_syn_sg_cases import F, Params, same_bits, surrogate  # noqa: F401  (for the tests that import this module)

#: the constants of csrc/be_neuron_sg_rec.hip the GPU sizes are derived from
CONSTS = {'kRecThreads': 1024, 'kRecMaxN': 8192, 'kRecRowLanes': 16, 'kRecUnroll': 4}
#: one neuron, a wave less one, a wave, a wave and one, past a quarter of the workgroup, one neuron past the workgroup
N_SIZES = (1, 63, 64, 65, 257, 1025)
B_SIZES = (1, 3)
T_SIZES = (1, 2, 3, 5)
MODES = S.MODES
EPS = 2.0 ** -24

Matrix = collections.namedtuple('Matrix', 'w indices indptr n')
Forward = collections.namedtuple('Forward', 's_out v_seq h_save th_save c_last v_last a_last r')
Backward = collections.namedtuple('Backward', 'g_x g_c0 g_v0 g_a0 g_s0')
Bound = collections.namedtuple('Bound', 'g_x g_c0 g_v0 g_a0 g_s0 terms')


# ------------------------------------------------------------------------------------------------ matrices
def _matrix(w, indices, counts, n):
    indptr = np.zeros(n + 1, np.int32)
    np.cumsum(counts, out=indptr[1:])
    assert indptr[-1] == len(w) == len(indices)
    return Matrix(np.asarray(w, F), np.asarray(indices, np.int32), indptr, n)


def random_matrix(n, seed, lo=1, hi=8, sigma=0.05):
    """``lo`` .. ``hi`` entries per row at random columns (duplicates and self-loops happen), N(0, sigma) weights."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(lo, hi + 1, n)
    nse = int(counts.sum())
    return _matrix(rng.normal(0.0, sigma, nse), rng.integers(0, n, nse), counts, n)


def dyadic_matrix(n, seed, lo=1, hi=8):
    """The same structure with weights that are multiples of 2**-6 in [-1/4, 1/4]: every sum of them is exact in f32 in any
    order, and in fixed point at any exponent >= 6."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(lo, hi + 1, n)
    nse = int(counts.sum())
    return _matrix(rng.integers(-16, 17, nse) / 64.0, rng.integers(0, n, nse), counts, n)


def empty_matrix(n):
    return _matrix([], [], np.zeros(n, np.int64), n)


def crafted_matrix(n=300, seed=5, long_row=600):
    """Row 0 empty; row 1 a self-loop alone; row 2 lists column 7 five times (and column 2 once: a self-loop among duplicates);
    row 3 has ``long_row`` entries — more than the workgroup has row lanes to give and, at 600, more than N; rows 5 and 6 have 65 and
    64 entries — one past, and exactly, what a row's lanes take in one trip (kRecUnroll * kRecRowLanes); every fourth row from row
    4 on is empty, the others have 1 .. 8 entries."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 9, n)
    counts[0], counts[1], counts[2], counts[3] = 0, 1, 6, long_row
    counts[5], counts[6] = 65, 64
    counts[4::4] = 0
    nse = int(counts.sum())
    indices = rng.integers(0, n, nse)
    start = np.concatenate(([0], np.cumsum(counts)))
    indices[start[1]] = 1
    indices[start[2]:start[3]] = [7, 7, 2, 7, 7, 7]
    return _matrix(rng.normal(0.0, 0.05, nse), indices, counts, n)


def rows_of(m):
    return np.repeat(np.arange(m.n), np.diff(m.indptr))


def dense(m):
    """``W [N, N]`` in f64 (duplicates summed)."""
    out = np.zeros((m.n, m.n))
    np.add.at(out, (rows_of(m), m.indices), m.w.astype(np.float64))
    return out


def exponent(m):
    """An exponent no sum can overflow at, by ``be_fixed_point_exponent``'s rule: the largest column sum of ``|w|`` times 1.001
    stays below ``2**(62 - e)`` (f64 sums here: the device's f32 sums may land one lower at a power of two)."""
    col = np.zeros(max(m.n, 1))
    np.add.at(col, m.indices, np.abs(m.w.astype(np.float64)))
    bound = col.max() * 1.001
    eb = int(np.frexp(bound)[1]) if bound > 0 else 0
    return int(np.clip(62 - eb, -90, 150))


# ------------------------------------------------------------------------------------------------ the forward pass
def fixed_from_f32(w, e):
    """csrc/be_common.h ``fixed_from_f32`` operation by operation: ``t = w * 2**(e - 32)``, ``hf = floor(t)``, the high word
    ``(int32)hf``, the low word ``(uint32)((t - hf) * 2**32)`` — as one ``int64`` per weight."""
    assert w.dtype == F
    scale = F(np.ldexp(1.0, e - 32))
    assert np.isfinite(scale) and scale >= np.finfo(F).tiny
    t = w * scale
    hf = np.floor(t)
    frac = t - hf
    low = frac * F(4294967296.0)
    assert t.dtype == hf.dtype == frac.dtype == low.dtype == F
    assert (np.abs(hf) < 2.0 ** 31).all() and (low < 2.0 ** 32).all() and (low >= 0).all()
    hi = hf.astype(np.int64)
    lo = low.astype(np.uint64).astype(np.int64)
    return (hi << 32) | lo


def recurrent_input(m, fixed, active, e):
    """``r [N]`` of one sample: the 64-bit wrapping sum of the fixed-point weights of the active rows, per column, scaled back in
    f64 and rounded to f32 once."""
    R = np.zeros(m.n, np.int64)
    on = active[rows_of(m)]
    np.add.at(R, m.indices[on], fixed[on])
    inv = np.ldexp(1.0, -e)
    return (R.astype(np.float64) * inv).astype(F)


def forward(x, m, s0, c0, v0, a0, p, e):
    """``x [T, B, N]``; ``s0`` / ``c0`` / ``v0`` / ``a0 [B, N]`` or None -> :class:`Forward` (``r [T, B, N]``: the recurrent input
    of every step, for the tests' own assertions)."""
    assert x.dtype == F and x.ndim == 3 and x.shape[2] == m.n
    T, B, N = x.shape
    fixed = fixed_from_f32(m.w, e)
    flat = lambda a: None if a is None else a.reshape(-1)
    c, v, a = flat(c0), flat(v0), flat(a0) if p.adaptive else None
    sp = np.zeros((B, N), bool) if s0 is None else (s0 != 0)
    outs = [np.empty_like(x) for _ in range(5)]
    s_out, v_seq, h_save, th_save, r_all = outs
    for t in range(T):
        r = np.stack([recurrent_input(m, fixed, sp[b], e) for b in range(B)]) if B else np.zeros((0, N), F)
        xin = x[t] + r
        assert xin.dtype == F
        f = S.forward(xin.reshape(1, -1), c, v, a, p)
        c, v, a = f.c_last, f.v_last, f.a_last
        s_out[t], v_seq[t], h_save[t], r_all[t] = f.s_out.reshape(B, N), f.v_seq.reshape(B, N), f.h_save.reshape(B, N), r
        if p.adaptive:
            th_save[t] = f.th_save.reshape(B, N)
        sp = s_out[t] != 0
    if T == 0:
        z = np.zeros(B * N, F)
        c, v, a = (z if c is None else c), (z if v is None else v), ((z if a is None else a) if p.adaptive else None)
    shape = lambda q: None if q is None else q.reshape(B, N)
    return Forward(s_out, v_seq, h_save, th_save if p.adaptive else None, shape(c), shape(v), shape(a), r_all)


# ------------------------------------------------------------------------------------------------ the backward pass
def gather(m, G, G_bound=None):
    """``out[b, i] = sum over row i of w[k] * G[b, col k]`` in f32, each product rounded, summed in ascending ``k``; with
    ``G_bound`` also the bound of the result: ``(len + 1) * 2**-24 * sum |w * G| + sum |w| * G_bound`` and ``sum |w * G|``."""
    B, N = G.shape
    rows = rows_of(m)
    out = np.zeros((B, N), F)
    prod = m.w[None, :] * G[:, m.indices]
    assert prod.dtype == F
    longest = int(np.diff(m.indptr).max()) if N else 0
    start = m.indptr[:-1]
    length = np.diff(m.indptr)
    for j in range(longest):                     # the j-th entry of every row that has one
        has = np.flatnonzero(length > j)
        out[:, has] = out[:, has] + prod[:, start[has] + j]
    assert out.dtype == F
    if G_bound is None:
        return out
    mag, carried = np.zeros((B, N)), np.zeros((B, N))
    aw = np.abs(m.w.astype(np.float64))
    for b in range(B):
        mag[b] = np.bincount(rows, weights=np.abs(prod[b].astype(np.float64)), minlength=N)
        carried[b] = np.bincount(rows, weights=aw * G_bound[b, m.indices], minlength=N)
    return out, (length[None, :] + 1) * EPS * mag + carried, mag


def backward(h_save, th_save, m, g_s, g_vseq, g_clast, g_vlast, g_alast, p, with_bound=False):
    """``h_save`` / ``th_save`` / ``g_s`` / ``g_vseq [T, B, N]``, ``g_clast`` / ``g_vlast`` / ``g_alast [B, N]`` (gradients may be
    None) -> :class:`Backward`, and with ``with_bound`` a :class:`Bound` (see the module's docstring).  Per step the operations
    and their order are tests/lif_syn_sg_cases.py's ``backward``, with ``g_sp = g_s[t] + g_rec`` for ``t < T - 1``."""
    assert h_save.dtype == F and h_save.ndim == 3
    syn_decay, beta, v_th, v_reset, rho, kappa = (F(c) for c in (p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa))
    T, B, N = h_save.shape
    hard = p.reset == 'hard'
    start = lambda g: np.zeros((B, N), F) if g is None else g.copy()
    cc, cv, ca = start(g_clast), start(g_vlast), start(g_alast)
    g_x = np.empty_like(h_save)
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
            sg = surrogate(u, p)
            g_sp = np.zeros((B, N), F) if g_s is None else g_s[t]
            e_r, mag_r = np.zeros((B, N)), np.zeros((B, N))
            if t < T - 1:
                g_rec, e_r, mag_r = gather(m, g_x[t + 1], bound[t + 1])
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
    if T > 0:
        g_s0, e_s0, _ = gather(m, g_x[0], bound[0])
    else:
        g_s0, e_s0 = np.zeros((B, N), F), np.zeros((B, N))
    out = Backward(g_x, cc, cv, ca if p.adaptive else None, g_s0)
    if with_bound:
        return out, Bound(bound, e_c, e_v, e_a if p.adaptive else None, e_s0, terms_x)
    return out


def weight_grad(m, s_out, s0, g_x, g_x_bound=None):
    """``g_w[k] = sum over t, b of sp[t][b][row k] * g_x[t][b][col k]``, ``sp = cat(s0, s_out[:-1])`` (``s0`` None: from step 1),
    in f32 over the active batch rows in ascending ``(t, b)`` — ``be_grad_rows``' order.  With ``g_x_bound`` also its bound:
    ``(number of active rows) * 2**-24 * sum |terms| + sum (bound of the terms)``."""
    T, B, N = s_out.shape
    if s0 is None:
        sp, g = s_out[:max(T - 1, 0)] != 0, g_x[1:]
        gb = None if g_x_bound is None else g_x_bound[1:]
    else:
        sp, g = np.concatenate(((s0 != 0)[None], s_out[:max(T - 1, 0)] != 0)), g_x
        gb = g_x_bound
    rows = rows_of(m)
    g_w = np.zeros(len(m.w), F)
    mag, carried, count = np.zeros(len(m.w)), np.zeros(len(m.w)), np.zeros(len(m.w))
    for t in range(sp.shape[0]):
        for b in range(B):
            on = sp[t, b][rows]
            term = g[t, b][m.indices]
            g_w = np.where(on, g_w + term, g_w).astype(F)
            mag += np.where(on, np.abs(term.astype(np.float64)), 0.0)
            count += on
            if gb is not None:
                carried += np.where(on, gb[t, b][m.indices], 0.0)
    if g_x_bound is None:
        return g_w
    return g_w, count * EPS * mag + carried


# ------------------------------------------------------------------------------------------------ inputs
def inputs(T, B, N, seed):
    """Seeded ``x [T, B, N]``, ``s0 [B, N]`` (a fifth active), the start state ``c0`` / ``v0`` / ``a0 [B, N]`` and the five output
    gradients in ``lif_syn_sg_cases.GRADS``' order."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.12, 0.25, (T, B, N)).astype(F)
    s0 = (rng.random((B, N)) < 0.2).astype(F)
    c0 = rng.normal(0.2, 0.3, (B, N)).astype(F)
    v0 = rng.normal(0.3, 0.5, (B, N)).astype(F)
    a0 = np.abs(rng.normal(0.5, 0.5, (B, N))).astype(F)
    g_s, g_vseq = rng.normal(0, 1, (T, B, N)).astype(F), rng.normal(0, 1, (T, B, N)).astype(F)
    g_clast, g_vlast, g_alast = (rng.normal(0, 1, (B, N)).astype(F) for _ in range(3))
    return x, s0, (c0, v0, a0), (g_s, g_vseq, g_clast, g_vlast, g_alast)
