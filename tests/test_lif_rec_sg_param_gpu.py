"""The fused recurrent layer with per-neuron, learnable parameters (csrc/be_neuron_sg_rec.hip, be_lif_rec_sg_forward_params /
be_lif_rec_sg_backward_params; brainevent_amd/_neuron_rec_sg.py, parametric_recurrent_lif_sequence) on the device, compared with the
numpy restatement of tests/lif_rec_sg_param_cases.py.  Forward outputs and the saved ``h`` / ``a_save`` / ``c_save`` are EQUALITIES, bit
for bit.  Backwards, everything is an equality wherever the restatement's order is the kernel's — one step, an empty matrix, a
matrix with one entry per row (a gather of one product has no order) — the five accumulators included; gradients that pass through
a gather of several products lie within the restatement's propagated bound.  Nothing is compared with torch's device kernels.
tests/test_lif_rec_sg_param_cpu.py holds the restatement to CPU autograd."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_rec_sg_param_cases as Q
import lif_syn_sg_cases as S
from lif_rec_sg_param_cases import F, Params, same_bits

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ALL = Q.GRAD_SETS['all']
STATE_OUT = ('g_c0', 'g_v0', 'g_a0', 'g_s0')
SLOT_OUT = Q.SLOTS
RESET = {'hard': 0, 'soft': 1}
SURROGATE = {'fast_sigmoid': 0, 'atan': 1, 'triangle': 2}
INVALID, RANGE = -1, -4


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()          # (a copy: the shared inputs are read-only)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def full(shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device='cuda')


@functools.lru_cache(maxsize=None)
def case(T, B, N, seed):
    x, s0, state, grads = Q.inputs(T, B, N, seed)
    for a in (x, s0) + state + grads:
        a.setflags(write=False)
    return x, s0, state, grads


@functools.lru_cache(maxsize=None)
def matrix(kind, N, seed=0):
    """One of the test matrices and an exponent no sum of it can overflow at (shared and left unchanged)."""
    build = {'random': lambda: Q.random_matrix(N, seed), 'dyadic': lambda: Q.dyadic_matrix(N, seed), 'empty': lambda: Q.empty_matrix(N),
             'crafted': lambda: Q.crafted_matrix(N), 'one': lambda: Q.one_entry_matrix(N, seed)}
    m = build[kind]()
    return m, (Q.exponent(m) - 1 if len(m.w) else 0)       # one below the restatement's own rule: what the library may choose


@functools.lru_cache(maxsize=None)
def params(pattern, N, seed=0):
    q = Q.param_inputs(Q.periods(pattern, N), seed)
    for a in q:
        a.setflags(write=False)
    return q


class DevMatrix:
    def __init__(self, m):
        self.w = dev(m.w) if len(m.w) else torch.zeros(1, device='cuda')
        self.indices = dev(m.indices) if len(m.w) else torch.zeros(1, dtype=torch.int32, device='cuda')
        self.indptr = dev(m.indptr)


def within(got, want, bound, what):
    got = host(got).astype(np.float64).reshape(np.shape(want))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, 'a NaN is a NaN in both, and nowhere else')
    err = np.where(nan, 0.0, np.abs(got - want))
    assert (err <= np.where(nan, 0.0, bound)).all(), (what, float(err.max()), float(np.asarray(bound).flat[err.argmax()]))


def period_args(A, dq):
    return [v for t in dq for v in (A.ptr(t), 1 if t is None else t.numel())]


# ======================================================================================================== the direct C call
class Direct:
    """``be_lif_rec_sg_forward_params`` on device copies of the inputs, then any number of ``be_lif_rec_sg_backward_params`` calls on
    what it saved; every output is compared with the restatement.  Every output buffer starts filled with SENTINEL; without
    adaptation the adaptation's buffers and parameters are passed all the same and must stay untouched."""

    def __init__(self, m, e, p, q, x, s0, state, save=True, want_v=True, want_c=True):
        from brainevent_amd import _array as A, _lib
        T, B, N = x.shape
        self.A, self.lib, self.dims, self.p, self.q, self.m, self.dm = A, _lib, (T, B, N), p, q, m, DevMatrix(m)
        self.state = state
        self.ref = Q.forward(x, m, s0, state[0], state[1], state[2] if p.adaptive else None, q, p, e)
        self.dq = [dev(a) for a in q]
        self.dstate = [dev(a) for a in state]
        ins = [dev(x), self.dm.w, self.dm.indices, self.dm.indptr, dev(s0)] + self.dstate
        self.s_out, self.v_seq, self.h_save, self.c_save, self.a_save = (full((T, B, N)) for _ in range(5))
        self.c_last, self.v_last, self.a_last = (full((B, N)) for _ in range(3))
        outs = [self.s_out, self.v_seq if want_v else None, self.h_save if save else None, self.c_save if want_c else None,
                self.a_save if save else None, self.c_last, self.v_last, self.a_last]
        rc = _lib.fn('be_lif_rec_sg_forward_params')(*[A.ptr(t) for t in ins], *period_args(A, self.dq), *[A.ptr(t) for t in outs], T, B,
                                                     N, p.v_reset, RESET[p.reset], int(p.adaptive), e, A.stream_ptr())
        assert rc == 0, _lib.last_error()
        r, what = self.ref, (self.dims, p)
        assert same_bits(host(self.s_out), r.s_out) and same_bits(host(self.c_last), r.c_last), what
        assert same_bits(host(self.v_last), r.v_last), what
        self.same_or_untouched(self.v_seq, r.v_seq if want_v else None, what)
        self.same_or_untouched(self.h_save, r.h_save if save else None, what)
        self.same_or_untouched(self.c_save, r.c_save if want_c else None, what)
        self.same_or_untouched(self.a_save, r.a_save if save else None, what)
        self.same_or_untouched(self.a_last, r.a_last, what)

    @staticmethod
    def same_or_untouched(t, ref, what):
        if ref is None:
            assert bool((t == SENTINEL).all()), what
        else:
            assert same_bits(host(t), ref), what

    def backward(self, grads, use=ALL, null=(), slots=SLOT_OUT, exact=False, state0=True):
        """One backward call: ``use`` picks the gradients that arrive, ``null`` names the state outputs not asked for, ``slots`` the
        accumulators that are; ``exact``: the restatement's order is the kernel's, everything is compared bit for bit."""
        A, (T, B, N), p, dm = self.A, self.dims, self.p, self.dm
        given = S.pick(grads, use, p)
        c0, v0 = (self.state[0], self.state[1]) if state0 else (None, None)
        r, info = Q.backward(self.ref.h_save, self.ref.c_save, self.ref.a_save, self.m, c0, v0, *given, self.q, p, with_bound=True)
        ins = [dev(g if u else None) for g, u in zip(grads, use)]
        g_x = full((T, B, N))
        outs = [full((B, N)) for _ in STATE_OUT]
        acc = [full((B, N)) for _ in SLOT_OUT]
        rc = self.lib.fn('be_lif_rec_sg_backward_params')(
            A.ptr(self.h_save), A.ptr(self.c_save), A.ptr(self.a_save), A.ptr(self.dstate[0] if state0 else None),
            A.ptr(self.dstate[1] if state0 else None), A.ptr(dm.w), A.ptr(dm.indices), A.ptr(dm.indptr), *[A.ptr(t) for t in ins],
            *period_args(A, self.dq), A.ptr(g_x), *[A.ptr(None if n in null else t) for n, t in zip(STATE_OUT, outs)],
            *[A.ptr(t if n in slots else None) for n, t in zip(SLOT_OUT, acc)], T, B, N, p.v_reset, RESET[p.reset],
            SURROGATE[p.surrogate], p.alpha, int(p.adaptive), int(p.detach_reset), A.stream_ptr())
        assert rc == 0, self.lib.last_error()
        what = (self.dims, p, use, null, slots)
        if exact:
            assert same_bits(host(g_x), r.g_x), what
        within(g_x, r.g_x, info['g_x'], ('g_x',) + what)
        for n, t, want in zip(STATE_OUT, outs, r[1:5]):
            if n in null or want is None:
                assert bool((t == SENTINEL).all()), (n,) + what
            elif exact and (n != 'g_s0' or np.diff(self.m.indptr).max() <= 1):   # g_s0 is a gather even after one step
                assert same_bits(host(t), want), (n,) + what
            else:
                within(t, want, info[n], (n,) + what)
        for n, name, t, want in zip(SLOT_OUT, Q.NAMES, acc, r[5:]):
            if n not in slots or want is None:
                assert bool((t == SENTINEL).all()), (n,) + what
            elif exact:
                assert same_bits(host(t), want), (n,) + what
            else:
                within(t, Q.param_exact(info, name, B * N).reshape(B, N), Q.param_bound(info, name, B * N).reshape(B, N), (n,) + what)
        return r, info, g_x, acc


# ======================================================================================================== sizes
@pytest.mark.parametrize('N', Q.N_SIZES)
def test_sizes(be, N):
    """One neuron, a wave less one, a wave, a wave and one, 257, one past the workgroup (a thread's second neuron); 1 and 3 samples
    (an accumulator indexed without the sample shows at 3); 1, 2, 3 and 5 steps (one step has no t - 1); five period patterns; s0
    given and NULL; general weights within the bound, one entry per row bit for bit."""
    ps = (Params(adaptive=True), Params(reset='soft', surrogate='atan', v_reset=-0.25), Params(adaptive=True, reset='soft'))
    f = r = None
    for k, (B, T, kind) in enumerate(itertools.product(Q.B_SIZES, Q.T_SIZES, ('random', 'one'))):
        m, e = matrix(kind, N)
        x, s0, state, grads = case(T, B, N, 0)
        d = Direct(m, e, ps[k % 3], params(Q.PATTERNS[k % 5], N), x, s0 if (k // 2) % 2 == 0 else None, state)
        f, (r, _, _, _) = d.ref, d.backward(grads, exact=(kind == 'one' or T == 1))
    assert N < 8 or (0 < f.s_out.mean() < 1 and np.abs(r.g_x).max() > 0 and np.count_nonzero(r.g_beta_slot) > 0)


def test_the_limit(be):
    """N = kRecMaxN once (96 KB of LDS forwards, all eight neurons of a thread); one more is refused with BE_ERR_RANGE by both."""
    from brainevent_amd import _array as A, _lib
    N = Q.CONSTS['kRecMaxN']
    m, e = matrix('random', N)
    x, s0, state, grads = case(2, 1, N, 0)
    d = Direct(m, e, Params(adaptive=True), params('NNNNN', N), x, s0, state)
    r = d.backward(grads)[0]
    assert 0.05 < d.ref.s_out.mean() < 0.6 and np.count_nonzero(d.ref.r[1]) > N // 4 and np.abs(r.g_s0).max() > 0
    assert all(np.count_nonzero(s[0, -1024:]) > 0 for s in r[5:])                  # the eighth neuron of the threads
    P, st, t = A.ptr, A.stream_ptr(), full((2, 1, N + 1))
    dm = DevMatrix(Q.empty_matrix(N + 1))
    one = torch.ones(1, device='cuda')
    five = [v for _ in range(5) for v in (P(one), 1)]
    rc = _lib.fn('be_lif_rec_sg_forward_params')(P(t), P(dm.w), P(dm.indices), P(dm.indptr), P(None), P(None), P(None), P(None), *five,
                                                 P(t), P(None), P(None), P(None), P(None), P(t[0]), P(t[0]), P(None), 2, 1, N + 1, 0.0,
                                                 0, 0, 0, st)
    assert rc == RANGE and '8192' in _lib.last_error() and _lib.last_error().startswith('be_lif_rec_sg_forward_params: ')
    rc = _lib.fn('be_lif_rec_sg_backward_params')(P(t), P(None), P(None), P(None), P(None), P(dm.w), P(dm.indices), P(dm.indptr),
                                                  P(None), P(None), P(None), P(None), P(None), *five, P(t), *[P(None)] * 9, 2, 1,
                                                  N + 1, 0.0, 0, 0, 10.0, 0, 0, st)
    assert rc == RANGE and '8192' in _lib.last_error() and _lib.last_error().startswith('be_lif_rec_sg_backward_params: ')
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all())


@pytest.mark.parametrize('kind', ('crafted', 'empty'))
def test_matrices(be, kind):
    """Empty rows, a self-loop, a row listing one column five times, a long row; and no entry at all (bit for bit)."""
    m, e = matrix(kind, 300)
    for p, T, B, with_s0 in ((Params(adaptive=True), 5, 3, True), (Params(reset='soft', surrogate='triangle', alpha=2.0), 3, 1, False)):
        x, s0, state, grads = case(T, B, 300, 4)
        s0 = s0.copy()
        s0[:, :8] = 1                                                    # the crafted rows are active before step 0 ...
        x = x.copy()
        x[:, :, :8] += 2.0                                               # ... and at most steps
        d = Direct(m, e, p, params('N1N1N', 300), x, s0 if with_s0 else None, state)
        r = d.backward(grads, exact=(kind == 'empty'))[0]
        if kind == 'crafted':
            assert d.ref.s_out[:-1, :, :8].mean() > 0.5 and np.count_nonzero(d.ref.r) > 0 and np.count_nonzero(r.g_s0) > 0
        else:
            assert not d.ref.r.any() and not r.g_s0.any()


# ======================================================================================================== modes
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', Q.MODES)
def test_modes(be, reset, surrogate, detach, adaptive):
    p = S.mode_params(reset, surrogate, detach, adaptive)
    T, B, N = 3, 3, 65
    x, s0, state, grads = case(T, B, N, 7)
    for kind in ('random', 'one'):
        m, e = matrix(kind, N)
        d = Direct(m, e, p, params('NNNNN', N), x, s0, state)
        assert 0 < d.ref.s_out.mean() < 1
        r = d.backward(grads, exact=(kind == 'one'))[0]
        assert np.count_nonzero(r.g_x) > 0


# ======================================================================================================== outputs and pointers
@pytest.mark.parametrize('adaptive', (False, True))
def test_slot_outputs_and_pointers(be, adaptive):
    """Each accumulator alone, all and none, with the buffers not asked for untouched; the optional forward outputs; NULL c0 / v0 /
    a0 / s0 equal zeros."""
    T, B, N = 3, 2, 65
    m, e = matrix('one', N)
    x, s0, state, grads = case(T, B, N, 8)
    p, q = Params(adaptive=adaptive, reset='soft'), params('NN11N', N)
    for save, want_v, want_c in ((False, False, False), (True, False, True), (False, True, False)):
        Direct(m, e, p, q, x, s0, state, save=save, want_v=want_v, want_c=want_c)
    d = Direct(m, e, p, q, x, s0, state)
    for slots in [()] + [(n,) for n in SLOT_OUT] + [SLOT_OUT]:
        d.backward(grads, slots=slots, exact=True)
    d.backward(grads, null=STATE_OUT, slots=('g_beta_slot',), exact=True)
    for k in (1, 2):
        for null in itertools.combinations(STATE_OUT, k):
            d.backward(grads, null=null, exact=True)
    # c_save is not read unless g_sd_slot is given
    no_c = Direct(m, e, p, q, x, s0, state, want_c=False)
    no_c.c_save = None
    no_c.backward(grads, slots=SLOT_OUT[1:], exact=True)
    # a NULL state entry, s0 or gradient is zeros — in the accumulators too (c0 / v0 are what step 0 started from)
    zeros = np.zeros((B, N), F)
    a, b = Direct(m, e, p, q, x, None, (None, None, None)), Direct(m, e, p, q, x, zeros, (zeros, zeros, zeros))
    names = ('s_out', 'v_seq', 'h_save', 'c_save', 'c_last', 'v_last') + (('a_save', 'a_last') if adaptive else ())
    assert all(same_bits(host(getattr(a, n)), host(getattr(b, n))) for n in names)
    a.state = b.state = (zeros, zeros, zeros)
    ga = a.backward(grads, use=(True, False, False, False, False), exact=True, state0=False)
    gb = b.backward((grads[0], np.zeros_like(x), zeros, zeros, zeros), exact=True)
    assert same_bits(host(ga[2]), host(gb[2])) and all(same_bits(host(i), host(j)) for i, j in zip(ga[3][:3], gb[3][:3]))


# ======================================================================================================== thresholds and NaNs
def test_the_threshold_is_the_neurons_own(be):
    """Differing per-neuron thresholds and a per-neuron kappa: h == th_i spikes, one ulp under does not."""
    T, B, N = 1, 2, 65
    m, e = matrix('random', N)
    rng = np.random.default_rng(3)
    vth = rng.uniform(0.8, 1.2, N).astype(F)
    kap = rng.uniform(0.1, 0.5, N).astype(F)
    a0 = np.abs(rng.normal(0.5, 0.5, (B, N))).astype(F)
    th = (vth[None] + (kap[None] * a0).astype(F)).astype(F)
    x = np.empty((T, B, N), F)
    x[0, 0], x[0, 1] = th[0], np.nextafter(th[1], F(-np.inf))          # c0 = v0 = 0, no s0: h = (beta * 0) + ((sd * 0) + (x + 0)) = x
    q = (np.array([0.8], F), np.array([0.9], F), vth, np.array([0.95], F), kap)
    d = Direct(m, e, Params(adaptive=True), q, x, None, (None, None, a0))
    s = host(d.s_out)
    assert s[0, 0].all() and not s[0, 1].any() and same_bits(host(d.h_save), x)
    assert len(np.unique(th)) > N                                         # the thresholds differ


def test_a_nan_stays_where_it_is(be):
    """A NaN parameter stays in its neuron; a NaN in x stays in its sample."""
    T, B, N = 4, 3, 257
    m, e = matrix('empty', N)
    x, s0, state, grads = case(T, B, N, 9)
    p, q = Params(adaptive=True), params('NNNNN', N)
    clean = Direct(m, e, p, q, x, s0, state)
    g_clean = clean.backward(grads, exact=True)
    for k in range(5):                                                   # one parameter of neuron 5 (no recurrence: nothing spreads)
        bad = tuple(a.copy() for a in q)
        bad[k][5] = np.nan
        d = Direct(m, e, p, bad, x, s0, state)
        g = d.backward(grads, exact=True)
        others = np.arange(N) != 5
        for a, b in zip((d.s_out, d.v_seq, d.h_save, g[2]) + tuple(g[3]), (clean.s_out, clean.v_seq, clean.h_save, g_clean[2]) + tuple(g_clean[3])):
            assert same_bits(host(a)[..., others], host(b)[..., others]), k
        assert np.isnan(host(g[3][k])[:, 5]).all(), k
    m, e = matrix('random', N)                                           # with the recurrence: a sample is a workgroup of its own
    clean = Direct(m, e, p, q, x, s0, state)
    g_clean = clean.backward(grads)
    bad = x.copy()
    bad[1, 1, 5] = np.nan
    d = Direct(m, e, p, q, bad, s0, state)
    g = d.backward(grads)
    assert np.isnan(host(d.v_seq)[1:, 1, 5]).all() and np.isnan(host(g[2])[:, 1]).any()
    for other in (0, 2):
        for a, b in zip((d.s_out, d.v_seq, d.h_save, d.a_save, d.c_save, g[2]),
                        (clean.s_out, clean.v_seq, clean.h_save, clean.a_save, clean.c_save, g_clean[2])):
            assert same_bits(host(a)[:, other], host(b)[:, other])
        for a, b in zip((d.c_last, d.v_last, d.a_last) + tuple(g[3]), (clean.c_last, clean.v_last, clean.a_last) + tuple(g_clean[3])):
            assert same_bits(host(a)[other], host(b)[other])


# ======================================================================================================== C error codes
def test_c_error_codes_each_followed_by_a_clean_call(be):
    from brainevent_amd import _array as A, _lib
    fwd, bwd = _lib.fn('be_lif_rec_sg_forward_params'), _lib.fn('be_lif_rec_sg_backward_params')
    T, B, N = 3, 2, 64
    m, e = matrix('one', N)
    x, s0, state, grads = case(T, B, N, 0)
    p, q = Params(adaptive=True), params('N1N1N', N)
    ref = Q.forward(x, m, s0, *state, q, p, e)
    rb = Q.backward(ref.h_save, ref.c_save, ref.a_save, m, state[0], state[1], *grads, q, p)
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    dm = DevMatrix(m)
    ins = [dev(a) for a in (x, s0) + state]
    gin = [dev(g) for g in grads]
    dq = [dev(a) for a in q]
    big = [full((T, B, N)) for _ in range(6)]
    small = [full((B, N)) for _ in range(12)]
    s_out, v_seq, h_save, c_save, a_save, g_x = big
    c_last, v_last, a_last, g_c0, g_v0, g_a0, g_s0 = small[:7]
    acc = small[7:]

    def five(periods, nulls):
        return [v for k in range(5) for v in (null if k in nulls else P(dq[k]), periods[k] if k in periods else dq[k].numel())]

    def forward(x=P(ins[0]), w=P(dm.w), indices=P(dm.indices), indptr=P(dm.indptr), s_out=P(s_out), h_save=P(h_save), a_save=P(a_save),
                c_last=P(c_last), v_last=P(v_last), a_last=P(a_last), T=T, B=B, N=N, mode=0, adaptive=1, e=e, periods={}, nulls=()):
        return fwd(x, w, indices, indptr, P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), *five(periods, nulls), s_out, P(v_seq), h_save,
                   P(c_save), a_save, c_last, v_last, a_last, T, B, N, 0.0, mode, adaptive, e, st)

    def backward(h_save=P(h_save), c_save=P(c_save), a_save=P(a_save), w=P(dm.w), indices=P(dm.indices), indptr=P(dm.indptr),
                 g_x=P(g_x), T=T, B=B, N=N, mode=0, sur=0, alpha=10.0, adaptive=1, periods={}, nulls=()):
        return bwd(h_save, c_save, a_save, P(ins[2]), P(ins[3]), w, indices, indptr, *[P(g) for g in gin], *five(periods, nulls), g_x,
                   P(g_c0), P(g_v0), P(g_a0), P(g_s0), *[P(t) for t in acc], T, B, N, 0.0, mode, sur, alpha, adaptive, 0, st)

    # nothing to do: BE_OK and nothing written
    assert forward(T=0) == 0 and forward(B=0) == 0 and backward(T=0) == 0 and backward(B=0) == 0
    shared = {k: 1 for k in range(5)}
    assert forward(N=0, periods=shared) == 0 and backward(N=0, periods=shared) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in big + small)
    common = (dict(w=null), dict(indices=null), dict(indptr=null), dict(T=-1), dict(B=-1), dict(N=-1), dict(mode=2), dict(mode=-1),
              dict(nulls=(0,)), dict(nulls=(1,)), dict(nulls=(2,)), dict(nulls=(3,)), dict(nulls=(4,)))
    for bad in (dict(x=null), dict(s_out=null), dict(c_last=null), dict(v_last=null), dict(a_last=null), dict(a_save=null),
                dict(e=-91), dict(e=151)) + common:
        assert forward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_rec_sg_forward_params: '), _lib.last_error()
        assert forward() == 0                                                  # a clean call after each refused one
    for bad in (dict(h_save=null), dict(g_x=null), dict(a_save=null), dict(c_save=null), dict(sur=3), dict(sur=-1), dict(alpha=0.0),
                dict(alpha=float('nan'))) + common:
        assert backward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_rec_sg_backward_params: '), _lib.last_error()
        assert backward() == 0
    # a period is 1 or N: the message names the two
    for call in (forward, backward):
        for k, period in itertools.product(range(5), (0, -1, 2, N // 2, B * N, N + 1)):
            assert call(periods={k: period}) == INVALID, (k, period)
            assert 'period 1' in _lib.last_error() and f'period N = {N}' in _lib.last_error(), _lib.last_error()
            assert call() == 0
    assert forward(N=Q.CONSTS['kRecMaxN'] + 1) == RANGE and forward() == 0
    assert backward(N=Q.CONSTS['kRecMaxN'] + 1) == RANGE and backward() == 0
    # without adaptation the adaptation's pointers and periods are not looked at
    assert forward(adaptive=0, a_last=null, a_save=null, nulls=(3, 4), periods={3: 0, 4: 7}) == 0
    assert backward(adaptive=0, a_save=null, nulls=(3, 4), periods={3: 0, 4: 7}) == 0
    assert forward() == 0 and backward() == 0
    got = [host(t) for t in (s_out, v_seq, h_save, c_save, a_save, c_last, v_last, a_last)]
    assert all(same_bits(a, b) for a, b in zip(got, ref[:8]))
    for t, want in zip([g_x, g_c0, g_v0, g_a0, g_s0] + acc, rb):
        assert same_bits(host(t), want)


# ======================================================================================================== the Python function
def csr_of(be, m, requires_grad=False):
    w = dev(m.w).requires_grad_(requires_grad)
    return be.CSR((w, dev(m.indices), dev(m.indptr)), shape=(m.n, m.n)), w


def kwargs(p, tensors):
    """The keyword arguments of the call with the five parameters as given in ``tensors``."""
    kw = p.kwargs()
    kw.update(syn_decay=tensors[0], beta=tensors[1], v_th=tensors[2], adapt=(tensors[3], tensors[4]) if p.adaptive else None)
    return kw


@pytest.mark.parametrize('shape', ('0-d', '[1]', '[N]'))
@pytest.mark.parametrize('leaf', (True, False))
def test_parameter_gradients(be, monkeypatch, shape, leaf):
    """One entry per row, so the accumulators are the restatement's bit for bit: every parameter's gradient lies within the reduce's
    bound of the restatement's partials — a leaf and a non-leaf; 0-d, [1] and [N]; only what requires grad gets an accumulator."""
    from brainevent_amd import _neuron_rec_sg
    calls = []
    real = _neuron_rec_sg.call
    monkeypatch.setattr(_neuron_rec_sg, 'call', lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    T, B, N = 5, 3, 257
    m, e = matrix('one', N)
    x, s0, state, grads = case(T, B, N, 11)
    p = Params(adaptive=True, reset='soft')
    q = Q.param_inputs(((N if shape == '[N]' else 1),) * 5, 4)
    rec, w = csr_of(be, m, True)
    leaves = [dev(a.reshape(()) if shape == '0-d' else a).requires_grad_() for a in q]
    used = leaves if leaf else [t * 1.0 for t in leaves]                 # a non-leaf: the gradient flows on to the leaf
    xs = dev(x).requires_grad_()
    s, v_seq, last = be.parametric_recurrent_lif_sequence(xs, rec, tuple(dev(a) for a in state), dev(s0), return_v=True, scale_exp=e,
                                                          **kwargs(p, used))
    f = Q.forward(x, m, s0, *state, q, p, e)
    assert same_bits(host(s), f.s_out) and same_bits(host(v_seq), f.v_seq) and same_bits(host(last[2]), f.a_last)
    assert 0.05 < f.s_out.mean() < 0.6 and np.count_nonzero(f.r) > 0
    outs = (s, v_seq) + tuple(last)
    got = torch.autograd.grad(outs, [xs, w] + leaves, [dev(g) for g in grads])
    r, info = Q.backward(f.h_save, f.c_save, f.a_save, m, state[0], state[1], *grads, q, p, with_bound=True)
    assert same_bits(host(got[0]), r.g_x)
    within(got[1], *Q.weight_grad(m, f.s_out, s0, r.g_x, info['g_x']), 'w')
    for g, leaf_t, slot, name in zip(got[2:], leaves, r[5:], Q.NAMES):
        assert g.shape == leaf_t.shape and Q.within_reduce_bound(host(g), slot, leaf_t.numel()), name
        assert np.count_nonzero(slot) > 0
    assert calls[-2][0] == 'be_lif_rec_sg_backward_params' or calls[-1][0] == 'be_lif_rec_sg_backward_params'
    # only what requires grad gets an accumulator, seen at the call
    calls.clear()
    only = [t.detach() for t in leaves]
    only[1].requires_grad_()
    s, _ = be.parametric_recurrent_lif_sequence(dev(x), rec, None, dev(s0), scale_exp=e, **kwargs(p, only))
    g_beta, = torch.autograd.grad([s], [only[1]], [dev(grads[0])])
    name, a = next(c for c in calls if c[0] == 'be_lif_rec_sg_backward_params')
    assert [t.value is not None for t in a[28:33]] == [False, True, False, False, False]
    assert a[1].value is None and a[3].value is None                    # no c_save, no c0: syn_decay needs no gradient
    fwd = next(c for c in calls if c[0] == 'be_lif_rec_sg_forward_params')[1]
    assert fwd[21].value is None and fwd[20].value is not None and fwd[22].value is not None
    f = Q.forward(x, m, s0, None, None, None, q, p, e)
    r = Q.backward(f.h_save, f.c_save, f.a_save, m, None, None, grads[0], None, None, None, None, q, p)
    assert Q.within_reduce_bound(host(g_beta), r.g_beta_slot, only[1].numel())


@pytest.mark.parametrize('adaptive', (False, True))
def test_equals_the_loop_of_steps_and_products(be, adaptive):
    """Dyadic weights: forwards bit for bit the loop of ``parametric_synaptic_lif_step`` on ``x[t] + BinaryArray(s) @ rec``."""
    T, B, N = 5, 3, 257
    m, _ = matrix('dyadic', N)
    x, s0, state, grads = case(T, B, N, 11)
    p, q = Params(adaptive=adaptive), params('NNNNN', N, 1)
    n = 3 if adaptive else 2
    rec, _ = csr_of(be, m)
    dq = [dev(a) for a in q]
    with torch.no_grad():
        s, v_seq, last = be.parametric_recurrent_lif_sequence(dev(x), rec, tuple(dev(a) for a in state[:n]), dev(s0), return_v=True,
                                                              **kwargs(p, dq))
        st, sp, ss, vs = tuple(dev(a) for a in state[:n]), dev(s0), [], []
        for t in range(T):
            sp, st = be.parametric_synaptic_lif_step(st, dev(x[t]) + be.BinaryArray(sp) @ rec, **kwargs(p, dq))
            ss.append(sp)
            vs.append(st[1])
    for a, b in zip((s, v_seq) + tuple(last), (torch.stack(ss), torch.stack(vs)) + tuple(st)):
        assert same_bits(host(a), host(b))
    assert 0.05 < float(s.mean()) < 0.6


@pytest.mark.parametrize('adaptive', (False, True))
def test_one_element_tensors_are_recurrent_lif_sequence(be, adaptive):
    """Bit for bit in s, v_seq, the state, g_x and the state's gradients; and x [T, N] equals B = 1."""
    T, B, N = 4, 3, 65
    m, e = matrix('random', N)
    x, s0, state, grads = case(T, B, N, 12)
    p = Params(adaptive=adaptive, reset='soft', surrogate='atan')
    n = 3 if adaptive else 2
    rec, _ = csr_of(be, m)
    given = [g for g in S.pick(grads, ALL, p) if g is not None]
    res = []
    for run, kw in ((be.recurrent_lif_sequence, p.kwargs()),
                    (be.parametric_recurrent_lif_sequence, kwargs(p, [dev(a) for a in Q.shared_params(p)]))):
        leaves = [dev(a).requires_grad_() for a in (x, s0) + state[:n]]
        s, v_seq, last = run(leaves[0], rec, tuple(leaves[2:]), leaves[1], return_v=True, scale_exp=e, **kw)
        outs = (s, v_seq) + tuple(last)
        res.append(outs + tuple(torch.autograd.grad(outs, leaves, [dev(g) for g in given])))
    assert all(same_bits(host(a), host(b)) for a, b in zip(*res)) and 0 < float(res[0][0].detach().mean()) < 1
    q = [dev(a) for a in params('NNNNN', N, 2)]
    a = be.parametric_recurrent_lif_sequence(dev(x[:, :1]), rec, tuple(dev(t[:1]) for t in state[:n]), dev(s0[:1]), return_v=True,
                                             scale_exp=e, **kwargs(p, q))
    b = be.parametric_recurrent_lif_sequence(dev(x[:, 0]), rec, tuple(dev(t[0]) for t in state[:n]), dev(s0[0]), return_v=True,
                                             scale_exp=e, **kwargs(p, q))
    assert b[0].shape == b[1].shape == (T, N) and all(t.shape == (N,) for t in b[2])
    assert all(same_bits(host(i).reshape(-1), host(j).reshape(-1)) for i, j in zip(a[:2] + a[2], b[:2] + b[2]))


def test_capture_sees_parameters_and_weights_changed_in_place(be):
    T, B, N = 3, 2, 200
    m, e = matrix('one', N)
    p = Params(reset='soft', surrogate='atan', adaptive=True)
    rec, w = csr_of(be, m, True)
    q = [a.copy() for a in params('NNNNN', N, 3)]
    dq = [dev(a).requires_grad_() for a in q]
    x, s0, state, grads = case(T, B, N, 2)
    x_in, s0_in, g_in = dev(x), dev(s0), [dev(grads[0])] + [dev(g) for g in grads[2:]]
    state_in = [dev(a) for a in state]

    def step():
        xs = x_in.detach().requires_grad_()
        s, last = be.parametric_recurrent_lif_sequence(xs, rec, tuple(state_in), s0_in, scale_exp=e, **kwargs(p, dq))
        outs = (s,) + tuple(last)
        return outs + tuple(torch.autograd.grad(outs, [xs, w] + dq, g_in))

    graphed = be.capture_step(step)

    def check(m_now, q_now):
        got = [host(t) for t in graphed()]
        f = Q.forward(x, m_now, s0, *state, q_now, p, e)
        r = Q.backward(f.h_save, f.c_save, f.a_save, m_now, state[0], state[1], grads[0], None, *grads[2:], q_now, p)
        assert same_bits(got[0], f.s_out) and same_bits(got[3], f.a_last) and same_bits(got[4], r.g_x)
        for g, slot, name in zip(got[6:], r[5:], Q.NAMES):
            assert Q.within_reduce_bound(g, slot, N), name
        return f

    first = check(m, q)
    with torch.no_grad():
        dq[1].data.mul_(0.5)                                             # an optimiser's in-place step: the replay reads it
    q[1] = (q[1] * F(0.5)).astype(F)
    second = check(m, q)
    assert not same_bits(first.v_seq, second.v_seq)
    with torch.no_grad():
        rec.data.mul_(-0.5)                                              # ... and the weights' (the exponent still bounds them)
    m2 = Q.Matrix((m.w * F(-0.5)).astype(F), m.indices, m.indptr, m.n)
    third = check(m2, q)
    assert not same_bits(second.r, third.r)


def test_no_grad_keeps_nothing_and_empty_shapes(be, monkeypatch):
    from brainevent_amd import _neuron_rec_sg
    calls = []
    real = _neuron_rec_sg.call
    monkeypatch.setattr(_neuron_rec_sg, 'call', lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    T, B, N = 3, 2, 65
    m, e = matrix('dyadic', N)
    x, s0, state, _ = case(T, B, N, 13)
    p = Params(adaptive=True)
    rec, w = csr_of(be, m, True)
    dq = [dev(a).requires_grad_() for a in params('NNNNN', N)]
    run = lambda: be.parametric_recurrent_lif_sequence(dev(x), rec, None, dev(s0), scale_exp=e, **kwargs(p, dq))[0]
    a = run()
    kept = lambda: [t.value is not None for t in calls[-1][1][20:23]]    # h_save, c_save, a_save
    assert a.grad_fn is not None and calls[-1][0] == 'be_lif_rec_sg_forward_params' and kept() == [True, True, True]
    with torch.no_grad():
        b = run()
    assert b.grad_fn is None and kept() == [False, False, False] and same_bits(host(a), host(b))
    # T = 0 and B = 0: the state passes through, every gradient is defined
    for shape in ((0, B, N), (T, 0, N)):
        xs = torch.zeros(shape, device='cuda', requires_grad=True)
        st = tuple(torch.full(shape[1:], 0.5, device='cuda', requires_grad=True) for _ in range(3))
        s, last = be.parametric_recurrent_lif_sequence(xs, rec, st, None, scale_exp=e, **kwargs(p, dq))
        assert s.shape == shape and all(t.shape == shape[1:] for t in last)
        assert shape[0] != 0 or all(same_bits(host(i), host(j)) for i, j in zip(last, st))
        got = torch.autograd.grad([s.sum() + sum(t.sum() for t in last)], [xs, w] + list(st) + dq)
        assert all(not g.any() for g in got[:2] + got[5:]) and got[0].shape == shape
        assert shape[0] != 0 or all(bool((g == 1).all()) for g in got[2:5])
