"""The fused recurrent spiking layer (csrc/be_neuron_sg_rec.hip, brainevent_amd/_neuron_rec_sg.py) on the device, compared with
the numpy restatement of tests/lif_rec_sg_cases.py.  Forward outputs and the saved ``h`` / ``th`` are compared as EQUALITIES, bit
for bit (``same_bits``): the recurrent sums are 64-bit integers, every other operation an individually rounded f32 one.  Gradients
are compared within the restatement's propagated bound (the order of the device's f32 gather is its own).  Nothing here is
compared with torch's device kernels.  tests/test_lif_rec_sg_cpu.py holds the restatement to CPU autograd and the sizes used here
to the kernels' source."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_rec_sg_cases as C
import lif_syn_sg_cases as S
from lif_rec_sg_cases import F, Params, same_bits

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ALL = S.GRAD_SETS['all']
STATE_OUT = ('g_c0', 'g_v0', 'g_a0', 'g_s0')
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
    """Seeded inputs of one size (shared and left unchanged: the arrays are read-only)."""
    x, s0, state, grads = C.inputs(T, B, N, seed)
    for a in (x, s0) + state + grads:
        a.setflags(write=False)
    return x, s0, state, grads


@functools.lru_cache(maxsize=None)
def matrix(kind, N, seed=0):
    """One of the test matrices and the exponent the library chooses for it (shared and left unchanged)."""
    build = {'random': lambda: C.random_matrix(N, seed), 'dyadic': lambda: C.dyadic_matrix(N, seed),
             'empty': lambda: C.empty_matrix(N), 'crafted': lambda: C.crafted_matrix(N)}
    m = build[kind]()
    return m, device_exponent(m)


class DevMatrix:
    """The CSR arrays on the device; a matrix without entries hands over one unused element (the entry points refuse NULL)."""

    def __init__(self, m):
        self.w = dev(m.w) if len(m.w) else torch.zeros(1, device='cuda')
        self.indices = dev(m.indices) if len(m.w) else torch.zeros(1, dtype=torch.int32, device='cuda')
        self.indptr = dev(m.indptr)


def device_exponent(m):
    """The exponent the library chooses (``be_fixed_point_exponent``); the restatement's own rule may land one higher at a power
    of two, never lower."""
    if len(m.w) == 0:
        return 0
    from brainevent_amd._csr import fixed_point_exponent
    e = fixed_point_exponent(dev(m.w), dev(m.indices), m.n)
    assert C.exponent(m) - 1 <= e <= C.exponent(m)
    return e


def within(got, want, bound, what):
    got = host(got).astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, 'a NaN is a NaN in both, and nowhere else')
    err = np.where(nan, 0.0, np.abs(got - want))
    assert (err <= np.where(nan, 0.0, bound)).all(), (what, float(err.max()), float(bound.flat[err.argmax()]))


# ======================================================================================================== the direct C call
class Direct:
    """``be_lif_rec_sg_forward`` on device copies of the inputs (``s0`` and the state entries may be None: NULL), then any number
    of ``be_lif_rec_sg_backward`` calls on what it saved; every output is compared with the restatement.  Every output buffer
    starts filled with SENTINEL; without adaptation the adaptation's buffers are passed all the same and must stay so."""

    def __init__(self, m, e, p, x, s0, state, save=True, want_v=True):
        from brainevent_amd import _array as A, _lib
        T, B, N = x.shape
        self.A, self.lib, self.dims, self.p, self.m, self.dm = A, _lib, (T, B, N), p, m, DevMatrix(m)
        self.ref = C.forward(x, m, s0, state[0], state[1], state[2] if p.adaptive else None, p, e)
        ins = [dev(x), self.dm.w, self.dm.indices, self.dm.indptr, dev(s0)] + [dev(a) for a in state]
        self.s_out, self.v_seq, self.h_save, self.th_save = (full((T, B, N)) for _ in range(4))
        self.c_last, self.v_last, self.a_last = (full((B, N)) for _ in range(3))
        outs = [self.s_out, self.v_seq if want_v else None, self.h_save if save else None, self.th_save if save else None,
                self.c_last, self.v_last, self.a_last]
        rc = _lib.fn('be_lif_rec_sg_forward')(*[A.ptr(t) for t in ins + outs], T, B, N, *self.scalars(), RESET[p.reset],
                                              int(p.adaptive), e, A.stream_ptr())
        assert rc == 0, _lib.last_error()
        r, what = self.ref, (self.dims, p)
        assert same_bits(host(self.s_out), r.s_out) and same_bits(host(self.c_last), r.c_last), what
        assert same_bits(host(self.v_last), r.v_last), what
        self.same_or_untouched(self.v_seq, r.v_seq if want_v else None, what)
        self.same_or_untouched(self.h_save, r.h_save if save else None, what)
        self.same_or_untouched(self.th_save, r.th_save if save else None, what)
        self.same_or_untouched(self.a_last, r.a_last, what)

    def scalars(self):
        p = self.p
        return p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa

    @staticmethod
    def same_or_untouched(t, ref, what):
        if ref is None:
            assert bool((t == SENTINEL).all()), what
        else:
            assert same_bits(host(t), ref), what

    def backward(self, grads, use=ALL, null=()):
        """One backward call: ``use`` picks the gradients that arrive, ``null`` names the outputs not asked for."""
        A, (T, B, N), p, dm = self.A, self.dims, self.p, self.dm
        given = S.pick(grads, use, p)
        r, b = C.backward(self.ref.h_save, self.ref.th_save, self.m, *given, p, with_bound=True)
        ins = [dev(g if u else None) for g, u in zip(grads, use)]
        g_x = full((T, B, N))
        outs = [full((B, N)) for _ in STATE_OUT]
        rc = self.lib.fn('be_lif_rec_sg_backward')(
            A.ptr(self.h_save), A.ptr(self.th_save), A.ptr(dm.w), A.ptr(dm.indices), A.ptr(dm.indptr), *[A.ptr(t) for t in ins],
            A.ptr(g_x), *[A.ptr(None if n in null else t) for n, t in zip(STATE_OUT, outs)], T, B, N, *self.scalars(), RESET[p.reset],
            SURROGATE[p.surrogate], p.alpha, int(p.adaptive), int(p.detach_reset), A.stream_ptr())
        assert rc == 0, self.lib.last_error()
        what = (self.dims, p, use, null)
        within(g_x, r.g_x, b.g_x, ('g_x',) + what)
        for n, t, want, bound in zip(STATE_OUT, outs, r[1:], b[1:5]):
            if n in null or want is None:
                assert bool((t == SENTINEL).all()), (n,) + what
            else:
                within(t, want, bound, (n,) + what)
        return r, b, g_x


def check_direct(m, e, p, T, B, seed=0, with_s0=True, use=ALL, null=()):
    x, s0, state, grads = case(T, B, m.n, seed)
    d = Direct(m, e, p, x, s0 if with_s0 else None, state)
    return d.ref, d.backward(grads, use, null)[0]


# ======================================================================================================== sizes
@pytest.mark.parametrize('N', C.N_SIZES)
def test_sizes(be, N):
    """One neuron, a wave less one, a wave, a wave and one, 257, one past the workgroup; 1 and 3 samples; 1, 2, 3 and 5 steps;
    general weights at the library's exponent and the dyadic matrix; with and without s0."""
    ps = (Params(adaptive=True), Params(reset='soft', surrogate='atan', v_reset=-0.25))
    for k, (B, T, kind) in enumerate(itertools.product(C.B_SIZES, C.T_SIZES, ('random', 'dyadic'))):
        m, e = matrix(kind, N)
        f, b = check_direct(m, e, ps[k % 2], T, B, with_s0=(k // 2) % 2 == 0)
    assert N < 8 or (0 < f.s_out.mean() < 1 and np.abs(b.g_x).max() > 0 and np.count_nonzero(f.r[-1]) > 0)


def test_the_limit(be):
    """N = kRecMaxN once (96 KB of LDS forwards, 8 neurons per thread); one more is refused with BE_ERR_RANGE by both calls."""
    from brainevent_amd import _array as A, _lib
    N = C.CONSTS['kRecMaxN']
    m, e = matrix('random', N)
    f, b = check_direct(m, e, Params(adaptive=True), 2, 1)
    assert 0.05 < f.s_out.mean() < 0.6 and np.count_nonzero(f.r[1]) > N // 4 and np.abs(b.g_s0).max() > 0
    P, st, t = A.ptr, A.stream_ptr(), full((2, 1, N + 1))
    dm = DevMatrix(C.empty_matrix(N + 1))
    rc = _lib.fn('be_lif_rec_sg_forward')(P(t), P(dm.w), P(dm.indices), P(dm.indptr), P(None), P(None), P(None), P(None), P(t), P(None),
                                          P(None), P(None), P(t[0]), P(t[0]), P(None), 2, 1, N + 1, 0.8, 0.9, 1.0, 0.0, 0.0, 0.0, 0, 0,
                                          0, st)
    assert rc == RANGE and '8192' in _lib.last_error() and _lib.last_error().startswith('be_lif_rec_sg_forward: ')
    rc = _lib.fn('be_lif_rec_sg_backward')(P(t), P(None), P(dm.w), P(dm.indices), P(dm.indptr), P(None), P(None), P(None), P(None),
                                           P(None), P(t), P(None), P(None), P(None), P(None), 2, 1, N + 1, 0.8, 0.9, 1.0, 0.0, 0.0, 0.0,
                                           0, 0, 10.0, 0, 0, st)
    assert rc == RANGE and '8192' in _lib.last_error() and _lib.last_error().startswith('be_lif_rec_sg_backward: ')
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all())


# ======================================================================================================== matrices and spikes
@pytest.mark.parametrize('kind', ('crafted', 'empty'))
def test_matrices(be, kind):
    """Empty rows, a self-loop, a row listing one column five times, a row of 600 entries at N = 300, rows of 64 and 65 entries (one
    trip of a row's lanes and one entry more); and no entry at all."""
    m, e = matrix(kind, 300)
    for p, T, B, with_s0 in ((Params(adaptive=True), 5, 3, True), (Params(reset='soft', surrogate='triangle', alpha=2.0), 3, 1, False)):
        x, s0, state, grads = case(T, B, 300, 4)
        s0 = s0.copy()
        s0[:, :8] = 1                                                    # the crafted rows are active before step 0 ...
        x = x.copy()
        x[:, :, :8] += 2.0                                               # ... and at most steps
        d = Direct(m, e, p, x, s0 if with_s0 else None, state)
        r, _, _ = d.backward(grads)
        if kind == 'crafted':
            assert d.ref.s_out[:-1, :, :8].mean() > 0.5 and np.count_nonzero(d.ref.r) > 0 and np.count_nonzero(r.g_s0) > 0
        else:
            assert not d.ref.r.any() and not r.g_s0.any()


@pytest.mark.parametrize('with_s0', (False, True))
def test_a_step_where_every_neuron_fires_and_one_where_none_does(be, with_s0):
    T, B, N = 5, 3, 257
    m, e = matrix('random', N)
    x, s0, state, grads = case(T, B, N, 6)
    x = x.copy()
    x[1], x[2] = 50.0, -500.0
    if with_s0:
        s0 = np.ones_like(s0)                                            # a full id list before step 0 as well
    for p in (Params(adaptive=True), Params(reset='soft')):
        d = Direct(m, e, p, x, s0 if with_s0 else None, state)
        assert d.ref.s_out[1].all() and not d.ref.s_out[2].any() and not d.ref.r[3].any() and np.count_nonzero(d.ref.r[2]) > N // 2
        d.backward(grads)


# ======================================================================================================== modes
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', C.MODES)
def test_modes_and_gradient_sets(be, reset, surrogate, detach, adaptive):
    """Every mode x (each gradient alone, all together)."""
    p = S.mode_params(reset, surrogate, detach, adaptive)
    T, B, N = 3, 3, 257
    m, e = matrix('random', N)
    x, s0, state, grads = case(T, B, N, 7)
    d = Direct(m, e, p, x, s0, state)
    assert 0 < d.ref.s_out.mean() < 1
    for which, use in S.GRAD_SETS.items():
        r, _, _ = d.backward(grads, use)
        assert np.count_nonzero(r.g_x) > 0 or (which == 'g_alast' and not adaptive)


@pytest.mark.parametrize('adaptive', (False, True))
def test_every_subset_of_the_optional_outputs(be, adaptive):
    T, B, N = 3, 2, 65
    m, e = matrix('random', N)
    x, s0, state, grads = case(T, B, N, 8)
    p = Params(adaptive=adaptive)
    for save, want_v in itertools.product((False, True), repeat=2):
        d = Direct(m, e, p, x, s0, state, save=save, want_v=want_v)
    for k in range(len(STATE_OUT) + 1):
        for null in itertools.combinations(STATE_OUT, k):
            d.backward(grads, null=null)
    # a NULL state entry, s0 or gradient is zeros
    zeros = np.zeros((B, N), F)
    a, b = Direct(m, e, p, x, None, (None, None, None)), Direct(m, e, p, x, zeros, (zeros, zeros, zeros))
    names = ('s_out', 'v_seq', 'h_save', 'c_last', 'v_last') + (('th_save', 'a_last') if adaptive else ())
    assert all(same_bits(host(getattr(a, n)), host(getattr(b, n))) for n in names)
    ga = a.backward(grads, use=(True, False, False, False, False))[2]
    gb = b.backward((grads[0], np.zeros_like(x), zeros, zeros, zeros))[2]
    assert same_bits(host(ga), host(gb))


def test_a_nan_stays_in_its_sample(be):
    T, B, N = 4, 3, 257
    m, e = matrix('random', N)
    x, s0, state, grads = case(T, B, N, 9)
    p = Params(adaptive=True)
    clean = Direct(m, e, p, x, s0, state)
    g_clean = clean.backward(grads)[2]
    bad = x.copy()
    bad[1, 1, 5] = np.nan
    d = Direct(m, e, p, bad, s0, state)
    g = d.backward(grads)[2]
    assert np.isnan(host(d.v_seq)[1:, 1, 5]).all() and np.isnan(host(g)[:, 1]).any()
    for other in (0, 2):
        for a, b in zip((d.s_out, d.v_seq, d.h_save, d.th_save, g), (clean.s_out, clean.v_seq, clean.h_save, clean.th_save, g_clean)):
            assert same_bits(host(a)[:, other], host(b)[:, other])
        for a, b in zip((d.c_last, d.v_last, d.a_last), (clean.c_last, clean.v_last, clean.a_last)):
            assert same_bits(host(a)[other], host(b)[other])


# ======================================================================================================== C error codes
def test_c_error_codes_each_followed_by_a_clean_call(be):
    from brainevent_amd import _array as A, _lib
    fwd, bwd = _lib.fn('be_lif_rec_sg_forward'), _lib.fn('be_lif_rec_sg_backward')
    T, B, N = 3, 2, 64
    m, e = matrix('random', N)
    x, s0, state, grads = case(T, B, N, 0)
    p = Params(adaptive=True)
    ref = C.forward(x, m, s0, *state, p, e)
    rb, bb = C.backward(ref.h_save, ref.th_save, m, *grads, p, with_bound=True)
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    dm = DevMatrix(m)
    ins = [dev(a) for a in (x, s0) + state]
    gin = [dev(g) for g in grads]
    big = [full((T, B, N)) for _ in range(5)]                                      # s_out, v_seq, h_save, th_save, g_x
    small = [full((B, N)) for _ in range(7)]                                       # c_last, v_last, a_last, g_c0, g_v0, g_a0, g_s0
    s_out, v_seq, h_save, th_save, g_x = big
    c_last, v_last, a_last, g_c0, g_v0, g_a0, g_s0 = small

    def forward(x=P(ins[0]), w=P(dm.w), indices=P(dm.indices), indptr=P(dm.indptr), s_out=P(s_out), h_save=P(h_save),
                th_save=P(th_save), c_last=P(c_last), v_last=P(v_last), a_last=P(a_last), T=T, B=B, N=N, mode=0, adaptive=1, e=e):
        return fwd(x, w, indices, indptr, P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), s_out, P(v_seq), h_save, th_save, c_last, v_last,
                   a_last, T, B, N, 0.8, 0.9, 1.0, 0.0, 0.95, 0.3, mode, adaptive, e, st)

    def backward(h_save=P(h_save), th_save=P(th_save), w=P(dm.w), indices=P(dm.indices), indptr=P(dm.indptr), g_x=P(g_x), T=T, B=B,
                 N=N, mode=0, sur=0, alpha=10.0, adaptive=1):
        return bwd(h_save, th_save, w, indices, indptr, *[P(g) for g in gin], g_x, P(g_c0), P(g_v0), P(g_a0), P(g_s0), T, B, N, 0.8,
                   0.9, 1.0, 0.0, 0.95, 0.3, mode, sur, alpha, adaptive, 0, st)

    # nothing to do: BE_OK and nothing written, whatever the pointers
    assert forward(T=0) == 0 and forward(B=0) == 0 and forward(N=0) == 0
    assert forward(N=0, x=null, w=null, indices=null, indptr=null, s_out=null, c_last=null, v_last=null, a_last=null) == 0
    assert backward(T=0) == 0 and backward(B=0) == 0 and backward(N=0, h_save=null, th_save=null, w=null, g_x=null) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in big + small)
    for bad in (dict(x=null), dict(s_out=null), dict(c_last=null), dict(v_last=null), dict(a_last=null), dict(th_save=null),
                dict(w=null), dict(indices=null), dict(indptr=null), dict(T=-1), dict(B=-1), dict(N=-1), dict(mode=2), dict(mode=-1),
                dict(e=-91), dict(e=151)):
        assert forward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_rec_sg_forward: '), _lib.last_error()
        assert forward() == 0                                                  # a clean call after each refused one
    assert forward(N=C.CONSTS['kRecMaxN'] + 1) == RANGE and forward() == 0
    assert forward(a_last=null, th_save=null, adaptive=0) == 0 and forward(h_save=null, th_save=null) == 0 and forward() == 0
    for bad in (dict(h_save=null), dict(g_x=null), dict(th_save=null), dict(w=null), dict(indices=null), dict(indptr=null),
                dict(T=-1), dict(B=-1), dict(N=-1), dict(mode=2), dict(sur=3), dict(sur=-1), dict(alpha=0.0), dict(alpha=float('nan'))):
        assert backward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_rec_sg_backward: '), _lib.last_error()
        assert backward() == 0
    assert backward(N=C.CONSTS['kRecMaxN'] + 1) == RANGE and backward() == 0
    got = [host(t) for t in (s_out, v_seq, h_save, th_save, c_last, v_last, a_last)]
    assert all(same_bits(a, b) for a, b in zip(got, ref[:7]))
    for t, want, bound in zip((g_x, g_c0, g_v0, g_a0, g_s0), rb, bb):
        within(t, want, bound, 'after the refusals')


# ======================================================================================================== the Python function
def csr_of(be, m, requires_grad=False):
    w = dev(m.w).requires_grad_(requires_grad)
    return be.CSR((w, dev(m.indices), dev(m.indptr)), shape=(m.n, m.n)), w


@pytest.mark.parametrize('adaptive', (False, True))
def test_equals_the_loop_of_steps_and_products(be, adaptive):
    """Dyadic weights: forwards bit for bit the loop of ``synaptic_lif_step`` on ``x[t] + BinaryArray(s) @ rec`` — the behaviour a
    user relies on; the gradients of x, the state, s0 and rec.data within the restatement's bound of the restatement."""
    T, B, N = 5, 3, 257
    m, _ = matrix('dyadic', N)
    x, s0, state, grads = case(T, B, N, 11)
    p = Params(adaptive=adaptive)
    n = 3 if adaptive else 2
    rec, w = csr_of(be, m, True)
    leaves = [dev(a).requires_grad_() for a in (x, s0) + state[:n]]
    s, v_seq, last = be.recurrent_lif_sequence(leaves[0], rec, tuple(leaves[2:]), leaves[1], return_v=True, **p.kwargs())
    assert s.shape == v_seq.shape == (T, B, N) and len(last) == n and all(t.shape == (B, N) for t in last)
    with torch.no_grad():
        rec2, _ = csr_of(be, m)
        st, sp, ss, vs = tuple(dev(a) for a in state[:n]), dev(s0), [], []
        for t in range(T):
            sp, st = be.synaptic_lif_step(st, dev(x[t]) + be.BinaryArray(sp) @ rec2, **p.kwargs())
            ss.append(sp)
            vs.append(st[1])
    for a, b in zip((s, v_seq) + tuple(last), (torch.stack(ss), torch.stack(vs)) + tuple(st)):
        assert same_bits(host(a), host(b))
    assert 0.05 < float(s.detach().mean()) < 0.6
    # ... and the restatement at the exponent the call chose is the same function
    e = device_exponent(m)
    f = C.forward(x, m, s0, *state[:n], *(None,) * (3 - n), p, e)
    assert same_bits(host(s), f.s_out) and same_bits(host(v_seq), f.v_seq) and np.count_nonzero(f.r) > 0
    given = S.pick(grads, ALL, p)
    outs = [(o, g) for o, g in zip((s, v_seq) + tuple(last), given) if g is not None]
    got = torch.autograd.grad([o for o, _ in outs], leaves + [w], [dev(g) for _, g in outs])
    r, b = C.backward(f.h_save, f.th_save, m, *given, p, with_bound=True)
    g_w, b_w = C.weight_grad(m, f.s_out, s0, r.g_x, b.g_x)
    wants = [('x', r.g_x, b.g_x), ('s0', r.g_s0, b.g_s0), ('c0', r.g_c0, b.g_c0), ('v0', r.g_v0, b.g_v0)] + \
        ([('a0', r.g_a0, b.g_a0)] if adaptive else []) + [('w', g_w, b_w)]
    assert len(got) == len(wants)
    for g, (name, want, bound) in zip(got, wants):
        within(g, want, bound, name)
        assert np.count_nonzero(want) > 0
    # without s0 the weight gradient starts at step 1; an input that needs no gradient gets none
    xt = dev(x).requires_grad_()
    s, _ = be.recurrent_lif_sequence(xt, rec, **p.kwargs())
    g_x2, g_w2 = torch.autograd.grad([s], [xt, w], [dev(grads[0])])
    f = C.forward(x, m, None, None, None, None, p, e)
    r, b = C.backward(f.h_save, f.th_save, m, grads[0], None, None, None, None, p, with_bound=True)
    within(g_x2, r.g_x, b.g_x, 'x, no s0')
    within(g_w2, *C.weight_grad(m, f.s_out, None, r.g_x, b.g_x), 'w, no s0')


def test_one_sample_without_a_batch_axis(be):
    T, N = 4, 65
    m, e = matrix('random', N)
    x, s0, state, _ = case(T, 1, N, 12)
    rec, _ = csr_of(be, m)
    p = Params(adaptive=True)
    a = be.recurrent_lif_sequence(dev(x), rec, tuple(dev(t) for t in state), dev(s0), return_v=True, **p.kwargs())
    b = be.recurrent_lif_sequence(dev(x[:, 0]), rec, tuple(dev(t[0]) for t in state), dev(s0[0]), return_v=True, scale_exp=e,
                                  **p.kwargs())
    assert b[0].shape == b[1].shape == (T, N) and all(t.shape == (N,) for t in b[2])
    for i, j in zip(a[:2] + a[2], b[:2] + b[2]):
        assert same_bits(host(i).reshape(-1), host(j).reshape(-1))
    assert 0 < float(a[0].mean()) < 1


@pytest.mark.parametrize('reset,surrogate', (('hard', 'fast_sigmoid'), ('soft', 'atan')))
def test_without_a_filter_and_a_matrix_it_is_lif_sequence(be, reset, surrogate):
    """syn_decay = 0 (the default), no adaptation, an empty rec: the s, v_seq, v_last, g_x and g_v0 of be.lif_sequence (inputs and
    gradients without zeros of either sign)."""
    import lif_sg_cases as C0
    T, B, N = 6, 2, 66
    x, v0, g_s, g_vseq, g_vlast = (a.reshape(a.shape[:-1] + (B, N)) for a in C0.inputs(T, B * N, 3))
    kw = dict(beta=0.9, v_th=1.0, v_reset=-0.25, reset=reset, surrogate=surrogate, alpha=10.0)
    rec, _ = csr_of(be, C.empty_matrix(N))
    gs = [dev(g_s), dev(g_vseq), dev(g_vlast)]
    xa, xb, va, vb = (dev(a).requires_grad_() for a in (x, x, v0, v0))
    s0, vseq0, vlast0 = be.lif_sequence(xa, va, return_v=True, **kw)
    s1, vseq1, (_, vlast1) = be.recurrent_lif_sequence(xb, rec, (None, vb), return_v=True, **kw)
    assert all(same_bits(host(a), host(b)) for a, b in ((s0, s1), (vseq0, vseq1), (vlast0, vlast1)))
    g0 = torch.autograd.grad([s0, vseq0, vlast0], [xa, va], gs)
    g1 = torch.autograd.grad([s1, vseq1, vlast1], [xb, vb], gs)
    assert all(same_bits(host(a), host(b)) and torch.count_nonzero(a).item() > 0 for a, b in zip(g0, g1))
    assert 0 < float(s0.detach().mean()) < 1


def test_weights_changed_in_place_are_seen_and_no_grad_keeps_nothing(be, monkeypatch):
    from brainevent_amd import _neuron_rec_sg
    calls = []
    real = _neuron_rec_sg.call
    monkeypatch.setattr(_neuron_rec_sg, 'call', lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    T, B, N = 3, 2, 65
    m, _ = matrix('dyadic', N)
    x, s0, state, _ = case(T, B, N, 13)
    p = Params()
    rec, w = csr_of(be, m, True)
    run = lambda: be.recurrent_lif_sequence(dev(x), rec, None, dev(s0), scale_exp=30, **p.kwargs())[0]
    a = run()
    assert a.grad_fn is not None and calls[-1][0] == 'be_lif_rec_sg_forward' and calls[-1][1][10].value is not None     # h is kept
    with torch.no_grad():
        b = run()
        assert b.grad_fn is None and calls[-1][1][10].value is None and same_bits(host(a), host(b))
        rec.data.mul_(-2.0)                                              # still dyadic, still far below the exponent's bound
        c = run()
    m2 = C.Matrix((m.w * F(-2.0)).astype(F), m.indices, m.indptr, m.n)
    assert same_bits(host(c), C.forward(x, m2, s0, None, None, None, p, 30).s_out) and not same_bits(host(c), host(a))


def test_capture_with_a_given_exponent(be):
    T, B, N = 3, 2, 200
    m, e = matrix('random', N)
    p = Params(reset='soft', surrogate='atan', adaptive=True)
    rec, w = csr_of(be, m, True)
    x_in, s0_in = torch.zeros(T, B, N, device='cuda'), torch.zeros(B, N, device='cuda')
    state_in = [torch.zeros(B, N, device='cuda') for _ in range(3)]
    g_in = [torch.zeros(T, B, N, device='cuda')] + [torch.zeros(B, N, device='cuda') for _ in range(3)]

    def step():
        x = x_in.detach().requires_grad_()                                       # leaves of this call, on the static memory
        start = [t.detach().requires_grad_() for t in state_in]
        s, last = be.recurrent_lif_sequence(x, rec, tuple(start), s0_in, scale_exp=e, **p.kwargs())
        outs = (s,) + tuple(last)
        return outs + tuple(torch.autograd.grad(outs, [x, w] + start, g_in))

    def load(seed):
        x, s0, state, grads = case(T, B, N, seed)
        for t, a in zip([x_in, s0_in] + state_in + g_in, (x, s0) + state + (grads[0],) + grads[2:]):
            t.copy_(dev(a))

    load(1)
    graphed = be.capture_step(step)
    for seed in (2, 3):
        load(seed)
        got = [t.detach().clone() for t in graphed()]
        want = step()
        assert all(same_bits(host(a), host(b)) for a, b in zip(got, want))
        assert 0 < float(got[0].mean()) < 1 and all(torch.count_nonzero(g).item() > 0 for g in got[-5:])
    x, s0, state, grads = case(T, B, N, 3)                                       # ... and the eager result is the restatement's
    f = C.forward(x, m, s0, *state, p, e)
    assert same_bits(host(want[0]), f.s_out) and same_bits(host(want[3]), f.a_last)


def test_refusals_that_need_a_device(be):
    N = 8
    m = C.random_matrix(N, 0)
    rec, _ = csr_of(be, m)
    x = torch.zeros(2, 3, N, device='cuda')
    kw = dict(beta=0.9)
    with pytest.raises(TypeError, match='indptr of rec must be int32'):
        be.recurrent_lif_sequence(x, be.CSR((dev(m.w), dev(m.indices), dev(m.indptr)), shape=(N, N), indptr_dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match='one shared weight is not built'):
        be.recurrent_lif_sequence(x, be.CSR((torch.ones(1, device='cuda'), dev(m.indices), dev(m.indptr)), shape=(N, N)), **kw)
    with pytest.raises(TypeError, match='weights of rec must be float32'):
        be.recurrent_lif_sequence(x, be.CSR((dev(m.w).double(), dev(m.indices), dev(m.indptr)), shape=(N, N)), **kw)
    with pytest.raises(TypeError, match='rec must be a CSR'):
        be.recurrent_lif_sequence(x, be.CSC((dev(m.w), dev(m.indices), dev(m.indptr)), shape=(N, N)), **kw)
    with pytest.raises(ValueError, match="size of x's last axis"):
        be.recurrent_lif_sequence(torch.zeros(2, 3, N + 1, device='cuda'), rec, **kw)
    with pytest.raises(ValueError, match='device tensor'):
        be.recurrent_lif_sequence(torch.zeros(2, 3, N), rec, **kw)
    # a prepared (planned, mirrored) container is read through its raw arrays: the same result
    a = be.recurrent_lif_sequence(x + 1.5, rec, **kw)[0]
    rec.prepare(mirror=True)
    assert same_bits(host(be.recurrent_lif_sequence(x + 1.5, rec, **kw)[0]), host(a)) and 0 < float(a.mean())
    # no step, no sample: the state passes through
    s, (c, v) = be.recurrent_lif_sequence(x[:0], rec, (None, torch.ones(3, N, device='cuda')), **kw)
    assert s.shape == (0, 3, N) and host(v).tolist() == [[1.0] * N] * 3 and not host(c).any()
    rec_g, w = csr_of(be, m, True)                                           # ... and so do its gradients; the weights get zeros
    c0, s0 = (torch.ones(3, N, device='cuda', requires_grad=True) for _ in range(2))
    s, (c, v) = be.recurrent_lif_sequence(x[:0], rec_g, (c0, None), s0, **kw)
    g = torch.autograd.grad([c, v], [c0, s0, w], [torch.full((3, N), 3.0, device='cuda'), torch.ones(3, N, device='cuda')])
    assert host(g[0]).tolist() == [[3.0] * N] * 3 and not host(g[1]).any() and not host(g[2]).any() and g[2].shape == w.shape
    s, (c, v) = be.recurrent_lif_sequence(x[:, :0], rec, **kw)
    assert s.shape == (2, 0, N) and c.shape == v.shape == (0, N)
