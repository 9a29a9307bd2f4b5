"""The synaptic / adaptive LIF neuron with per-slot, learnable parameters (csrc/be_neuron_sg.hip: be_lif_syn_sg_forward_params /
be_lif_syn_sg_backward_params; brainevent_amd/_neuron_syn_sg.py) on the device, compared with the numpy restatement of
tests/lif_syn_sg_param_cases.py as EQUALITIES, bit for bit: every operation of both passes is an individually rounded IEEE f32 add,
multiply, divide, abs or compare.  Only the reduce over the batch rows (be_lif_sg_reduce_slots, tests/test_lif_sg_param_gpu.py) has a
bound.  Nothing here is compared with torch's device kernels.  tests/test_lif_syn_sg_param_cpu.py holds the restatement to CPU
autograd."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_syn_sg_cases as S
import lif_syn_sg_param_cases as Q
from lif_syn_sg_cases import Params
from lif_syn_sg_param_cases import F, same_bits

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
INVALID = -1
ALL = Q.GRAD_SETS['all']
STATE_OUT = ('g_c0', 'g_v0', 'g_a0')
OUTS = STATE_OUT + Q.SLOTS                      # what a backward call may leave out
RESET = {'hard': 0, 'soft': 1}
SURROGATE = {'fast_sigmoid': 0, 'atan': 1, 'triangle': 2}


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def misaligned(a):
    flat = torch.empty(a.size + 1, dtype=torch.float32, device='cuda')
    flat[1:].copy_(torch.tensor(np.asarray(a).reshape(-1)))
    view = flat[1:].view(a.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def case(T, N, seed):
    x, state, grads = Q.inputs(T, N, seed)
    for a in (x,) + state + grads:
        a.setflags(write=False)
    return x, state, grads


@functools.lru_cache(maxsize=None)
def params(periods, seed):
    q = Q.param_inputs(periods, seed)
    for a in q:
        a.setflags(write=False)
    return q


class Direct:
    """``be_lif_syn_sg_forward_params`` on device copies (state entries may be None: NULL), then any number of
    ``be_lif_syn_sg_backward_params`` calls on what it saved; every output is compared with the restatement.  ``off``: the names of
    the arrays whose base is put 4 bytes past a 16-byte boundary ('all': every one).  Every output buffer starts filled with
    SENTINEL; without adaptation the adaptation's arrays are passed all the same and must stay so, as must ``c_save`` / ``a_save``
    where they are not asked for."""

    def __init__(self, T, N, p, x, state, q, off=(), save=True, want_v=True, want_c=True):
        from brainevent_amd import _array as A, _lib
        self.A, self.lib, self.T, self.N, self.p, self.off, self.q, self.state = A, _lib, T, N, p, off, q, state
        self.bwd = _lib.fn('be_lif_syn_sg_backward_params')
        st = (state[0], state[1], state[2] if p.adaptive else None)
        self.ref = Q.forward(x, *st, q, p)
        ins = [self.given('x', x)] + [self.given(n, a) for n, a in zip(('c0', 'v0', 'a0'), state)]
        self.c0, self.v0 = ins[1], ins[2]
        self.qd = [self.given(n, a) for n, a in zip(Q.NAMES, q)]
        names = ('s_out', 'v_seq', 'h_save', 'c_save', 'a_save')
        self.s_out, self.v_seq, self.h_save, self.c_save, self.a_save = (self.out(n, (T, N)) for n in names)
        self.c_last, self.v_last, self.a_last = (self.out(n, (N,)) for n in ('c_last', 'v_last', 'a_last'))
        outs = [self.s_out, self.v_seq if want_v else None, self.h_save if save else None, self.c_save if want_c else None,
                self.a_save, self.c_last, self.v_last, self.a_last]       # a_save always: untouched where h_save is NULL
        rc = _lib.fn('be_lif_syn_sg_forward_params')(*[A.ptr(t) for t in ins], *self.param_args(), *[A.ptr(t) for t in outs], T, N,
                                                     p.v_reset, RESET[p.reset], int(p.adaptive), A.stream_ptr())
        assert rc == 0, _lib.last_error()
        r, what = self.ref, (T, N, p, off, [a.size for a in q])
        assert same_bits(host(self.s_out), r.s_out) and same_bits(host(self.c_last), r.c_last), what
        assert same_bits(host(self.v_last), r.v_last), what
        self.same_or_untouched(self.v_seq, r.v_seq if want_v else None, what)
        self.same_or_untouched(self.h_save, r.h_save if save else None, what)
        self.same_or_untouched(self.c_save, r.c_save if want_c else None, what)
        self.same_or_untouched(self.a_save, r.a_save if save else None, what)
        self.same_or_untouched(self.a_last, r.a_last, what)

    def param_args(self):
        return [v for t in self.qd for v in (self.A.ptr(t), t.numel())]

    def is_off(self, name):
        return self.off == 'all' or name in self.off

    def given(self, name, a):
        if a is None:
            return None
        return misaligned(a) if self.is_off(name) else dev(a)

    def out(self, name, shape):
        n = int(np.prod(shape))
        flat = torch.full((n + 1,), SENTINEL, dtype=torch.float32, device='cuda')
        t = (flat[1:] if self.is_off(name) else flat[:n]).view(shape)
        assert t.data_ptr() % 16 == (4 if self.is_off(name) else 0)
        return t

    @staticmethod
    def same_or_untouched(t, ref, what):
        if ref is None:
            assert bool((t == SENTINEL).all()), what
        else:
            assert same_bits(host(t), ref), what

    def reference(self, grads, use):
        p = self.p
        r = self.ref
        st = self.state
        return Q.backward(r.h_save, r.c_save, r.a_save, st[0], st[1], *S.pick(grads, use, p), self.q, p)

    def call_backward(self, ins, outs, null):
        """One call; ``outs``: g_x and the eight optional outputs, in the entry point's order."""
        A, T, N, p = self.A, self.T, self.N, self.p
        c_save = None if 'g_sd_slot' in null else self.c_save       # needed for the syn_decay gradient alone
        rc = self.bwd(A.ptr(self.h_save), A.ptr(c_save), A.ptr(self.a_save), A.ptr(self.c0), A.ptr(self.v0), *[A.ptr(t) for t in ins],
                      *self.param_args(), A.ptr(outs[0]), *[A.ptr(None if n in null else t) for n, t in zip(OUTS, outs[1:])], T, N,
                      p.v_reset, RESET[p.reset], SURROGATE[p.surrogate], p.alpha, int(p.adaptive), int(p.detach_reset), A.stream_ptr())
        assert rc == 0, self.lib.last_error()

    def backward(self, grads, use=ALL, null=()):
        T, N = self.T, self.N
        r = self.reference(grads, use)
        ins = [self.given(n, g) for n, g in zip(Q.GRADS, S.pick(grads, use, self.p))]
        outs = [self.out('g_x', (T, N))] + [self.out(n, (N,)) for n in OUTS]
        self.call_backward(ins, outs, null)
        what = (T, N, self.p, self.off, use, null, [a.size for a in self.q])
        assert same_bits(host(outs[0]), r.g_x), what
        for n, t, want in zip(OUTS, outs[1:], r[1:]):
            self.same_or_untouched(t, None if n in null else want, (n,) + what)
        return r


def check_direct(T, N, p, periods, seed=0, off=(), use=ALL, null=()):
    x, state, grads = case(T, N, seed)
    d = Direct(T, N, p, x, state, params(tuple(periods), seed), off=off)
    return d.ref, d.backward(grads, use, null)


# ======================================================================================================== sizes and periods
@pytest.mark.parametrize('N', Q.N_SIZES)
def test_sizes_and_periods(be, N):
    """Every N x T x the periods 1, N, N / 2, N / 3 (84 / 2 = 42 is no multiple of 4: the 4-byte kernel; 96 / 3 = 32 is)."""
    ran = 0
    for which in ('1', 'N', 'N/2', 'N/3'):
        P = Q.periods_of(N, which)
        if P is None:
            continue
        for T in Q.T_SIZES:
            for p in (Params(adaptive=True, v_reset=-0.25), Params(reset='soft', surrogate='atan', v_reset=-0.25)):
                f, b = check_direct(T, N, p, (P,) * 5)
                ran += 1
    assert ran >= 2 * len(Q.T_SIZES) and (N < 8 or (0 < f.s_out.mean() < 1 and np.abs(b.g_sd_slot).max() > 0))


@pytest.mark.parametrize('N,periods', [(96, (1, 96, 48, 32, 16)), (96, (8, 4, 96, 1, 24)), (84, (1, 84, 42, 28, 21)),
                                       (84, (28, 4, 84, 12, 1))])
def test_five_different_periods(be, N, periods):
    """Independent periods in one call: all multiples of 4 (the 16-byte kernel), and with one that is not (the 4-byte kernel)."""
    for T in (1, 6):
        for p in (Params(adaptive=True), Params(adaptive=True, reset='soft', surrogate='triangle', alpha=2.0)):
            f, b = check_direct(T, N, p, periods, seed=4)
    assert 0 < f.s_out.mean() < 1 and all(np.count_nonzero(a) > 0 for a in b[4:])


@pytest.mark.parametrize('off', [(n,) for n in Q.NAMES] + [('c_save',), ('a_save',), ('g_rho_slot',), 'all'])
def test_base_off_16_bytes(be, off):
    """N % 4 == 0, periods that allow the 16-byte kernel, and one base — each parameter's, a saved array's, a slot output's, every
    array's — 4 bytes past a 16-byte boundary: only the alignment refuses the 16-byte kernels."""
    for T in (1, 6):
        check_direct(T, 64, Params(adaptive=True), (16, 64, 32, 8, 4), off=off)
        check_direct(T, 64, Params(reset='soft', surrogate='triangle', alpha=2.0), (16, 64, 32, 8, 4), off=off)


@pytest.mark.parametrize('N', Q.N_PAST_ONE_PASS)
def test_past_one_pass_of_the_capped_grid(be, N):
    """A second trip of the grid-stride loop: of the 4-byte kernel (one slot) and of the 16-byte kernel (one lane); adaptive, the
    decay and kappa per slot."""
    f, b = check_direct(2, N, Params(adaptive=True, surrogate='triangle', alpha=2.0), (N, 1, 1, 1, N), seed=3)
    assert 0.05 < f.s_out.mean() < 0.6 and np.count_nonzero(b.g_kappa_slot) > 0


# ======================================================================================================== modes
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', Q.MODES)
def test_modes_gradient_sets_and_null_outputs(be, reset, surrogate, detach, adaptive):
    """Every mode x (each gradient alone, all together) x every subset of the eight optional outputs not asked for x both widths.
    The restatement's result does not depend on what is left out: it is uploaded once per gradient set and every call is compared
    with it on the device (one boolean per gradient set comes back)."""
    p = S.mode_params(reset, surrogate, detach, adaptive)
    subsets = [frozenset(s) for k in range(len(OUTS) + 1) for s in itertools.combinations(OUTS, k)]
    assert len(subsets) == 256
    for N, periods in ((132, (44, 132, 4, 1, 12)), (65, (13, 65, 1, 5, 65))):            # the 16-byte and the 4-byte kernel
        x, state, grads = case(5, N, 7)
        d = Direct(5, N, p, x, state, params(periods, 7))
        assert 0 < d.ref.s_out.mean() < 1
        for which, use in Q.GRAD_SETS.items():
            r = d.reference(grads, use)
            want = [None if a is None else bits(dev(a)) for a in r]
            ins = [dev(g) for g in S.pick(grads, use, p)]
            ok = torch.ones((), dtype=torch.bool, device='cuda')
            sentinel = bits(torch.full((N,), SENTINEL, device='cuda'))
            for null in subsets:
                outs = [torch.full((5, N), SENTINEL, device='cuda')] + [torch.full((N,), SENTINEL, device='cuda') for _ in OUTS]
                d.call_backward(ins, outs, null)
                ok &= (bits(outs[0]) == want[0]).all()
                for n, t, w in zip(OUTS, outs[1:], want[1:]):
                    ok &= (bits(t) == (sentinel if n in null or w is None else w)).all()
            assert bool(ok), (p, N, which)
            assert np.count_nonzero(r.g_x) > 0 or (which == 'g_alast' and not adaptive)


def test_null_state_is_zeros(be):
    for N, periods in ((64, (64, 1, 16, 4, 32)), (65, (65, 5, 13, 1, 65))):
        x, state, grads = case(5, N, 0)
        q = params(periods, 0)
        zeros = np.zeros(N, F)
        for p in (Params(adaptive=True), Params()):
            a = Direct(5, N, p, x, (None, None, None), q)
            b = Direct(5, N, p, x, (zeros, zeros, zeros), q)
            assert all(same_bits(host(getattr(a, n)), host(getattr(b, n))) for n in Q.Forward._fields)
            for given in itertools.product((False, True), repeat=3):
                Direct(5, N, p, x, tuple(s if g else None for s, g in zip(state, given)), q).backward(grads)
            ra, rb = a.backward(grads), b.backward(grads)
            assert all(x is None or same_bits(x, y) for x, y in zip(ra, rb))


def test_forward_without_the_saved_arrays(be):
    """h_save NULL: a_save is not written either; c_save alone NULL; v_seq NULL."""
    x, state, _ = case(5, 64, 0)
    q = params((64, 32, 1, 16, 4), 0)
    for p in (Params(adaptive=True), Params()):
        Direct(5, 64, p, x, state, q, save=False, want_c=False)
        Direct(5, 64, p, x, state, q, save=False, want_v=False)
        Direct(5, 64, p, x, state, q, want_c=False).backward(case(5, 64, 0)[2], null=('g_sd_slot',))


# ======================================================================================================== crafted values
@pytest.mark.parametrize('adaptive', (False, True))
def test_on_the_threshold(be, adaptive):
    """h == th_i spikes and one ulp under does not: with differing per-neuron base thresholds, and with a per-neuron kappa that
    raises th."""
    zeros = np.zeros(4, F)
    if not adaptive:
        vth = np.array([1.0, 1.0, 1.5, 1.5], F)
        q = (np.array([0.5], F), np.array([0.5], F), vth, np.array([0.9], F), np.array([0.3], F))
        x0, state, p = vth.copy(), (zeros, zeros, None), Params()
    else:
        kappa = np.array([0.25, 0.25, 0.5, 0.5], F)
        q = (np.array([0.5], F), np.array([0.5], F), np.array([1.0], F), np.array([0.75], F), kappa)
        x0, state, p = (F(1.0) + kappa * F(2.0)).astype(F), (zeros, zeros, np.full(4, 2.0, F)), Params(adaptive=True)
        assert x0.tolist() == [1.5, 1.5, 2.0, 2.0]
    x0[1::2] = np.nextafter(x0[1::2], F(0))
    x = np.stack([x0, zeros])
    d = Direct(2, 4, p, x, state, q)
    assert host(d.s_out)[0].tolist() == [1.0, 0.0, 1.0, 0.0]
    d.backward((np.ones((2, 4), F), None, None, None, None), use=(True, False, False, False, False))


def test_nan_stays_in_its_slot(be):
    """A NaN in one element of a per-neuron parameter, and in one input: every other slot's outputs are those of the clean call."""
    T, N = 5, 64
    x, state, grads = case(T, N, 5)
    p = Params(adaptive=True)
    q = params((N,) * 5, 5)
    clean = Direct(T, N, p, x, state, q)
    rc = clean.backward(grads)
    for k in range(6):
        x2, q2 = x, list(q)
        if k < 5:
            q2[k] = q[k].copy()
            q2[k][9] = np.nan
        else:
            x2 = x.copy()
            x2[1, 9] = np.nan
        d = Direct(T, N, p, x2, state, tuple(q2))
        rb = d.backward(grads)
        keep = np.arange(N) != 9
        assert all(same_bits(a[..., keep], b[..., keep]) for a, b in zip(d.ref, clean.ref))
        assert all(same_bits(a[..., keep], b[..., keep]) for a, b in zip(rb, rc))
        assert any(np.isnan(a[..., 9]).any() for a in tuple(d.ref) + tuple(rb))     # (a NaN kappa shows backwards alone: th is NaN)


def test_infinite_threshold_per_neuron(be):
    """v_th = inf in some slots: no spike there, and every gradient stays finite."""
    T, N = 5, 64
    x, state, grads = case(T, N, 6)
    q = list(params((N,) * 5, 6))
    q[2] = q[2].copy()
    q[2][::3] = np.inf
    for sur in S.SURROGATES:
        for adaptive in (False, True):
            p = Params(adaptive=adaptive, surrogate=sur, alpha=2.0 if sur == 'triangle' else 10.0)
            d = Direct(T, N, p, x, state, tuple(q))
            r = d.backward(grads)
            assert d.ref.s_out[:, ::3].sum() == 0 and d.ref.s_out.sum() > 0
            assert all(a is None or np.isfinite(a).all() for a in r) and np.abs(r.g_x[:, ::3]).max() > 0


@pytest.mark.parametrize('reset,surrogate,detach,adaptive', Q.MODES[::5])
def test_one_element_parameters_equal_the_float_entry_points(be, reset, surrogate, detach, adaptive):
    from brainevent_amd import _array as A, _lib
    p = S.mode_params(reset, surrogate, detach, adaptive)
    for N in (64, 65):
        T = 6
        x, state, grads = case(T, N, 8)
        d = Direct(T, N, p, x, state, Q.shared_params(p))
        r = d.backward(grads)
        st = [dev(a) for a in state]
        s, v_seq, h, th, g_x = (torch.empty(T, N, device='cuda') for _ in range(5))
        c_last, v_last, a_last, g_c0, g_v0, g_a0 = (torch.empty(N, device='cuda') for _ in range(6))
        scal = (p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa)
        xd, gd = dev(x), [dev(g) for g in S.pick(grads, ALL, p)]                   # (held: a freed block would be handed out again)
        rc = _lib.fn('be_lif_syn_sg_forward')(A.ptr(xd), *[A.ptr(t) for t in st], *[A.ptr(t) for t in (s, v_seq, h, th, c_last, v_last, a_last)],
                                              T, N, *scal, RESET[reset], int(adaptive), A.stream_ptr())
        assert rc == 0
        rc = _lib.fn('be_lif_syn_sg_backward')(A.ptr(h), A.ptr(th), *[A.ptr(t) for t in gd], A.ptr(g_x), A.ptr(g_c0),
                                               A.ptr(g_v0), A.ptr(g_a0), T, N, *scal, RESET[reset], SURROGATE[surrogate], p.alpha,
                                               int(adaptive), int(detach), A.stream_ptr())
        assert rc == 0
        f = d.ref
        pairs = [(s, f.s_out), (v_seq, f.v_seq), (h, f.h_save), (c_last, f.c_last), (v_last, f.v_last), (g_x, r.g_x), (g_c0, r.g_c0),
                 (g_v0, r.g_v0)]
        if adaptive:
            q = Q.shared_params(p)
            pairs += [(a_last, f.a_last), (g_a0, r.g_a0), (th, (q[2] + q[4] * f.a_save).astype(F))]
        assert all(same_bits(host(a), b) for a, b in pairs)


# ======================================================================================================== C error codes
def test_c_error_codes_then_a_clean_call(be):
    from brainevent_amd import _array as A, _lib
    fwd, bwd = (_lib.fn(f'be_lif_syn_sg_{n}_params') for n in ('forward', 'backward'))
    T, N = 3, 64
    periods = (32, 16, 64, 1, 8)
    xn, state, grads = case(T, N, 0)
    qn = params(periods, 0)
    ptr = A.ptr
    x, (c0, v0, a0), g = dev(xn), [dev(a) for a in state], [dev(a) for a in grads]
    q = [dev(a) for a in qn]
    big = [torch.full((T, N), 7.0, device='cuda') for _ in range(6)]
    small = [torch.full((N,), 7.0, device='cuda') for _ in range(11)]
    s, v_seq, h, c_save, a_save, g_x = big
    c_last, v_last, a_last, g_c0, g_v0, g_a0, *slots = small
    null, st = ptr(None), A.stream_ptr()

    def forward(T=T, N=N, mode=0, adaptive=1, **over):
        arg = lambda name, t: over.get(name, ptr(t))
        pq = [v for name, t, P in zip(Q.NAMES, q, periods) for v in (arg(name, t), over.get('P_' + name, P))]
        return fwd(arg('x', x), ptr(c0), ptr(v0), ptr(a0), *pq, arg('s', s), ptr(v_seq), arg('h', h), ptr(c_save), arg('a_save', a_save),
                   arg('c_last', c_last), arg('v_last', v_last), arg('a_last', a_last), T, N, 0.0, mode, adaptive, st)

    def backward(T=T, N=N, mode=0, sur=0, alpha=10.0, adaptive=1, **over):
        arg = lambda name, t: over.get(name, ptr(t))
        pq = [v for name, t, P in zip(Q.NAMES, q, periods) for v in (arg(name, t), over.get('P_' + name, P))]
        return bwd(arg('h', h), arg('c_save', c_save), arg('a_save', a_save), ptr(c0), ptr(v0), *[ptr(t) for t in g], *pq, arg('g_x', g_x),
                   ptr(g_c0), ptr(g_v0), ptr(g_a0), *[ptr(t) for t in slots], T, N, 0.0, mode, sur, alpha, adaptive, 0, st)

    bad_periods = tuple(dict([('P_' + n, v)]) for n in Q.NAMES for v in (0, -1, 3, 128))
    nulls = tuple(dict([(n, null)]) for n in Q.NAMES)
    for bad in bad_periods + nulls + (dict(x=null), dict(s=null), dict(c_last=null), dict(v_last=null), dict(a_last=null),
                                      dict(a_save=null), dict(T=-1), dict(N=-1), dict(mode=2)):
        assert forward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_syn_sg_forward_params: ')
    for bad in bad_periods + nulls + (dict(h=null), dict(g_x=null), dict(a_save=null), dict(c_save=null), dict(T=-1), dict(N=-1),
                                      dict(mode=2), dict(sur=3), dict(alpha=0.0), dict(alpha=float('nan'))):
        assert backward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_syn_sg_backward_params: ')
    # a zero period is refused also where there is nothing to do; without adaptation rho / kappa and their periods are not looked at
    assert forward(T=0, P_beta=0) == INVALID and backward(N=0, P_syn_decay=0) == INVALID
    assert forward(T=0) == 0 and forward(N=0) == 0 and forward(T=0, x=null, beta=null, s=null, v_last=null) == 0
    assert backward(T=0) == 0 and backward(N=0) == 0 and backward(N=0, h=null, g_x=null) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in big + small)
    # clean calls after the refused ones: adaptive, then not adaptive with the adaptation's arguments unusable
    p = Params(adaptive=True)
    f = Q.forward(xn, *state, qn, p)
    assert forward() == 0
    assert all(same_bits(host(a), b) for a, b in zip((s, v_seq, h, c_save, a_save, c_last, v_last, a_last), f))
    r = Q.backward(f.h_save, f.c_save, f.a_save, state[0], state[1], *grads, qn, p)
    assert backward() == 0
    assert all(same_bits(host(a), b) for a, b in zip([g_x, g_c0, g_v0, g_a0] + slots, r))
    p = Params()
    f = Q.forward(xn, state[0], state[1], None, qn, p)
    for t in (a_save, a_last):
        t.fill_(7.0)
    assert forward(adaptive=0, rho=null, kappa=null, P_rho=0, P_kappa=7) == 0
    assert all(same_bits(host(a), b) for a, b in zip((s, v_seq, h, c_save, c_last, v_last), (f.s_out, f.v_seq, f.h_save, f.c_save, f.c_last, f.v_last)))
    assert bool((a_save == 7.0).all()) and bool((a_last == 7.0).all())


# ======================================================================================================== through Python
def mode_kwargs(p):
    return dict(v_reset=p.v_reset, reset=p.reset, surrogate=p.surrogate, alpha=p.alpha, detach_reset=p.detach_reset)


def reference(T, B, n, seed, periods, p):
    """The restatement's two passes for ``x [T, B, n]`` and parameters with ``periods``: inputs, forward, slots."""
    N = B * n
    x, state, grads = case(T, N, seed)
    q = params(tuple(periods), seed)
    st = (state[0], state[1], state[2] if p.adaptive else None)
    f = Q.forward(x, *st, q, p)
    r = Q.backward(f.h_save, f.c_save, f.a_save, st[0], st[1], *S.pick(grads, ALL, p), q, p)
    return x, st, grads, q, f, r


def run_sequence(be, T, B, n, x, st, q_t, p, **kw):
    state = tuple(dev(a.reshape(B, n)) for a in st if a is not None)
    adapt = (q_t[3], q_t[4]) if p.adaptive else None
    return be.parametric_synaptic_lif_sequence(dev(x.reshape(T, B, n)), state, syn_decay=q_t[0], beta=q_t[1], v_th=q_t[2], adapt=adapt,
                                               return_v=True, **mode_kwargs(p), **kw)


def out_grads(T, B, n, grads, p):
    g = [dev(grads[0].reshape(T, B, n)), dev(grads[1].reshape(T, B, n))] + [dev(a.reshape(B, n)) for a in grads[2:]]
    return g if p.adaptive else g[:4]


def flat_outs(outs):
    return list(outs[:2]) + list(outs[2])


@pytest.mark.parametrize('shape', ['0-d', '[1]', '[n]', '[B, n]'])
@pytest.mark.parametrize('leaf', (True, False))
def test_parameter_gradients(be, shape, leaf):
    """Each parameter's .grad for a leaf and a non-leaf (a scaled leaf), in the parameter's own shape: within the reduce's bound
    of the restatement's per-slot partials."""
    T, B, n = 5, 3, 44
    P = {'0-d': 1, '[1]': 1, '[n]': n, '[B, n]': B * n}[shape]
    view = {'0-d': (), '[1]': (1,), '[n]': (n,), '[B, n]': (B, n)}[shape]
    for p in (Params(adaptive=True, v_reset=-0.25), Params(adaptive=True, reset='soft', surrogate='atan')):
        x, st, grads, q, f, r = reference(T, B, n, 9, (P,) * 5, p)
        if leaf:
            leaves = [dev(a.reshape(view)).requires_grad_() for a in q]
            q_t = leaves
        else:                                    # exact: a power of two
            leaves = [dev((a * F(2)).reshape(view)).requires_grad_() for a in q]
            q_t = [w * 0.5 for w in leaves]
            assert all(same_bits(host(t).reshape(-1), a) for t, a in zip(q_t, q))
        outs = flat_outs(run_sequence(be, T, B, n, x, st, q_t, p))
        assert same_bits(host(outs[0]).reshape(T, -1), f.s_out) and same_bits(host(outs[1]).reshape(T, -1), f.v_seq)
        got = torch.autograd.grad(outs, leaves, out_grads(T, B, n, grads, p))
        for name, g, slot in zip(Q.NAMES, got, r[4:]):
            assert tuple(g.shape) == view, name
            scaled = (slot * F(0.5)).astype(F) if not leaf else slot
            assert Q.within_reduce_bound(host(g), scaled, P) and np.count_nonzero(host(g)) > 0, (name, shape, leaf)


def test_only_what_requires_grad_gets_a_gradient(be, monkeypatch):
    """beta and kappa alone are leaves: the other slot pointers go in as NULL, c_save is not kept, and x / the state get theirs."""
    from brainevent_amd import _neuron_syn_sg
    seen = {}
    real = _neuron_syn_sg.call

    def spy(name, *args):
        seen[name] = [getattr(a, 'value', a) for a in args]
        return real(name, *args)
    monkeypatch.setattr(_neuron_syn_sg, 'call', spy)
    T, B, n = 4, 2, 44
    p = Params(adaptive=True)
    x, st, grads, q, f, r = reference(T, B, n, 10, (n, n, 1, 1, n), p)
    q_t = [dev(a) for a in q]
    q_t[1].requires_grad_(), q_t[4].requires_grad_()
    outs = flat_outs(run_sequence(be, T, B, n, x, st, q_t, p))
    assert seen['be_lif_syn_sg_forward_params'][17] is None                       # c_save
    sum((o * g).sum() for o, g in zip(outs, out_grads(T, B, n, grads, p))).backward()
    slots = seen['be_lif_syn_sg_backward_params'][24:29]
    assert [s is None for s in slots] == [True, False, True, True, False] and seen['be_lif_syn_sg_backward_params'][1] is None
    assert [t.grad is None for t in q_t] == [True, False, True, True, False]
    assert Q.within_reduce_bound(host(q_t[1].grad), r.g_beta_slot, n) and Q.within_reduce_bound(host(q_t[4].grad), r.g_kappa_slot, n)


@pytest.mark.parametrize('reset,surrogate,detach,adaptive', Q.MODES[::5])
def test_sequence_equals_steps(be, reset, surrogate, detach, adaptive):
    """Outputs, g_x and the state gradients bit for bit; the parameter gradients within the any-order f32 bound of their T * R
    terms, since autograd adds the per-step gradients in another order than the kernel adds a slot's steps."""
    T, B, n = 6, 3, 44
    p = S.mode_params(reset, surrogate, detach, adaptive)
    periods = (n, 1, n, n, 1)
    x, st, grads, q, f, r = reference(T, B, n, 11, periods, p)
    info = Q.backward(f.h_save, f.c_save, f.a_save, st[0], st[1], *S.pick(grads, ALL, p), q, p, with_bound=True)[1]
    k = 5 if adaptive else 3

    def leaves():
        return ([dev(x.reshape(T, B, n)).requires_grad_()] + [dev(a.reshape(B, n)).requires_grad_() for a in st if a is not None],
                [dev(a).requires_grad_() for a in q])

    (xa, *sa), qa = leaves()
    adapt = lambda qq: (qq[3], qq[4]) if adaptive else None
    outs_a = flat_outs(be.parametric_synaptic_lif_sequence(xa, tuple(sa), syn_decay=qa[0], beta=qa[1], v_th=qa[2], adapt=adapt(qa),
                                                           return_v=True, **mode_kwargs(p)))
    (xb, *sb), qb = leaves()
    state, ss, vs = tuple(sb), [], []
    for t in range(T):
        s, state = be.parametric_synaptic_lif_step(state, xb[t], syn_decay=qb[0], beta=qb[1], v_th=qb[2], adapt=adapt(qb), **mode_kwargs(p))
        ss.append(s)
        vs.append(state[1])
    outs_b = [torch.stack(ss), torch.stack(vs)] + list(state)
    assert all(same_bits(host(a), host(b)) for a, b in zip(outs_a, outs_b))
    assert same_bits(host(outs_a[0]).reshape(T, -1), f.s_out)
    gs = out_grads(T, B, n, grads, p)
    ga = torch.autograd.grad(outs_a, [xa] + sa + qa[:k], gs)
    gb = torch.autograd.grad(outs_b, [xb] + sb + qb[:k], gs)
    ns = 1 + len(sa)
    assert all(same_bits(host(a), host(b)) for a, b in zip(ga[:ns], gb[:ns])) and same_bits(host(ga[0]).reshape(T, -1), r.g_x)
    for name, a, b, P in zip(Q.NAMES[:k], ga[ns:], gb[ns:], periods):
        bound = Q.any_order_bound(info[f'{name}_terms'], P)
        diff = np.abs(host(a).astype(np.float64) - host(b)).reshape(-1)
        print(f'{name}: max difference {diff.max():.3e}, bound there {bound[diff.argmax()]:.3e}')
        assert (diff <= bound).all() and np.count_nonzero(host(a)) > 0, name


def test_no_grad_keeps_nothing(be, monkeypatch):
    from brainevent_amd import _neuron_syn_sg
    saved = []
    real = _neuron_syn_sg.call

    def spy(name, *args):
        if name == 'be_lif_syn_sg_forward_params':
            saved.append([args[k].value for k in (16, 17, 18)])             # h_save, c_save, a_save
        return real(name, *args)
    monkeypatch.setattr(_neuron_syn_sg, 'call', spy)
    T, B, n = 4, 3, 44
    p = Params(adaptive=True)
    x, st, grads, q, f, r = reference(T, B, n, 0, (n,) * 5, p)
    q_t = [dev(a).requires_grad_() for a in q]
    want = flat_outs(run_sequence(be, T, B, n, x, st, q_t, p))
    assert all(v is not None for v in saved[-1]) and all(o.grad_fn is not None for o in want)
    with torch.no_grad():
        got = flat_outs(run_sequence(be, T, B, n, x, st, q_t, p))
    fixed = flat_outs(run_sequence(be, T, B, n, x, st, [t.detach() for t in q_t], p))     # heterogeneous, nothing requires grad
    assert saved[-2:] == [[None, None, None]] * 2
    for outs in (got, fixed):
        assert all(o.grad_fn is None and not o.requires_grad for o in outs)
        assert all(same_bits(host(a), host(b)) for a, b in zip(outs, want))
    assert same_bits(host(want[0]).reshape(T, -1), f.s_out)


def test_capture_forward_and_backward_follows_in_place_updates(be):
    """A captured forward + backward step, replayed with new inputs and then after ``beta.data.mul_(0.5)`` and
    ``kappa.data.add_(0.1)``: the replay follows the new values, so nothing went through the host when the graph was recorded."""
    T, B, n = 3, 2, 100
    N = B * n
    p = Params(adaptive=True, reset='soft', surrogate='atan')
    kw = mode_kwargs(p)
    x_in = torch.zeros(T, B, n, device='cuda')
    st_in = [torch.zeros(B, n, device='cuda') for _ in range(3)]
    g_in = [torch.zeros(T, B, n, device='cuda'), torch.zeros(T, B, n, device='cuda')] + [torch.zeros(B, n, device='cuda') for _ in range(3)]
    q0 = params((n, n, 1, 1, n), 2)
    sd, beta, v_th, rho, kappa = (torch.nn.Parameter(dev(a)) for a in q0)
    leaves = [sd, beta, v_th, rho, kappa]

    def step():
        x = x_in.detach().requires_grad_()
        st = [t.detach().requires_grad_() for t in st_in]
        s, v_seq, last = be.parametric_synaptic_lif_sequence(x, tuple(st), syn_decay=sd, beta=beta, v_th=v_th, adapt=(rho, kappa),
                                                             return_v=True, **kw)
        outs = (s, v_seq) + tuple(last)
        return outs + tuple(torch.autograd.grad(outs, [x] + st + leaves, g_in))

    def load(seed):
        x, state, grads = case(T, N, seed)
        for t, a in zip([x_in] + st_in + g_in, (x,) + state + grads):
            t.copy_(dev(a).reshape(t.shape))

    load(1)
    graphed = be.capture_step(step)
    replays = []
    for seed, update in ((2, False), (3, False), (3, True)):
        load(seed)
        if update:
            beta.data.mul_(0.5)
            kappa.data.add_(0.1)
        got = [t.detach().clone() for t in graphed()]
        want = step()
        assert all(same_bits(host(a), host(b)) for a, b in zip(got, want))
        assert 0 < float(got[0].mean()) < 1 and all(torch.count_nonzero(g).item() > 0 for g in got[-5:])
        replays.append(got)
    assert not same_bits(host(replays[1][1]), host(replays[2][1]))                 # the membranes moved
    x, state, grads = case(T, N, 3)
    qn = (q0[0], (q0[1] * F(0.5)).astype(F), q0[2], q0[3], (q0[4] + F(0.1)).astype(F))
    assert same_bits(host(beta), qn[1]) and same_bits(host(kappa), qn[4])
    f = Q.forward(x, *state, qn, p)
    r = Q.backward(f.h_save, f.c_save, f.a_save, state[0], state[1], *grads, qn, p)
    assert same_bits(host(want[0]).reshape(T, N), f.s_out) and same_bits(host(want[1]).reshape(T, N), f.v_seq)
    assert same_bits(host(want[5]).reshape(T, N), r.g_x)
    for g, slot, P in zip(want[-5:], r[4:], (n, n, 1, 1, n)):
        assert Q.within_reduce_bound(host(g), slot, P)


def test_non_contiguous_parameter_is_made_contiguous(be):
    """kappa as a column of an [n, 2] leaf: the values are the column's, and the gradient comes back into the column."""
    T, B, n = 4, 2, 44
    p = Params(adaptive=True)
    x, st, grads, q, f, r = reference(T, B, n, 12, (1, n, 1, 1, n), p)
    wide = dev(np.stack([q[4], np.zeros_like(q[4])], axis=1)).requires_grad_()
    kappa = wide[:, 0]
    assert not kappa.is_contiguous()
    outs = flat_outs(run_sequence(be, T, B, n, x, st, [float(q[0][0]), dev(q[1]), 1.0 * float(q[2][0]), float(q[3][0]), kappa], p))
    assert same_bits(host(outs[0]).reshape(T, -1), f.s_out) and same_bits(host(outs[4]).reshape(-1), f.a_last)
    g, = torch.autograd.grad(outs, [wide], out_grads(T, B, n, grads, p))
    g = host(g)
    assert g.shape == (n, 2) and Q.within_reduce_bound(g[:, 0], r.g_kappa_slot, n) and np.count_nonzero(g[:, 0]) and not g[:, 1].any()
