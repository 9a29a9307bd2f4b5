"""The recurrent spiking layer with synaptic delays (csrc/be_neuron_sg_rec_delay.hip, brainevent_amd/_neuron_rec_sg.py) on the
device, compared with the numpy restatement of tests/lif_rec_delay_cases.py.  Forward outputs and the saved ``h`` / ``th`` are
compared as EQUALITIES, bit for bit (``same_bits``): the recurrent sums are 64-bit integers, every other operation an individually
rounded f32 one.  Gradients are compared within the restatement's propagated bound (the order of the device's f32 gathers is its
own).  Nothing here is compared with torch's device kernels.  tests/test_lif_rec_delay_cpu.py holds the restatement to CPU autograd
and the sizes used here to the kernels' source."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_rec_delay_cases as D
import lif_rec_sg_cases as R
import lif_syn_sg_cases as S
from lif_rec_delay_cases import F, same_bits
from lif_syn_sg_cases import Params

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ALL = S.GRAD_SETS['all']
STATE_OUT = ('g_c0', 'g_v0', 'g_a0', 'g_s_hist')
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
def case(T, B, N, A, seed):
    """Seeded inputs of one size and the history ``[A, B, N]`` (None for A = 0); shared and left unchanged."""
    x, _, state, grads = D.inputs(T, B, N, seed)
    hist = D.history(A, B, N, seed + 1000)
    for a in (x,) + state + grads + (() if hist is None else (hist,)):
        a.setflags(write=False)
    return x, hist, state, grads


@functools.lru_cache(maxsize=None)
def delayed(kind, N, depth, delays='random', seed=0):
    """One of the test matrices split by delay, and the exponent the library chooses for its stacked matrix."""
    build = {'random': lambda: R.random_matrix(N, seed), 'dyadic': lambda: R.dyadic_matrix(N, seed), 'empty': lambda: R.empty_matrix(N),
             'crafted': lambda: R.crafted_matrix(N), 'parallel': lambda: D.parallel_matrix(N, seed),
             'dense': lambda: R.random_matrix(N, seed, lo=8, hi=24)}
    m = build[kind]()
    dl = D.split(m, D.delays_for(delays, m, depth, seed + 7), depth)
    return dl, device_exponent(dl)


class DevMatrix:
    """The stacked arrays on the device; a matrix without entries hands over one unused element (the entry points refuse NULL)."""

    def __init__(self, dl):
        st = dl.stacked
        self.w = dev(st.w) if len(st.w) else torch.zeros(1, device='cuda')
        self.indices = dev(st.indices) if len(st.w) else torch.zeros(1, dtype=torch.int32, device='cuda')
        self.indptr = dev(st.indptr)
        self.row_mask = dev(dl.row_mask.view(np.int32))
        self.depth = dl.depth


def device_exponent(dl):
    """The exponent the library chooses for the stacked matrix; the restatement's own rule may land one higher at a power of two,
    never lower."""
    st = dl.stacked
    if len(st.w) == 0:
        return 0
    from brainevent_amd._csr import fixed_point_exponent
    e = fixed_point_exponent(dev(st.w), dev(st.indices), st.n)
    assert D.exponent(st) - 1 <= e <= D.exponent(st)
    return e


def within(got, want, bound, what):
    got = host(got).astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, 'a NaN is a NaN in both, and nowhere else')
    err = np.where(nan, 0.0, np.abs(got - want))
    assert (err <= np.where(nan, 0.0, bound)).all(), (what, float(err.max()), float(bound.flat[err.argmax()]))


# ======================================================================================================== the direct C call
class Direct:
    """``be_lif_rec_delay_sg_forward`` on device copies of the inputs (the history and the state entries may be None: NULL), then any
    number of ``be_lif_rec_delay_sg_backward`` calls on what it saved; every output is compared with the restatement.  Every output
    buffer starts filled with SENTINEL; without adaptation the adaptation's buffers are passed all the same and must stay so."""

    def __init__(self, dl, e, p, x, hist, state, save=True, want_v=True, mask=True):
        from brainevent_amd import _array as A, _lib
        T, B, N = x.shape
        self.A, self.lib, self.dims, self.p, self.dl, self.dm, self.mask = A, _lib, (T, B, N), p, dl, DevMatrix(dl), mask
        self.ages = 0 if hist is None else hist.shape[0]
        self.ref = D.forward(x, dl, hist, state[0], state[1], state[2] if p.adaptive else None, p, e)
        self.s_out, self.v_seq, self.h_save, self.th_save = (full((T, B, N)) for _ in range(4))
        self.c_last, self.v_last, self.a_last = (full((B, N)) for _ in range(3))
        outs = [self.s_out, self.v_seq if want_v else None, self.h_save if save else None, self.th_save if save else None,
                self.c_last, self.v_last, self.a_last]
        ins = [dev(x), dev(hist)] + [dev(a) for a in state]                       # (held until the call has been made)
        rc = _lib.fn('be_lif_rec_delay_sg_forward')(A.ptr(ins[0]), *self.matrix_args(), A.ptr(ins[1]), self.ages,
                                                    *[A.ptr(t) for t in ins[2:]], *[A.ptr(t) for t in outs], T, B, N,
                                                    *self.scalars(), RESET[p.reset], int(p.adaptive), e, A.stream_ptr())
        assert rc == 0, _lib.last_error()
        r, what = self.ref, (self.dims, dl.depth, self.ages, p)
        assert same_bits(host(self.s_out), r.s_out) and same_bits(host(self.c_last), r.c_last), what
        assert same_bits(host(self.v_last), r.v_last), what
        self.same_or_untouched(self.v_seq, r.v_seq if want_v else None, what)
        self.same_or_untouched(self.h_save, r.h_save if save else None, what)
        self.same_or_untouched(self.th_save, r.th_save if save else None, what)
        self.same_or_untouched(self.a_last, r.a_last, what)

    def matrix_args(self):
        A, dm = self.A, self.dm
        return A.ptr(dm.w), A.ptr(dm.indices), A.ptr(dm.indptr), A.ptr(dm.row_mask if self.mask else None), dm.depth

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
        A, (T, B, N), p = self.A, self.dims, self.p
        given = S.pick(grads, use, p)
        r, b = D.backward(self.ref.h_save, self.ref.th_save, self.dl, *given, p, hist_ages=self.ages, with_bound=True)
        ins = [dev(g if u else None) for g, u in zip(grads, use)]
        g_x = full((T, B, N))
        outs = [full((B, N)) for _ in STATE_OUT[:3]] + [full((max(self.ages, 1), B, N))]
        w, indices, indptr, row_mask, depth = self.matrix_args()
        rc = self.lib.fn('be_lif_rec_delay_sg_backward')(
            A.ptr(self.h_save), A.ptr(self.th_save), w, indices, indptr, row_mask, depth, *[A.ptr(t) for t in ins], A.ptr(g_x),
            *[A.ptr(None if n in null else t) for n, t in zip(STATE_OUT, outs)], self.ages, T, B, N, *self.scalars(), RESET[p.reset],
            SURROGATE[p.surrogate], p.alpha, int(p.adaptive), int(p.detach_reset), A.stream_ptr())
        assert rc == 0, self.lib.last_error()
        what = (self.dims, depth, self.ages, p, use, null)
        within(g_x, r.g_x, b.g_x, ('g_x',) + what)
        for n, t, want, bound in zip(STATE_OUT, outs, r[1:], b[1:5]):
            if n in null or want is None:
                assert bool((t == SENTINEL).all()), (n,) + what
            elif n == 'g_s_hist':
                within(t[:self.ages], want, bound, (n,) + what)
                assert bool((t[self.ages:] == SENTINEL).all()), (n,) + what
            else:
                within(t, want, bound, (n,) + what)
        self.g_x, self.state_out = g_x, outs
        return r, b, g_x


def check_direct(dl, e, p, T, B, A, seed=0, use=ALL, null=(), mask=True):
    x, hist, state, grads = case(T, B, dl.m.n, A, seed)
    d = Direct(dl, e, p, x, hist, state, mask=mask)
    return d.ref, d.backward(grads, use, null)[0]


# ======================================================================================================== sizes
COMBOS = list(itertools.product(D.DELAY_KINDS, (0, 1, None), ('random', 'dyadic')))       # (delays, hist_ages (None: depth), weights)


@pytest.mark.parametrize('B', D.B_SIZES)
@pytest.mark.parametrize('N', D.N_SIZES)
def test_sizes(be, N, B):
    """One neuron, a wave less one, a wave, a wave and one, 257 (an odd number of 32-bit mask words), one past the workgroup; 1 and
    3 samples; every (T, depth) pair; the delay patterns, history lengths and weight kinds in rotation: over the twelve cases of this
    test every one of their 18 combinations is met four times."""
    ps = (Params(adaptive=True), Params(reset='soft', surrogate='atan', v_reset=-0.25))
    first = (D.N_SIZES.index(N) * len(D.B_SIZES) + D.B_SIZES.index(B)) * len(D.T_DEPTHS)
    active = 0
    for k, (T, depth) in enumerate(D.T_DEPTHS, first):
        delays, A, kind = COMBOS[k % len(COMBOS)]
        dl, e = delayed(kind, N, depth, delays)
        f, b = check_direct(dl, e, ps[k % 2], T, B, depth if A is None else A)
        active += np.count_nonzero(f.r)
        assert N < 8 or (0 < f.s_out.mean() < 1 and np.abs(b.g_x).max() > 0)
    assert N < 8 or active > 0


def test_the_limits_and_the_rounds(be):
    """N = 8192 at depth 16, T = 2, B = 1 is accepted; with a full history every non-empty stacked row — several times the id list's
    capacity — is active at step 0, so the list is filled and walked in rounds.  N = 8193, and N = 8192 at depth 256 (past the LDS
    rule), are refused with BE_ERR_RANGE by both calls, each followed by a clean call."""
    from brainevent_amd import _array as A, _lib
    N, depth = D.CONSTS['kDelMaxN'], 16
    assert D.fits(N, depth) and not D.fits(N + 1, 1) and not D.fits(N, 256)
    dl, e = delayed('dense', N, depth)
    x, _, state, grads = case(2, 1, N, 0, 0)
    cap = (D.LDS_BYTES - 8 * N - 8 * depth * (N // 64)) // 4
    rows = np.count_nonzero(np.diff(dl.stacked.indptr))
    assert rows > 3 * cap                                                        # more than three rounds at step 0
    d = Direct(dl, e, Params(adaptive=True), x, np.ones((depth, 1, N), F), state)
    r, _, _ = d.backward(grads)
    assert 0.05 < d.ref.s_out.mean() < 0.9 and np.count_nonzero(d.ref.r[0]) > N // 2 and np.abs(r.g_s_hist).max() > 0
    P, st, t = A.ptr, A.stream_ptr(), full((2, 1, N + 1))
    fwd, bwd = _lib.fn('be_lif_rec_delay_sg_forward'), _lib.fn('be_lif_rec_delay_sg_backward')
    for n, dp, word in ((N + 1, 1, '8192'), (N, 256, 'depth 256')):
        dm = DevMatrix(D.split(R.empty_matrix(n), [], dp))
        rc = fwd(P(t), P(dm.w), P(dm.indices), P(dm.indptr), P(dm.row_mask), dp, P(None), 0, P(None), P(None), P(None), P(t), P(None),
                 P(None), P(None), P(t[0]), P(t[0]), P(None), 2, 1, n, 0.8, 0.9, 1.0, 0.0, 0.0, 0.0, 0, 0, 0, st)
        assert rc == RANGE and word in _lib.last_error() and _lib.last_error().startswith('be_lif_rec_delay_sg_forward: ')
        assert 'ceil(N / 64)' in _lib.last_error()
        check_direct(*delayed('random', 65, 2), Params(), 2, 1, 1)
        rc = bwd(P(t), P(None), P(dm.w), P(dm.indices), P(dm.indptr), P(dm.row_mask), dp, P(None), P(None), P(None), P(None), P(None),
                 P(t), P(None), P(None), P(None), P(None), 0, 2, 1, n, 0.8, 0.9, 1.0, 0.0, 0.0, 0.0, 0, 0, 10.0, 0, 0, st)
        assert rc == RANGE and word in _lib.last_error() and _lib.last_error().startswith('be_lif_rec_delay_sg_backward: ')
        check_direct(*delayed('random', 65, 2), Params(), 2, 1, 1)
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all())


# ======================================================================================================== matrices and spikes
@pytest.mark.parametrize('kind', ('parallel', 'crafted', 'empty'))
def test_matrices(be, kind):
    """Parallel synapses (the same (row, col) with different delays) and empty rows; the crafted matrix — a row of 600 entries at
    N = 300, a self-loop, duplicates; no entry at all.  Empty stacked rows everywhere: with row_mask given and with NULL the bits
    are the same, in both passes."""
    N, depth = 300, 7
    dl, e = delayed(kind, N, depth)
    lens = np.diff(dl.stacked.indptr)
    assert (lens == 0).any() and (kind != 'crafted' or np.diff(dl.m.indptr).max() == 600)
    for p, T, B, A in ((Params(adaptive=True), 5, 3, depth), (Params(reset='soft', surrogate='triangle', alpha=2.0), 3, 1, 0)):
        x, hist, state, grads = case(T, B, N, A, 4)
        x = x.copy()
        x[:, :, :8] += 2.0                                               # the crafted rows are active at most steps ...
        if hist is not None:
            hist = hist.copy()
            hist[:, :, :8] = 1                                           # ... and before step 0
        outs = []
        for mask in (True, False):
            d = Direct(dl, e, p, x, hist, state, mask=mask)
            r, _, g_x = d.backward(grads)
            outs.append([host(t) for t in (d.s_out, d.v_seq, d.h_save, d.c_last, d.v_last, g_x) + tuple(d.state_out[:2])] +
                        [host(d.state_out[3])[:A]])
        assert all(same_bits(u, v) for u, v in zip(*outs))
        if kind == 'empty':
            assert not d.ref.r.any() and not r.g_s_hist.any()
        else:
            assert d.ref.s_out[:-1, :, :8].mean() > 0.5 and np.count_nonzero(d.ref.r) > 0 and (A == 0 or np.count_nonzero(r.g_s_hist) > 0)


@pytest.mark.parametrize('A', (0, 7))
def test_a_step_where_every_neuron_fires_and_one_where_none_does(be, A):
    """depth = 7, 8 to 24 entries per row (most stacked rows are not empty): after two steps where every neuron fires the active
    stacked rows outnumber N; then a silent step; with A = 7 a full history before step 0 as well."""
    T, B, N, depth = 6, 3, 257, 7
    dl, e = delayed('dense', N, depth)
    x, hist, state, grads = case(T, B, N, A, 6)
    x = x.copy()
    x[1], x[2], x[3] = 50.0, 50.0, -500.0
    if A:
        hist = np.ones_like(hist)
    act = lambda f, t: D.active_rows(f.s_out, hist, t, depth) & (np.diff(dl.stacked.indptr) > 0)[None]
    for p in (Params(adaptive=True), Params(reset='soft')):
        d = Direct(dl, e, p, x, hist, state)
        f = d.ref
        assert f.s_out[1].all() and f.s_out[2].all() and not f.s_out[3].any() and np.count_nonzero(f.r[4]) > N // 2
        assert act(f, 3).sum(axis=1).min() > N and (not A or act(f, 0).sum(axis=1).min() > 3 * N)
        d.backward(grads)


# ======================================================================================================== modes
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', R.MODES)
def test_modes_and_gradient_sets(be, reset, surrogate, detach, adaptive):
    """Every mode x (each gradient alone, all together)."""
    p = S.mode_params(reset, surrogate, detach, adaptive)
    T, B, N, depth, A = 4, 2, 129, 3, 2
    dl, e = delayed('random', N, depth)
    x, hist, state, grads = case(T, B, N, A, 7)
    d = Direct(dl, e, p, x, hist, state)
    assert 0 < d.ref.s_out.mean() < 1
    for which, use in S.GRAD_SETS.items():
        r, _, _ = d.backward(grads, use)
        assert np.count_nonzero(r.g_x) > 0 or (which == 'g_alast' and not adaptive)


@pytest.mark.parametrize('adaptive', (False, True))
def test_every_subset_of_the_optional_outputs(be, adaptive):
    T, B, N, depth, A = 3, 2, 65, 3, 2
    dl, e = delayed('random', N, depth)
    x, hist, state, grads = case(T, B, N, A, 8)
    p = Params(adaptive=adaptive)
    for save, want_v in itertools.product((False, True), repeat=2):
        d = Direct(dl, e, p, x, hist, state, save=save, want_v=want_v)
    for k in range(len(STATE_OUT) + 1):
        for null in itertools.combinations(STATE_OUT, k):
            d.backward(grads, null=null)
    # a NULL state entry, history or gradient is zeros
    zeros = np.zeros((B, N), F)
    a, b = Direct(dl, e, p, x, None, (None, None, None)), Direct(dl, e, p, x, np.zeros((A, B, N), F), (zeros, zeros, zeros))
    names = ('s_out', 'v_seq', 'h_save', 'c_last', 'v_last') + (('th_save', 'a_last') if adaptive else ())
    assert all(same_bits(host(getattr(a, n)), host(getattr(b, n))) for n in names)
    ga = a.backward(grads, use=(True, False, False, False, False))[2]
    gb = b.backward((grads[0], np.zeros_like(x), zeros, zeros, zeros))[2]
    assert same_bits(host(ga), host(gb))


def test_a_nan_stays_in_its_sample_and_two_calls_give_the_same_bits(be):
    T, B, N, depth, A = 4, 3, 257, 3, 3
    dl, e = delayed('random', N, depth)
    x, hist, state, grads = case(T, B, N, A, 9)
    p = Params(adaptive=True)
    clean = Direct(dl, e, p, x, hist, state)
    g_clean = clean.backward(grads)[2]
    again = Direct(dl, e, p, x, hist, state)
    g_again = again.backward(grads)[2]
    assert same_bits(host(g_clean), host(g_again)) and all(same_bits(host(u), host(v)) for u, v in zip(clean.state_out, again.state_out))
    assert all(same_bits(host(getattr(clean, n)), host(getattr(again, n))) for n in ('s_out', 'v_seq', 'h_save', 'th_save', 'a_last'))
    bad = x.copy()
    bad[1, 1, 5] = np.nan
    d = Direct(dl, e, p, bad, hist, state)
    g = d.backward(grads)[2]
    assert np.isnan(host(d.v_seq)[1:, 1, 5]).all() and np.isnan(host(g)[:, 1]).any()
    for other in (0, 2):
        for u, v in zip((d.s_out, d.v_seq, d.h_save, d.th_save, g), (clean.s_out, clean.v_seq, clean.h_save, clean.th_save, g_clean)):
            assert same_bits(host(u)[:, other], host(v)[:, other])
        for u, v in zip((d.c_last, d.v_last, d.a_last), (clean.c_last, clean.v_last, clean.a_last)):
            assert same_bits(host(u)[other], host(v)[other])
        assert same_bits(host(d.state_out[3])[:, other], host(clean.state_out[3])[:, other])


def test_the_aged_activity_mask(be):
    """``be_grad_pack_activity_aged`` against the restatement, word for word: T * B not a multiple of 32, more than one word, every
    history length, depth above T."""
    from brainevent_amd import _array as A, _lib
    rng = np.random.default_rng(3)
    for T, B, N, depth, ages in ((5, 3, 65, 7, 2), (1, 1, 1, 1, 0), (13, 5, 33, 3, 3), (2, 3, 257, 256, 256), (4, 8, 64, 2, 1)):
        s_out = (rng.random((T, B, N)) < 0.3).astype(F)
        hist = D.history(ages, B, N, 5)
        nw = (T * B + 31) // 32
        assert _lib.fn('be_grad_mask_bytes')(depth * N, T * B) >= depth * N * nw * 4
        mask = torch.full((_lib.fn('be_grad_mask_bytes')(depth * N, T * B) // 4,), -1, dtype=torch.int32, device='cuda')
        d_s, d_hist = dev(s_out), dev(hist)
        rc = _lib.fn('be_grad_pack_activity_aged')(A.ptr(d_s), A.ptr(d_hist), N, B, T, depth, ages, A.ptr(mask), A.stream_ptr())
        assert rc == 0, _lib.last_error()
        got = host(mask)[:depth * N * nw].view(np.uint32).reshape(depth * N, nw)
        assert np.array_equal(got, D.aged_mask(s_out, hist, depth)), (T, B, N, depth, ages)
    null, st = A.ptr(None), A.stream_ptr()
    pack = _lib.fn('be_grad_pack_activity_aged')
    s, m = A.ptr(d_s), A.ptr(mask)
    for bad in ((s, null, 64, 8, 4, 2, 1, m), (null, null, 64, 8, 4, 2, 0, m), (s, null, 64, 8, 4, 2, 0, null), (s, null, 64, 0, 4, 2, 0, m),
                (s, null, 64, 8, 0, 2, 0, m), (s, null, 64, 8, 4, 0, 0, m), (s, null, 64, 8, 4, 257, 0, m), (s, s, 64, 8, 4, 2, 3, m),
                (s, null, 64, 8, 8192, 2, 0, m), (s, null, -1, 8, 4, 2, 0, m)):
        assert pack(*bad, st) == INVALID and _lib.last_error().startswith('be_grad_pack_activity_aged: '), bad
    assert pack(s, null, 64, 8, 4, 2, 0, m, st) == 0


# ======================================================================================================== C error codes
def test_c_error_codes_each_followed_by_a_clean_call(be):
    from brainevent_amd import _array as A, _lib
    fwd, bwd = _lib.fn('be_lif_rec_delay_sg_forward'), _lib.fn('be_lif_rec_delay_sg_backward')
    T, B, N, depth, ages = 3, 2, 64, 3, 2
    dl, e = delayed('random', N, depth)
    x, hist, state, grads = case(T, B, N, ages, 0)
    p = Params(adaptive=True)
    ref = D.forward(x, dl, hist, *state, p, e)
    rb, bb = D.backward(ref.h_save, ref.th_save, dl, *grads, p, hist_ages=ages, with_bound=True)
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    dm = DevMatrix(dl)
    ins = [dev(a) for a in (x, hist) + state]
    gin = [dev(g) for g in grads]
    big = [full((T, B, N)) for _ in range(5)]                                      # s_out, v_seq, h_save, th_save, g_x
    small = [full((B, N)) for _ in range(6)] + [full((ages, B, N))]                # c_last, v_last, a_last, g_c0, g_v0, g_a0, g_s_hist
    s_out, v_seq, h_save, th_save, g_x = big
    c_last, v_last, a_last, g_c0, g_v0, g_a0, g_s_hist = small

    def forward(x=P(ins[0]), w=P(dm.w), indices=P(dm.indices), indptr=P(dm.indptr), row_mask=P(dm.row_mask), depth=depth,
                s_hist=P(ins[1]), ages=ages, s_out=P(s_out), h_save=P(h_save), th_save=P(th_save), c_last=P(c_last), v_last=P(v_last),
                a_last=P(a_last), T=T, B=B, N=N, mode=0, adaptive=1, e=e):
        return fwd(x, w, indices, indptr, row_mask, depth, s_hist, ages, P(ins[2]), P(ins[3]), P(ins[4]), s_out, P(v_seq), h_save,
                   th_save, c_last, v_last, a_last, T, B, N, 0.8, 0.9, 1.0, 0.0, 0.95, 0.3, mode, adaptive, e, st)

    def backward(h_save=P(h_save), th_save=P(th_save), w=P(dm.w), indices=P(dm.indices), indptr=P(dm.indptr), row_mask=P(dm.row_mask),
                 depth=depth, g_x=P(g_x), g_s_hist=P(g_s_hist), ages=ages, T=T, B=B, N=N, mode=0, sur=0, alpha=10.0, adaptive=1):
        return bwd(h_save, th_save, w, indices, indptr, row_mask, depth, *[P(g) for g in gin], g_x, P(g_c0), P(g_v0), P(g_a0), g_s_hist,
                   ages, T, B, N, 0.8, 0.9, 1.0, 0.0, 0.95, 0.3, mode, sur, alpha, adaptive, 0, st)

    # nothing to do: BE_OK and nothing written, whatever the pointers
    assert forward(T=0) == 0 and forward(B=0) == 0 and forward(N=0) == 0
    assert forward(N=0, x=null, w=null, indices=null, indptr=null, row_mask=null, s_out=null, c_last=null, v_last=null, a_last=null) == 0
    assert backward(T=0) == 0 and backward(B=0) == 0 and backward(N=0, h_save=null, th_save=null, w=null, g_x=null) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in big + small)
    for bad in (dict(x=null), dict(s_out=null), dict(c_last=null), dict(v_last=null), dict(a_last=null), dict(th_save=null),
                dict(w=null), dict(indices=null), dict(indptr=null), dict(T=-1), dict(B=-1), dict(N=-1), dict(mode=2), dict(mode=-1),
                dict(e=-91), dict(e=151), dict(depth=0), dict(depth=257), dict(depth=-1), dict(ages=-1), dict(ages=depth + 1),
                dict(s_hist=null), dict(s_hist=null, ages=1)):
        assert forward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_rec_delay_sg_forward: '), _lib.last_error()
        assert forward() == 0                                                  # a clean call after each refused one
    assert forward(N=D.CONSTS['kDelMaxN'] + 1) == RANGE and forward(depth=256, ages=0, N=4096) == RANGE and forward() == 0
    assert forward(a_last=null, th_save=null, adaptive=0) == 0 and forward(h_save=null, th_save=null) == 0 and forward() == 0
    for bad in (dict(h_save=null), dict(g_x=null), dict(th_save=null), dict(w=null), dict(indices=null), dict(indptr=null),
                dict(T=-1), dict(B=-1), dict(N=-1), dict(mode=2), dict(sur=3), dict(sur=-1), dict(alpha=0.0), dict(alpha=float('nan')),
                dict(depth=0), dict(depth=257), dict(ages=-1), dict(ages=depth + 1)):
        assert backward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_rec_delay_sg_backward: '), _lib.last_error()
        assert backward() == 0
    assert backward(N=D.CONSTS['kDelMaxN'] + 1) == RANGE and backward(depth=256, ages=0, N=4096) == RANGE and backward() == 0
    got = [host(t) for t in (s_out, v_seq, h_save, th_save, c_last, v_last, a_last)]
    assert all(same_bits(u, v) for u, v in zip(got, ref[:7]))
    for t, want, bound in zip((g_x, g_c0, g_v0, g_a0, g_s_hist), rb, bb):
        within(t, want, bound, 'after the refusals')


# ======================================================================================================== the Python function
def delayed_of(be, dl, requires_grad=False):
    """``csr.with_delays`` on the device; its stacked arrays must be the restatement's."""
    m = dl.m
    rec = be.CSR((dev(m.w), dev(m.indices), dev(m.indptr)), shape=(m.n, m.n)).with_delays(dev(dl.delays), dl.depth)
    assert np.array_equal(host(rec.stacked.indptr), dl.stacked.indptr) and np.array_equal(host(rec.stacked.indices), dl.stacked.indices)
    assert same_bits(host(rec.stacked.data), dl.stacked.w) and np.array_equal(host(rec.row_mask).view(np.uint32), dl.row_mask)
    if requires_grad:
        rec.stacked.data.requires_grad_()
    return rec


@pytest.mark.parametrize('adaptive', (False, True))
def test_equals_the_loop_of_steps_and_products(be, adaptive):
    """Dyadic weights: forwards bit for bit the loop of ``synaptic_lif_step`` on ``x[t] + sum over d of BinaryArray(s[t-1-d]) @ W_d``
    — what was possible before; the gradients of x, the state, s0 [A, B, N] and rec.stacked.data within the restatement's bound."""
    T, B, N, depth, A = 5, 3, 257, 3, 3
    dl, _ = delayed('dyadic', N, depth)
    x, hist, state, grads = case(T, B, N, A, 11)
    p = Params(adaptive=adaptive)
    n = 3 if adaptive else 2
    rec = delayed_of(be, dl, True)
    w = rec.stacked.data
    leaves = [dev(a).requires_grad_() for a in (x, hist) + state[:n]]
    s, v_seq, last = be.recurrent_lif_sequence(leaves[0], rec, tuple(leaves[2:]), leaves[1], return_v=True, **p.kwargs())
    assert s.shape == v_seq.shape == (T, B, N) and len(last) == n and all(t.shape == (B, N) for t in last)
    with torch.no_grad():
        W = [be.CSR((dev(q.w), dev(q.indices), dev(q.indptr)), shape=(N, N)) for q in (D.of_delay(dl, d) for d in range(depth))]
        st, ss, vs = tuple(dev(a) for a in state[:n]), [], []
        past = lambda tau: ss[tau] if tau >= 0 else dev(hist[-1 - tau])
        for t in range(T):
            r = sum(be.BinaryArray(past(t - 1 - d)) @ W[d] for d in range(depth) if t - 1 - d >= -A)
            sp, st = be.synaptic_lif_step(st, dev(x[t]) + r, **p.kwargs())
            ss.append(sp)
            vs.append(st[1])
    for u, v in zip((s, v_seq) + tuple(last), (torch.stack(ss), torch.stack(vs)) + tuple(st)):
        assert same_bits(host(u), host(v))
    assert 0.05 < float(s.detach().mean()) < 0.6
    # ... and the restatement at the exponent the call chose is the same function
    e = device_exponent(dl)
    f = D.forward(x, dl, hist, *state[:n], *(None,) * (3 - n), p, e)
    assert same_bits(host(s), f.s_out) and same_bits(host(v_seq), f.v_seq) and np.count_nonzero(f.r) > 0
    given = S.pick(grads, ALL, p)
    outs = [(o, g) for o, g in zip((s, v_seq) + tuple(last), given) if g is not None]
    got = torch.autograd.grad([o for o, _ in outs], leaves + [w], [dev(g) for _, g in outs])
    r, b = D.backward(f.h_save, f.th_save, dl, *given, p, hist_ages=A, with_bound=True)
    g_w, b_w = D.weight_grad(dl, f.s_out, hist, r.g_x, b.g_x)
    wants = [('x', r.g_x, b.g_x), ('s0', r.g_s_hist, b.g_s_hist), ('c0', r.g_c0, b.g_c0), ('v0', r.g_v0, b.g_v0)] + \
        ([('a0', r.g_a0, b.g_a0)] if adaptive else []) + [('w', g_w, b_w)]
    assert len(got) == len(wants) and got[1].shape == (A, B, N)
    for g, (name, want, bound) in zip(got, wants):
        within(g, want, bound, name)
        assert np.count_nonzero(want) > 0
    # the weight gradient in the order the synapses were given in
    within(rec.stacked_to_original(got[-1]), D.to_original(dl, g_w), D.to_original(dl, b_w), 'w, original order')
    # s0 [B, N] is age 0 alone, with its gradient in that shape; without s0 the history is silent
    s0 = dev(hist[0]).requires_grad_()
    s1, _ = be.recurrent_lif_sequence(dev(x), rec, None, s0, **p.kwargs())
    g_s0, g_w1 = torch.autograd.grad([s1], [s0, w], [dev(grads[0])])
    f1 = D.forward(x, dl, hist[:1], None, None, None, p, e)
    r1, b1 = D.backward(f1.h_save, f1.th_save, dl, grads[0], None, None, None, None, p, hist_ages=1, with_bound=True)
    assert same_bits(host(s1), f1.s_out) and g_s0.shape == (B, N)
    within(g_s0, r1.g_s_hist[0], b1.g_s_hist[0], 's0 [B, N]')
    within(g_w1, *D.weight_grad(dl, f1.s_out, hist[:1], r1.g_x, b1.g_x), 'w, one age')
    s2, _ = be.recurrent_lif_sequence(dev(x), rec, **p.kwargs())
    assert same_bits(host(s2), D.forward(x, dl, None, None, None, None, p, e).s_out)


def test_without_delays_it_is_the_recurrent_layer(be):
    """depth = 1 with every delay 0 gives the bits of ``recurrent_lif_sequence(x, csr, ...)`` forwards."""
    T, B, N = 4, 3, 257
    m = R.random_matrix(N, 0)
    x, hist, state, _ = case(T, B, N, 1, 12)
    p = Params(adaptive=True)
    csr = be.CSR((dev(m.w), dev(m.indices), dev(m.indptr)), shape=(N, N))
    rec = csr.with_delays(torch.zeros(len(m.w), dtype=torch.int32, device='cuda'), 1)
    start = tuple(dev(a) for a in state)
    a = be.recurrent_lif_sequence(dev(x), csr, start, dev(hist[0]), return_v=True, **p.kwargs())
    b = be.recurrent_lif_sequence(dev(x), rec, start, dev(hist[0]), return_v=True, **p.kwargs())
    c = be.parametric_recurrent_lif_sequence(dev(x), rec, start, dev(hist), return_v=True, **p.kwargs())       # all numbers: delegates
    for u, v, q in zip(a[:2] + a[2], b[:2] + b[2], c[:2] + c[2]):
        assert same_bits(host(u), host(v)) and same_bits(host(u), host(q))
    assert 0.05 < float(a[0].mean()) < 0.6
    with pytest.raises(NotImplementedError, match='together with synaptic delays are not built'):
        be.parametric_recurrent_lif_sequence(dev(x), rec, start, dev(hist), **{**p.kwargs(), 'beta': torch.full((N,), 0.9, device='cuda')})


def test_one_sample_without_a_batch_axis_and_empty_shapes(be):
    T, N, depth, A = 4, 65, 3, 2
    dl, e = delayed('random', N, depth)
    x, hist, state, _ = case(T, 1, N, A, 12)
    rec = delayed_of(be, dl)
    p = Params(adaptive=True)
    a = be.recurrent_lif_sequence(dev(x), rec, tuple(dev(t) for t in state), dev(hist), return_v=True, **p.kwargs())
    b = be.recurrent_lif_sequence(dev(x[:, 0]), rec, tuple(dev(t[0]) for t in state), dev(hist[:, 0]), return_v=True, scale_exp=e,
                                  **p.kwargs())
    assert b[0].shape == b[1].shape == (T, N) and all(t.shape == (N,) for t in b[2])
    for i, j in zip(a[:2] + a[2], b[:2] + b[2]):
        assert same_bits(host(i).reshape(-1), host(j).reshape(-1))
    assert 0 < float(a[0].mean()) < 1
    # no step, no sample: the state passes through, and so do its gradients; the history and the weights get zeros
    kw = dict(beta=0.9)
    xz = torch.zeros(2, 3, N, device='cuda')
    s, (c, v) = be.recurrent_lif_sequence(xz[:0], rec, (None, torch.ones(3, N, device='cuda')), **kw)
    assert s.shape == (0, 3, N) and host(v).tolist() == [[1.0] * N] * 3 and not host(c).any()
    rec_g = delayed_of(be, dl, True)
    c0 = torch.ones(3, N, device='cuda', requires_grad=True)
    s0 = torch.ones(A, 3, N, device='cuda', requires_grad=True)
    s, (c, v) = be.recurrent_lif_sequence(xz[:0], rec_g, (c0, None), s0, **kw)
    g = torch.autograd.grad([c, v], [c0, s0, rec_g.stacked.data], [torch.full((3, N), 3.0, device='cuda'), torch.ones(3, N, device='cuda')])
    assert host(g[0]).tolist() == [[3.0] * N] * 3 and g[1].shape == (A, 3, N) and not host(g[1]).any() and not host(g[2]).any()
    s, (c, v) = be.recurrent_lif_sequence(xz[:, :0], rec, **kw)
    assert s.shape == (2, 0, N) and c.shape == v.shape == (0, N)


def test_weights_changed_in_place_are_seen_and_no_grad_keeps_nothing(be, monkeypatch):
    from brainevent_amd import _neuron_rec_sg
    calls = []
    real = _neuron_rec_sg.call
    monkeypatch.setattr(_neuron_rec_sg, 'call', lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    T, B, N, depth, A = 3, 2, 65, 3, 2
    dl, _ = delayed('dyadic', N, depth)
    x, hist, state, _ = case(T, B, N, A, 13)
    p = Params()
    rec = delayed_of(be, dl, True)
    run = lambda: be.recurrent_lif_sequence(dev(x), rec, None, dev(hist), scale_exp=30, **p.kwargs())[0]
    a = run()
    assert a.grad_fn is not None and calls[-1][0] == 'be_lif_rec_delay_sg_forward' and calls[-1][1][13].value is not None     # h is kept
    with torch.no_grad():
        b = run()
        assert b.grad_fn is None and calls[-1][1][13].value is None and same_bits(host(a), host(b))
        rec.stacked.data.mul_(-2.0)                                      # still dyadic, still far below the exponent's bound
        c = run()
    dl2 = D.split(R.Matrix((dl.m.w * F(-2.0)).astype(F), dl.m.indices, dl.m.indptr, N), dl.delays, depth)
    assert same_bits(host(c), D.forward(x, dl2, hist, None, None, None, p, 30).s_out) and not same_bits(host(c), host(a))


def test_capture_with_a_given_exponent(be):
    T, B, N, depth, A = 3, 2, 200, 3, 2
    dl, e = delayed('random', N, depth)
    p = Params(reset='soft', surrogate='atan', adaptive=True)
    rec = delayed_of(be, dl, True)
    w = rec.stacked.data
    x_in, s0_in = torch.zeros(T, B, N, device='cuda'), torch.zeros(A, B, N, device='cuda')
    state_in = [torch.zeros(B, N, device='cuda') for _ in range(3)]
    g_in = [torch.zeros(T, B, N, device='cuda')] + [torch.zeros(B, N, device='cuda') for _ in range(3)]

    def step():
        x = x_in.detach().requires_grad_()                                       # leaves of this call, on the static memory
        s0 = s0_in.detach().requires_grad_()
        start = [t.detach().requires_grad_() for t in state_in]
        s, last = be.recurrent_lif_sequence(x, rec, tuple(start), s0, scale_exp=e, **p.kwargs())
        outs = (s,) + tuple(last)
        return outs + tuple(torch.autograd.grad(outs, [x, w, s0] + start, g_in))

    def load(seed):
        x, hist, state, grads = case(T, B, N, A, seed)
        for t, a in zip([x_in, s0_in] + state_in + g_in, (x, hist) + state + (grads[0],) + grads[2:]):
            t.copy_(dev(a))

    load(1)
    graphed = be.capture_step(step)
    for seed in (2, 3):
        load(seed)
        got = [t.detach().clone() for t in graphed()]
        want = step()
        assert all(same_bits(host(a), host(b)) for a, b in zip(got, want))
        assert 0 < float(got[0].mean()) < 1 and all(torch.count_nonzero(g).item() > 0 for g in got[-6:])
    x, hist, state, grads = case(T, B, N, A, 3)                                  # ... and the eager result is the restatement's
    f = D.forward(x, dl, hist, *state, p, e)
    assert same_bits(host(want[0]), f.s_out) and same_bits(host(want[3]), f.a_last)
