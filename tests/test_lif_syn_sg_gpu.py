"""The differentiable neuron with a synaptic current and an adaptive threshold (csrc/be_neuron_sg.hip,
brainevent_amd/_neuron_syn_sg.py) on the device, compared with the numpy restatement of tests/lif_syn_sg_cases.py as EQUALITIES,
bit for bit (``lif_sg_cases.same_bits``): every operation of both passes is an individually rounded IEEE f32 add, multiply,
divide, abs or compare.  Nothing here is compared with torch's device kernels.  tests/test_lif_syn_sg_cpu.py holds the
restatement to CPU autograd and the sizes used here to the kernels' source."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_sg_cases as C0
import lif_syn_sg_cases as C
from lif_syn_sg_cases import F, Params, same_bits

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ALL = C.GRAD_SETS['all']
STATE_OUT = ('g_c0', 'g_v0', 'g_a0')


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()          # (a copy: the shared inputs are read-only)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def misaligned(a):
    """The same values as a contiguous device tensor whose base is 4 bytes past a 16-byte boundary (a sliced view)."""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device='cuda')
    flat[1:].copy_(torch.tensor(np.asarray(a).reshape(-1)))
    view = flat[1:].view(a.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def case(T, N, seed):
    """Seeded inputs of one size (shared and left unchanged: the arrays are read-only)."""
    x, state, grads = C.inputs(T, N, seed)
    for a in (x,) + state + grads:
        a.setflags(write=False)
    return x, state, grads


# ======================================================================================================== the direct C call
class Direct:
    """``be_lif_syn_sg_forward`` on device copies of ``x`` and ``state`` (entries may be None: NULL), then any number of
    ``be_lif_syn_sg_backward`` calls on what it saved; every output is compared with the restatement.  ``off``: the names of the
    arrays whose base is put 4 bytes past a 16-byte boundary ('all': every one).  Every output buffer starts filled with
    SENTINEL; without adaptation the adaptation's buffers are passed all the same and must stay so."""

    def __init__(self, T, N, p, x, state, off=(), save=True, want_v=True):
        from brainevent_amd import _array as A, _lib
        self.A, self.lib, self.T, self.N, self.p, self.off = A, _lib, T, N, p, off
        self.bwd = _lib.fn('be_lif_syn_sg_backward')
        self.ref = C.forward(x, state[0], state[1], state[2] if p.adaptive else None, p)
        ins = [self.given('x', x)] + [self.given(n, a) for n, a in zip(('c0', 'v0', 'a0'), state)]
        self.s_out, self.v_seq, self.h_save, self.th_save = (self.out(n, (T, N)) for n in ('s_out', 'v_seq', 'h_save', 'th_save'))
        self.c_last, self.v_last, self.a_last = (self.out(n, (N,)) for n in ('c_last', 'v_last', 'a_last'))
        outs = [self.s_out, self.v_seq if want_v else None, self.h_save if save else None, self.th_save if save else None,
                self.c_last, self.v_last, self.a_last]
        rc = _lib.fn('be_lif_syn_sg_forward')(*[A.ptr(t) for t in ins + outs], T, N, *self.scalars(), RESET[p.reset],
                                              int(p.adaptive), A.stream_ptr())
        assert rc == 0, _lib.last_error()
        r, what = self.ref, (T, N, p, off)
        assert same_bits(host(self.s_out), r.s_out) and same_bits(host(self.c_last), r.c_last), what
        assert same_bits(host(self.v_last), r.v_last), what
        self.same_or_untouched(self.v_seq, r.v_seq if want_v else None, what)
        self.same_or_untouched(self.h_save, r.h_save if save else None, what)
        self.same_or_untouched(self.th_save, r.th_save if save else None, what)
        self.same_or_untouched(self.a_last, r.a_last, what)

    def scalars(self):
        p = self.p
        return p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa

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

    def backward(self, grads, use=ALL, null=()):
        """One backward call: ``use`` picks the gradients that arrive, ``null`` names the state gradients not asked for."""
        A, T, N, p = self.A, self.T, self.N, self.p
        r = C.backward(self.ref.h_save, self.ref.th_save, *C.pick(grads, use, p), p)
        ins = [self.given(n, g if u else None) for n, g, u in zip(C.GRADS, grads, use)]
        g_x = self.out('g_x', (T, N))
        state = [self.out(n, (N,)) for n in STATE_OUT]
        rc = self.bwd(A.ptr(self.h_save), A.ptr(self.th_save), *[A.ptr(t) for t in ins], A.ptr(g_x),
                      *[A.ptr(None if n in null else t) for n, t in zip(STATE_OUT, state)], T, N, *self.scalars(), RESET[p.reset],
                      SURROGATE[p.surrogate], p.alpha, int(p.adaptive), int(p.detach_reset), A.stream_ptr())
        assert rc == 0, self.lib.last_error()
        what = (T, N, p, self.off, use, null)
        assert same_bits(host(g_x), r.g_x), what
        for n, t, want in zip(STATE_OUT, state, r[1:]):
            self.same_or_untouched(t, None if n in null else want, (n,) + what)
        return r


RESET = {'hard': 0, 'soft': 1}
SURROGATE = {'fast_sigmoid': 0, 'atan': 1, 'triangle': 2}


def check_direct(T, N, p, seed=0, off=(), use=ALL, null=()):
    x, state, grads = case(T, N, seed)
    d = Direct(T, N, p, x, state, off=off)
    return d.ref, d.backward(grads, use, null)


# ======================================================================================================== sizes
@pytest.mark.parametrize('N', C.N_SIZES)
def test_sizes(be, N):
    """One slot, a wave less one, a wave, a wave and one; one step, two, every ring's depth and its neighbours, and 25."""
    for T in C.T_SIZES:
        for p in (Params(adaptive=True), Params(reset='soft', surrogate='atan', v_reset=-0.25)):
            f, b = check_direct(T, N, p)
    assert N < 8 or (0 < f.s_out.mean() < 1 and np.abs(b.g_x).max() > 0)


@pytest.mark.parametrize('N', C.N_PAST_ONE_PASS)
def test_past_one_pass_of_the_capped_grid(be, N):
    """A second trip of the grid-stride loop: of the 4-byte kernel (one slot) and of the 16-byte kernel (one lane)."""
    f, _ = check_direct(2, N, Params(adaptive=True, surrogate='triangle', alpha=2.0), seed=3)
    assert 0.1 < f.s_out.mean() < 0.6


@pytest.mark.parametrize('off', (('x',), ('th_save',), 'all'))
def test_base_off_16_bytes(be, off):
    """N % 4 == 0 and one base — an input, the saved threshold (an output forwards, an input backwards), every array — 4 bytes
    past a 16-byte boundary: only the alignment refuses the 16-byte kernels."""
    for T in (1, 6):
        check_direct(T, 64, Params(adaptive=True), off=off)
        check_direct(T, 64, Params(reset='soft', surrogate='triangle', alpha=2.0), off=off)


def test_the_scalar_tail(be):
    for T in (1, 6):
        for off in ((), 'all'):
            check_direct(T, 67, Params(adaptive=True), off=off)


# ======================================================================================================== modes
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', C.MODES)
def test_modes_gradient_sets_and_null_outputs(be, reset, surrogate, detach, adaptive):
    """Every mode x (each gradient alone, all together) x every subset of the state gradients not asked for x both widths."""
    p = C.mode_params(reset, surrogate, detach, adaptive)
    subsets = [s for k in range(4) for s in itertools.combinations(STATE_OUT, k)]
    for N in (132, 65):                  # the 16-byte and the 4-byte kernel
        x, state, grads = case(5, N, 7)
        d = Direct(5, N, p, x, state)
        assert 0 < d.ref.s_out.mean() < 1
        for which, use in C.GRAD_SETS.items():
            for null in subsets:
                r = d.backward(grads, use, null)
            assert np.count_nonzero(r.g_x) > 0 or (which == 'g_alast' and not adaptive)


def test_null_state_is_zeros(be):
    for N in (64, 65):
        x, state, grads = case(5, N, 0)
        zeros = np.zeros(N, F)
        for p in (Params(adaptive=True), Params()):
            a = Direct(5, N, p, x, (None, None, None))
            b = Direct(5, N, p, x, (zeros, zeros, zeros))
            assert all(same_bits(host(getattr(a, n)), host(getattr(b, n))) for n in C.Forward._fields)
            for given in itertools.product((False, True), repeat=3):            # any one of them alone, too
                Direct(5, N, p, x, tuple(s if g else None for s, g in zip(state, given)))
            a.backward(grads, use=(True, False, False, False, False))
            b.backward((grads[0], None, zeros, zeros, zeros), use=(True, False, True, True, True))


def test_forward_without_the_saved_arrays(be):
    """h_save NULL (no backward pass): nothing is written to th_save either; v_seq NULL."""
    x, state, _ = case(5, 64, 0)
    for p in (Params(adaptive=True), Params()):
        Direct(5, 64, p, x, state, save=False)
        Direct(5, 64, p, x, state, save=False, want_v=False)


# ======================================================================================================== edge values
@pytest.mark.parametrize('adaptive', (False, True))
def test_threshold_exactly(be, adaptive):
    p, x, state, want = C.threshold_case(adaptive)
    d = Direct(2, 2, p, x, state)
    assert host(d.s_out)[0].tolist() == want['s0'] == [1.0, 0.0]
    if adaptive:
        assert host(d.th_save)[0].tolist() == [1.5, 1.5] and host(d.th_save)[1].tolist() == want['th1'] == [1.625, 1.375]
    d.backward((np.ones((2, 2), F), None, None, None, None), use=(True, False, False, False, False))


def test_the_surrogate_peak(be):
    """u = 0 is where each surrogate is largest: 1, alpha / 2, alpha."""
    u = np.linspace(-0.5, 0.5, 101).astype(F)
    assert u[50] == 0
    zeros = torch.zeros(101, device='cuda')
    for sur, peak in (('fast_sigmoid', 1.0), ('atan', 5.0), ('triangle', 10.0)):
        for adaptive, th in ((False, 1.0), (True, 1.5)):
            p = Params(surrogate=sur, detach_reset=True, kappa=0.25, adaptive=adaptive)
            xt = dev(u + F(th)).requires_grad_()
            state = (zeros, zeros) + ((torch.full((101,), 2.0, device='cuda'),) if adaptive else ())
            s, _ = be.synaptic_lif_step(state, xt, **p.kwargs())
            g, = torch.autograd.grad(s, xt, torch.ones_like(s))
            g = host(g)
            f = C.forward((u + F(th))[None], None, None, np.full(101, 2.0, F), p)
            assert same_bits(g[None], C.backward(f.h_save, f.th_save, np.ones((1, 101), F), None, None, None, None, p).g_x)
            assert g.argmax() == 50 and g[50] == F(peak) and (g[:50] <= g[50]).all() and (g >= 0).all(), sur


@pytest.mark.parametrize('drive,rate', ((0.0, 0.0), (3.0, 1.0)))
def test_no_spike_at_all_and_a_spike_at_every_step(be, drive, rate):
    T, N = 6, 68
    x = np.full((T, N), drive, F)
    grads = case(T, N, 0)[2]
    for reset, surrogate, detach, adaptive in C.MODES:
        d = Direct(T, N, Params(reset=reset, surrogate=surrogate, detach_reset=detach, adaptive=adaptive), x, (None, None, None))
        assert d.ref.s_out.mean() == rate
        d.backward(grads)


def test_nan_stays_in_its_slot(be):
    T, N = 5, 72
    x, state, grads = case(T, N, 0)
    x = x.copy()
    x[1, 3] = x[0, 70] = np.nan
    for reset, adaptive in itertools.product(C.RESETS, (False, True)):
        p = Params(reset=reset, adaptive=adaptive)
        d = Direct(T, N, p, x, state)
        r = d.backward(grads)
        nan = np.isnan(host(d.v_seq))
        assert nan[1:, 3].all() and not nan[0, 3] and nan[:, 70].all() and nan.sum() == 4 + 5
        assert host(d.s_out)[1:, 3].sum() == 0 and host(d.s_out)[:, 70].sum() == 0
        for out in (d.h_save, d.c_last, d.v_last) + ((d.th_save, d.a_last) if adaptive else ()):
            cols = np.flatnonzero(np.isnan(host(out)).reshape(-1, N).any(axis=0))
            assert set(cols) <= {3, 70}
        assert list(np.flatnonzero(np.isnan(host(d.v_last)))) == [3, 70]
        for g in r:                                   # (the device's gradients equal these: Direct.backward compared them)
            if g is not None:
                cols = np.flatnonzero(np.isnan(g).reshape(-1, N).any(axis=0))
                assert list(cols) == [3, 70]


def test_infinite_threshold_is_a_leaky_integrator_readout(be):
    """v_th = inf: no spike, v_seq is the filtered membrane, and the gradient through it is finite — every surrogate is 0 at -inf."""
    T, N = 6, 68
    x, _, grads = case(T, N, 0)
    for sur in C.SURROGATES:
        p = Params(v_th=float('inf'), surrogate=sur)
        xt = dev(x).requires_grad_()
        s, v_seq, (c, v) = be.synaptic_lif_sequence(xt, return_v=True, **p.kwargs())
        f = C.forward(x, None, None, None, p)
        assert not host(s).any() and same_bits(host(v_seq), f.v_seq) and same_bits(f.v_seq, f.h_save)
        gx, = torch.autograd.grad([s, v_seq], [xt], [dev(grads[0]), dev(grads[1])])
        r = C.backward(f.h_save, None, grads[0], grads[1], None, None, None, p)
        assert np.isfinite(host(gx)).all() and same_bits(host(gx), r.g_x) and np.count_nonzero(r.g_x) == r.g_x.size


def test_no_step_and_no_slot(be):
    s, (c, v, a) = be.synaptic_lif_sequence(torch.empty(0, 5, device='cuda'), (None, torch.ones(5, device='cuda'), None),
                                            syn_decay=0.8, beta=0.9, adapt=(0.95, 0.3))
    assert s.shape == (0, 5) and host(v).tolist() == [1.0] * 5 and host(c).tolist() == host(a).tolist() == [0.0] * 5
    c0 = torch.ones(5, device='cuda', requires_grad=True)                      # ... and so do its gradients
    s, v_seq, (c, v) = be.synaptic_lif_sequence(torch.empty(0, 5, device='cuda'), (c0, None), syn_decay=0.8, beta=0.9, return_v=True)
    g, = torch.autograd.grad([c, v], [c0], [torch.full((5,), 3.0, device='cuda'), torch.ones(5, device='cuda')])
    assert v_seq.shape == (0, 5) and host(g).tolist() == [3.0] * 5
    s, (c, v) = be.synaptic_lif_sequence(torch.empty(3, 0, device='cuda'), syn_decay=0.8, beta=0.9)
    assert s.shape == (3, 0) and c.shape == v.shape == (0,)


# ======================================================================================================== C error codes
def test_c_error_codes_each_followed_by_a_clean_call(be):
    from brainevent_amd import _array as A, _lib
    fwd, bwd = _lib.fn('be_lif_syn_sg_forward'), _lib.fn('be_lif_syn_sg_backward')
    T, N = 3, 64
    x, state, grads = case(T, N, 0)
    p = Params(adaptive=True)
    ref = C.forward(x, *state, p)
    rb = C.backward(ref.h_save, ref.th_save, *grads, p)
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    ins = [dev(a) for a in (x,) + state]
    gin = [dev(g) for g in grads]
    big = [torch.full((T, N), SENTINEL, device='cuda') for _ in range(5)]          # s_out, v_seq, h_save, th_save, g_x
    small = [torch.full((N,), SENTINEL, device='cuda') for _ in range(6)]          # c_last, v_last, a_last, g_c0, g_v0, g_a0
    s_out, v_seq, h_save, th_save, g_x = big
    c_last, v_last, a_last, g_c0, g_v0, g_a0 = small
    INVALID = -1

    def forward(x=P(ins[0]), s_out=P(s_out), h_save=P(h_save), th_save=P(th_save), c_last=P(c_last), v_last=P(v_last),
                a_last=P(a_last), T=T, N=N, mode=0, adaptive=1):
        return fwd(x, P(ins[1]), P(ins[2]), P(ins[3]), s_out, P(v_seq), h_save, th_save, c_last, v_last, a_last, T, N, 0.8, 0.9, 1.0,
                   0.0, 0.95, 0.3, mode, adaptive, st)

    def backward(h_save=P(h_save), th_save=P(th_save), g_x=P(g_x), T=T, N=N, mode=0, sur=0, alpha=10.0, adaptive=1):
        return bwd(h_save, th_save, *[P(g) for g in gin], g_x, P(g_c0), P(g_v0), P(g_a0), T, N, 0.8, 0.9, 1.0, 0.0, 0.95, 0.3, mode,
                   sur, alpha, adaptive, 0, st)

    # nothing to do: BE_OK and nothing written, whatever the pointers
    assert forward(T=0) == 0 and forward(N=0) == 0 and forward(T=0, x=null, s_out=null, c_last=null, v_last=null, a_last=null) == 0
    assert backward(T=0) == 0 and backward(N=0) == 0 and backward(N=0, h_save=null, th_save=null, g_x=null) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in big + small)
    for bad in (dict(x=null), dict(s_out=null), dict(c_last=null), dict(v_last=null), dict(a_last=null), dict(th_save=null),
                dict(T=-1), dict(N=-1), dict(mode=2), dict(mode=-1)):
        assert forward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_syn_sg_forward: '), _lib.last_error()
        assert forward() == 0                                                  # a clean call after each refused one
    # what adaptive alone makes required is not required without it; th_save is not required where h_save is not given
    assert forward(a_last=null, th_save=null, adaptive=0) == 0 and forward(h_save=null, th_save=null) == 0 and forward() == 0
    for bad in (dict(h_save=null), dict(g_x=null), dict(th_save=null), dict(T=-1), dict(N=-1), dict(mode=2), dict(mode=-1),
                dict(sur=3), dict(sur=-1), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float('nan'))):
        assert backward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_syn_sg_backward: '), _lib.last_error()
        assert backward() == 0
    got = [host(t) for t in (s_out, v_seq, h_save, th_save, c_last, v_last, a_last, g_x, g_c0, g_v0, g_a0)]
    assert all(same_bits(a, b) for a, b in zip(got, tuple(ref) + tuple(rb)))


# ======================================================================================================== the Python functions
def leaves(arrays, wrap=dev, shape=None):
    return [None if a is None else wrap(a if shape is None else a.reshape(a.shape[:a.ndim - 1] + tuple(shape))).requires_grad_()
            for a in arrays]


def check_sequence(be, T, N, p, shape=None, seed=0, wrap=dev, use=ALL):
    """synaptic_lif_sequence forwards and backwards against the restatement."""
    x, state, grads = case(T, N, seed)
    n = 3 if p.adaptive else 2
    slots = (N,) if shape is None else tuple(shape)
    xt, *st = leaves((x,) + state[:n], wrap, slots)
    s, v_seq, last = be.synaptic_lif_sequence(xt, tuple(st), return_v=True, **p.kwargs())
    f = C.forward(x, *state[:n], *(None,) * (3 - n), p)
    assert s.shape == v_seq.shape == xt.shape and len(last) == n and all(t.shape == slots for t in last) and s.dtype == torch.float32
    for got, want in zip((s, v_seq) + tuple(last), (f.s_out, f.v_seq, f.c_last, f.v_last, f.a_last)):
        assert same_bits(host(got).reshape(want.shape), want), (T, N, p, shape)
    given = C.pick(grads, use, p)
    outs = [(o, g) for o, g in zip((s, v_seq) + tuple(last), given) if g is not None]
    got = torch.autograd.grad([o for o, _ in outs], [xt] + st, [wrap(g.reshape(o.shape)) for o, g in outs])
    r = C.backward(f.h_save, f.th_save, *given, p)
    for g, want in zip(got, r):
        assert same_bits(host(g).reshape(want.shape), want), (T, N, p, shape)


@pytest.mark.parametrize('shape', C.SHAPES)
def test_shapes(be, shape):
    N = int(np.prod(shape))
    for p in (Params(adaptive=True), Params(reset='soft')):
        check_sequence(be, 3, N, p, shape=shape)
        x, state, grads = case(1, N, 0)
        n = 3 if p.adaptive else 2
        xt, *st = leaves((x[0],) + state[:n], shape=shape)
        s, new = be.synaptic_lif_step(tuple(st), xt, **p.kwargs())
        assert s.shape == tuple(shape) and len(new) == n and all(t.shape == tuple(shape) for t in new)
        f = C.forward(x, *state[:n], *(None,) * (3 - n), p)
        given = C.pick(grads, (True, False, True, True, True), p)
        r = C.backward(f.h_save, f.th_save, *given, p)
        got = torch.autograd.grad([s] + list(new), [xt] + st, [dev(g.reshape(shape)) for g in given if g is not None])
        for a, b in zip([s] + list(new) + list(got), (f.s_out, f.c_last, f.v_last, f.a_last)[:n + 1] + tuple(r)):
            assert same_bits(host(a).reshape(b.shape), b)


def test_misaligned_and_non_contiguous_tensors(be):
    for N in (64, 67):
        check_sequence(be, 6, N, Params(adaptive=True), wrap=misaligned)
    # a non-contiguous input or state entry is made contiguous
    T, N = 3, 64
    x, state, _ = case(T, N, 0)
    p = Params(adaptive=True)
    xt = dev(np.ascontiguousarray(x.T)).T
    st = tuple(dev(np.repeat(a, 2))[::2] for a in state)
    assert not xt.is_contiguous() and not any(t.is_contiguous() for t in st)
    s, last = be.synaptic_lif_sequence(xt, st, **p.kwargs())
    f = C.forward(x, *state, p)
    assert same_bits(host(s), f.s_out) and all(same_bits(host(a), b) for a, b in zip(last, (f.c_last, f.v_last, f.a_last)))
    s1, new = be.synaptic_lif_step(st, xt[0], **p.kwargs())
    f1 = C.forward(x[:1], *state, p)
    assert same_bits(host(s1), f1.s_out[0]) and all(same_bits(host(a), b) for a, b in zip(new, (f1.c_last, f1.v_last, f1.a_last)))


def spy_on(monkeypatch):
    from brainevent_amd import _neuron_syn_sg
    calls = []
    real = _neuron_syn_sg.call

    def spy(name, *args):
        calls.append((name, [a.value if isinstance(a, ctypes.c_void_p) else a for a in args]))
        return real(name, *args)
    monkeypatch.setattr(_neuron_syn_sg, 'call', spy)
    return calls


def test_gradients_asked_for_and_gradients_that_arrive(be, monkeypatch):
    """A state input that does not require grad gets a NULL output pointer and None; an unused output's gradient goes in as NULL."""
    calls = spy_on(monkeypatch)
    T, N = 3, 64
    x, state, grads = case(T, N, 0)
    p = Params(adaptive=True)
    for needs in itertools.product((False, True), repeat=4):
        if not any(needs):
            continue
        ins = [dev(a).requires_grad_(n) for a, n in zip((x,) + state, needs)]
        s, v_seq, last = be.synaptic_lif_sequence(ins[0], tuple(ins[1:]), return_v=True, **p.kwargs())
        calls.clear()
        got = torch.autograd.grad([s, v_seq] + list(last), [t for t, n in zip(ins, needs) if n], [dev(g) for g in grads])
        (name, args), = calls
        assert name == 'be_lif_syn_sg_backward' and all(a is not None for a in args[:8])
        assert [a is not None for a in args[8:11]] == list(needs[1:]), needs
        f = C.forward(x, *state, p)
        r = C.backward(f.h_save, f.th_save, *grads, p)
        assert all(same_bits(host(g), want) for g, want in zip(got, [w for w, n in zip(r, needs) if n]))
    for which, use in C.GRAD_SETS.items():
        ins = [dev(a).requires_grad_() for a in (x,) + state]
        s, v_seq, last = be.synaptic_lif_sequence(ins[0], tuple(ins[1:]), return_v=True, **p.kwargs())
        picked = [(o, dev(g)) for o, g, u in zip([s, v_seq] + list(last), grads, use) if u]
        calls.clear()
        torch.autograd.grad([o for o, _ in picked], ins, [g for _, g in picked])
        (name, args), = calls
        assert [a is not None for a in args[2:7]] == list(use), which
    # without adaptation the adaptation's pointers are NULL in both calls
    calls.clear()
    xt = dev(x).requires_grad_()
    s, (c, v) = be.synaptic_lif_sequence(xt, **Params().kwargs())
    torch.autograd.grad([s, c], [xt], [dev(grads[0]), dev(grads[2])])
    (_, a), (_, b) = calls
    assert [a[i] for i in (1, 2, 3, 5, 7, 10)] == [None] * 6 and a[6] is not None and a[20] == 0
    assert [b[i] for i in (1, 3, 5, 6, 8, 9, 10)] == [None] * 7 and b[2] is not None and b[4] is not None and b[22] == 0


def test_no_grad_keeps_nothing(be, monkeypatch):
    calls = spy_on(monkeypatch)
    x, state, _ = case(4, 132, 0)
    p = Params(adaptive=True)
    ins = [dev(a).requires_grad_() for a in (x,) + state]
    flat = lambda outs: list(outs[:-1]) + list(outs[-1])
    want = flat(be.synaptic_lif_sequence(ins[0], tuple(ins[1:]), return_v=True, **p.kwargs()))
    assert calls[-1][1][6] is not None and calls[-1][1][7] is not None and all(o.grad_fn is not None for o in want)
    with torch.no_grad():
        got = flat(be.synaptic_lif_sequence(ins[0], tuple(ins[1:]), return_v=True, **p.kwargs()))
        got1 = flat(be.synaptic_lif_step(tuple(ins[1:]), ins[0][0], **p.kwargs()))
    plain = flat(be.synaptic_lif_sequence(dev(x), tuple(dev(a) for a in state), return_v=True, **p.kwargs()))   # nothing requires grad
    assert [(c[1][6], c[1][7]) for c in calls[-3:]] == [(None, None)] * 3
    for outs in (got, plain):
        assert all(o.grad_fn is None and not o.requires_grad for o in outs)
        assert all(same_bits(host(a), host(b)) for a, b in zip(outs, want))
    assert same_bits(host(got1[0]), host(want[0][0])) and all(o.grad_fn is None for o in got1)


# ======================================================================================================== cross-checks
@pytest.mark.parametrize('reset,surrogate', (('hard', 'fast_sigmoid'), ('soft', 'atan'), ('hard', 'atan'), ('soft', 'fast_sigmoid')))
def test_without_a_filter_it_is_lif_sequence(be, reset, surrogate):
    """syn_decay = 0, no adaptation, no start current: the s, v_seq, v_last, g_x, g_v0 of be.lif_sequence on the same x (inputs
    and gradients without zeros of either sign: 0 * c + x turns a negative zero into a positive one)."""
    T, N = 7, 132
    x, v0, g_s, g_vseq, g_vlast = C0.inputs(T, N, 3)
    assert all(np.count_nonzero(a) == a.size for a in (x, v0, g_s, g_vseq, g_vlast))
    kw = dict(beta=0.9, v_th=1.0, v_reset=-0.25, reset=reset, surrogate=surrogate, alpha=10.0)
    gs = [dev(g_s), dev(g_vseq), dev(g_vlast)]
    for with_v0 in (False, True):
        xa, xb = dev(x).requires_grad_(), dev(x).requires_grad_()
        va, vb = (dev(v0).requires_grad_(), dev(v0).requires_grad_()) if with_v0 else (None, None)
        s0, vseq0, vlast0 = be.lif_sequence(xa, va, return_v=True, **kw)
        s1, vseq1, (_, vlast1) = be.synaptic_lif_sequence(xb, (None, vb) if with_v0 else None, syn_decay=0.0, return_v=True, **kw)
        assert all(same_bits(host(a), host(b)) for a, b in ((s0, s1), (vseq0, vseq1), (vlast0, vlast1)))
        g0 = torch.autograd.grad([s0, vseq0, vlast0], [xa, va] if with_v0 else [xa], gs)
        g1 = torch.autograd.grad([s1, vseq1, vlast1], [xb, vb] if with_v0 else [xb], gs)
        assert all(same_bits(host(a), host(b)) and torch.count_nonzero(a).item() > 0 for a, b in zip(g0, g1))
    assert 0 < float(s0.detach().mean()) < 1


@pytest.mark.parametrize('reset,surrogate,detach,adaptive', C.MODES[::5] + C.MODES[1::7])
def test_sequence_equals_steps(be, reset, surrogate, detach, adaptive):
    T, N = 6, 132
    p = C.mode_params(reset, surrogate, detach, adaptive)
    n = 3 if adaptive else 2
    x, state, grads = case(T, N, 11)
    gs = [dev(g) for g in C.pick(grads, ALL, p) if g is not None]
    xa, *sa = leaves((x,) + state[:n])
    s, v_seq, last = be.synaptic_lif_sequence(xa, tuple(sa), return_v=True, **p.kwargs())
    outs_a = [s, v_seq] + list(last)
    xb, *sb = leaves((x,) + state[:n])
    st, ss, vs = tuple(sb), [], []
    for t in range(T):
        s, st = be.synaptic_lif_step(st, xb[t], **p.kwargs())
        ss.append(s)
        vs.append(st[1])
    outs_b = [torch.stack(ss), torch.stack(vs)] + list(st)
    assert len(outs_a) == len(outs_b) == 2 + n
    for a, b in zip(outs_a, outs_b):
        assert same_bits(host(a), host(b))
    # (a membrane's gradient is the sum of two, what the next step hands back and g_vseq[t]: the same sum in either order)
    ga = torch.autograd.grad(outs_a, [xa] + sa, gs)
    gb = torch.autograd.grad(outs_b, [xb] + sb, gs)
    assert len(ga) == 1 + n
    for a, b in zip(ga, gb):
        assert same_bits(host(a), host(b)) and torch.count_nonzero(a).item() > 0


# ======================================================================================================== integration
class HostNeuron(torch.autograd.Function):
    """synaptic_lif_step (adaptive) with both passes computed by the restatement on the host."""

    @staticmethod
    def forward(ctx, c, v, a, x, p):
        ctx.set_materialize_grads(False)
        f = C.forward(host(x).reshape(1, -1), *(host(t).reshape(-1) for t in (c, v, a)), p)
        ctx.f, ctx.p, ctx.shape = f, p, x.shape
        return tuple(dev(t).reshape(x.shape) for t in (f.s_out, f.c_last, f.v_last, f.a_last))

    @staticmethod
    def backward(ctx, g_s, g_c, g_v, g_a):
        flat = lambda g, shape: None if g is None else host(g).reshape(shape)
        r = C.backward(ctx.f.h_save, ctx.f.th_save, flat(g_s, (1, -1)), None, flat(g_c, -1), flat(g_v, -1), flat(g_a, -1), ctx.p)
        return tuple(dev(g).reshape(ctx.shape) for g in (r.g_c0, r.g_v0, r.g_a0, r.g_x)) + (None,)


def test_recurrent_loop_through_a_csr_parameter(be):
    """BinaryArray(s) @ csr -> synaptic_lif_step (adaptive), three steps, a Parameter in the CSR: w.grad, x.grad and the state's
    gradients equal the same loop with the neuron computed on the host.  (Weights, parameters and sums are small dyadic numbers:
    the scatter's sums are exact in any order.)"""
    rng = np.random.default_rng(21)
    batch, n, n_conn, T = 4, 96, 12, 3
    indptr = torch.arange(n + 1, dtype=torch.int32, device='cuda') * n_conn
    indices = dev(rng.integers(0, n, n * n_conn).astype(np.int32))
    w0 = (rng.integers(-8, 9, n * n_conn) / 32.0).astype(F)
    x0 = (rng.integers(0, 48, (T, batch, n)) / 32.0).astype(F)
    state0 = [(rng.integers(lo, hi, (batch, n)) / 32.0).astype(F) for lo, hi in ((-8, 16), (-16, 32), (0, 48))]
    g_out = [(rng.integers(-8, 9, (batch, n)) / 8.0).astype(F) for _ in range(4)]
    p = Params(syn_decay=0.5, beta=0.5, rho=0.75, kappa=0.25, adaptive=True)

    def loop(neuron):
        w = torch.nn.Parameter(dev(w0))
        csr = be.CSR((w, indices, indptr), shape=(n, n))
        x = dev(x0).requires_grad_()
        start = [dev(a).requires_grad_() for a in state0]
        state, s, rate = tuple(start), torch.zeros(batch, n, device='cuda'), []
        for t in range(T):
            s, state = neuron(state, x[t] + be.BinaryArray(s) @ csr)
            rate.append(float(s.detach().mean()))
        sum((o * dev(g)).sum() for o, g in zip((s,) + tuple(state), g_out)).backward()
        return rate, [host(t) for t in (s,) + tuple(state) + (w.grad, x.grad) + tuple(t.grad for t in start)]

    def on_host(state, i):
        s, *new = HostNeuron.apply(*state, i, p)
        return s, tuple(new)

    rate_a, a = loop(lambda state, i: be.synaptic_lif_step(state, i, **p.kwargs()))
    rate_b, b = loop(on_host)
    assert all(0.05 < r < 0.95 for r in rate_a) and rate_a == rate_b
    names = ('s', 'c', 'v', 'a', 'w.grad', 'x.grad', 'c0.grad', 'v0.grad', 'a0.grad')
    for name, i, j in zip(names, a, b):
        assert same_bits(i, j) and np.count_nonzero(i) > 0, name


# ======================================================================================================== graph capture
def test_capture_forward_and_backward(be):
    T, N = 3, 200
    p = Params(reset='soft', surrogate='atan', adaptive=True)
    x_in = torch.zeros(T, N, device='cuda')
    state_in = [torch.zeros(N, device='cuda') for _ in range(3)]
    g_in = [torch.zeros(T, N, device='cuda'), torch.zeros(T, N, device='cuda')] + [torch.zeros(N, device='cuda') for _ in range(3)]

    def step():
        x = x_in.detach().requires_grad_()                                       # leaves of this call, on the static memory
        start = [t.detach().requires_grad_() for t in state_in]
        s, state = be.synaptic_lif_step(tuple(start), x[0], **p.kwargs())
        s_all, v_seq, last = be.synaptic_lif_sequence(x, state, return_v=True, **p.kwargs())
        outs = (s_all, v_seq) + tuple(last)
        return (s,) + outs + tuple(torch.autograd.grad(outs, [x] + start, g_in))

    def load(seed):
        x, state, grads = case(T, N, seed)
        for t, a in zip([x_in] + state_in + g_in, (x,) + state + grads):
            t.copy_(dev(a))

    load(1)
    graphed = be.capture_step(step)
    for seed in (2, 3):
        load(seed)
        got = [t.detach().clone() for t in graphed()]
        want = step()
        assert all(same_bits(host(a), host(b)) for a, b in zip(got, want))
        assert 0 < float(got[1].mean()) < 1 and all(torch.count_nonzero(g).item() > 0 for g in got[-4:])
    x, state, grads = case(T, N, 3)                                              # ... and the eager result is the restatement's
    f1 = C.forward(x[:1], *state, p)
    f = C.forward(x, f1.c_last, f1.v_last, f1.a_last, p)
    r = C.backward(f.h_save, f.th_save, *grads, p)
    assert same_bits(host(want[1]), f.s_out) and same_bits(host(want[5]), f.a_last) and same_bits(host(want[6])[1:], r.g_x[1:])
