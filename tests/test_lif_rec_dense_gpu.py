"""The fused recurrent layer with a Dense recurrence (csrc/be_neuron_sg_rec_dense.hip) on the device.  Expected
values come only from tests/lif_rec_sg_cases.py, run on the FULLY STORED matrix of ``W`` (``indices = tile(arange(N), N)``):
forward outputs are compared as equalities, bit for bit; backward outputs within the restatement's propagated bound.  Nothing is
compared with a torch device kernel."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_rec_sg_cases as C
import lif_syn_sg_cases as S
from lif_rec_dense_cases import stored                     # the CSR that stores every entry of W, as the restatement takes it
from lif_rec_sg_cases import F, Params, same_bits
from test_lif_rec_sg_gpu import dev, host, within          # device copy, host copy, |got - want| <= bound with NaN for NaN

pytestmark = pytest.mark.gpu

SENTINEL, PAD = 7.0, 64
RESET = {'hard': 0, 'soft': 1}
SURROGATE = {'fast_sigmoid': 0, 'atan': 1, 'triangle': 2}
INVALID, RANGE = -1, -4
#: a wave's edge, every row-group count (16, 8, 4, 2, 1), past one column per thread, both backward paths past one lane trip
N_SIZES = (1, 63, 64, 65, 129, 260, 513, 1032)
FWD = ('s_out', 'v_seq', 'h_save', 'th_save', 'c_last', 'v_last', 'a_last')
BWD = ('g_x', 'g_c0', 'g_v0', 'g_a0', 'g_s0')


@functools.lru_cache(maxsize=None)
def weights(N, seed=0):
    """N(0, 0.05) weights, a tenth of them exact zeros, one all-zero row and one all-zero column (from 8 neurons on); read-only."""
    rng = np.random.default_rng(seed)
    W = rng.normal(0.0, 0.05, (N, N)).astype(F)
    if N >= 8:
        W[rng.random((N, N)) < 0.1] = 0
        W[N // 2, :] = 0
        W[:, N // 3] = 0
    W.setflags(write=False)
    return W, stored(W)


@functools.lru_cache(maxsize=None)
def case(T, B, N, seed=0):
    x, s0, state, grads = C.inputs(T, B, N, seed)
    for a in (x, s0) + state + grads:
        a.setflags(write=False)
    return x, s0, state, grads


def out(*shape):
    """An output buffer full of SENTINEL with PAD more elements behind it: ``(view, whole)``."""
    n = int(np.prod(shape))
    whole = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device='cuda')
    return whole[:n].view(shape), whole


class Direct:
    """``be_lif_rec_dense_sg_forward`` on device copies, then ``be_lif_rec_dense_sg_backward`` on what it saved; every output against
    the restatement on the stored matrix ``m`` (``stored(W)``, or a sparser pattern with the same dense matrix)."""

    def __init__(self, W, m, p, x, s0, state, e=None):
        from brainevent_amd import _array as A, _lib
        T, B, N = x.shape
        self.A, self.lib, self.dims, self.p, self.m, self.w = A, _lib, (T, B, N), p, m, dev(W)
        self.e = C.exponent(m) if e is None else e
        self.ref = C.forward(x, m, s0, state[0], state[1], state[2] if p.adaptive else None, p, self.e)
        self.ins = [dev(x), self.w, dev(s0)] + [dev(a) for a in state]
        self.outs = dict(zip(FWD, [out(T, B, N) for _ in range(4)] + [out(B, N) for _ in range(3)]))
        rc = _lib.fn('be_lif_rec_dense_sg_forward')(*[A.ptr(t) for t in self.ins], *[A.ptr(self.outs[n][0]) for n in FWD], T, B, N,
                                                    *self.scalars(), RESET[p.reset], int(p.adaptive), self.e, A.stream_ptr())
        assert rc == 0, _lib.last_error()
        self.check(self.outs, self.ref, None)

    def scalars(self):
        p = self.p
        return p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa

    def check(self, outs, ref, bounds):
        """Equal bits (``bounds`` None) or within the bound; an output the mode does not write, and every tail, keeps the SENTINEL."""
        for name, (view, whole) in outs.items():
            want, what = getattr(ref, name), (name, self.dims, self.p)
            if want is None:
                assert bool((whole == SENTINEL).all()), what
                continue
            assert bool((whole[view.numel():] == SENTINEL).all()), what
            if bounds is None:
                assert same_bits(host(view), want), what
            else:
                within(view, want, getattr(bounds, name), what)

    def backward(self, grads, use=S.GRAD_SETS['all']):
        A, (T, B, N), p = self.A, self.dims, self.p
        r, b = C.backward(self.ref.h_save, self.ref.th_save, self.m, *S.pick(grads, use, p), p, with_bound=True)
        outs = dict(zip(BWD, [out(T, B, N)] + [out(B, N) for _ in range(4)]))
        gin = [dev(g if u else None) for g, u in zip(grads, use)]                     # (kept alive over the call)
        rc = self.lib.fn('be_lif_rec_dense_sg_backward')(
            A.ptr(self.outs['h_save'][0]), A.ptr(self.outs['th_save'][0]), A.ptr(self.w), *[A.ptr(g) for g in gin],
            *[A.ptr(outs[n][0]) for n in BWD], T, B, N, *self.scalars(), RESET[p.reset], SURROGATE[p.surrogate], p.alpha,
            int(p.adaptive), int(p.detach_reset), A.stream_ptr())
        assert rc == 0, self.lib.last_error()
        self.check(outs, r, b)
        return r, outs


@pytest.mark.parametrize('N', N_SIZES)
def test_sizes(be, N):
    """1 and 3 samples, 1, 2, 3 and 5 steps (one pair at the two largest N), s0 given and NULL, both passes, every output."""
    W, m = weights(N)
    ps = (Params(adaptive=True), Params(reset='soft', surrogate='atan', v_reset=-0.25))
    pairs = list(itertools.product((1, 3), (1, 2, 3, 5))) if N < 513 else [(3, 5)] * 2
    fired = recurrent = grad = False
    for k, (B, T) in enumerate(pairs):
        x, s0, state, grads = case(T, B, N)
        d = Direct(W, m, ps[k % 2], x, s0 if k % 2 == 0 else None, state)
        r, _ = d.backward(grads)
        fired |= bool(d.ref.s_out[:-1].any())
        recurrent |= bool(np.count_nonzero(d.ref.r))
        grad |= bool(np.count_nonzero(r.g_x))
    assert fired and recurrent and grad, 'a silent network cannot pass'


@pytest.mark.parametrize('N', (63, 260, 513))
def test_forward_bits_equal_the_csr_kernel_on_the_stored_matrix(be, N):
    from brainevent_amd import _array as A, _lib
    T, B = 3, 3
    W, m = weights(N)
    x, s0, state, _ = case(T, B, N)
    p = Params(adaptive=True)
    d = Direct(W, m, p, x, s0, state)
    outs = dict(zip(FWD, [out(T, B, N) for _ in range(4)] + [out(B, N) for _ in range(3)]))
    csr = [dev(m.w), dev(m.indices), dev(m.indptr)]
    rc = _lib.fn('be_lif_rec_sg_forward')(A.ptr(d.ins[0]), *[A.ptr(t) for t in csr],
                                          *[A.ptr(t) for t in d.ins[2:]], *[A.ptr(outs[n][0]) for n in FWD], T, B, N, *d.scalars(),
                                          RESET[p.reset], 1, d.e, A.stream_ptr())
    assert rc == 0, _lib.last_error()
    assert all(same_bits(host(outs[n][0]), host(d.outs[n][0])) for n in FWD) and np.count_nonzero(d.ref.r) > 0


@pytest.mark.parametrize('N,B,T', ((260, 3, 3), (1032, 1, 3)))
def test_every_neuron_fires_and_none_does(be, N, B, T):
    W, m = weights(N)
    x, s0, state, grads = case(T, B, N, 6)
    every = Direct(W, m, Params(adaptive=True, v_th=-100.0), x, None, state)          # a full mask at every step
    assert every.ref.s_out.all() and np.count_nonzero(every.ref.r[1]) > N // 2
    every.backward(grads)
    none = Direct(W, m, Params(v_th=np.inf), x, np.ones_like(s0), state)              # a full mask before step 0, an empty one after
    assert not none.ref.s_out.any() and not none.ref.r[1:].any() and np.count_nonzero(none.ref.r[0]) > N // 2
    none.backward(grads)


@pytest.mark.parametrize('reset,surrogate,detach,adaptive', C.MODES)
def test_modes_and_two_identical_backward_calls(be, reset, surrogate, detach, adaptive):
    T, B, N = 3, 2, 129
    W, m = weights(N)
    x, s0, state, grads = case(T, B, N, 7)
    d = Direct(W, m, S.mode_params(reset, surrogate, detach, adaptive), x, s0, state)
    assert 0 < d.ref.s_out[:-1].mean() < 1 and np.count_nonzero(d.ref.r) > 0
    (r, a), (_, b) = d.backward(grads), d.backward(grads)
    assert np.count_nonzero(r.g_x) > 0 and all(same_bits(host(a[n][0]), host(b[n][0])) for n in BWD)


def test_the_limit_and_the_error_codes(be):
    from brainevent_amd import _array as A, _lib
    N, T, B = 8192, 2, 1
    rng = np.random.default_rng(1)
    rows = np.repeat(np.arange(N), 8)
    cols = (rows * 7 + np.tile(np.arange(8) * 1021, N)) % N                           # 8 distinct columns per row
    m = C.Matrix(rng.normal(0.0, 0.3, N * 8).astype(F), cols.astype(np.int32), (np.arange(N + 1) * 8).astype(np.int32), N)
    W = np.zeros((N, N), F)
    W[rows, cols] = m.w
    x, s0, state, grads = case(T, B, N)
    d = Direct(W, m, Params(adaptive=True), x, s0, state)
    r, _ = d.backward(grads)
    assert 0.05 < d.ref.s_out[0].mean() < 0.6 and np.count_nonzero(d.ref.r[1]) > N // 4 and np.abs(r.g_s0).max() > 0
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    fwd, bwd = _lib.fn('be_lif_rec_dense_sg_forward'), _lib.fn('be_lif_rec_dense_sg_backward')
    T, B, N = 2, 2, 64
    W, m = weights(N)
    x, s0, state, grads = case(T, B, N)
    d = Direct(W, m, Params(adaptive=True), x, s0, state)
    big, small, gin = [out(T, B, N)[0] for _ in range(5)], [out(B, N)[0] for _ in range(7)], [dev(g) for g in grads]

    def forward(x=P(d.ins[0]), w=P(d.w), s_out=P(big[0]), a_last=P(small[2]), T=T, N=N, mode=0, e=d.e):
        return fwd(x, w, *[P(t) for t in d.ins[2:]], s_out, *[P(t) for t in big[1:4]], P(small[0]), P(small[1]), a_last, T, B, N, 0.8,
                   0.9, 1.0, 0.0, 0.95, 0.3, mode, 1, e, st)

    def backward(h=P(big[2]), w=P(d.w), g_x=P(big[4]), T=T, N=N, mode=0, sur=0, alpha=10.0):
        return bwd(h, P(big[3]), w, *[P(g) for g in gin], g_x, *[P(t) for t in small[3:]], T, B, N, 0.8, 0.9, 1.0, 0.0, 0.95, 0.3, mode,
                   sur, alpha, 1, 0, st)

    assert forward(T=0) == 0 and forward(N=0, x=null, w=null, s_out=null) == 0 and backward(T=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in big + small)
    for call, name, bads in ((forward, 'forward', (dict(x=null), dict(w=null), dict(s_out=null), dict(a_last=null), dict(T=-1),
                                                   dict(mode=2), dict(e=-91), dict(e=151, x=null))),
                             (backward, 'backward', (dict(h=null), dict(w=null), dict(g_x=null), dict(T=-1), dict(mode=2), dict(sur=3),
                                                     dict(alpha=0.0)))):
        for bad in bads:
            assert call(**bad) == INVALID and _lib.last_error().startswith(f'be_lif_rec_dense_sg_{name}: '), (name, bad)
            assert call() == 0
        assert call(N=8193) == RANGE and '8192' in _lib.last_error() and call(N=8193, w=null) == RANGE and call() == 0
    rb, bb = C.backward(d.ref.h_save, d.ref.th_save, m, *grads, Params(adaptive=True), with_bound=True)
    assert all(same_bits(host(t), w) for t, w in zip(big[:4] + small[:3], d.ref[:7]))
    for t, want, bound in zip([big[4]] + small[3:], rb, bb):
        within(t, want, bound, 'after the refusals')
    with pytest.raises(ValueError, match='the limit is 8192'):
        be.recurrent_lif_sequence(torch.zeros(1, 1, 8193, device='cuda'), be.Dense(torch.zeros(8193, 8193, device='cuda')), beta=0.9)
    s, _ = be.recurrent_lif_sequence(dev(x), be.Dense(dev(W)), tuple(dev(a) for a in state), dev(s0), scale_exp=d.e,
                                     **Params(adaptive=True).kwargs())
    assert same_bits(host(s), d.ref.s_out)


@pytest.mark.parametrize('with_s0,parameter,batch', ((True, True, True), (False, False, True), (True, False, False)))
def test_python_equals_the_csr_call_and_the_gradients_are_within_the_bound(be, with_s0, parameter, batch):
    T, B, N = 4, (3 if batch else 1), 260
    W, m = weights(N)
    x, s0, state, grads = case(T, B, N, 11)
    p = Params(adaptive=True)
    cut = (lambda a: a) if batch else (lambda a: a[..., 0, :])                         # x [T, N]: no batch axis
    w = torch.nn.Parameter(dev(W)) if parameter else dev(W).requires_grad_()
    leaves = [dev(cut(a)).requires_grad_() for a in (x,) + state] + ([dev(cut(s0)).requires_grad_()] if with_s0 else [])
    run = lambda rec, ls, **kw: be.recurrent_lif_sequence(ls[0], rec, tuple(ls[1:4]), ls[4] if with_s0 else None, return_v=True,
                                                          **kw, **p.kwargs())
    s, v_seq, last = run(be.Dense(w), leaves)
    e = be._neuron_rec_sg._scale_exp('test', None, be.Dense(w), N)
    from brainevent_amd._csr import fixed_point_exponent
    assert e == fixed_point_exponent(dev(m.w), dev(m.indices), N) and C.exponent(m) - 1 <= e <= C.exponent(m)
    csr = be.CSR((dev(m.w), dev(m.indices), dev(m.indptr)), shape=(N, N))
    with torch.no_grad():
        s2, v2, last2 = run(csr, [t.detach() for t in leaves], scale_exp=e)
    assert s.shape == v_seq.shape == cut(x).shape and all(t.shape == cut(s0).shape for t in last)
    assert all(same_bits(host(a), host(b)) for a, b in zip((s, v_seq) + tuple(last), (s2, v2) + tuple(last2)))
    f = C.forward(x, m, s0 if with_s0 else None, *state, p, e)
    assert same_bits(host(s).reshape(T, B, N), f.s_out) and 0 < f.s_out[:-1].mean() < 1 and np.count_nonzero(f.r) > 0
    got = torch.autograd.grad((s, v_seq) + tuple(last), leaves + [w], [dev(cut(g)) for g in grads])
    r, b = C.backward(f.h_save, f.th_save, m, *grads, p, with_bound=True)
    g_w, b_w = C.weight_grad(m, f.s_out, s0 if with_s0 else None, r.g_x, b.g_x)
    wants = [(r.g_x, b.g_x), (r.g_c0, b.g_c0), (r.g_v0, b.g_v0), (r.g_a0, b.g_a0)] + ([(r.g_s0, b.g_s0)] if with_s0 else []) + \
        [(g_w.reshape(N, N), b_w.reshape(N, N))]
    assert len(got) == len(wants) and got[-1].shape == (N, N)
    for g, (want, bound) in zip(got, wants):
        within(g.reshape(want.shape), want, bound, (with_s0, parameter, batch))
        assert np.count_nonzero(want) > 0


def test_in_place_updates_capture_and_refusals(be):
    T, B, N = 3, 2, 129
    W, m = weights(N)
    x, s0, state, grads = case(T, B, N, 13)
    p, e = Params(), C.exponent(m) - 2                                                # (room for the weights to double)
    w = dev(W).requires_grad_()
    rec = be.Dense(w)
    s0_dev = dev(s0)
    run = lambda xs: be.recurrent_lif_sequence(xs, rec, None, s0_dev, scale_exp=e, **p.kwargs())[0]
    m2 = stored((W * F(-2.0)).astype(F))
    with torch.no_grad():            # (no autograd graph of w from before the capture: its node would belong to another stream)
        a = run(dev(x))
        w.mul_(-2.0)                                                                  # seen by the next call
        b = run(dev(x))
    assert same_bits(host(b), C.forward(x, m2, s0, None, None, None, p, e).s_out) and not same_bits(host(b), host(a))
    x_in, g_in = torch.zeros(T, B, N, device='cuda'), dev(grads[0])                   # a captured training step replays with new x

    def step():
        xs = x_in.detach().requires_grad_()
        s = run(xs)
        return (s,) + torch.autograd.grad([s], [xs, w], [g_in])

    x_in.copy_(dev(x))
    graphed = be.capture_step(step)
    for seed in (2, 3):
        x_in.copy_(dev(case(T, B, N, seed)[0]))
        got = [t.detach().clone() for t in graphed()]
        assert all(same_bits(host(g), host(t)) for g, t in zip(got, step())) and all(torch.count_nonzero(g).item() for g in got)
    assert same_bits(host(got[0]), C.forward(case(T, B, N, 3)[0], m2, s0, None, None, None, p, e).s_out)
    with pytest.raises(NotImplementedError, match='Dense recurrence are not built'):
        be.parametric_recurrent_lif_sequence(dev(x), rec, beta=torch.full((N,), 0.9, device='cuda'), scale_exp=e)
    with pytest.raises(TypeError, match='rec must be a CSR'):
        be.recurrent_lif_sequence(dev(x), dev(W), beta=0.9)
    with pytest.raises(TypeError, match='weights of rec must be float32'):
        be.recurrent_lif_sequence(dev(x), be.Dense(dev(W).double()), beta=0.9)
    with pytest.raises(ValueError, match='must be square'):
        be.recurrent_lif_sequence(dev(x), be.Dense(dev(W)[:, :N - 1].contiguous()), beta=0.9)
