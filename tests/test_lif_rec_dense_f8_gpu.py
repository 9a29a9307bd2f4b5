"""The fused recurrent layer with a Float8Dense recurrence (csrc/be_neuron_sg_rec_dense_f8.hip) on the device.
Expected values come only from tests/lif_rec_sg_cases.py.  Forwards ``forward_with`` on ``recurrent(active) = F(F(dec64[active].sum(0))
* F(scale))`` — the float64 sum of the decoded codes is exact (at most 45 significant bits) — compared as equalities, bit for bit.
Backwards ``backward(with_bound=True)`` on the stored matrix of ``W8.todense()``: with a power-of-two scale that matrix and the
kernel's ``* scale`` are exact and the outputs lie within the propagated bound as it stands; with a general scale the kernel differs
by two more roundings per row product (the rounded ``decode * scale`` inside ``todense()``, the kernel's final ``* scale``), each at
most ``2**-24 * sum |w * G|`` where the bound's own gather term is ``(N + 1) * 2**-24 * sum |w * G|``: TWICE the bound covers them.
Nothing is compared with another device kernel."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_rec_sg_cases as C
import lif_syn_sg_cases as S
from lif_rec_dense_cases import stored
from lif_rec_sg_cases import F, Params, same_bits
from test_lif_rec_dense_gpu import BWD, FWD, INVALID, RANGE, RESET, SENTINEL, SURROGATE, case, out
from test_lif_rec_sg_gpu import dev, host, within

pytestmark = pytest.mark.gpu

#: torch dtype, BE_F8_ code, the largest finite code, a power-of-two scale that keeps N(0, 0.05) weights in range
FMTS = {'e4m3': (torch.float8_e4m3fn, 0, 0x7e, 2.0 ** -11), 'e5m2': (torch.float8_e5m2, 1, 0x7b, 2.0 ** -18)}
fmts = pytest.mark.parametrize('fmt', sorted(FMTS))
#: forwards — one neuron, a partial quad, a wave's edge, a wave's 256 columns, each side of every row-group count (16 | 8 | 4 | 2 | 1
#: at 256, 512, 1024, 2048), one against two quads per thread (4096 | 4097); N % 4 != 0 takes the byte loads, and so does True:
#: the codes lie one byte off their allocation
FORWARD_N = ((1, False), (3, False), (63, False), (64, False), (65, False), (255, False), (256, False), (257, False), (260, True),
             (512, False), (513, False), (1024, False), (1025, False), (2048, False), (2049, False), (4096, False), (4097, False))
#: backwards — both ends of every L (1, 2, 4, 8, 16, 32, 64 lanes per row: up to 16, 32, 64, 128, 256, 512 neurons and beyond),
#: N % 16 == 0 (16-byte loads) and not, past one row trip (N > 8 * 1024 / L: 257 on) and past one lane trip (more than 64 chunks:
#: 1030, 1040); True: the codes lie one byte off a 16-byte boundary.  The scale alternates: a power of two, a general one.
BACKWARD_N = ((1, False), (16, False), (17, False), (32, False), (33, False), (64, False), (65, False), (128, False), (129, False),
              (256, False), (256, True), (257, False), (512, False), (513, False), (1030, False), (1040, False), (1040, True))


@functools.lru_cache(maxsize=None)
def weights(be, N, fmt, general=True, seed=0):
    """N(0, 0.05) weights quantised by ``quantize_fp8`` (default scale ``amax / FMT_MAX``, or the format's power of two), a tenth of
    them exact zeros, one all-zero row and column (from 8 neurons on), a share of the zero codes -0: ``(W8, dec64)``."""
    rng = np.random.default_rng(seed)
    W = rng.normal(0.0, 0.05, (N, N)).astype(F)
    if N >= 8:
        W[rng.random((N, N)) < 0.1] = 0
        W[N // 2, :] = 0
        W[:, N // 3] = 0
    q = be.quantize_fp8(dev(W), fmt, None if general else FMTS[fmt][3])
    codes = q.codes.view(torch.uint8).clone()
    codes[(codes == 0) & dev(rng.random((N, N)) < 0.3)] = 0x80
    W8 = be.Float8Dense(codes.view(FMTS[fmt][0]), q.scale)
    dec64 = W8.codes.cpu().float().numpy().astype(np.float64)
    dec64.setflags(write=False)
    return W8, dec64


def shifted(W8):
    """The same matrix one byte off its (16-byte aligned) allocation."""
    flat = torch.empty(W8.codes.numel() + 16, dtype=torch.uint8, device='cuda')
    flat[1:1 + W8.codes.numel()] = W8.codes.view(torch.uint8).reshape(-1)
    return flat[1:1 + W8.codes.numel()].view(W8.shape)


def recurrent(dec64, scale):
    return lambda active: F(F(dec64[active].sum(0)) * F(scale))


class Direct:
    """``be_lif_rec_dense_f8_sg_forward`` on device copies, then ``_backward`` on what it saved; every output and its tail against
    the restatement (forwards equal bits, backwards within ``factor`` times the bound).  ``dec64``: the decoded codes, or the
    function ``recurrent`` would make of them."""

    def __init__(self, W8, dec64, p, x, s0, state, codes=None):
        from brainevent_amd import _array as A, _lib
        T, B, N = x.shape
        self.A, self.lib, self.dims, self.p, self.W8 = A, _lib, (T, B, N), p, W8
        self.codes = W8.codes if codes is None else codes
        self.w = (A.ptr(self.codes), FMTS[W8.fmt][1], W8.scale)
        rec = dec64 if callable(dec64) else recurrent(dec64, W8.scale)
        self.ref = C.forward_with(x, rec, s0, state[0], state[1], state[2] if p.adaptive else None, p)
        self.back = None
        self.ins = [dev(x), dev(s0)] + [dev(a) for a in state]
        self.outs = dict(zip(FWD, [out(T, B, N) for _ in range(4)] + [out(B, N) for _ in range(3)]))
        rc = _lib.fn('be_lif_rec_dense_f8_sg_forward')(
            A.ptr(self.ins[0]), *self.w, *[A.ptr(t) for t in self.ins[1:]], *[A.ptr(self.outs[n][0]) for n in FWD], T, B, N,
            *self.scalars(), RESET[p.reset], int(p.adaptive), A.stream_ptr())
        assert rc == 0, _lib.last_error()
        self.check(self.outs, self.ref, None)

    def scalars(self):
        p = self.p
        return p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa

    def check(self, outs, ref, bounds, factor=1.0):
        """Equal bits (``bounds`` None) or within the bound; an output the mode does not write, and every tail, keeps the SENTINEL."""
        for name, (view, whole) in outs.items():
            want, what = getattr(ref, name), (name, self.dims, self.p, self.W8)
            if want is None:
                assert bool((whole == SENTINEL).all()), what
                continue
            assert bool((whole[view.numel():] == SENTINEL).all()), what
            if bounds is None:
                assert same_bits(host(view), want), what
            else:
                within(view, want, factor * getattr(bounds, name), what)

    def backward(self, grads, general, state_outs=True):
        """``state_outs`` False: g_c0 / g_v0 / g_a0 / g_s0 go in as NULL, their buffers stay untouched."""
        A, (T, B, N), p = self.A, self.dims, self.p
        if self.back is None:                                                         # (one set of gradients per instance)
            m = stored(host(self.W8.todense()))
            self.back = C.backward(self.ref.h_save, self.ref.th_save, m, *S.pick(grads, S.GRAD_SETS['all'], p), p, with_bound=True)
        r, b = self.back
        outs = dict(zip(BWD, [out(T, B, N)] + [out(B, N) for _ in range(4)]))
        gin = [dev(g) for g in grads]                                                 # (kept alive over the call)
        rc = self.lib.fn('be_lif_rec_dense_f8_sg_backward')(
            A.ptr(self.outs['h_save'][0]), A.ptr(self.outs['th_save'][0]), *self.w, *[A.ptr(g) for g in gin],
            *[A.ptr(outs[n][0] if state_outs or n == 'g_x' else None) for n in BWD], T, B, N, *self.scalars(), RESET[p.reset],
            SURROGATE[p.surrogate], p.alpha, int(p.adaptive), int(p.detach_reset), A.stream_ptr())
        assert rc == 0, self.lib.last_error()
        if not state_outs:
            r = r._replace(g_c0=None, g_v0=None, g_a0=None, g_s0=None)
        self.check(outs, r, b, 2.0 if general else 1.0)
        return r, outs


@fmts
@pytest.mark.parametrize('N,off', FORWARD_N)
def test_forward_bits(be, N, off, fmt):
    """1 and 3 samples, 1, 2, 3 and 5 steps (one pair from 1024 neurons on), s0 given and NULL, both resets, with and without
    adaptation; every output and its tail."""
    W8, dec64 = weights(be, N, fmt)
    ps = (Params(adaptive=True), Params(reset='soft', surrogate='atan', v_reset=-0.25))
    pairs = list(itertools.product((1, 3), (1, 2, 3, 5))) if N < 1024 else [(3, 2)]
    fired = rec = False
    for k, (B, T) in enumerate(pairs, start=0 if N < 1024 else N % 2):
        x, s0, state, _ = case(T, B, N)
        d = Direct(W8, dec64, ps[k % 2], x, s0 if k % 2 == 0 else None, state, shifted(W8) if off else None)
        assert (d.codes.data_ptr() % 4 != 0) == off
        fired |= bool(d.ref.s_out[:-1].any())
        rec |= bool(np.count_nonzero(d.ref.r))
    assert N == 1 or (fired and rec), 'a silent network cannot pass'


@fmts
@pytest.mark.parametrize('sign', (0x00, 0x80))
def test_accumulator_width(be, fmt, sign):
    """8192 active rows of the format's largest (most negative) value: 8192 * 448 * 2**9 needs 31 bits, 8192 * 57344 * 2**16 45."""
    N, mx = 8192, be._dense_f8.FMT_MAX[fmt]
    W8 = be.Float8Dense(torch.full((N, N), FMTS[fmt][2] | sign, dtype=torch.uint8, device='cuda').view(FMTS[fmt][0]), 1e-3)
    x, s0 = np.zeros((2, 1, N), F), np.ones((1, N), F)
    value = lambda rows: F(F(-rows * mx if sign else rows * mx) * F(W8.scale))
    d = Direct(W8, lambda active: np.full(N, value(int(active.sum())), F), Params(syn_decay=0.0), x, s0, (None, None, None))
    want = value(N)
    assert same_bits(host(d.outs['h_save'][0][0]), np.full((1, N), want, F)) and np.isfinite(want) and want != 0


@fmts
@pytest.mark.parametrize('k,N,off', [(k,) + c for k, c in enumerate(BACKWARD_N)])
def test_backward_within_the_bound_and_two_calls_agree(be, k, N, off, fmt):
    T, B = (3, 2) if N < 1024 else (2, 1)
    general = k % 2 == 0
    W8, dec64 = weights(be, N, fmt, general)
    assert general or np.frexp(W8.scale)[0] == 0.5
    x, s0, state, grads = case(T, B, N, 7)
    d = Direct(W8, dec64, Params(adaptive=True), x, s0, state, shifted(W8) if off else None)
    assert (d.codes.data_ptr() % 16 != 0) == off
    (r, a), (_, b) = d.backward(grads, general), d.backward(grads, general)
    assert N < 8 or (np.count_nonzero(r.g_x) > 0 and np.count_nonzero(r.g_s0) > 0)
    assert all(same_bits(host(a[n][0]), host(b[n][0])) for n in BWD)


@fmts
@pytest.mark.parametrize('k,mode', list(enumerate(C.MODES)))
def test_modes(be, k, mode, fmt):
    T, B, N = 3, 2, 129
    general = k % 2 == 1
    W8, dec64 = weights(be, N, fmt, general)
    x, s0, state, grads = case(T, B, N, 7)
    d = Direct(W8, dec64, S.mode_params(*mode), x, s0, state)
    assert 0 < d.ref.s_out[:-1].mean() < 1 and np.count_nonzero(d.ref.r) > 0
    assert np.count_nonzero(d.backward(grads, general)[0].g_x) > 0
    d.backward(grads, general, state_outs=False)


@fmts
def test_through_python(be, fmt):
    """Outputs equal the forward reference; the gradients of x, the state and s0 lie within twice the bound (a general scale); x [T, N];
    a captured step replays with new x and scale_exp=None; the parametric function delegates."""
    T, B, N = 4, 3, 260
    W8, dec64 = weights(be, N, fmt)
    x, s0, state, grads = case(T, B, N, 11)
    p = Params(adaptive=True)
    leaves = [dev(a).requires_grad_() for a in (x,) + state + (s0,)]
    s, v_seq, last = be.recurrent_lif_sequence(leaves[0], W8, tuple(leaves[1:4]), leaves[4], return_v=True, **p.kwargs())
    f = C.forward_with(x, recurrent(dec64, W8.scale), s0, *state, p)
    for got, want in zip((s, v_seq) + tuple(last), (f.s_out, f.v_seq, f.c_last, f.v_last, f.a_last)):
        assert same_bits(host(got), want)
    assert 0 < f.s_out[:-1].mean() < 1 and np.count_nonzero(f.r) > 0
    got = torch.autograd.grad((s, v_seq) + tuple(last), leaves, [dev(g) for g in grads])
    r, b = C.backward(f.h_save, f.th_save, stored(host(W8.todense())), *grads, p, with_bound=True)
    for g, name in zip(got, BWD):
        assert np.count_nonzero(getattr(r, name)) > 0
        within(g, getattr(r, name), 2.0 * getattr(b, name), (fmt, name))
    one = C.forward_with(x[:, :1], recurrent(dec64, W8.scale), None, None, None, None, Params())
    for run in (be.recurrent_lif_sequence, be.parametric_recurrent_lif_sequence):     # x [T, N]; all numbers: delegated
        assert same_bits(host(run(dev(x[:, 0]), W8, **Params().kwargs())[0]), one.s_out[:, 0])
    x_in, g_in, s0_dev = torch.zeros(T, B, N, device='cuda'), dev(grads[0]), dev(s0)

    def step():
        xs = x_in.detach().requires_grad_()
        s = be.recurrent_lif_sequence(xs, W8, None, s0_dev, scale_exp=None, **p.kwargs())[0]
        return (s,) + torch.autograd.grad([s], [xs], [g_in])

    x_in.copy_(dev(x))
    graphed = be.capture_step(step)
    for seed in (2, 3):
        x_in.copy_(dev(case(T, B, N, seed)[0]))
        got = [t.detach().clone() for t in graphed()]
        assert all(same_bits(host(g), host(t)) for g, t in zip(got, step())) and all(torch.count_nonzero(g).item() for g in got)
    assert same_bits(host(got[0]), C.forward_with(case(T, B, N, 3)[0], recurrent(dec64, W8.scale), s0, None, None, None, p).s_out)


def test_refusals(be):
    from brainevent_amd import _array as A, _lib
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    fwd, bwd = _lib.fn('be_lif_rec_dense_f8_sg_forward'), _lib.fn('be_lif_rec_dense_f8_sg_backward')
    T, B, N = 2, 2, 64
    W8, dec64 = weights(be, N, 'e4m3', False)
    x, s0, state, grads = case(T, B, N)
    d = Direct(W8, dec64, Params(adaptive=True), x, s0, state)
    big, small, gin = [out(T, B, N)[0] for _ in range(5)], [out(B, N)[0] for _ in range(7)], [dev(g) for g in grads]

    def forward(x=P(d.ins[0]), w=P(W8.codes), code=0, scale=W8.scale, T=T, N=N, mode=0):
        return fwd(x, w, code, scale, *[P(t) for t in d.ins[1:]], *[P(t) for t in big[:4]], *[P(t) for t in small[:3]], T, B, N, 0.8,
                   0.9, 1.0, 0.0, 0.95, 0.3, mode, 1, st)

    def backward(h=P(big[2]), w=P(W8.codes), code=0, scale=W8.scale, T=T, N=N, mode=0, sur=0):
        return bwd(h, P(big[3]), w, code, scale, *[P(g) for g in gin], P(big[4]), *[P(t) for t in small[3:]], T, B, N, 0.8, 0.9, 1.0,
                   0.0, 0.95, 0.3, mode, sur, 10.0, 1, 0, st)

    assert forward(T=0) == 0 and forward(N=0, x=null, w=null) == 0 and backward(T=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in big + small)
    # an unknown format, a scale that is no finite f32, a size: refused before the pointers are looked at; then a clean call
    for call, name, bads in ((forward, 'forward', (dict(code=2, w=null), dict(code=-1, x=null), dict(scale=float('inf'), x=null),
                                                   dict(scale=float('nan'), w=null), dict(scale=1e300), dict(w=null), dict(mode=2))),
                             (backward, 'backward', (dict(code=2, w=null), dict(scale=float('nan'), h=null), dict(w=null),
                                                     dict(sur=3)))):
        for bad in bads:
            assert call(**bad) == INVALID and _lib.last_error().startswith(f'be_lif_rec_dense_f8_sg_{name}: '), (name, bad)
            assert call() == 0
        assert call(N=8193, w=null) == RANGE and '8192' in _lib.last_error() and call() == 0
    rb, bb = C.backward(d.ref.h_save, d.ref.th_save, stored(host(W8.todense())), *grads, Params(adaptive=True), with_bound=True)
    assert all(same_bits(host(t), w) for t, w in zip(big[:4] + small[:3], d.ref[:7]))
    for t, want, bound in zip([big[4]] + small[3:], rb, bb):
        within(t, want, bound, 'after the refusals')
    xs, f8 = dev(x), torch.float8_e4m3fn
    with pytest.raises(ValueError, match='take no exponent'):
        be.recurrent_lif_sequence(xs, W8, beta=0.9, scale_exp=3)
    with pytest.raises(ValueError, match='must be square'):
        be.recurrent_lif_sequence(xs, be.Float8Dense(torch.zeros(N, N + 1, device='cuda').to(f8)), beta=0.9)
    with pytest.raises(ValueError, match='the limit is 8192'):
        be.recurrent_lif_sequence(torch.zeros(1, 1, 8193, device='cuda'),
                                  be.Float8Dense(torch.zeros(8193, 8193, dtype=torch.uint8, device='cuda').view(f8)), beta=0.9)
    away = be.Float8Dense(W8.codes.cpu(), W8.scale)
    away._dev = away.codes                                                            # (as if the device copy lay elsewhere)
    with pytest.raises(ValueError, match='must share a device'):
        be.recurrent_lif_sequence(xs, away, beta=0.9)
    with pytest.raises(TypeError, match='rec must be a CSR'):
        be.recurrent_lif_sequence(xs, W8.todense(), beta=0.9)
    with pytest.raises(NotImplementedError, match='Float8Dense recurrence are not built'):
        be.parametric_recurrent_lif_sequence(xs, W8, beta=torch.full((N,), 0.9, device='cuda'))
