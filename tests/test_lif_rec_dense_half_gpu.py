"""The fused recurrent layer with a Dense recurrence in f16 / bf16 weights (csrc/be_neuron_sg_rec_dense_half.hip) on
the device.  The layer is the f32 layer on ``W16.float()``: expected values come only from tests/lif_rec_sg_cases.py run on the
matrix that stores all ``N * N`` up-converted entries — forward outputs as equalities, bit for bit, backward outputs within the
restatement's propagated bound.  Nothing is compared with another device kernel."""
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

DTYPES = {'f16': (torch.float16, 2, 2.0 ** -11), 'bf16': (torch.bfloat16, 3, 2.0 ** -8)}      # torch dtype, BE_ code, half an ulp
dtypes = pytest.mark.parametrize('dtype', sorted(DTYPES))
#: forwards — a wave's edge, each side of every row-group count (16 | 8 | 4 | 2 | 1 at 128, 256, 512, 1024), one against two
#: owned pairs per thread (2048 | 2049); the odd sizes take the 2-byte loads and leave the last pair half empty
FORWARD_N = (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049)
#: backwards — every L (1, 2, 4, 8, 16, 32, 64 lanes per row), N % 8 == 0 (16-byte loads) and not, past one row trip (N > 4 * 1024 / L:
#: 520 on) and past one lane trip (more than 2 * 64 chunks: 1028, 1032); True: W lies one element off a 16-byte boundary
BACKWARD_N = ((8, False), (24, False), (63, False), (100, False), (136, False), (136, True), (260, False), (520, False), (1028, False),
              (1032, False))


@functools.lru_cache(maxsize=None)
def weights(N, dtype, seed=0):
    """N(0, 0.05) weights rounded to ``dtype``, a tenth of them exact zeros, one all-zero row and one all-zero column (from 8 neurons
    on): the device tensor and the stored matrix of its up-converted entries (read-only)."""
    rng = np.random.default_rng(seed)
    W = rng.normal(0.0, 0.05, (N, N)).astype(F)
    if N >= 8:
        W[rng.random((N, N)) < 0.1] = 0
        W[N // 2, :] = 0
        W[:, N // 3] = 0
    W16 = dev(W).to(DTYPES[dtype][0])
    up = host(W16.float())
    up.setflags(write=False)
    return W16, stored(up)


def shifted(W16):
    """The same matrix one element off its (16-byte aligned) allocation."""
    flat = torch.empty(W16.numel() + 8, dtype=W16.dtype, device='cuda')
    flat[1:1 + W16.numel()] = W16.reshape(-1)
    return flat[1:1 + W16.numel()].view(W16.shape)


class Direct:
    """``be_lif_rec_dense_half_sg_forward`` on device copies, then ``_backward`` on what it saved; every output against the
    restatement on ``m`` (the stored up-converted matrix, or a sparser pattern with the same dense matrix)."""

    def __init__(self, W16, m, p, x, s0, state, e=None):
        from brainevent_amd import _array as A, _lib
        T, B, N = x.shape
        self.A, self.lib, self.dims, self.p, self.m, self.w = A, _lib, (T, B, N), p, m, W16
        self.code = {v[0]: v[1] for v in DTYPES.values()}[W16.dtype]
        self.e = C.exponent(m) if e is None else e
        self.ref = C.forward(x, m, s0, state[0], state[1], state[2] if p.adaptive else None, p, self.e)
        self.ins = [dev(x), dev(s0)] + [dev(a) for a in state]
        self.outs = dict(zip(FWD, [out(T, B, N) for _ in range(4)] + [out(B, N) for _ in range(3)]))
        rc = _lib.fn('be_lif_rec_dense_half_sg_forward')(
            A.ptr(self.ins[0]), A.ptr(W16), self.code, *[A.ptr(t) for t in self.ins[1:]], *[A.ptr(self.outs[n][0]) for n in FWD], T, B,
            N, *self.scalars(), RESET[p.reset], int(p.adaptive), self.e, A.stream_ptr())
        assert rc == 0, _lib.last_error()
        self.check(self.outs, self.ref, None)

    def scalars(self):
        p = self.p
        return p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa

    def check(self, outs, ref, bounds):
        """Equal bits (``bounds`` None) or within the bound; an output the mode does not write, and every tail, keeps the SENTINEL."""
        for name, (view, whole) in outs.items():
            want, what = getattr(ref, name), (name, self.dims, self.p, self.w.dtype)
            if want is None:
                assert bool((whole == SENTINEL).all()), what
                continue
            assert bool((whole[view.numel():] == SENTINEL).all()), what
            if bounds is None:
                assert same_bits(host(view), want), what
            else:
                within(view, want, getattr(bounds, name), what)

    def backward(self, grads):
        A, (T, B, N), p = self.A, self.dims, self.p
        r, b = C.backward(self.ref.h_save, self.ref.th_save, self.m, *S.pick(grads, S.GRAD_SETS['all'], p), p, with_bound=True)
        outs = dict(zip(BWD, [out(T, B, N)] + [out(B, N) for _ in range(4)]))
        gin = [dev(g) for g in grads]                                                 # (kept alive over the call)
        rc = self.lib.fn('be_lif_rec_dense_half_sg_backward')(
            A.ptr(self.outs['h_save'][0]), A.ptr(self.outs['th_save'][0]), A.ptr(self.w), self.code, *[A.ptr(g) for g in gin],
            *[A.ptr(outs[n][0]) for n in BWD], T, B, N, *self.scalars(), RESET[p.reset], SURROGATE[p.surrogate], p.alpha,
            int(p.adaptive), int(p.detach_reset), A.stream_ptr())
        assert rc == 0, self.lib.last_error()
        self.check(outs, r, b)
        return r, outs


@dtypes
@pytest.mark.parametrize('N', FORWARD_N)
def test_forward_bits(be, N, dtype):
    """1 and 3 samples, 1, 2, 3 and 5 steps (two pairs from 1024 neurons on), s0 given and NULL, both resets, with and without
    adaptation; every output and its tail."""
    W16, m = weights(N, dtype)
    ps = (Params(adaptive=True), Params(reset='soft', surrogate='atan', v_reset=-0.25))
    pairs = list(itertools.product((1, 3), (1, 2, 3, 5))) if N < 1024 else [(3, 2), (1, 3)]
    fired = recurrent = False
    for k, (B, T) in enumerate(pairs):
        x, s0, state, _ = case(T, B, N)
        d = Direct(W16, m, ps[k % 2], x, s0 if k % 2 == 0 else None, state)
        fired |= bool(d.ref.s_out[:-1].any())
        recurrent |= bool(np.count_nonzero(d.ref.r))
    assert N == 1 or (fired and recurrent), 'a silent network cannot pass'


@dtypes
def test_forward_bits_at_the_limit(be, dtype):
    """8192 neurons, 8 non-zero entries per row: the restatement runs on that sparse pattern (a zero entry adds the integer 0)."""
    N, T, B = 8192, 2, 1
    rng = np.random.default_rng(1)
    rows = np.repeat(np.arange(N), 8)
    cols = (rows * 7 + np.tile(np.arange(8) * 1021, N)) % N                           # 8 distinct columns per row
    w16 = dev(rng.normal(0.0, 0.3, N * 8).astype(F)).to(DTYPES[dtype][0])
    W16 = torch.zeros((N, N), dtype=w16.dtype, device='cuda')
    W16[dev(rows), dev(cols)] = w16
    m = C.Matrix(host(w16.float()), cols.astype(np.int32), (np.arange(N + 1) * 8).astype(np.int32), N)
    x, s0, state, _ = case(T, B, N)
    d = Direct(W16, m, Params(adaptive=True), x, s0, state)
    assert 0.05 < d.ref.s_out[0].mean() < 0.6 and np.count_nonzero(d.ref.r[1]) > N // 4


@dtypes
@pytest.mark.parametrize('N,off', BACKWARD_N)
def test_backward_within_the_bound_and_two_calls_agree(be, N, off, dtype):
    T, B = (3, 2) if N < 1024 else (2, 1)
    W16, m = weights(N, dtype)
    x, s0, state, grads = case(T, B, N, 7)
    d = Direct(shifted(W16) if off else W16, m, Params(adaptive=True), x, s0, state)
    assert (d.w.data_ptr() % 16 != 0) == off
    (r, a), (_, b) = d.backward(grads), d.backward(grads)
    assert np.count_nonzero(r.g_x) > 0 and np.count_nonzero(r.g_s0) > 0
    assert all(same_bits(host(a[n][0]), host(b[n][0])) for n in BWD)


@dtypes
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', C.MODES)
def test_modes(be, reset, surrogate, detach, adaptive, dtype):
    T, B, N = 3, 2, 129
    W16, m = weights(N, dtype)
    x, s0, state, grads = case(T, B, N, 7)
    d = Direct(W16, m, S.mode_params(reset, surrogate, detach, adaptive), x, s0, state)
    assert 0 < d.ref.s_out[:-1].mean() < 1 and np.count_nonzero(d.ref.r) > 0
    assert np.count_nonzero(d.backward(grads)[0].g_x) > 0


@dtypes
@pytest.mark.parametrize('with_s0', (True, False))
def test_python_outputs_and_gradients(be, with_s0, dtype):
    """Through ``recurrent_lif_sequence``: the outputs are the restatement's, ``W.grad`` has ``W.dtype`` and lies within the
    restatement's ``weight_grad`` bound plus ONE rounding to the dtype (half an ulp: relative 2**-11 / 2**-8 of the device's f32
    value, which is within the bound of the expected one; below f16's normal range half a subnormal step, 2**-25)."""
    T, B, N = 4, 3, 260
    tdtype, _, half_ulp = DTYPES[dtype]
    W16, m = weights(N, dtype)
    x, s0, state, grads = case(T, B, N, 11)
    p = Params(adaptive=True)
    w = torch.nn.Parameter(W16.clone())
    leaves = [dev(a).requires_grad_() for a in (x,) + state] + ([dev(s0).requires_grad_()] if with_s0 else [])
    s, v_seq, last = be.recurrent_lif_sequence(leaves[0], be.Dense(w), tuple(leaves[1:4]), leaves[4] if with_s0 else None,
                                               return_v=True, **p.kwargs())
    e = be._neuron_rec_sg._scale_exp('test', None, be.Dense(w), N)
    from brainevent_amd._csr import fixed_point_exponent
    assert e == fixed_point_exponent(dev(m.w), dev(m.indices), N) and C.exponent(m) - 1 <= e <= C.exponent(m)
    f = C.forward(x, m, s0 if with_s0 else None, *state, p, e)
    for got, want in zip((s, v_seq) + tuple(last), (f.s_out, f.v_seq, f.c_last, f.v_last, f.a_last)):
        assert same_bits(host(got), want)
    assert 0 < f.s_out[:-1].mean() < 1 and np.count_nonzero(f.r) > 0
    got = torch.autograd.grad((s, v_seq) + tuple(last), leaves + [w], [dev(g) for g in grads])
    r, b = C.backward(f.h_save, f.th_save, m, *grads, p, with_bound=True)
    wants = [(r.g_x, b.g_x), (r.g_c0, b.g_c0), (r.g_v0, b.g_v0), (r.g_a0, b.g_a0)] + ([(r.g_s0, b.g_s0)] if with_s0 else [])
    for g, (want, bound) in zip(got, wants):
        within(g, want, bound, (with_s0, dtype))
    g_w, b_w = (a.reshape(N, N) for a in C.weight_grad(m, f.s_out, s0 if with_s0 else None, r.g_x, b.g_x))
    assert got[-1].dtype == tdtype and got[-1].shape == (N, N) and np.count_nonzero(g_w) > 0
    within(got[-1].float(), g_w, b_w + half_ulp * (np.abs(g_w) + b_w) + 2.0 ** -25, (with_s0, dtype, 'g_w'))


@dtypes
def test_in_place_updates_and_capture(be, dtype):
    T, B, N = 3, 2, 129
    W16, m = weights(N, dtype)
    x, s0, state, grads = case(T, B, N, 13)
    p, e = Params(), C.exponent(m) - 2                                                # (room for the weights to double)
    w = W16.clone().requires_grad_()
    rec, s0_dev = be.Dense(w), dev(s0)
    run = lambda xs: be.recurrent_lif_sequence(xs, rec, None, s0_dev, scale_exp=e, **p.kwargs())[0]
    with torch.no_grad():            # (no autograd graph of w from before the capture: its node would belong to another stream)
        a = run(dev(x))
        w.mul_(-2.0)                                                                  # seen by the next call
        b = run(dev(x))
    m2 = stored(host(w.float()))                                                      # the up-converted matrix as it now is
    assert np.array_equal(m2.w, m.w * F(-2.0))
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
        assert all(same_bits(host(g.float()), host(t.float())) for g, t in zip(got, step()))
        assert all(torch.count_nonzero(g).item() for g in got) and got[2].dtype == w.dtype
    assert same_bits(host(got[0]), C.forward(case(T, B, N, 3)[0], m2, s0, None, None, None, p, e).s_out)


def test_refusals(be):
    from brainevent_amd import _array as A, _lib
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    fwd, bwd = _lib.fn('be_lif_rec_dense_half_sg_forward'), _lib.fn('be_lif_rec_dense_half_sg_backward')
    T, B, N = 2, 2, 64
    W16, m = weights(N, 'f16')
    x, s0, state, grads = case(T, B, N)
    d = Direct(W16, m, Params(adaptive=True), x, s0, state)
    big, small, gin = [out(T, B, N)[0] for _ in range(5)], [out(B, N)[0] for _ in range(7)], [dev(g) for g in grads]

    def forward(x=P(d.ins[0]), w=P(W16), code=2, T=T, N=N, mode=0, e=d.e):
        return fwd(x, w, code, *[P(t) for t in d.ins[1:]], *[P(t) for t in big[:4]], *[P(t) for t in small[:3]], T, B, N, 0.8, 0.9, 1.0,
                   0.0, 0.95, 0.3, mode, 1, e, st)

    def backward(h=P(big[2]), w=P(W16), code=2, T=T, N=N, mode=0, sur=0):
        return bwd(h, P(big[3]), w, code, *[P(g) for g in gin], P(big[4]), *[P(t) for t in small[3:]], T, B, N, 0.8, 0.9, 1.0, 0.0, 0.95,
                   0.3, mode, sur, 10.0, 1, 0, st)

    assert forward(T=0) == 0 and forward(N=0, x=null, w=null) == 0 and backward(T=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in big + small)
    # a wrong dtype code, an exponent out of range, a size: refused before the pointers are looked at; then a clean call
    for call, name, bads in ((forward, 'forward', (dict(code=0, w=null), dict(code=1, x=null), dict(code=4), dict(e=-91, x=null),
                                                   dict(e=151, w=null), dict(w=null), dict(mode=2))),
                             (backward, 'backward', (dict(code=0, w=null), dict(code=7, h=null), dict(w=null), dict(sur=3)))):
        for bad in bads:
            assert call(**bad) == INVALID and _lib.last_error().startswith(f'be_lif_rec_dense_half_sg_{name}: '), (name, bad)
            assert call() == 0
        assert call(N=8193, w=null) == RANGE and '8192' in _lib.last_error() and call() == 0
    rb, bb = C.backward(d.ref.h_save, d.ref.th_save, m, *grads, Params(adaptive=True), with_bound=True)
    assert all(same_bits(host(t), w) for t, w in zip(big[:4] + small[:3], d.ref[:7]))
    for t, want, bound in zip([big[4]] + small[3:], rb, bb):
        within(t, want, bound, 'after the refusals')
    xs = dev(x)
    with pytest.raises(ValueError, match='the limit is 8192'):
        be.recurrent_lif_sequence(torch.zeros(1, 1, 8193, device='cuda'),
                                  be.Dense(torch.zeros(8193, 8193, dtype=torch.float16, device='cuda')), beta=0.9)
    with pytest.raises(TypeError, match='weights of rec must be float32'):
        be.recurrent_lif_sequence(xs, be.Dense(W16.double()), beta=0.9)
    with pytest.raises(NotImplementedError, match='Dense recurrence are not built'):
        be.parametric_recurrent_lif_sequence(xs, be.Dense(W16), beta=torch.full((N,), 0.9, device='cuda'), scale_exp=d.e)
    s, _ = be.parametric_recurrent_lif_sequence(xs, be.Dense(W16), tuple(dev(a) for a in state), dev(s0), scale_exp=d.e,
                                                **Params(adaptive=True).kwargs())    # all numbers: delegated
    assert same_bits(host(s), d.ref.s_out)
