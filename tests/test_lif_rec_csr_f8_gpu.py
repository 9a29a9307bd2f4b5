"""The fused recurrent layer with a Float8CSR recurrence (csrc/be_neuron_sg_rec_f8.hip) on the device.  Expected
values come only from tests/lif_rec_sg_cases.py.  Forwards ``forward_with`` on ``recurrent(active)[j] = F(float64(R[j]) * ldexp(float64(
F(scale)), -E))`` with ``R`` the int64 sum of ``Q = codes.float() * 2**E`` over the active rows' entries of column ``j`` — compared as
equalities, bit for bit.  Backwards ``backward(with_bound=True)`` on ``Matrix(F(decode) * F(scale), indices, indptr, N)``: with a
power-of-two scale that matrix and the kernel's final ``* scale`` are exact and the bound holds as it stands; with a general scale
the kernel differs by two more roundings per row product, each at most ``2**-24 * sum |w * G|`` where the bound's own gather term is
at least that (the derivation is in tests/test_lif_rec_dense_f8_gpu.py): TWICE the bound.  The bound covers any order of a row's sum."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_rec_sg_cases as C
import lif_syn_sg_cases as S
from lif_rec_sg_cases import F, Params, same_bits
from test_lif_rec_dense_f8_gpu import FMTS
from test_lif_rec_dense_gpu import BWD, INVALID, RANGE, SENTINEL, out
from test_lif_rec_sg_gpu import case, dev, host, within

pytestmark = pytest.mark.gpu

E = {'e4m3': 9, 'e5m2': 16}
fmts = pytest.mark.parametrize('fmt', sorted(FMTS))
#: the crafted rows (empty, a lone self-loop, duplicates, 600 / 65 / 64 entries); one neuron, each side of a wave, two neurons per
#: thread, the LDS limit (rows of 1 .. 8 entries start at every residue mod 4: heads and tails of quads); no entries at all
MATRICES = (('crafted', 300), ('random', 1), ('random', 63), ('random', 65), ('random', 1025), ('random', 8192), ('empty', 65))


@functools.lru_cache(maxsize=None)
def quantised(be, kind, N, fmt, general, shifted=False):
    """``(W8, m, Q, w)``: the matrix of tests/lif_rec_sg_cases.py quantised by ``CSR.quantize_fp8`` (its default scale, or the format's
    power of two), the integers ``Q``, and the f32 weights ``F(decode) * F(scale)``.  ``shifted``: the same container with ``codes``
    one byte and ``indices`` one element off their allocations."""
    m = {'crafted': C.crafted_matrix, 'random': lambda: C.random_matrix(N, 0), 'empty': lambda: C.empty_matrix(N)}[kind]()
    assert m.n == N
    W8 = be.CSR((dev(m.w), dev(m.indices), dev(m.indptr)), shape=(N, N)).quantize_fp8(fmt, None if general else FMTS[fmt][3])
    if shifted:
        cb, ib = torch.zeros(len(m.w) + 16, dtype=torch.uint8, device='cuda'), torch.zeros(len(m.w) + 16, dtype=torch.int32, device='cuda')
        cb[1:1 + len(m.w)], ib[1:1 + len(m.w)] = W8.codes.view(torch.uint8), W8.indices
        W8 = be.Float8CSR((cb[1:1 + len(m.w)].view(FMTS[fmt][0]), ib[1:1 + len(m.w)], W8.indptr), shape=(N, N), scale=W8.scale)
        codes, indices, _ = W8._rows.device_arrays()
        assert codes.data_ptr() % 4 == 1 and indices.data_ptr() % 16 == 4
    dec = host(W8.codes.float())
    Q = (dec.astype(np.float64) * 2.0 ** E[fmt]).astype(np.int64)
    assert (Q.astype(np.float64) == dec.astype(np.float64) * 2.0 ** E[fmt]).all() and (len(Q) == 0 or np.count_nonzero(Q))
    return W8, m, Q, dec * F(W8.scale)


def recurrent(m, Q, scale, fmt):
    rows, unit = C.rows_of(m), np.ldexp(np.float64(F(scale)), -E[fmt])

    def r(active):
        R, on = np.zeros(m.n, np.int64), active[rows]
        np.add.at(R, m.indices[on], Q[on])
        return F(R.astype(np.float64) * unit)
    return r


def run_forward(be, W8, m, Q, fmt, p, T, B, with_s0):
    """The public function against the restatement, bit for bit: ``s``, ``v_seq`` and the last state.  Returns the restatement."""
    x, s0, state, _ = case(T, B, m.n, 3)
    n = 3 if p.adaptive else 2
    s0 = s0 if with_s0 else None
    got = be.recurrent_lif_sequence(dev(x), W8, tuple(dev(a) for a in state[:n]), dev(s0), return_v=True, **p.kwargs())
    f = C.forward_with(x, recurrent(m, Q, W8.scale, fmt), s0, *state[:n], *(None,) * (3 - n), p)
    for a, b in zip(got[:2] + tuple(got[2]), (f.s_out, f.v_seq, f.c_last, f.v_last, f.a_last)):
        assert same_bits(host(a), b), (fmt, m.n, p, T, B, with_s0)
    return f


@fmts
@pytest.mark.parametrize('general', (False, True))
@pytest.mark.parametrize('kind,N', MATRICES)
def test_forward_bits(be, kind, N, fmt, general):
    """Both resets, with and without adaptation, T in {1, 3}, B in {1, 3}, s0 given and None (one mode and T = 3 from 1025 on)."""
    W8, m, Q, _ = quantised(be, kind, N, fmt, general)
    modes = list(itertools.product(('hard', 'soft'), (False, True))) if N < 1024 else [('hard', True)]
    shapes = [(3, 3, True), (3, 1, False), (1, 3, True), (1, 1, False)] if N < 1024 else [(3, 3, True), (3, 1, False)]
    for (reset, adaptive), (T, B, with_s0) in itertools.product(modes, shapes):
        f = run_forward(be, W8, m, Q, fmt, Params(reset=reset, adaptive=adaptive, v_reset=-0.25), T, B, with_s0)
        if T == 3 and N > 1:                                                          # a silent network cannot pass
            assert 0 < f.s_out[:-1].mean() < 1 and (np.count_nonzero(f.r) > 0) == (len(Q) > 0)


@fmts
def test_forward_bits_on_the_byte_path(be, fmt):
    W8, m, Q, _ = quantised(be, 'crafted', 300, fmt, True, shifted=True)
    f = run_forward(be, W8, m, Q, fmt, Params(adaptive=True), 3, 3, True)
    assert 0 < f.s_out[:-1].mean() < 1 and np.count_nonzero(f.r) > 0


@fmts
@pytest.mark.parametrize('k,kind,N,surrogate', [(k,) + c for k, c in enumerate(
    [('crafted', 300, sg) for sg in S.SURROGATES] + [('random', N, 'fast_sigmoid') for N in (1, 65, 1025)])])
def test_backward_within_the_bound(be, k, kind, N, surrogate, fmt):
    T, B, general = 3, 2, k % 2 == 0
    W8, m, Q, w = quantised(be, kind, N, fmt, general)
    assert general or np.frexp(W8.scale)[0] == 0.5
    p = S.mode_params('hard', surrogate, False, True)
    x, s0, state, grads = case(T, B, N, 7)
    leaves = [dev(a).requires_grad_() for a in (x,) + state + (s0,)]
    s, v_seq, last = be.recurrent_lif_sequence(leaves[0], W8, tuple(leaves[1:4]), leaves[4], return_v=True, **p.kwargs())
    got = torch.autograd.grad((s, v_seq) + tuple(last), leaves, [dev(g) for g in grads])
    f = C.forward_with(x, recurrent(m, Q, W8.scale, fmt), s0, *state, p)
    assert same_bits(host(s), f.s_out)
    r, b = C.backward(f.h_save, f.th_save, C.Matrix(w, m.indices, m.indptr, N), *grads, p, with_bound=True)
    for g, name in zip(got, BWD):
        assert np.count_nonzero(getattr(r, name)) > 0, name
        within(g, getattr(r, name), (2.0 if general else 1.0) * getattr(b, name), (fmt, kind, N, surrogate, name))


def test_host_behaviour(be):
    from brainevent_amd import _array as A, _lib
    T, B, N, fmt = 3, 2, 65, 'e4m3'
    W8, m, Q, w = quantised(be, 'random', N, fmt, False)
    p = Params(adaptive=True)
    x, s0, state, grads = case(T, B, N, 3)
    rec = recurrent(m, Q, W8.scale, fmt)
    # a captured step replays with new x and equals the eager result; all-number parameters delegate
    x_in, g_in, s0_dev = dev(x), dev(grads[0]), dev(s0)

    def step():
        xs = x_in.detach().requires_grad_()
        s = be.recurrent_lif_sequence(xs, W8, None, s0_dev, **p.kwargs())[0]
        return (s,) + torch.autograd.grad([s], [xs], [g_in])

    graphed = be.capture_step(step)
    for seed in (2, 3):
        x_in.copy_(dev(case(T, B, N, seed)[0]))
        got = [t.detach().clone() for t in graphed()]
        assert all(same_bits(host(g), host(t)) for g, t in zip(got, step())) and all(torch.count_nonzero(g).item() for g in got)
    want = C.forward_with(case(T, B, N, 3)[0], rec, s0, None, None, None, p).s_out
    assert same_bits(host(got[0]), want)
    assert same_bits(host(be.parametric_recurrent_lif_sequence(dev(x), W8, None, s0_dev, **p.kwargs())[0]), want)
    # the refusals
    xs = dev(x)
    with pytest.raises(ValueError, match='take no exponent'):
        be.recurrent_lif_sequence(xs, W8, beta=0.9, scale_exp=3)
    with pytest.raises(TypeError, match='rec must be a CSR'):
        be.recurrent_lif_sequence(xs, W8.T, beta=0.9)
    wide = be.Float8CSR((W8.codes, W8.indices, W8.indptr), shape=(N, N), scale=W8.scale)
    wide._rows.indptr = W8.indptr.long()                                              # (as 2^31 entries or more would leave it)
    with pytest.raises(TypeError, match='indptr of rec must be int32'):
        be.recurrent_lif_sequence(xs, wide, beta=0.9)
    none = torch.zeros(0, dtype=torch.int32, device='cuda')
    big8 = be.Float8CSR((none.to(torch.uint8), none, torch.zeros(8194, dtype=torch.int32, device='cuda')), shape=(8193, 8193), fmt=fmt)
    with pytest.raises(ValueError, match='the limit is 8192'):
        be.recurrent_lif_sequence(torch.zeros(1, 1, 8193, device='cuda'), big8, beta=0.9)
    with pytest.raises(NotImplementedError, match='Float8CSR recurrence are not built'):
        be.parametric_recurrent_lif_sequence(xs, W8, beta=torch.full((N,), 0.9, device='cuda'))
    # the C entry points: refused before a pointer is looked at, nothing written, and a clean call after each refusal
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    fwd, bwd = _lib.fn('be_lif_rec_f8_sg_forward'), _lib.fn('be_lif_rec_f8_sg_backward')
    codes, indices, indptr = W8._rows.device_arrays()
    ins = [dev(a) for a in (x, s0) + state]
    big, small, gin = [out(T, B, N)[0] for _ in range(5)], [out(B, N)[0] for _ in range(7)], [dev(g) for g in grads]

    def forward(x=P(ins[0]), w=P(codes), code=0, scale=W8.scale, nse=len(Q), T=T, N=N, mode=0):
        return fwd(x, w, code, scale, P(indices), P(indptr), nse, *[P(t) for t in ins[1:]], *[P(t) for t in big[:4]],
                   *[P(t) for t in small[:3]], T, B, N, p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa, mode, 1, st)

    def backward(h=P(big[2]), w=P(codes), code=0, scale=W8.scale, nse=len(Q), T=T, N=N, mode=0, sur=0):
        return bwd(h, P(big[3]), w, code, scale, P(indices), P(indptr), nse, *[P(g) for g in gin], P(big[4]), *[P(t) for t in small[3:]],
                   T, B, N, p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa, mode, sur, p.alpha, 1, 0, st)

    assert forward(T=0) == 0 and forward(N=0, x=null, w=null) == 0 and backward(T=0) == 0 and backward(N=0, h=null) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in big + small)
    bads = (dict(code=2, w=null), dict(scale=float('nan'), w=null), dict(scale=float('inf')), dict(nse=-1, w=null), dict(mode=2))
    for call, name, more in ((forward, 'forward', (dict(x=null),)), (backward, 'backward', (dict(sur=3), dict(h=null)))):
        for bad in bads + more:
            assert call(**bad) == INVALID and _lib.last_error().startswith(f'be_lif_rec_f8_sg_{name}: '), (name, bad)
            assert call() == 0
        assert call(N=8193, w=null) == RANGE and '8192' in _lib.last_error() and call() == 0
    f = C.forward_with(x, rec, s0, *state, p)
    assert all(same_bits(host(t), a) for t, a in zip(big[:4] + small[:3], f[:7]))
    rb, bb = C.backward(f.h_save, f.th_save, C.Matrix(w, m.indices, m.indptr, N), *grads, p, with_bound=True)
    for t, a, bound in zip([big[4]] + small[3:], rb, bb):
        within(t, a, bound, 'after the refusals')
