"""The differentiable LIF neuron (csrc/be_neuron_sg.hip, brainevent_amd/_neuron_sg.py) on the device, compared with the numpy
restatement of tests/lif_sg_cases.py as EQUALITIES, bit for bit (``lif_sg_cases.same_bits``): every operation of both passes is an
individually rounded IEEE f32 add, multiply, divide, abs, max or compare.  Nothing here is compared with torch's device kernels.
tests/test_lif_sg_cpu.py holds the restatement to CPU autograd and the sizes used here to the kernels' source."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lif_sg_cases as C
from lif_sg_cases import F, Params, same_bits

pytestmark = pytest.mark.gpu


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
    arrays = C.inputs(T, N, seed)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def check_sequence(be, T, N, p, which='all', shape=None, seed=0, wrap=dev, use_v0=True):
    """lif_sequence forwards and backwards at one size against the restatement; ``which``: the gradients that arrive."""
    x, v0, g_s, g_vseq, g_vlast = case(T, N, seed)
    if not use_v0:
        v0 = None
    use = C.GRAD_SETS[which]
    s_ref, vseq_ref, h_ref, vlast_ref = C.forward(x, v0, p)
    gx_ref, gv0_ref = C.backward(h_ref, g_s if use[0] else None, g_vseq if use[1] else None, g_vlast if use[2] else None, p)
    slots = (N,) if shape is None else tuple(shape)
    xt = wrap(x.reshape((T,) + slots)).requires_grad_()
    vt = None if v0 is None else wrap(v0.reshape(slots)).requires_grad_()
    s, v_seq, v_last = be.lif_sequence(xt, vt, return_v=True, **p.kwargs())
    assert s.shape == xt.shape == v_seq.shape and v_last.shape == slots and s.dtype == torch.float32
    what = (T, N, p, which, shape)
    assert same_bits(host(s).reshape(T, N), s_ref), what
    assert same_bits(host(v_seq).reshape(T, N), vseq_ref), what
    assert same_bits(host(v_last).reshape(N), vlast_ref), what
    outs = [o for o, u in zip((s, v_seq, v_last), use) if u]
    grads = [wrap(g.reshape(o.shape)) for (g, o), u in zip(((g_s, s), (g_vseq, v_seq), (g_vlast, v_last)), use) if u]
    got = torch.autograd.grad(outs, [xt] if vt is None else [xt, vt], grads)
    assert same_bits(host(got[0]).reshape(T, N), gx_ref), what
    if vt is not None:
        assert same_bits(host(got[1]).reshape(N), gv0_ref), what
    return s_ref, gx_ref


# ======================================================================================================== sizes
@pytest.mark.parametrize('N', C.N_SIZES)
def test_sizes(be, N):
    """One slot, a wave less one, a wave, a wave and one; one step, two, the ring's depth and its neighbours, and 25."""
    for T in C.T_SIZES:
        for p in (Params(), Params(reset='soft', surrogate='atan', v_reset=-0.25)):
            s_ref, gx_ref = check_sequence(be, T, N, p)
    assert N < 8 or (0 < s_ref.mean() < 1 and np.abs(gx_ref).max() > 0)


@pytest.mark.parametrize('N', C.N_PAST_ONE_PASS)
@pytest.mark.parametrize('T', (2, C.CONSTS['kSgPrefetch'] + 1))
def test_past_one_pass_of_the_capped_grid(be, N, T):
    """A second trip of the grid-stride loop: of the 4-byte kernel (one slot) and of the 16-byte kernel (one lane)."""
    check_sequence(be, T, N, Params(surrogate='triangle', alpha=2.0), seed=3)


@pytest.mark.parametrize('shape', C.SHAPES)
def test_shapes(be, shape):
    N = int(np.prod(shape))
    check_sequence(be, 3, N, Params(), shape=shape)
    x, v0, g_s, _, g_vlast = case(1, N, 0)
    p = Params(reset='soft')
    xt, vt = dev(x.reshape(shape)).requires_grad_(), dev(v0.reshape(shape)).requires_grad_()
    s, v = be.lif_step(vt, xt, **p.kwargs())
    assert s.shape == v.shape == tuple(shape)
    s_ref, _, h_ref, v_ref = C.forward(x, v0, p)
    gx_ref, gv_ref = C.backward(h_ref, g_s, None, g_vlast, p)
    gx, gv = torch.autograd.grad([s, v], [xt, vt], [dev(g_s.reshape(shape)), dev(g_vlast.reshape(shape))])
    assert same_bits(host(s).reshape(1, N), s_ref) and same_bits(host(v).reshape(N), v_ref)
    assert same_bits(host(gx).reshape(1, N), gx_ref) and same_bits(host(gv).reshape(N), gv_ref)


@pytest.mark.parametrize('N', (64, 67))
def test_base_off_16_bytes_and_the_scalar_tail(be, N):
    """A base pointer 4 bytes past a 16-byte boundary (N % 4 == 0: only the alignment refuses the 16-byte kernel), and N % 4 != 0."""
    for T in (1, 6):
        check_sequence(be, T, N, Params(), wrap=misaligned)
        check_sequence(be, T, N, Params(reset='soft', surrogate='triangle', alpha=2.0), wrap=misaligned, which='g_vseq')
    # a non-contiguous input is made contiguous
    x, v0, *_ = case(3, N, 0)
    p = Params()
    xt = dev(np.ascontiguousarray(x.T)).T
    vt = dev(np.repeat(v0, 2))[::2]
    assert not xt.is_contiguous() and not vt.is_contiguous()
    s, v_last = be.lif_sequence(xt, vt, **p.kwargs())
    s_ref, _, _, vlast_ref = C.forward(x, v0, p)
    assert same_bits(host(s), s_ref) and same_bits(host(v_last), vlast_ref)


# ======================================================================================================== modes
@pytest.mark.parametrize('reset,surrogate,detach', C.MODES)
def test_modes_and_gradient_sets(be, reset, surrogate, detach):
    p = Params(reset=reset, surrogate=surrogate, detach_reset=detach, v_reset=-0.25, alpha=2.0 if surrogate == 'triangle' else 10.0)
    for which in C.GRAD_SETS:
        for N in (132, 65):              # the 16-byte and the 4-byte kernel
            s_ref, gx_ref = check_sequence(be, 5, N, p, which=which, seed=7)
            assert 0 < s_ref.mean() < 1 and np.count_nonzero(gx_ref) > 0


def test_unused_gradients_go_in_as_null(be, monkeypatch):
    from brainevent_amd import _neuron_sg
    calls = []
    real = _neuron_sg.call

    def spy(name, *args):
        calls.append((name, [a.value if isinstance(a, ctypes.c_void_p) else a for a in args]))
        return real(name, *args)
    monkeypatch.setattr(_neuron_sg, 'call', spy)
    x, v0, g_s, g_vseq, g_vlast = case(3, 64, 0)
    for which, use in C.GRAD_SETS.items():
        xt, vt = dev(x).requires_grad_(), dev(v0)                  # v0 does not require grad: g_v0 is not asked for
        outs = be.lif_sequence(xt, vt, beta=0.9, return_v=True)
        picked = [(o, dev(g)) for o, g, u in zip(outs, (g_s, g_vseq, g_vlast), use) if u]
        calls.clear()
        torch.autograd.grad([o for o, _ in picked], [xt], [g for _, g in picked])
        (name, args), = calls
        assert name == 'be_lif_sg_backward' and args[0] is not None and args[4] is not None
        assert [a is not None for a in args[1:4]] == list(use), which
        assert args[5] is None                                     # v0's gradient was not asked for


# ======================================================================================================== edge values
def test_threshold_exactly_and_the_surrogate_peak(be):
    """h == v_th spikes (beta = 0.5, v = 1, x = 0.5, v_th = 1); u = 0 is where each surrogate is largest."""
    for reset in C.RESETS:
        v, x = dev(np.array([1.0, 1.0], F)), dev(np.array([0.5, 0.5 - 2.0 ** -24], F))   # h = 1 and 1 - 2^-24
        s, vn = be.lif_step(v, x, beta=0.5, v_th=1.0, v_reset=-2.0, reset=reset)
        assert host(s).tolist() == [1.0, 0.0] and host(vn)[0] == (-2.0 if reset == 'hard' else 0.0) and host(vn)[1] < 1.0
    u = np.linspace(-0.5, 0.5, 101).astype(F)
    assert u[50] == 0
    for sur, peak in (('fast_sigmoid', 1.0), ('atan', 5.0), ('triangle', 10.0)):
        p = Params(surrogate=sur, detach_reset=True, beta=1.0)
        xt = dev(u + F(1.0)).requires_grad_()
        s, _ = be.lif_step(torch.zeros(101, device='cuda'), xt, **p.kwargs())
        g, = torch.autograd.grad(s, xt, torch.ones_like(s))
        g = host(g)
        h = C.forward((u + F(1.0))[None], None, p)[2]
        assert same_bits(g[None], C.backward(h, np.ones((1, 101), F), None, None, p)[0])
        assert g.argmax() == 50 and g[50] == F(peak) and (g[:50] <= g[50]).all() and (g >= 0).all(), sur


@pytest.mark.parametrize('drive,rate', ((-1.0, 0.0), (3.0, 1.0)))
def test_no_spike_at_all_and_a_spike_at_every_step(be, drive, rate):
    T, N = 6, 68
    x = np.full((T, N), drive, F)
    g_s, g_vseq, g_vlast = case(T, N, 0)[2:]
    for reset, surrogate, detach in C.MODES:
        p = Params(reset=reset, surrogate=surrogate, detach_reset=detach)
        xt = dev(x).requires_grad_()
        s, v_seq, v_last = be.lif_sequence(xt, return_v=True, **p.kwargs())
        s_ref, vseq_ref, h_ref, vlast_ref = C.forward(x, None, p)
        assert s_ref.mean() == rate and same_bits(host(s), s_ref) and same_bits(host(v_seq), vseq_ref)
        gx, = torch.autograd.grad([s, v_seq, v_last], [xt], [dev(g_s), dev(g_vseq), dev(g_vlast)])
        assert same_bits(host(gx), C.backward(h_ref, g_s, g_vseq, g_vlast, p)[0]), p


def test_nan_stays_in_its_slot(be):
    T, N = 5, 72
    x = case(T, N, 0)[0].copy()
    x[1, 3] = x[0, 70] = np.nan
    for reset in C.RESETS:
        p = Params(reset=reset)
        s, v_seq, v_last = be.lif_sequence(dev(x), return_v=True, **p.kwargs())
        s_ref, vseq_ref, _, vlast_ref = C.forward(x, None, p)
        assert same_bits(host(s), s_ref) and same_bits(host(v_seq), vseq_ref) and same_bits(host(v_last), vlast_ref)
        nan = np.isnan(host(v_seq))
        assert nan[1:, 3].all() and not nan[0, 3] and nan[:, 70].all() and nan.sum() == 4 + 5
        assert host(s)[1:, 3].sum() == 0 and host(s)[:, 70].sum() == 0 and list(np.flatnonzero(np.isnan(host(v_last)))) == [3, 70]


def test_v0_none_is_zeros(be):
    for N in (64, 65):
        check_sequence(be, 5, N, Params(), use_v0=False)
        x = dev(case(5, N, 0)[0])
        a = be.lif_sequence(x, None, beta=0.9, return_v=True)
        b = be.lif_sequence(x, torch.zeros(N, device='cuda'), beta=0.9, return_v=True)
        assert all(same_bits(host(i), host(j)) for i, j in zip(a, b))
    # no step at all: the state passes through
    s, v_last = be.lif_sequence(torch.empty(0, 5, device='cuda'), torch.ones(5, device='cuda'), beta=0.9)
    assert s.shape == (0, 5) and host(v_last).tolist() == [1.0] * 5
    s, v_last = be.lif_sequence(torch.empty(3, 0, device='cuda'), beta=0.9)
    assert s.shape == (3, 0) and v_last.shape == (0,)


# ======================================================================================================== step against sequence
@pytest.mark.parametrize('reset,surrogate,detach', C.MODES[::3] + C.MODES[1::5])
def test_sequence_equals_steps(be, reset, surrogate, detach):
    T, N = 6, 132
    p = Params(reset=reset, surrogate=surrogate, detach_reset=detach, alpha=2.0 if surrogate == 'triangle' else 10.0)
    x, v0, g_s, g_vseq, g_vlast = case(T, N, 11)
    gs = [dev(g_s), dev(g_vseq), dev(g_vlast)]
    xa, va = dev(x).requires_grad_(), dev(v0).requires_grad_()
    outs_a = be.lif_sequence(xa, va, return_v=True, **p.kwargs())
    xb, vb = dev(x).requires_grad_(), dev(v0).requires_grad_()
    v, ss, vs = vb, [], []
    for t in range(T):
        s, v = be.lif_step(v, xb[t], **p.kwargs())
        ss.append(s)
        vs.append(v)
    outs_b = (torch.stack(ss), torch.stack(vs), v)
    for a, b in zip(outs_a, outs_b):
        assert same_bits(host(a), host(b))
    # (a membrane's gradient is the sum of two, what the next step hands back and g_vseq[t]: the same sum in either order)
    ga = torch.autograd.grad(outs_a, [xa, va], gs)
    gb = torch.autograd.grad(outs_b, [xb, vb], gs)
    for a, b in zip(ga, gb):
        assert same_bits(host(a), host(b)) and torch.count_nonzero(a).item() > 0


# ======================================================================================================== integration
class HostLif(torch.autograd.Function):
    """lif_step with both passes computed by the restatement on the host."""

    @staticmethod
    def forward(ctx, v, x, p):
        ctx.set_materialize_grads(False)
        s, _, h, v_new = C.forward(host(x).reshape(1, -1), host(v).reshape(-1), p)
        ctx.h, ctx.p, ctx.shape = h, p, x.shape
        return dev(s).reshape(x.shape), dev(v_new).reshape(x.shape)

    @staticmethod
    def backward(ctx, g_s, g_v):
        g_x, g_v0 = C.backward(ctx.h, None if g_s is None else host(g_s).reshape(1, -1), None,
                               None if g_v is None else host(g_v).reshape(-1), ctx.p)
        return dev(g_v0).reshape(ctx.shape), dev(g_x).reshape(ctx.shape), None


def test_recurrent_loop_through_a_csr_parameter(be):
    """BinaryArray(s) @ csr -> lif_step, three steps, a Parameter in the CSR: w.grad, x.grad, v0.grad equal the same loop with the
    neuron computed on the host.  (Weights and sums are small dyadic numbers: the scatter's sums are exact in any order.)"""
    rng = np.random.default_rng(21)
    batch, n, n_conn, T = 4, 96, 12, 3
    indptr = torch.arange(n + 1, dtype=torch.int32, device='cuda') * n_conn
    indices = dev(rng.integers(0, n, n * n_conn).astype(np.int32))
    w0 = (rng.integers(-8, 9, n * n_conn) / 32.0).astype(F)
    x0 = (rng.integers(0, 64, (T, batch, n)) / 32.0).astype(F)
    v00 = (rng.integers(-16, 32, (batch, n)) / 32.0).astype(F)
    g_s, g_v = (rng.integers(-8, 9, (batch, n)) / 8.0).astype(F), (rng.integers(-8, 9, (batch, n)) / 8.0).astype(F)
    p = Params(beta=0.5)

    def loop(neuron):
        w = torch.nn.Parameter(dev(w0))
        csr = be.CSR((w, indices, indptr), shape=(n, n))
        x, v0 = dev(x0).requires_grad_(), dev(v00).requires_grad_()
        v, s, rate = v0, torch.zeros(batch, n, device='cuda'), []
        for t in range(T):
            s, v = neuron(v, x[t] + be.BinaryArray(s) @ csr)
            rate.append(float(s.detach().mean()))
        ((s * dev(g_s)).sum() + (v * dev(g_v)).sum()).backward()
        return rate, [host(t) for t in (s, v, w.grad, x.grad, v0.grad)]

    rate_a, a = loop(lambda v, i: be.lif_step(v, i, **p.kwargs()))
    rate_b, b = loop(lambda v, i: HostLif.apply(v, i, p))
    assert all(0.05 < r < 0.95 for r in rate_a) and rate_a == rate_b
    for name, i, j in zip(('s', 'v', 'w.grad', 'x.grad', 'v0.grad'), a, b):
        assert same_bits(i, j) and np.count_nonzero(i) > 0, name


def test_no_grad_keeps_nothing(be, monkeypatch):
    from brainevent_amd import _neuron_sg
    h_ptrs = []
    real = _neuron_sg.call

    def spy(name, *args):
        if name == 'be_lif_sg_forward':
            h_ptrs.append(args[4].value)
        return real(name, *args)
    monkeypatch.setattr(_neuron_sg, 'call', spy)
    x, v0, *_ = case(4, 132, 0)
    xt, vt = dev(x).requires_grad_(), dev(v0).requires_grad_()
    want = be.lif_sequence(xt, vt, beta=0.9, return_v=True)
    assert h_ptrs[-1] is not None and all(o.grad_fn is not None for o in want)
    with torch.no_grad():
        got = be.lif_sequence(xt, vt, beta=0.9, return_v=True)
        got1 = be.lif_step(vt, xt[0], beta=0.9)
    plain = be.lif_sequence(dev(x), dev(v0), beta=0.9, return_v=True)         # nothing requires grad
    assert h_ptrs[-3:] == [None, None, None]
    for outs in (got, plain):
        assert all(o.grad_fn is None and not o.requires_grad for o in outs)
        assert all(same_bits(host(a), host(b)) for a, b in zip(outs, want))
    assert same_bits(host(got1[0]), host(want[0][0])) and got1[1].grad_fn is None


# ======================================================================================================== graph capture
def test_capture_forward_and_backward(be):
    T, N = 3, 200
    p = Params(reset='soft', surrogate='atan')
    x_in, v_in = torch.zeros(T, N, device='cuda'), torch.zeros(N, device='cuda')
    g_in = [torch.zeros(T, N, device='cuda'), torch.zeros(T, N, device='cuda'), torch.zeros(N, device='cuda')]

    def step():
        x, v0 = x_in.detach().requires_grad_(), v_in.detach().requires_grad_()      # leaves of this call, on the static memory
        s, v = be.lif_step(v0, x[0], **p.kwargs())
        outs = be.lif_sequence(x, v, return_v=True, **p.kwargs())
        return (s,) + tuple(outs) + tuple(torch.autograd.grad(outs, [x, v0], g_in))

    def load(seed):
        for t, a in zip([x_in, v_in] + g_in, case(T, N, seed)):
            t.copy_(dev(a))

    load(1)
    graphed = be.capture_step(step)
    for seed in (2, 3):
        load(seed)
        got = [t.detach().clone() for t in graphed()]
        want = step()
        assert all(same_bits(host(a), host(b)) for a, b in zip(got, want))
        assert 0 < float(got[1].mean()) < 1 and torch.count_nonzero(got[-2]).item() > 0
    x, v0, g_s, g_vseq, g_vlast = case(T, N, 3)                                # ... and the eager result is the restatement's
    v1 = C.forward(x[:1], v0, p)[3]
    s_ref, _, h_ref, _ = C.forward(x, v1, p)
    assert same_bits(host(want[1]), s_ref) and same_bits(host(want[4])[1:], C.backward(h_ref, g_s, g_vseq, g_vlast, p)[0][1:])


# ======================================================================================================== C error codes
def test_c_error_codes_then_a_clean_call(be):
    from brainevent_amd import _array as A, _lib
    fwd, bwd = _lib.fn('be_lif_sg_forward'), _lib.fn('be_lif_sg_backward')
    T, N = 3, 64
    x, v0, g_s, g_vseq, g_vlast = (dev(a) for a in case(T, N, 0))
    s, v_seq, h, g_x = (torch.full((T, N), 7.0, device='cuda') for _ in range(4))
    v_last, g_v0 = torch.full((N,), 7.0, device='cuda'), torch.full((N,), 7.0, device='cuda')
    P, null, st = A.ptr, A.ptr(None), A.stream_ptr()
    INVALID = -1

    def forward(x=P(x), v0=P(v0), s=P(s), v_seq=P(v_seq), h=P(h), v_last=P(v_last), T=T, N=N, mode=0):
        return fwd(x, v0, s, v_seq, h, v_last, T, N, 0.9, 1.0, 0.0, mode, st)

    def backward(h=P(h), g_s=P(g_s), g_vseq=P(g_vseq), g_vlast=P(g_vlast), g_x=P(g_x), g_v0=P(g_v0), T=T, N=N, mode=0, sur=0,
                 alpha=10.0):
        return bwd(h, g_s, g_vseq, g_vlast, g_x, g_v0, T, N, 0.9, 1.0, 0.0, mode, sur, alpha, 0, st)

    for bad in (dict(x=null), dict(s=null), dict(v_last=null), dict(T=-1), dict(N=-1), dict(mode=2), dict(mode=-1)):
        assert forward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_sg_forward: ')
    for bad in (dict(h=null), dict(g_x=null), dict(T=-1), dict(N=-1), dict(mode=2), dict(sur=3), dict(sur=-1), dict(alpha=0.0),
                dict(alpha=-1.0), dict(alpha=float('nan'))):
        assert backward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_sg_backward: ')
    # nothing to do: BE_OK and nothing written, whatever the pointers
    assert forward(T=0) == 0 and forward(N=0) == 0 and forward(T=0, x=null, s=null, v_last=null) == 0
    assert backward(T=0) == 0 and backward(N=0) == 0 and backward(N=0, h=null, g_x=null) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (s, v_seq, h, g_x, v_last, g_v0))
    # a clean call after the refused ones, optional pointers NULL and given
    p = Params()
    s_ref, vseq_ref, h_ref, vlast_ref = C.forward(host(x), host(v0), p)
    assert forward(v_seq=null, h=null) == 0
    assert same_bits(host(s), s_ref) and same_bits(host(v_last), vlast_ref) and bool((v_seq == 7.0).all()) and bool((h == 7.0).all())
    assert forward() == 0 and same_bits(host(v_seq), vseq_ref) and same_bits(host(h), h_ref)
    assert backward(g_v0=null) == 0
    gx_ref, gv0_ref = C.backward(h_ref, host(g_s), host(g_vseq), host(g_vlast), p)
    assert same_bits(host(g_x), gx_ref) and bool((g_v0 == 7.0).all())
    assert backward() == 0 and same_bits(host(g_v0), gv0_ref)


# ======================================================================================================== Python refusals
def test_python_refusals(be, monkeypatch):
    from brainevent_amd import _neuron_sg

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron_sg, 'call', no_call)
    v, x, seq = torch.zeros(4, device='cuda'), torch.zeros(4, device='cuda'), torch.zeros(3, 4, device='cuda')
    for kw, match in ((dict(reset='none'), 'reset'), (dict(surrogate='relu'), 'surrogate'), (dict(alpha=0.0), 'alpha'),
                      (dict(alpha=-1.0), 'alpha')):
        with pytest.raises(ValueError, match=match):
            be.lif_step(v, x, beta=0.9, **kw)
        with pytest.raises(ValueError, match=match):
            be.lif_sequence(seq, v, beta=0.9, **kw)
    for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
        with pytest.raises(TypeError, match='float32'):
            be.lif_step(v.to(dtype), x, beta=0.9)
        with pytest.raises(TypeError, match='float32'):
            be.lif_step(v, x.to(dtype), beta=0.9)
        with pytest.raises(TypeError, match='float32'):
            be.lif_sequence(seq.to(dtype), v, beta=0.9)
        with pytest.raises(TypeError, match='float32'):
            be.lif_sequence(seq, v.to(dtype), beta=0.9)
    for args in ((v.cpu(), x), (v, x.cpu())):
        with pytest.raises(ValueError, match='device tensor'):
            be.lif_step(*args, beta=0.9)
    for args in ((seq.cpu(), v), (seq, v.cpu()), (seq.cpu(), None)):
        with pytest.raises(ValueError, match='device tensor'):
            be.lif_sequence(*args, beta=0.9)
    with pytest.raises(ValueError, match='one shape'):
        be.lif_step(torch.zeros(5, device='cuda'), x, beta=0.9)
    with pytest.raises(ValueError, match='one shape'):
        be.lif_step(v, seq, beta=0.9)
    with pytest.raises(ValueError, match='shape of a step'):
        be.lif_sequence(seq, torch.zeros(3, device='cuda'), beta=0.9)
    with pytest.raises(ValueError, match='shape of a step'):
        be.lif_sequence(seq, seq, beta=0.9)
