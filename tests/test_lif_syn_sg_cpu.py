"""The differentiable neuron with a synaptic current and an adaptive threshold without a device: the numpy restatement the GPU
tests compare with (tests/lif_syn_sg_cases.py) is held to torch's CPU autograd of the plain formula and, where the two coincide,
to the restatement of the plain LIF neuron (tests/lif_sg_cases.py); the constants the GPU sizes come from are held to the text of
csrc/be_neuron_sg.hip and csrc/be_sg_lane.h, the prototypes to the header, and the refusals that need no device are raised.

Forward values must be equal.  Gradients are compared within the propagated bound of ``lif_syn_sg_cases.backward(with_bound=True)``:
``4 * 2**-24 * sum |terms of g_c|`` per step, carried through the three coupled carries — autograd sums the same terms in an
order that is not ours to fix, and that is what two orderings of a short f32 sum can differ by."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lif_sg_cases as C0
import lif_syn_sg_cases as C
from lif_syn_sg_cases import F

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron_sg.hip'
LANE = ROOT / 'brainevent_amd' / 'csrc' / 'be_sg_lane.h'
HEADER = ROOT / 'include' / 'brainevent_amd.h'


class Spike(torch.autograd.Function):
    """Heaviside of ``h - th`` forwards; backwards the surrogate's derivative to ``h`` and its negative to ``th``, every operation
    a torch f32 operation of its own."""

    @staticmethod
    def forward(ctx, h, th, p):
        ctx.save_for_backward(h, th)
        ctx.p = p
        return (h >= th).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        h, th = ctx.saved_tensors
        p = ctx.p
        one, alpha = torch.tensor(F(1)), torch.tensor(F(p.alpha))
        u = h - th
        if p.surrogate == 'fast_sigmoid':
            d = one + alpha * u.abs()
            sg = one / (d * d)
        elif p.surrogate == 'atan':
            q = torch.tensor(F(np.pi / 2 * p.alpha)) * u
            sg = torch.tensor(F(p.alpha / 2)) / (one + q * q)
        else:
            sg = alpha * torch.clamp_min(one - alpha * u.abs(), 0.0)
        gs = g * sg
        return gs, -gs, None


def plain(x, c0, v0, a0, p):
    """The plain formula in torch: ``(s [T, N], v_seq [T, N], c_last, v_last, a_last [N])``."""
    syn_decay, beta, v_th, v_reset, rho, kappa = (torch.tensor(F(k)) for k in (p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa))
    c, v, a, ss, vs = c0, v0, a0, [], []
    for t in range(x.shape[0]):
        c = syn_decay * c + x[t]
        h = beta * v + c
        th = v_th + kappa * a if p.adaptive else v_th.expand_as(h)
        s = Spike.apply(h, th, p)
        sr = s.detach() if p.detach_reset else s
        v = h * (1 - sr) + v_reset * sr if p.reset == 'hard' else h - sr * v_th
        if p.adaptive:
            a = rho * a + s
        ss.append(s)
        vs.append(v)
    return torch.stack(ss), torch.stack(vs), c, v, a


@pytest.mark.parametrize('T', (1, 2, 5))
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', C.MODES)
def test_restatement_against_cpu_autograd(reset, surrogate, detach, adaptive, T):
    p = C.mode_params(reset, surrogate, detach, adaptive)
    x, state, grads = C.inputs(T, 257, seed=T)
    ref = C.forward(x, *state, p)
    assert 0.1 < ref.s_out.mean() < 0.6
    leaves = [torch.tensor(a, requires_grad=True) for a in (x,) + state]
    s, v_seq, c_last, v_last, a_last = plain(*leaves, p)
    for got, want in ((s, ref.s_out), (v_seq, ref.v_seq), (c_last, ref.c_last), (v_last, ref.v_last)):
        assert np.array_equal(got.detach().numpy(), want)              # all slots, none left out
    if adaptive:
        assert np.array_equal(a_last.detach().numpy(), ref.a_last)
    else:
        assert ref.th_save is None and ref.a_last is None
    n_in = 4 if adaptive else 3
    for which, use in C.GRAD_SETS.items():
        if which == 'g_alast' and not adaptive:
            continue
        given = C.pick(grads, use, p)
        outs = [o for o, g in zip((s, v_seq, c_last, v_last, a_last), given) if g is not None]
        got = torch.autograd.grad(outs, leaves[:n_in], [torch.tensor(g) for g in given if g is not None], retain_graph=True,
                                  allow_unused=True)
        got = [np.zeros(l.shape, F) if g is None else g.numpy() for g, l in zip(got, leaves)]
        r, b = C.backward(ref.h_save, ref.th_save, *given, p, with_bound=True)
        for name, g, want, bound in zip(('g_x', 'g_c0', 'g_v0', 'g_a0'), got, r, b):
            err = np.abs(g.astype(np.float64) - want)
            print(f'{which} {name}: max |autograd - ref| {err.max():.3e} (bound there {bound.flat[err.argmax()]:.3e})')
            assert (err <= bound).all(), (which, name)
        assert np.abs(r.g_x).max() > 1e-3
        assert b.g_x.max() < 1e-3 * b.terms.max()                      # the bound is a rounding bound, not a tolerance


def _f64_backward(h, th, g, p, drop=None, alpha=None):
    """The derivative in f64 in one possible order; ``drop`` leaves one term out ('kappa_gu', 'ca', 'cc')."""
    T, N = h.shape
    g_s, g_vseq, g_clast, g_vlast, g_alast = (None if a is None else a.astype(np.float64) for a in g)
    z = np.zeros(N)
    cc, cv, ca = (z if a is None else a for a in (g_clast, g_vlast, g_alast))
    q = C.Params(**{**p.__dict__, 'alpha': p.alpha if alpha is None else alpha})
    g_x = np.zeros((T, N))
    for t in range(T - 1, -1, -1):
        ht, tt = h[t].astype(np.float64), (th[t].astype(np.float64) if p.adaptive else np.full(N, p.v_th))
        s = ht >= tt
        sg = C.surrogate((ht - tt).astype(F), q).astype(np.float64)
        g_vo = cv + (0 if g_vseq is None else g_vseq[t])
        g_sp = (0 if g_s is None else g_s[t]) + (ca if p.adaptive and drop != 'ca' else 0)
        if not p.detach_reset:
            g_sp = g_sp + (g_vo * (F(p.v_reset) - ht) if p.reset == 'hard' else -g_vo * F(p.v_th))
        g_u = g_sp * sg
        g_h = g_u + (np.where(s, 0.0, g_vo) if p.reset == 'hard' else g_vo)
        g_c = cc + g_h
        g_x[t] = g_h if drop == 'cc' else g_c
        cc, cv = F(p.syn_decay) * g_c, F(p.beta) * g_h
        ca = F(p.rho) * ca - (0 if drop == 'kappa_gu' else F(p.kappa) * g_u)
    return g_x, cc, cv, ca


@pytest.mark.parametrize('reset', C.RESETS)
def test_the_comparison_can_fail(reset):
    """Inside the bound: the same derivative in f64.  Outside it: a surrogate off by a part in a thousand, a backward without the
    ``- kappa * g_u`` term, one without the ``+ ca`` term, and one whose ``g_x`` omits ``cc``."""
    p = C.Params(reset=reset, adaptive=True)
    x, state, grads = C.inputs(5, 257, seed=5)
    ref = C.forward(x, *state, p)
    r, b = C.backward(ref.h_save, ref.th_save, *grads, p, with_bound=True)
    outside = lambda got: any((np.abs(g - want.astype(np.float64)) > bound).any() for g, want, bound in zip(got, r, b))
    assert not outside(_f64_backward(ref.h_save, ref.th_save, grads, p))
    assert outside(_f64_backward(ref.h_save, ref.th_save, grads, p, alpha=p.alpha * 1.001))
    for drop in ('kappa_gu', 'ca', 'cc'):
        assert outside(_f64_backward(ref.h_save, ref.th_save, grads, p, drop=drop)), drop
    # the f32 restatement itself with the surrogate off by a part in a thousand
    off = C.backward(ref.h_save, ref.th_save, *grads, C.Params(reset=reset, adaptive=True, alpha=p.alpha * 1.001))
    assert (np.abs(off.g_x.astype(np.float64) - r.g_x) > b.g_x).any()


def test_spike_rate_of_the_inputs():
    for mode in C.MODES:
        p = C.Params(reset=mode[0], surrogate=mode[1], detach_reset=mode[2], adaptive=mode[3])
        x, state, _ = C.inputs(12, 4000, seed=0)
        assert 0.2 <= C.forward(x, *state, p).s_out.mean() <= 0.45, mode


@pytest.mark.parametrize('reset,surrogate,detach', C0.MODES)
def test_reduces_to_the_plain_lif(reset, surrogate, detach):
    """syn_decay = 0, no adaptation, zero c0 and g_clast: the restatement of tests/lif_sg_cases.py, bit for bit."""
    x, v0, g_s, g_vseq, g_vlast = C0.inputs(7, 1000, 3)
    kw = dict(beta=0.9, v_th=1.0, v_reset=-0.25, reset=reset, surrogate=surrogate, detach_reset=detach,
              alpha=2.0 if surrogate == 'triangle' else 10.0)
    p0, p = C0.Params(**kw), C.Params(syn_decay=0.0, **kw)
    s0, vseq0, h0, vlast0 = C0.forward(x, v0, p0)
    for c0 in (None, np.zeros(1000, F)):
        f = C.forward(x, c0, v0, None, p)
        assert all(C.same_bits(a, b) for a, b in ((f.s_out, s0), (f.v_seq, vseq0), (f.h_save, h0), (f.v_last, vlast0)))
    for which, (use_s, use_vseq, use_vlast) in C0.GRAD_SETS.items():
        gx0, gv0 = C0.backward(h0, g_s if use_s else None, g_vseq if use_vseq else None, g_vlast if use_vlast else None, p0)
        b = C.backward(f.h_save, None, g_s if use_s else None, g_vseq if use_vseq else None, None, g_vlast if use_vlast else None,
                       None, p)
        assert C.same_bits(b.g_x, gx0) and C.same_bits(b.g_v0, gv0) and b.g_a0 is None, which


def test_restatement_edges():
    """The crafted on-threshold cases; a NaN does not spike and stays in its slot; a NULL state entry or gradient is zeros."""
    for adaptive in (False, True):
        p, x, state, want = C.threshold_case(adaptive)
        f = C.forward(x, *state, p)
        assert f.s_out[0].tolist() == want['s0']
        if adaptive:
            assert f.th_save[0].tolist() == want['th0'] == [1.5, 1.5] and f.th_save[1].tolist() == want['th1']
            assert want['th1'] == [1.0 + 0.25 * 2.5, 1.0 + 0.25 * 1.5] and f.a_last[0] == 2.5 * 0.75
    x, state, grads = C.inputs(3, 9, seed=1)
    x[1, 4] = np.nan
    p = C.Params(adaptive=True)
    f = C.forward(x, *state, p)
    assert np.isnan(f.v_seq[1:, 4]).all() and f.s_out[1:, 4].sum() == 0 and np.isnan(f.h_save).sum() == 2
    x, state, grads = C.inputs(2, 9, seed=1)
    zeros = np.zeros(9, F)
    a, b = C.forward(x, None, None, None, p), C.forward(x, zeros, zeros, zeros, p)
    assert all(C.same_bits(i, j) for i, j in zip(a, b))
    g = C.backward(a.h_save, a.th_save, grads[0], None, None, None, None, p)
    h = C.backward(a.h_save, a.th_save, grads[0], np.zeros_like(x), zeros, zeros, zeros, p)
    assert all(C.same_bits(i, j) for i, j in zip(g, h))
    # v_th = inf: no spike, the membrane is the input filtered twice, every surrogate is 0 at u = -inf
    for sur in C.SURROGATES:
        q = C.Params(v_th=float('inf'), surrogate=sur)
        f = C.forward(x, None, None, None, q)
        assert f.s_out.sum() == 0 and C.same_bits(f.v_seq, f.h_save)
        r = C.backward(f.h_save, None, grads[0], grads[1], None, None, None, q)
        assert np.isfinite(r.g_x).all() and np.abs(r.g_x).max() > 0


# ------------------------------------------------------------------------------------------------ the constants and the source
PATTERNS = {
    'kSgThreads': (r'constexpr int kSgThreads = (\d+);', 'N_PAST_ONE_PASS'),
    'kSgGridCap': (r'constexpr int kSgGridCap = (\d+);', 'N_PAST_ONE_PASS'),
    'kSgVec': (r'constexpr int kSgVec = (\d+);', 'N_PAST_ONE_PASS and the scalar-path cases'),
    'kSgPrefetch': (r'constexpr int kSgPrefetch = (\d+);', 'T_SIZES'),
}

SOURCE_TEXT = [
    # which kernel a call takes, and how many blocks
    ('const bool vec = (N % kSgVec == 0) && lane::all_aligned16(x, c0, v0, a0, s_out, v_seq, h_save, th_save, c_last, v_last, a_last);', 1),
    ('const bool vec = (N % kSgVec == 0) && lane::all_aligned16(h_save, th_save, g_s, g_vseq, g_clast, g_vlast, g_alast, g_x, g_c0, g_v0, g_a0);', 1),
    ('constexpr int S = decltype(V)::value ? kSgVec : 1;', 2),
    ('dim3(lane_grid(N, S)),', 2),
    ('return (int)std::min<int64_t>((groups + kSgThreads - 1) / kSgThreads, kSgGridCap);', 1),
    ('__launch_bounds__(kSgThreads)', 2),
    # the rings: filled a depth ahead, walked in blocks of the depth
    ('for (int64_t t0 = 0; t0 < T; t0 += kSgPrefetch) {', 1),
    ('if (t + kSgPrefetch < T) ring[r] = lane::load<S>(x + (t + kSgPrefetch) * N + i);', 1),
    ('for (int64_t k0 = 0; k0 < T; k0 += kSgPrefetch) {', 1),
    ('if (k + kSgPrefetch < T) {', 1),
    ('V ring_h[kSgPrefetch], ring_t[M::ADAPT ? kSgPrefetch : 1], ring_s[kSgPrefetch], ring_v[kSgPrefetch];', 1),
    ('#pragma clang fp contract(off)', 2),
]


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, cases = PATTERNS[key]
    found = re.findall(pattern, SOURCE.read_text())
    assert len(found) == 1 and int(found[0]) == C.CONSTS[key], (f'{key}: be_neuron_sg.hip says {found}, '
                                                               f'tests/lif_syn_sg_cases.py assumes {C.CONSTS[key]}: re-size {cases}')


def test_sizes_follow_the_constants():
    assert set(PATTERNS) == set(C.CONSTS)
    text = SOURCE.read_text()
    for line, times in SOURCE_TEXT:
        assert text.count(line) == times, f'be_neuron_sg.hip holds {line!r} {text.count(line)} times, not {times}'
    assert len(re.findall(r'constexpr int kSg\w+ = ', text)) == len(C.CONSTS)                  # no depth the table does not know
    k = C.CONSTS
    scalar, vector = C.N_PAST_ONE_PASS
    assert scalar % k['kSgVec'] != 0 and scalar == k['kSgThreads'] * k['kSgGridCap'] + 1     # 4-byte kernel, second trip: one slot
    assert vector % k['kSgVec'] == 0 and vector // k['kSgVec'] == k['kSgThreads'] * k['kSgGridCap'] + 1   # 16-byte kernel: one lane
    assert C.PREFETCH_DEPTHS == (k['kSgPrefetch'],)
    assert {1, 2, 25} | {d + j for d in C.PREFETCH_DEPTHS for j in (-1, 0, 1)} == set(C.T_SIZES)
    assert any(n % k['kSgVec'] for n in C.N_SIZES) and any(n % k['kSgVec'] == 0 for n in C.N_SIZES)
    # plain stores: no atomic read-modify-write, no LDS — here and in the lane helpers, which hold the arithmetic: the derivative,
    # the reset, the forward step, the backward step and its carries, each under a contract(off) of its own
    lane = LANE.read_text()
    for t in (text, lane):
        assert 'atomicAdd' not in t and '__hip_atomic' not in t and '__shared__' not in t
    assert '#include "be_sg_lane.h"' in text and lane.count('#pragma clang fp contract(off)') == 5


def test_prototypes_against_the_header():
    from brainevent_amd import _abi, _neuron_sg, _neuron_syn_sg
    counts = {'be_lif_syn_sg_forward': 22, 'be_lif_syn_sg_backward': 25}
    header = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    for name, n in counts.items():
        restype, argtypes = _abi.PROTOTYPES[name]
        args, = re.findall(rf'\b{name}\(([^)]*)\);', header)
        args = [a.strip() for a in args.split(',')]
        assert restype is ctypes.c_int and len(argtypes) == len(args) == n, name
        for a, ct in zip(args, argtypes):
            want = (ctypes.c_void_p if '*' in a or a.startswith('be_stream_t') else ctypes.c_int64 if a.startswith('int64_t')
                    else ctypes.c_double if a.startswith('double') else ctypes.c_int)
            assert ct is want, (name, a)
    # no new numeric code, and the Python side reuses the float path's tables
    assert len(re.findall(r'#define (BE_LIF_\w+) (\d+)', HEADER.read_text())) == 5
    assert _neuron_syn_sg.RESETS is _neuron_sg.RESETS and _neuron_syn_sg.SURROGATES is _neuron_sg.SURROGATES
    assert set(_neuron_sg.RESETS) == set(C.RESETS) and set(_neuron_sg.SURROGATES) == set(C.SURROGATES)
    # the header states the contract the restatement follows
    doc = HEADER.read_text()
    for line in ('c  = (syn_decay * c) + x[t][i]', 'th = adaptive ? v_th + (kappa * a) : v_th', 'g_c  = cc + g_h;    g_x[t][i] = g_c',
                 'adaptive: ca = (rho * ca) - (kappa * g_u)'):
        assert line in doc, line


# ------------------------------------------------------------------------------------------------ refusals that need no device
class FakeDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: lets the checks that come after ``is_cuda`` run without one."""

    @staticmethod
    def wrap(t):
        return t.as_subclass(FakeDevice)

    @property
    def is_cuda(self):
        return True


def test_refusals_without_a_device(be, monkeypatch):
    from brainevent_amd import _neuron_syn_sg

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron_syn_sg, 'call', no_call)
    monkeypatch.setattr(_neuron_syn_sg.A, 'stream_ptr', lambda: None)           # (evaluated before the call it is an argument of)
    fake = FakeDevice.wrap
    x, seq = fake(torch.zeros(3, 4)), fake(torch.zeros(5, 3, 4))
    c, v, a = (fake(torch.zeros(3, 4)) for _ in range(3))
    kw = dict(syn_decay=0.8, beta=0.9)
    ad = dict(kw, adapt=(0.95, 0.3))

    def both(error, match, state=(c, v), **over):
        with pytest.raises(error, match=match):
            be.synaptic_lif_step(state, x, **{**kw, **over})
        with pytest.raises(error, match=match):
            be.synaptic_lif_sequence(seq, state, **{**kw, **over})

    for over, match in ((dict(reset='none'), 'reset'), (dict(surrogate='relu'), 'surrogate'), (dict(alpha=0.0), 'alpha'),
                        (dict(alpha=-1.0), 'alpha'), (dict(alpha=float('nan')), 'alpha')):
        both(ValueError, match, **over)
    # parameters are Python numbers: a tensor is refused, and told where learnable parameters live
    for name in ('syn_decay', 'beta', 'v_th', 'v_reset', 'alpha'):
        both(TypeError, 'learnable parameters exist for lif_step only', **{name: fake(torch.full((4,), 0.9))})
        both(TypeError, 'Python number', **{name: 'x'})
    both(TypeError, 'learnable parameters exist for lif_step only', state=(c, v, a), adapt=(torch.tensor(0.9), 0.3))
    # adapt: None or a pair of numbers
    for bad, error in ((0.95, TypeError), ('ab', TypeError), ((0.95,), ValueError), ((0.95, 0.3, 0.1), ValueError),
                       ((0.95, None), TypeError), ((0.95, '0.3'), TypeError)):
        both(error, 'adapt', state=(c, v, a), adapt=bad)
    # the state: a tuple of the length adapt asks for, f32 tensors of a step's shape
    both(ValueError, r'without adapt it is \(c, v\)', state=(c, v, a))
    both(ValueError, r'takes \(c, v, a\)', state=(c, v), adapt=(0.95, 0.3))
    both(ValueError, 'entries', state=(c,))
    both(TypeError, 'tuple', state=c)
    for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
        both(TypeError, 'float32', state=(c.to(dtype), v))
        both(TypeError, 'float32', state=(c, v, fake(torch.zeros(3, 4, dtype=dtype))), adapt=(0.95, 0.3))
        with pytest.raises(TypeError, match='float32'):
            be.synaptic_lif_step((c, v), x.to(dtype), **kw)
        with pytest.raises(TypeError, match='float32'):
            be.synaptic_lif_sequence(seq.to(dtype), (c, v), **kw)
    both(ValueError, 'shape of a step', state=(c, fake(torch.zeros(4))))
    both(ValueError, 'shape of a step', state=(fake(torch.zeros(3, 5)), v))
    both(ValueError, 'shape of a step', state=(c, v, seq), adapt=(0.95, 0.3))
    both(TypeError, 'Tensor', state=(c, np.zeros((3, 4), F)))
    with pytest.raises(TypeError, match='Tensor'):                             # a step needs its whole state ...
        be.synaptic_lif_step((c, None), x, **kw)
    with pytest.raises(TypeError, match='tuple'):
        be.synaptic_lif_step(None, x, **kw)
    with pytest.raises(TypeError, match='Tensor'):
        be.synaptic_lif_sequence([[0.0]], **kw)
    with pytest.raises(ValueError, match=r'\[T, \.\.\.\]'):
        be.synaptic_lif_sequence(fake(torch.zeros(())), **kw)
    # CPU tensors: there is no CPU implementation
    cpu = torch.zeros(3, 4)
    for state in ((cpu, v), (c, cpu)):
        both(ValueError, 'device tensor', state=state)
    with pytest.raises(ValueError, match='device tensor'):
        be.synaptic_lif_step((c, v), cpu, **kw)
    with pytest.raises(ValueError, match='device tensor'):
        be.synaptic_lif_sequence(torch.zeros(5, 3, 4), **kw)
    with pytest.raises(ValueError, match='device tensor'):
        be.synaptic_lif_sequence(seq, (None, None, cpu), **ad)
    with pytest.raises(TypeError):                                             # syn_decay and beta have no default
        be.synaptic_lif_step((c, v), x, beta=0.9)
    with pytest.raises(TypeError):
        be.synaptic_lif_sequence(seq, syn_decay=0.8)
    # ... and what is accepted passes every check: the first thing it reaches is the device call
    for args, k in (((seq,), kw), ((seq, None), ad), ((seq, (None, v)), kw), ((seq, [c, None, a]), ad), ((seq, (c, v, a)), ad)):
        with pytest.raises(AssertionError, match='reached the device call'):
            be.synaptic_lif_sequence(*args, **k)
    with pytest.raises(AssertionError, match='reached the device call'):
        be.synaptic_lif_step((c, v, a), x, **dict(ad, v_th=float('inf'), alpha=np.float32(2.0), syn_decay=1))


def test_the_call_and_the_unchanged_old_path(be, monkeypatch):
    """Spied on, not run: the arguments the new entry point gets, and two Python floats through lif_step still reach
    be_lif_sg_forward."""
    from brainevent_amd import _neuron_sg, _neuron_syn_sg
    calls = []

    def spy(name, *args):
        calls.append((name, args))
    for m in (_neuron_sg, _neuron_syn_sg):
        monkeypatch.setattr(m, 'call', spy)
    monkeypatch.setattr(_neuron_sg.A, 'stream_ptr', lambda: None)
    fake = FakeDevice.wrap
    v, x, seq = fake(torch.zeros(3, 4)), fake(torch.zeros(3, 4)), fake(torch.zeros(5, 3, 4))
    be.lif_step(v, x, beta=0.9, v_th=1.25)
    be.lif_sequence(seq, v, beta=np.float32(0.5), v_th=2)
    assert [c[0] for c in calls] == ['be_lif_sg_forward', 'be_lif_sg_forward']
    (_, a), (_, b) = calls
    assert a[6:11] == (1, 12, 0.9, 1.25, 0.0) and b[6:11] == (5, 12, 0.5, 2.0, 0.0) and len(a) == 13
    calls.clear()
    be.synaptic_lif_step((v, v), x, syn_decay=0.8, beta=0.9)
    be.synaptic_lif_sequence(seq, (None, v, v), syn_decay=0.5, beta=0.25, v_th=2, reset='soft', adapt=(0.75, 0.125), return_v=True)
    assert [c[0] for c in calls] == ['be_lif_syn_sg_forward', 'be_lif_syn_sg_forward']
    (_, a), (_, b) = calls
    assert len(a) == len(b) == 22
    assert a[11:21] == (1, 12, 0.8, 0.9, 1.0, 0.0, 0.0, 0.0, 0, 0) and b[11:21] == (5, 12, 0.5, 0.25, 2.0, 0.0, 0.75, 0.125, 1, 1)
    null = [i for i, p in enumerate(a[:11]) if p.value is None]
    assert null == [3, 5, 6, 7, 10]                  # a0, v_seq, h_save, th_save, a_last: no adaptation, nothing requires grad
    assert [i for i, p in enumerate(b[:11]) if p.value is None] == [1, 6, 7]          # c0 None; no backward pass: no h / th
