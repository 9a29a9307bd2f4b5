"""The differentiable LIF neuron without a device: the numpy restatement the GPU tests compare with (tests/lif_sg_cases.py) is held
to torch's CPU autograd of the plain formula, the constants the GPU sizes come from are held to the text of csrc/be_neuron_sg.hip,
and the refusals that need no device are raised.

Forward values must be equal.  Gradients are compared within ``4 * 2**-24 * sum |terms of g_h|`` per element, carried through the
T steps (``lif_sg_cases.backward(with_bound=True)``): autograd sums the same terms in an order that is not ours to fix, and that
is what two orderings of a short f32 sum can differ by."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lif_sg_cases as C
from lif_sg_cases import F

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron_sg.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'


class Spike(torch.autograd.Function):
    """Heaviside forward; backward the surrogate's derivative, every operation a torch f32 operation of its own."""

    @staticmethod
    def forward(ctx, h, p):
        ctx.save_for_backward(h)
        ctx.p = p
        return (h >= torch.tensor(F(p.v_th))).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        h, = ctx.saved_tensors
        p = ctx.p
        one, alpha = torch.tensor(F(1)), torch.tensor(F(p.alpha))
        u = h - torch.tensor(F(p.v_th))
        if p.surrogate == 'fast_sigmoid':
            d = one + alpha * u.abs()
            sg = one / (d * d)
        elif p.surrogate == 'atan':
            q = torch.tensor(F(np.pi / 2 * p.alpha)) * u
            sg = torch.tensor(F(p.alpha / 2)) / (one + q * q)
        else:
            sg = alpha * torch.clamp_min(one - alpha * u.abs(), 0.0)
        return g * sg, None


def plain(x, v0, p):
    """The plain formula in torch: ``(s [T, N], v_seq [T, N], v_last [N])``."""
    beta, v_th, v_reset = (torch.tensor(F(c)) for c in (p.beta, p.v_th, p.v_reset))
    v, ss, vs = v0, [], []
    for t in range(x.shape[0]):
        h = beta * v + x[t]
        s = Spike.apply(h, p)
        sr = s.detach() if p.detach_reset else s
        v = h * (1 - sr) + v_reset * sr if p.reset == 'hard' else h - sr * v_th
        ss.append(s)
        vs.append(v)
    return torch.stack(ss), torch.stack(vs), v


@pytest.mark.parametrize('T', (1, 3))
@pytest.mark.parametrize('v_reset', (0.0, -0.25))
@pytest.mark.parametrize('reset,surrogate,detach', C.MODES)
def test_restatement_against_cpu_autograd(reset, surrogate, detach, v_reset, T):
    p = C.Params(reset=reset, surrogate=surrogate, detach_reset=detach, v_reset=v_reset, alpha=2.0 if surrogate == 'triangle' else 10.0)
    x, v0, g_s, g_vseq, g_vlast = C.inputs(T, 257, seed=T)
    s_ref, vseq_ref, h_ref, vlast_ref = C.forward(x, v0, p)
    assert 0.1 < s_ref.mean() < 0.9
    xt, vt = torch.tensor(x, requires_grad=True), torch.tensor(v0, requires_grad=True)
    s, v_seq, v_last = plain(xt, vt, p)
    assert np.array_equal(s.detach().numpy(), s_ref) and np.array_equal(v_seq.detach().numpy(), vseq_ref)
    assert np.array_equal(v_last.detach().numpy(), vlast_ref)
    for which, (use_s, use_vseq, use_vlast) in C.GRAD_SETS.items():
        outs = [o for o, use in ((s, use_s), (v_seq, use_vseq), (v_last, use_vlast)) if use]
        grads = [torch.tensor(g) for g, use in ((g_s, use_s), (g_vseq, use_vseq), (g_vlast, use_vlast)) if use]
        gx, gv0 = torch.autograd.grad(outs, [xt, vt], grads, retain_graph=True, allow_unused=True)
        gx = np.zeros_like(x) if gx is None else gx.numpy()
        gv0 = np.zeros_like(v0) if gv0 is None else gv0.numpy()
        rx, rv0, bound, bound_v0 = C.backward(h_ref, g_s if use_s else None, g_vseq if use_vseq else None,
                                              g_vlast if use_vlast else None, p, with_bound=True)
        ex, ev0 = np.abs(gx.astype(np.float64) - rx), np.abs(gv0.astype(np.float64) - rv0)
        print(f'{which}: max |g_x - ref| {ex.max():.3e} (bound there {bound.flat[ex.argmax()]:.3e}), '
              f'max |g_v0 - ref| {ev0.max():.3e} (bound there {bound_v0.flat[ev0.argmax()]:.3e})')
        assert np.abs(rx).max() > 1e-3 and (ex <= bound).all() and (ev0 <= bound_v0).all(), which
        assert bound.max() < 1e-3 * max(1.0, np.abs(rx).max())        # the bound is a rounding bound, not a tolerance


def test_the_comparison_can_fail():
    """A surrogate that is off by a part in a thousand is outside the bound."""
    p, q = C.Params(alpha=10.0), C.Params(alpha=10.01)
    x, v0, g_s, g_vseq, g_vlast = C.inputs(3, 257, seed=5)
    h = C.forward(x, v0, p)[2]
    rx, _, bound, _ = C.backward(h, g_s, g_vseq, g_vlast, p, with_bound=True)
    ox, _ = C.backward(h, g_s, g_vseq, g_vlast, q)
    assert (np.abs(ox.astype(np.float64) - rx) > bound).any()


def test_restatement_edges():
    """h == v_th spikes; u = 0 is where each surrogate is largest; a NaN does not spike; the unused gradients are zeros."""
    p = C.Params(beta=0.5)
    s, v_seq, h, v_last = C.forward(np.array([[0.5, 0.25, np.nan]], F), np.array([1.0, 1.0, 1.0], F), p)
    assert h[0, 0] == 1.0 and list(s[0]) == [1.0, 0.0, 0.0] and v_last[0] == 0.0 and v_last[1] == 0.75 and np.isnan(v_last[2])
    u = np.linspace(-1, 1, 2001).astype(F)
    for sur, peak in (('fast_sigmoid', 1.0), ('atan', 5.0), ('triangle', 10.0)):
        sg = C.surrogate(u, C.Params(surrogate=sur))
        assert sg.argmax() == 1000 and u[1000] == 0 and sg[1000] == F(peak) and (sg >= 0).all()
    x, v0, g_s, g_vseq, g_vlast = C.inputs(2, 9, seed=1)
    h = C.forward(x, v0, p)[2]
    a = C.backward(h, g_s, None, None, p)
    b = C.backward(h, g_s, np.zeros_like(g_vseq), np.zeros_like(g_vlast), p)
    assert all(C.same_bits(i, j) for i, j in zip(a, b))
    assert not C.same_bits(np.array([0.0], F), np.array([-0.0], F)) and C.same_bits(np.array([np.nan], F), -np.array([np.nan], F))


# ------------------------------------------------------------------------------------------------ the constants and the source
PATTERNS = {
    'kSgThreads': (r'constexpr int kSgThreads = (\d+);', 'N_PAST_ONE_PASS'),
    'kSgGridCap': (r'constexpr int kSgGridCap = (\d+);', 'N_PAST_ONE_PASS'),
    'kSgVec': (r'constexpr int kSgVec = (\d+);', 'N_PAST_ONE_PASS and the scalar-path cases'),
    'kSgPrefetch': (r'constexpr int kSgPrefetch = (\d+);', 'T_SIZES'),
}

SOURCE_TEXT = [
    # which kernel a call takes, and how many blocks
    ('const bool vec = (N % kSgVec == 0) && lane::all_aligned16(x, v0, s_out, v_seq, h_save, v_last);', 1),
    ('const bool vec = (N % kSgVec == 0) && lane::all_aligned16(h_save, g_s, g_vseq, g_vlast, g_x, g_v0);', 1),
    ('constexpr int S = decltype(V)::value ? kSgVec : 1;', 2),
    ('dim3(lane_grid(N, S)),', 2),
    ('return (int)std::min<int64_t>((groups + kSgThreads - 1) / kSgThreads, kSgGridCap);', 1),
    ('__launch_bounds__(kSgThreads)', 2),
    # the ring: filled kSgPrefetch steps ahead, walked in blocks of kSgPrefetch
    ('for (int64_t t0 = 0; t0 < T; t0 += kSgPrefetch) {', 1),
    ('for (int64_t k0 = 0; k0 < T; k0 += kSgPrefetch) {', 1),
    ('if (t + kSgPrefetch < T) ring[r] = lane::load<S>(x + (t + kSgPrefetch) * N + i);', 1),
    ('if (k + kSgPrefetch < T) {', 1),
    ('#pragma clang fp contract(off)', 2),            # the two kernels; the arithmetic's are be_sg_lane.h's (test_lif_syn_sg_cpu.py)
]

#: the six entry points of the one file, and what must be stated in exactly one file under csrc/
ENTRY_POINTS = ('be_lif_sg_forward', 'be_lif_sg_backward', 'be_lif_sg_forward_params', 'be_lif_sg_backward_params',
                'be_lif_syn_sg_forward', 'be_lif_syn_sg_backward')
STATED_ONCE = {
    "the surrogate's derivative": r'1\.0f / \(d \* d\)',
    'the 16-byte pack': r'struct \w*Pack<4> \{ using type = float4; \};',
    "the backward pass's reset term": r'g_vo \* \(p\.v_reset - h\)',
    "the forward pass's soft reset": r's \? h - \w+ : h',
}


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, cases = PATTERNS[key]
    found = re.findall(pattern, SOURCE.read_text())
    assert len(found) == 1 and int(found[0]) == C.CONSTS[key], (f'{key}: be_neuron_sg.hip says {found}, tests/lif_sg_cases.py assumes '
                                                               f'{C.CONSTS[key]}: re-size {cases}')


def test_sizes_follow_the_constants():
    assert set(PATTERNS) == set(C.CONSTS)
    text = SOURCE.read_text()
    for line, times in SOURCE_TEXT:
        assert text.count(line) == times, f'be_neuron_sg.hip holds {line!r} {text.count(line)} times, not {times}'
    k = C.CONSTS
    scalar, vector = C.N_PAST_ONE_PASS
    assert scalar % k['kSgVec'] != 0 and scalar == k['kSgThreads'] * k['kSgGridCap'] + 1             # 4-byte kernel, second trip: one slot
    assert vector % k['kSgVec'] == 0 and vector // k['kSgVec'] == k['kSgThreads'] * k['kSgGridCap'] + 1  # 16-byte kernel: one lane
    assert {k['kSgPrefetch'] - 1, k['kSgPrefetch'], k['kSgPrefetch'] + 1, 1, 2, 25} == set(C.T_SIZES)
    assert any(n % k['kSgVec'] for n in C.N_SIZES) and any(n % k['kSgVec'] == 0 for n in C.N_SIZES)
    # plain stores: no atomic read-modify-write, no LDS
    assert 'atomicAdd' not in text and '__hip_atomic' not in text and '__shared__' not in text


def test_the_lane_is_stated_once():
    """One file defines the six feed-forward entry points, each once, and the lane's arithmetic exists in one file under csrc/."""
    text = SOURCE.read_text()
    for name in ENTRY_POINTS:
        assert len(re.findall(rf'^int {name}\(', text, flags=re.M)) == 1, name
    sources = [p for p in sorted(SOURCE.parent.iterdir()) if p.suffix in ('.hip', '.h')]
    assert SOURCE in sources and len(sources) > 10
    for what, pattern in STATED_ONCE.items():
        holders = {p.name: len(re.findall(pattern, p.read_text())) for p in sources}
        holders = {name: n for name, n in holders.items() if n}
        assert holders == {'be_sg_lane.h': 1}, f'{what}: {holders}'


def test_abi_and_codes():
    from brainevent_amd import _abi, _neuron_sg
    assert {'be_lif_sg_forward', 'be_lif_sg_backward'} <= set(_abi.PROTOTYPES)
    assert len(_abi.PROTOTYPES['be_lif_sg_forward'][1]) == 13 and len(_abi.PROTOTYPES['be_lif_sg_backward'][1]) == 16
    codes = {n: int(v) for n, v in re.findall(r'#define (BE_LIF_\w+) (\d+)', HEADER.read_text())}
    assert {f'BE_LIF_RESET_{k.upper()}': v for k, v in _neuron_sg.RESETS.items()}.items() <= codes.items()
    assert {f'BE_LIF_SG_{k.upper()}': v for k, v in _neuron_sg.SURROGATES.items()}.items() <= codes.items()
    assert len(codes) == 5 and set(_neuron_sg.RESETS) == set(C.RESETS) and set(_neuron_sg.SURROGATES) == set(C.SURROGATES)


# ------------------------------------------------------------------------------------------------ refusals that need no device
def test_refusals_without_a_device(be, monkeypatch):
    from brainevent_amd import _neuron_sg

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron_sg, 'call', no_call)
    v, x = torch.zeros(4), torch.zeros(4)
    seq = torch.zeros(3, 4)
    for kw, match in ((dict(reset='none'), 'reset'), (dict(surrogate='relu'), 'surrogate'), (dict(alpha=0.0), 'alpha'),
                      (dict(alpha=-1.0), 'alpha'), (dict(alpha=float('nan')), 'alpha')):
        with pytest.raises(ValueError, match=match):
            be.lif_step(v, x, beta=0.9, **kw)
        with pytest.raises(ValueError, match=match):
            be.lif_sequence(seq, v, beta=0.9, **kw)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(TypeError, match='float32'):
            be.lif_step(bad, x, beta=0.9)
        with pytest.raises(TypeError, match='float32'):
            be.lif_step(v, bad, beta=0.9)
        with pytest.raises(TypeError, match='float32'):
            be.lif_sequence(seq, bad, beta=0.9)
    with pytest.raises(TypeError, match='float32'):
        be.lif_sequence(seq.double(), v, beta=0.9)
    with pytest.raises(TypeError, match='Tensor'):
        be.lif_step(v, np.zeros(4, F), beta=0.9)
    with pytest.raises(TypeError, match='Tensor'):
        be.lif_sequence([[0.0]], beta=0.9)
    with pytest.raises(ValueError, match='one shape'):
        be.lif_step(torch.zeros(5), x, beta=0.9)
    with pytest.raises(ValueError, match='one shape'):
        be.lif_step(torch.zeros(1, 4), x, beta=0.9)
    with pytest.raises(ValueError, match='shape of a step'):
        be.lif_sequence(seq, torch.zeros(3), beta=0.9)
    with pytest.raises(ValueError, match='shape of a step'):
        be.lif_sequence(seq, seq, beta=0.9)
    with pytest.raises(ValueError, match=r'\[T, \.\.\.\]'):
        be.lif_sequence(torch.zeros(()), beta=0.9)
    with pytest.raises(ValueError, match='device tensor'):          # CPU tensors: there is no CPU implementation
        be.lif_step(v, x, beta=0.9)
    with pytest.raises(ValueError, match='device tensor'):
        be.lif_sequence(seq, beta=0.9)
    with pytest.raises(TypeError):                                  # beta has no default
        be.lif_step(v, x)
