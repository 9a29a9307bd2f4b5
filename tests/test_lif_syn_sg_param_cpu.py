"""The synaptic / adaptive neuron with per-slot, learnable parameters without a device: the numpy restatement the GPU tests compare
with (tests/lif_syn_sg_param_cases.py) is held to torch's CPU autograd of the plain formula with the five parameters as leaves, to
the same derivative in f64, and — with one-element parameters — to tests/lif_syn_sg_cases.py bit for bit; plausible mistakes are
shown to fall outside the bound; the prototypes are held to the header; the Python refusals are raised with the device call barred.

Forward values must be equal.  ``g_x`` and the state gradients are compared within the propagated bound of
``lif_syn_sg_cases.backward`` (with the slot's own coefficients), a parameter's gradient within the sum of what its terms' factors
carry plus ``(n + 1) * 2**-23 * sum |terms|`` for its ``n = T * R`` terms (``lif_syn_sg_param_cases.param_bound``).

The tests of the restatement (against autograd, f64, the wrong versions, the float restatement, the spike rate) hold the numpy
reference the GPU file compares with, and pass whatever the library does; the tests of the source, the prototypes, the refusals and
the calls are the ones here that fail without the feature, as does every test of tests/test_lif_syn_sg_param_gpu.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lif_syn_sg_cases as S
import lif_syn_sg_param_cases as Q
from lif_syn_sg_param_cases import F

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron_sg.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'
DESIGN = ROOT / 'DESIGN.md'
n = 85                                          # neurons of a row; R rows make N = R * n slots
#: the seeds of the autograd comparison are SEED + 10 T + R.  They are chosen on the restatement alone, so that EVERY element's bound
#: stays under 1e-3 of the sum of its absolute terms: with T * R = 1 a per-neuron element is a single product (g_h * v_prev,
#: g_c * c_prev), and a g_h whose two terms (g_u and the pass-through g_vo) cancel to under a per cent carries a bound that is over a
#: thousandth of it — one such element in 85 turned up with the seeds 10 T + R (beta, soft / atan, T = R = 1: 7.2e-3), 100 + and 200 +.
SEED = 300


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
            k = torch.tensor(F(np.pi / 2 * p.alpha)) * u
            sg = torch.tensor(F(p.alpha / 2)) / (one + k * k)
        else:
            sg = alpha * torch.clamp_min(one - alpha * u.abs(), 0.0)
        gs = g * sg
        return gs, -gs, None


class FakeDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: lets the checks that come after ``is_cuda`` run without one."""

    @staticmethod
    def wrap(t):
        return t.as_subclass(FakeDevice)

    @property
    def is_cuda(self):
        return True


def plain(x, c0, v0, a0, q, p):
    """The plain formula in torch with the five parameters ``[P]`` leaves, slot ``i`` reading ``param[i % P]``."""
    N = x.shape[1]
    sd, beta, v_th, rho, kappa = (t.repeat(N // t.numel()) for t in q)
    v_reset = torch.tensor(F(p.v_reset))
    c, v, a, ss, vs = c0, v0, a0, [], []
    for t in range(x.shape[0]):
        c = sd * c + x[t]
        h = beta * v + c
        th = v_th + kappa * a if p.adaptive else v_th
        s = Spike.apply(h, th, p)
        sr = s.detach() if p.detach_reset else s
        v = h * (1 - sr) + v_reset * sr if p.reset == 'hard' else h - sr * v_th
        if p.adaptive:
            a = rho * a + s
        ss.append(s)
        vs.append(v)
    return torch.stack(ss), torch.stack(vs), c, v, a


def setting(T, R, per_neuron, seed, p):
    N = R * n
    x, state, grads = Q.inputs(T, N, seed)
    if not p.adaptive:
        state = (state[0], state[1], None)
    q = Q.param_inputs((n if per_neuron else 1,) * 5, seed)
    return N, x, state, S.pick(grads, Q.GRAD_SETS['all'], p), q


@pytest.mark.parametrize('T', (1, 2, 5))
@pytest.mark.parametrize('R', (1, 3))
@pytest.mark.parametrize('per_neuron', (False, True))
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', Q.MODES)
def test_restatement_against_cpu_autograd(reset, surrogate, detach, adaptive, per_neuron, R, T):
    p = S.mode_params(reset, surrogate, detach, adaptive)
    N, x, state, given, q = setting(T, R, per_neuron, SEED + 10 * T + R, p)
    P = q[0].size
    ref = Q.forward(x, *state, q, p)
    # the conditions on the inputs
    assert 0.05 <= ref.s_out.mean() <= 0.6
    assert not adaptive or all(np.count_nonzero(ref.a_save[t]) > 0 for t in range(1, T))
    k = 5 if adaptive else 3
    zero = torch.zeros(N)
    leaves = [torch.tensor(a, requires_grad=True) for a in (x,) + state[:3 if adaptive else 2]]
    params = [torch.tensor(a, requires_grad=True) for a in q]
    s, v_seq, c_last, v_last, a_last = plain(leaves[0], leaves[1], leaves[2], leaves[3] if adaptive else zero, params, p)
    for got, want in ((s, ref.s_out), (v_seq, ref.v_seq), (c_last, ref.c_last), (v_last, ref.v_last)):
        assert np.array_equal(got.detach().numpy(), want)
    assert not adaptive or np.array_equal(a_last.detach().numpy(), ref.a_last)
    outs = [o for o, g in zip((s, v_seq, c_last, v_last, a_last), given) if g is not None]
    got = torch.autograd.grad(outs, leaves + params[:k], [torch.tensor(g) for g in given if g is not None])
    got = [g.numpy() for g in got]
    r, info = Q.backward(ref.h_save, ref.c_save, ref.a_save, state[0], state[1], *given, q, p, with_bound=True)
    for name, g, want in zip(('g_x', 'g_c0', 'g_v0', 'g_a0'), got[:len(leaves)], r):
        err = np.abs(g.astype(np.float64) - want)
        assert (err <= info[name]).all(), name
    for name, g, slot in zip(Q.NAMES[:k], got[len(leaves):], r[4:]):
        bound, terms = Q.param_bound(info, name, P), np.abs(info[f'{name}_terms']).reshape(-1, P).sum(axis=0)
        err = np.abs(g.astype(np.float64) - Q.param_exact(info, name, P))
        print(f'{name}: max |autograd - ref| {err.max():.3e} (bound there {bound[err.argmax()]:.3e})')
        assert (err <= bound).all(), name
        # the restatement's own f32 sum, reduced exactly, is inside it too; and the bound is a rounding bound, not a tolerance
        assert (np.abs(Q.reduce_ref(slot, P).astype(np.float64) - Q.param_exact(info, name, P)) <= bound).all(), name
        assert terms.max() > 0 and (bound <= 1e-3 * terms).all(), name         # element by element
    assert info['g_x'].max() < 1e-3 * np.abs(r.g_x).max() and np.abs(r.g_x).max() > 1e-3


def f64_backward(f, c0, v0, given, q, p, variant=None):
    """The derivative in f64 in one possible order, from the f32 forward values: ``(g_x, g_c0, g_v0, g_a0, five [N] sums)``."""
    T, N = f.h_save.shape
    d = lambda a: None if a is None else np.asarray(a, np.float64)
    g_s, g_vseq, g_clast, g_vlast, g_alast = (d(a) for a in given)
    sd, beta, vth = (d(Q.expand(a, N)) for a in q[:3])
    rho, kap = (d(Q.expand(a, N)) for a in q[3:])
    z = np.zeros(N)
    cc, cv, ca = (z if a is None else a for a in (g_clast, g_vlast, g_alast))
    acc = {k: np.zeros(N) for k in Q.NAMES}
    g_x = np.zeros((T, N))

    def th32(t):                                 # the f32 threshold the forward pass compared with
        vt = Q.expand(q[2], N)
        return (vt + Q.expand(q[4], N) * f.a_save[t]).astype(F) if p.adaptive else vt

    for t in range(T - 1, -1, -1):
        h, th = d(f.h_save[t]), d(th32(t))
        a_in = d(f.a_save[t]) if p.adaptive else z
        s = h >= th
        sg = d(Q.surrogate((f.h_save[t] - th32(t)).astype(F), p))
        g_vo = cv + (0 if g_vseq is None else g_vseq[t])
        g_sp = (0 if g_s is None else g_s[t]) + (ca if p.adaptive else 0)
        if not p.detach_reset:
            g_sp = g_sp + (g_vo * (F(p.v_reset) - h) if p.reset == 'hard' else -g_vo * vth)
        g_u = g_sp * sg
        g_h = g_u + (np.where(s, 0.0, g_vo) if p.reset == 'hard' else g_vo)
        g_c = cc + g_h
        g_x[t] = g_c
        ca_in = ca
        cc, cv = sd * g_c, beta * g_h
        ca = rho * ca - kap * g_u
        if t > 0:
            v_prev = d(Q.membrane_after(f.h_save[t - 1], th32(t - 1), Q.expand(q[2], N), p))
            c_prev = d(f.c_save[t - 1])
        else:
            v_prev, c_prev = (z if a is None else d(a) for a in (v0, c0))
        acc['syn_decay'] += g_c * c_prev
        acc['beta'] += g_h * v_prev
        acc['v_th'] -= g_u + (np.where(s, g_vo, 0.0) if p.reset == 'soft' else 0.0)
        acc['kappa'] -= g_u * a_in
        acc['rho'] += ca_in * a_in
    return g_x, cc, cv, ca, acc


@pytest.mark.parametrize('reset', S.RESETS)
@pytest.mark.parametrize('detach', (False, True))
def test_the_comparison_can_fail(reset, detach):
    """Inside the bound: the same derivative in f64.  Outside it, each in the gradient it spoils: ``acc_rho`` with the outgoing carry,
    ``acc_kappa`` without the ``a_in`` factor, ``acc_sd`` with ``c[t]`` for ``c[t-1]``, ``v_prev`` decided with the base threshold,
    and (soft) a ``v_th`` gradient without the reset's direct term."""
    p = S.mode_params(reset, 'fast_sigmoid', detach, True)
    N, x, state, given, q = setting(5, 3, True, 5, p)
    f = Q.forward(x, *state, q, p)
    r, info = Q.backward(f.h_save, f.c_save, f.a_save, state[0], state[1], *given, q, p, with_bound=True)
    g64 = f64_backward(f, state[0], state[1], given, q, p)
    for name, got, want in zip(('g_x', 'g_c0', 'g_v0', 'g_a0'), g64[:4], r):
        assert (np.abs(got - want) <= info[name]).all(), name
    outside = {}
    for name in Q.NAMES:
        bound = Q.param_bound(info, name, n)
        assert (np.abs(g64[4][name].reshape(-1, n).sum(axis=0) - Q.param_exact(info, name, n)) <= bound).all(), name
    spoils = {'rho_outgoing_carry': 'rho', 'kappa_without_a': 'kappa', 'sd_with_c_t': 'syn_decay', 'v_prev_base_threshold': 'beta',
              'vth_without_direct': 'v_th'}
    assert set(spoils) == set(Q.WRONG)
    for variant, name in spoils.items():
        w = Q.backward(f.h_save, f.c_save, f.a_save, state[0], state[1], *given, q, p, variant=variant)
        slot = dict(zip(Q.NAMES, w[4:]))[name]
        err = np.abs(Q.reduce_ref(slot, n).astype(np.float64) - Q.param_exact(info, name, n))
        outside[variant] = bool((err > Q.param_bound(info, name, n)).any())
        # ... and what the mistake does not touch is unchanged
        assert all(Q.same_bits(a, b) for a, b in zip(w[:4], r[:4]))
    hard_only_same = outside.pop('vth_without_direct')
    assert hard_only_same == (reset == 'soft')          # the hard reset has no direct term to leave out
    assert all(outside.values()), outside


@pytest.mark.parametrize('reset,surrogate,detach,adaptive', Q.MODES)
def test_one_element_parameters_are_the_float_restatement(reset, surrogate, detach, adaptive):
    """Bit for bit in every shared output of both passes; ``th`` recomputed from ``a_save`` equals ``th_save``."""
    p = S.mode_params(reset, surrogate, detach, adaptive)
    q = Q.shared_params(p)
    for T in (1, 5):
        x, state, grads = S.inputs(T, 257, seed=T)
        state = state if adaptive else (state[0], state[1], None)
        f0, f1 = S.forward(x, *state, p), Q.forward(x, *state, q, p)
        shared = ('s_out', 'v_seq', 'h_save', 'c_last', 'v_last') + (('a_last',) if adaptive else ())
        assert all(Q.same_bits(getattr(f0, k), getattr(f1, k)) for k in shared)
        if adaptive:
            ka = q[4] * f1.a_save
            assert Q.same_bits((q[2] + ka).astype(F), f0.th_save)
        else:
            assert f0.th_save is None and f1.a_save is None
        for which, use in Q.GRAD_SETS.items():
            given = S.pick(grads, use, p)
            b0 = S.backward(f0.h_save, f0.th_save, *given, p)
            b1 = Q.backward(f1.h_save, f1.c_save, f1.a_save, state[0], state[1], *given, q, p)
            assert all(a is None or Q.same_bits(a, b) for a, b in zip(b0, b1[:4])), which


def test_spike_rate_and_trace_of_the_inputs():
    for mode in Q.MODES:
        p = S.mode_params(*mode)
        x, state, _ = Q.inputs(12, 4000, seed=0)
        f = Q.forward(x, state[0], state[1], state[2] if p.adaptive else None, Q.param_inputs((4000,) * 5, 0), p)
        assert 0.05 <= f.s_out.mean() <= 0.6, mode
        assert not p.adaptive or all(np.count_nonzero(f.a_save[t]) > 0 for t in range(1, 12))


# ------------------------------------------------------------------------------------------------ the source and the header
def test_the_source_holds_the_new_model_in_the_one_kernel_pair():
    text = SOURCE.read_text()
    assert 'using SynapticPerSlot = Model<true, ADAPT, true>;' in text and 'per-slot parameters exist for the plain neuron' not in text
    assert text.count('launch_forward<SynapticPerSlot<decltype(A)::value>>(') == 1
    assert text.count('launch_backward<SynapticPerSlot<decltype(A)::value>>(') == 1
    assert text.count('__global__') == 2 and text.count('V ring_c[M::PSYN ? kSgPrefetch : 1];') == 1
    for name in ('be_lif_syn_sg_forward_params', 'be_lif_syn_sg_backward_params'):
        assert len(re.findall(rf'^int {name}\(', text, flags=re.M)) == 1, name
    design = DESIGN.read_text()
    assert '### 2.24' in design and 'be_lif_syn_sg_backward_params' in design


def test_prototypes_against_the_header():
    from brainevent_amd import _abi
    counts = {'be_lif_syn_sg_forward_params': 28, 'be_lif_syn_sg_backward_params': 38}
    header = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    for name, count in counts.items():
        restype, argtypes = _abi.PROTOTYPES[name]
        args, = re.findall(rf'\b{name}\(([^)]*)\);', header)
        args = [a.strip() for a in args.split(',')]
        assert restype is ctypes.c_int and len(argtypes) == len(args) == count, name
        for a, ct in zip(args, argtypes):
            want = (ctypes.c_void_p if '*' in a or a.startswith('be_stream_t') else ctypes.c_int64 if a.startswith('int64_t')
                    else ctypes.c_double if a.startswith('double') else ctypes.c_int)
            assert ct is want, (name, a)
        periods = [a for a in args if a.endswith('_period')]
        assert periods == ['int64_t sd_period', 'int64_t beta_period', 'int64_t vth_period', 'int64_t rho_period', 'int64_t kappa_period']
    assert len(re.findall(r'#define (BE_LIF_\w+) (\d+)', HEADER.read_text())) == 5             # no new numeric code
    doc = HEADER.read_text()
    for line in ('c  = (sd_i * c) + x[t][i]', 'th = adaptive ? vth_i + (kappa_i * a_in) : vth_i', 'a_save[t][i] = a_in',
                 'th_prev = adaptive ? vth_i + (kappa_i * a_save[t-1][i]) : vth_i', 'acc_sd    = acc_sd    + (g_c * c_prev)',
                 'acc_beta  = acc_beta  + (g_h * v_prev)', 'acc_kappa = acc_kappa - (g_u * a_in)', 'acc_rho   = acc_rho   + (ca_in * a_in)'):
        assert line in doc, line


# ------------------------------------------------------------------------------------------------ Python, the device call barred
def test_refusals_without_a_device(be, monkeypatch):
    from brainevent_amd import _neuron_syn_sg

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron_syn_sg, 'call', no_call)
    monkeypatch.setattr(_neuron_syn_sg.A, 'stream_ptr', lambda: None)
    fake = FakeDevice.wrap
    x, seq = fake(torch.zeros(3, 4)), fake(torch.zeros(5, 3, 4))
    c, v, a = (fake(torch.zeros(3, 4)) for _ in range(3))
    per = lambda *shape: fake(torch.full(shape, 0.9))
    kw = dict(syn_decay=per(4), beta=0.9)

    def both(error, match, state=(c, v), **over):
        with pytest.raises(error, match=match):
            be.parametric_synaptic_lif_step(state, x, **{**kw, **over})
        with pytest.raises(error, match=match):
            be.parametric_synaptic_lif_sequence(seq, state, **{**kw, **over})

    for over, match in ((dict(reset='none'), 'reset'), (dict(surrogate='relu'), 'surrogate'), (dict(alpha=0.0), 'alpha'),
                        (dict(alpha=float('nan')), 'alpha')):
        both(ValueError, match, **over)
    # v_reset and alpha stay Python numbers; anything else that is no number or tensor is refused
    for name in ('v_reset', 'alpha'):
        both(TypeError, 'Python number', **{name: per(4)})
    for name in ('beta', 'v_th'):
        both(TypeError, 'Python number', **{name: 'x'})
    # a tensor parameter: f32, on the device, one element or the last dimensions of a step
    for name in ('syn_decay', 'beta', 'v_th'):
        for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
            both(TypeError, 'must be float32', **{name: fake(torch.ones(4, dtype=dtype))})
        both(ValueError, 'must be a device tensor', **{name: torch.ones(4)})
        for shape in ((3,), (5,), (4, 3), (1, 4), (1, 1), (5, 3, 4), (3, 4, 1)):
            both(ValueError, 'last dimensions of a step', **{name: per(*shape)})
    for k in (0, 1):
        pair = lambda value: tuple(value if j == k else 0.5 for j in (0, 1))
        both(TypeError, 'must be float32', state=(c, v, a), adapt=pair(fake(torch.ones(4, dtype=torch.float64))))
        both(ValueError, 'must be a device tensor', state=(c, v, a), adapt=pair(torch.ones(4)))
        both(ValueError, 'last dimensions of a step', state=(c, v, a), adapt=pair(per(3)))
        both(TypeError, 'Python number', state=(c, v, a), adapt=pair('x'))
    for bad, error in ((0.95, TypeError), ('ab', TypeError), ((0.95,), ValueError), ((0.95, 0.3, 0.1), ValueError)):
        both(error, 'adapt', state=(c, v, a), adapt=bad)
    # the state and x: as synaptic_lif_step
    both(ValueError, r'without adapt it is \(c, v\)', state=(c, v, a))
    both(ValueError, r'takes \(c, v, a\)', state=(c, v), adapt=(per(4), 0.3))
    both(TypeError, 'tuple', state=c)
    both(TypeError, 'float32', state=(c.to(torch.float64), v))
    both(ValueError, 'shape of a step', state=(c, fake(torch.zeros(4))))
    both(ValueError, 'device tensor', state=(torch.zeros(3, 4), v))
    with pytest.raises(ValueError, match='device tensor'):
        be.parametric_synaptic_lif_step((c, v), torch.zeros(3, 4), **kw)
    with pytest.raises(ValueError, match=r'\[T, \.\.\.\]'):
        be.parametric_synaptic_lif_sequence(fake(torch.zeros(())), **kw)
    with pytest.raises(TypeError):                                             # syn_decay and beta have no default
        be.parametric_synaptic_lif_step((c, v), x, beta=per(4))
    # the float functions and the recurrent layer still refuse a tensor, and say where to go
    with pytest.raises(TypeError, match='parametric_synaptic_lif_step'):
        be.synaptic_lif_step((c, v), x, **kw)
    with pytest.raises(TypeError):
        be.recurrent_lif_sequence(seq, None, syn_decay=per(4), beta=0.9)
    # ... and what is accepted passes every check: the first thing it reaches is the device call
    for params in (kw, dict(syn_decay=0.8, beta=per()), dict(syn_decay=per(1), beta=per(3, 4), v_th=per(4)),
                   dict(syn_decay=0.8, beta=0.9, adapt=(per(4), 0.3)), dict(syn_decay=0.8, beta=0.9, adapt=[0.9, per(3, 4)])):
        state = (c, v, a) if 'adapt' in params else (c, v)
        with pytest.raises(AssertionError, match='reached the device call'):
            be.parametric_synaptic_lif_step(state, x, **params)
        with pytest.raises(AssertionError, match='reached the device call'):
            be.parametric_synaptic_lif_sequence(seq, None, **params)


def test_the_calls(be, monkeypatch):
    """Spied on, not run: all numbers still reach be_lif_syn_sg_forward; one tensor sends all five to be_lif_syn_sg_forward_params
    with their periods, a number beside it as a one-element tensor."""
    from brainevent_amd import _neuron_syn_sg
    calls = []
    monkeypatch.setattr(_neuron_syn_sg, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(_neuron_syn_sg.A, 'stream_ptr', lambda: None)
    made = []
    real_as_param = _neuron_syn_sg._as_param

    def as_param(value, like):
        out = real_as_param(value, like)
        if out is not value:
            made.append(out)
        return out
    monkeypatch.setattr(_neuron_syn_sg, '_as_param', as_param)
    fake = FakeDevice.wrap
    x, seq, v = fake(torch.zeros(3, 4)), fake(torch.zeros(5, 3, 4)), fake(torch.zeros(3, 4))
    be.parametric_synaptic_lif_step((v, v), x, syn_decay=0.8, beta=0.9)
    be.parametric_synaptic_lif_sequence(seq, (None, v, v), syn_decay=0.5, beta=0.25, v_th=2, reset='soft', adapt=(0.75, 0.125), return_v=True)
    assert [name for name, _ in calls] == ['be_lif_syn_sg_forward', 'be_lif_syn_sg_forward'] and not made
    assert calls[1][1][11:21] == (5, 12, 0.5, 0.25, 2.0, 0.0, 0.75, 0.125, 1, 1)
    calls.clear()
    beta, kappa = fake(torch.full((4,), 0.9)), fake(torch.full((3, 4), 0.3))
    be.parametric_synaptic_lif_sequence(seq, (None, v, v), syn_decay=0.5, beta=beta, v_th=2, v_reset=-0.25, reset='soft',
                                        adapt=(0.75, kappa), return_v=True)
    (name, args), = calls
    assert name == 'be_lif_syn_sg_forward_params' and len(args) == 28
    assert [args[k] for k in (5, 7, 9, 11, 13)] == [1, 4, 1, 1, 12] and [(tuple(t.shape), float(t)) for t in made[:3]] == [((1,), 0.5), ((1,), 2.0), ((1,), 0.75)]
    assert args[6].value == beta.data_ptr() and args[12].value == kappa.data_ptr() and args[4].value == made[0].data_ptr()
    assert args[22:27] == (5, 12, -0.25, 1, 1)
    null = [i for i, a in enumerate(args[:22]) if getattr(a, 'value', 0) is None]
    assert null == [1, 16, 17, 18]                   # c0 None; nothing requires grad: no h_save, c_save, a_save
    calls.clear()
    be.parametric_synaptic_lif_step((v, v), x, syn_decay=beta, beta=0.9)
    (name, args), = calls
    assert name == 'be_lif_syn_sg_forward_params' and args[10].value is None and args[12].value is None and args[21].value is None
    assert args[22:27] == (1, 12, 0.0, 0, 0)
