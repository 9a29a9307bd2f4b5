"""The fused recurrent layer with per-neuron, learnable parameters without a device: the numpy restatement the GPU
tests compare with (tests/lif_rec_sg_param_cases.py) is held to torch's CPU autograd of the plain composition — ``s_prev @ W_dense``
plus the plain formula of the synaptic neuron with the five parameters as leaves — to tests/lif_rec_sg_cases.py with one-element
parameters and to tests/lif_syn_sg_param_cases.py with an empty matrix, bit for bit; planted mistakes must fall outside the bounds;
the prototypes are held to the header and ``_abi.py``; and the refusals that need no device are raised.

The weights of the comparison with autograd are multiples of 2**-6 (exact sums, forwards EQUAL).  The gradients of ``x``, the state,
``s0`` and the weights lie within §2.22's propagated bound; a parameter's gradient within §2.24's: what its terms' factors carry plus
``(n + 1) * 2**-23 * sum |terms|``."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lif_rec_sg_cases as R
import lif_rec_sg_param_cases as Q
import lif_syn_sg_cases as S
import lif_syn_sg_param_cases as P
from lif_rec_sg_param_cases import F
from test_lif_rec_sg_cpu import fake_csr
from test_lif_syn_sg_param_cpu import FakeDevice, Spike

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron_sg_rec.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'
DESIGN = ROOT / 'DESIGN.md'
EXP = 40                                     # the dyadic weights are exact from 6 on
B, N = 2, 97
#: the seeds of the autograd comparison are SEED + T.  They are chosen on the restatement alone so that the conditions the test
#: asserts hold in every mode: the spike rate, recurrent input and a trace at every step, and EVERY parameter-gradient element's bound
#: under 1e-3 of the sum of its absolute terms — a per-neuron element is the sum of T * B terms, and at T = 1 of the two samples'
#: alone, where one g_h whose two terms nearly cancel is enough to miss it.
SEED = 100


def plain(x, w, m, s0, c0, v0, a0, q, p):
    """The plain composition in torch with the five parameters leaves of 1 or N elements (broadcast over the samples)."""
    sd, beta, v_th, rho, kappa = q
    v_reset = torch.tensor(F(p.v_reset))
    rows, cols = torch.tensor(R.rows_of(m)), torch.tensor(m.indices.astype(np.int64))
    W = torch.zeros(m.n, m.n).index_put((rows, cols), w, accumulate=True)
    c, v, a, sp, ss, vs = c0, v0, a0, s0, [], []
    for t in range(x.shape[0]):
        xin = x[t] + sp @ W
        c = sd * c + xin
        h = beta * v + c
        th = v_th + kappa * a if p.adaptive else v_th.expand_as(h)
        s = Spike.apply(h, th, p)
        sr = s.detach() if p.detach_reset else s
        v = h * (1 - sr) + v_reset * sr if p.reset == 'hard' else h - sr * v_th
        if p.adaptive:
            a = rho * a + s
        ss.append(s)
        vs.append(v)
        sp = s
    return torch.stack(ss), torch.stack(vs), c, v, a


def case(T, per_neuron, seed):
    m = Q.dyadic_matrix(N, seed)
    x, s0, state, grads = Q.inputs(T, B, N, seed)
    q = Q.param_inputs((N if per_neuron else 1,) * 5, seed)
    return m, x, s0, state, grads, q


def check_inputs(ref, T, adaptive):
    """The conditions the inputs must meet."""
    assert 0.05 <= ref.s_out.mean() <= 0.6
    assert all(np.count_nonzero(ref.r[t]) > 0 for t in range(1, T))
    assert not adaptive or all(np.count_nonzero(ref.a_save[t]) > 0 for t in range(1, T))


@pytest.mark.parametrize('T', (1, 2, 5))
@pytest.mark.parametrize('per_neuron', (False, True))
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', Q.MODES)
def test_restatement_against_cpu_autograd(reset, surrogate, detach, adaptive, per_neuron, T):
    p = S.mode_params(reset, surrogate, detach, adaptive)
    m, x, s0, state, grads, q = case(T, per_neuron, SEED + T)
    period = q[0].size
    ref = Q.forward(x, m, s0, *state, q, p, EXP)
    check_inputs(ref, T, adaptive)
    k = 5 if adaptive else 3
    leaves = [torch.tensor(a, requires_grad=True) for a in (x, m.w, s0) + state]
    params = [torch.tensor(a, requires_grad=True) for a in q]
    s, v_seq, c_last, v_last, a_last = plain(leaves[0], leaves[1], m, *leaves[2:], params, p)
    for got, want in ((s, ref.s_out), (v_seq, ref.v_seq), (c_last, ref.c_last), (v_last, ref.v_last)):
        assert np.array_equal(got.detach().numpy(), want)
    assert not adaptive or np.array_equal(a_last.detach().numpy(), ref.a_last)
    n_in = 6 if adaptive else 5
    for which, use in Q.GRAD_SETS.items():
        if which == 'g_alast' and not adaptive:
            continue
        given = S.pick(grads, use, p)
        outs = [o for o, g in zip((s, v_seq, c_last, v_last, a_last), given) if g is not None]
        got = torch.autograd.grad(outs, leaves[:n_in] + params[:k], [torch.tensor(g) for g in given if g is not None],
                                  retain_graph=True, allow_unused=True)
        got = [np.zeros(l.shape, F) if g is None else g.numpy() for g, l in zip(got, leaves[:n_in] + params[:k])]
        r, info = Q.backward(ref.h_save, ref.c_save, ref.a_save, m, state[0], state[1], *given, q, p, with_bound=True)
        g_w, b_w = Q.weight_grad(m, ref.s_out, s0, r.g_x, info['g_x'])
        wants = [('g_x', r.g_x, info['g_x']), ('g_w', g_w, b_w), ('g_s0', r.g_s0, info['g_s0']), ('g_c0', r.g_c0, info['g_c0']),
                 ('g_v0', r.g_v0, info['g_v0']), ('g_a0', r.g_a0, info['g_a0'])]
        for g, (name, want, bound) in zip(got, wants[:n_in]):
            err = np.abs(g.astype(np.float64) - want)
            assert (err <= bound).all(), (which, name)
        for name, g, slot in zip(Q.NAMES[:k], got[n_in:], r[5:]):
            bound, terms = Q.param_bound(info, name, period), np.abs(info[f'{name}_terms']).reshape(-1, period).sum(axis=0)
            err = np.abs(g.astype(np.float64) - Q.param_exact(info, name, period))
            print(f'{which} {name}: max |autograd - ref| {err.max():.3e} (bound there {bound[err.argmax()]:.3e})')
            assert (err <= bound).all(), (which, name)
            # the restatement's own f32 accumulators, reduced exactly, are inside it too
            assert (np.abs(Q.reduce_ref(slot, period).astype(np.float64) - Q.param_exact(info, name, period)) <= bound).all(), name
            if which == 'all':                                  # a rounding bound, not a tolerance: element by element, so no
                assert terms.max() > 0 and (bound <= 1e-3 * terms).all(), name      # element is a single cancelling term
        if which == 'all':
            assert info['g_x'].max() < 1e-3 * np.abs(r.g_x).max() and np.abs(r.g_x).max() > 1e-3


@pytest.mark.parametrize('reset', S.RESETS)
def test_the_comparison_can_fail(reset):
    """Each planted mistake is outside the bound in the gradient it spoils."""
    p = S.mode_params(reset, 'fast_sigmoid', False, True)
    T = 5
    m, x, s0, state, grads, q = case(T, True, SEED + T)
    f = Q.forward(x, m, s0, *state, q, p, EXP)
    r, info = Q.backward(f.h_save, f.c_save, f.a_save, m, state[0], state[1], *grads, q, p, with_bound=True)
    spoils = {'no_recurrent_term': 'g_x', 'v_prev_from_step_t': 'beta', 'vth_without_direct': 'v_th', 'rho_outgoing_carry': 'rho',
              'neighbour_parameters': 'g_x'}
    assert set(spoils) == set(Q.WRONG)
    outside = {}
    for variant, name in spoils.items():
        w = Q.backward(f.h_save, f.c_save, f.a_save, m, state[0], state[1], *grads, q, p, variant=variant)
        if name == 'g_x':
            outside[variant] = bool((np.abs(w.g_x.astype(np.float64) - r.g_x) > info['g_x']).any())
        else:
            slot = dict(zip(Q.NAMES, w[5:]))[name]
            err = np.abs(Q.reduce_ref(slot, N).astype(np.float64) - Q.param_exact(info, name, N))
            outside[variant] = bool((err > Q.param_bound(info, name, N)).any())
            assert all(Q.same_bits(a, b) for a, b in zip(w[:5], r[:5]))         # what the mistake does not touch is unchanged
    direct = outside.pop('vth_without_direct')
    assert direct == (reset == 'soft')                   # the hard reset has no direct term to leave out
    assert all(outside.values()), outside


@pytest.mark.parametrize('reset,surrogate,detach,adaptive', Q.MODES)
def test_one_element_parameters_are_the_float_restatement(reset, surrogate, detach, adaptive):
    """Bit for bit in every shared output of both passes; ``th`` recomputed from ``a_save`` equals ``th_save``."""
    p = S.mode_params(reset, surrogate, detach, adaptive)
    q = Q.shared_params(p)
    for T in (1, 4):
        m = Q.random_matrix(65, seed=T)
        e = Q.exponent(m)
        x, s0, state, grads = Q.inputs(T, 3, 65, seed=T)
        f0, f1 = R.forward(x, m, s0, *state, p, e), Q.forward(x, m, s0, *state, q, p, e)
        shared = ('s_out', 'v_seq', 'h_save', 'c_last', 'v_last', 'r') + (('a_last',) if adaptive else ())
        assert all(Q.same_bits(getattr(f0, k), getattr(f1, k)) for k in shared)
        if adaptive:
            assert Q.same_bits(Q.thresholds(f1.a_save, q, p), f0.th_save)
        else:
            assert f0.th_save is None and f1.a_save is None
        for which, use in Q.GRAD_SETS.items():
            given = S.pick(grads, use, p)
            b0 = R.backward(f0.h_save, f0.th_save, m, *given, p)
            b1 = Q.backward(f1.h_save, f1.c_save, f1.a_save, m, state[0], state[1], *given, q, p)
            assert all(a is None or Q.same_bits(a, b) for a, b in zip(b0, b1[:5])), which


@pytest.mark.parametrize('adaptive', (False, True))
@pytest.mark.parametrize('pattern', Q.PATTERNS)
def test_an_empty_matrix_is_the_feed_forward_neuron(pattern, adaptive):
    """nse = 0: both passes are tests/lif_syn_sg_param_cases.py's over B * N slots, the accumulators included."""
    p = S.mode_params('soft', 'atan', False, adaptive)
    T, B, N = 4, 3, 65
    x, s0, state, grads = Q.inputs(T, B, N, seed=2)
    q = Q.param_inputs(Q.periods(pattern, N), seed=2)
    m = Q.empty_matrix(N)
    f = Q.forward(x, m, s0, *state, q, p, 0)
    flat = lambda a: None if a is None else a.reshape(a.shape[:a.ndim - 2] + (B * N,))
    st = tuple(flat(a) for a in state[:3 if adaptive else 2]) + (() if adaptive else (None,))
    f0 = P.forward(flat(x), *st, q, p)
    assert not f.r.any() and not np.signbit(f.r).any()
    for a, b in zip(f[:8], f0):
        assert (a is None and b is None) or Q.same_bits(flat(a), b)
    r = Q.backward(f.h_save, f.c_save, f.a_save, m, state[0], state[1], *grads, q, p)
    r0 = P.backward(f0.h_save, f0.c_save, f0.a_save, st[0], st[1], *(flat(g) for g in grads), q, p)
    for a, b in zip(r[:4] + r[5:], r0):
        assert (a is None and b is None) or Q.same_bits(flat(a), b)
    assert not r.g_s0.any()


def test_one_entry_rows_and_the_patterns():
    m = Q.one_entry_matrix(65, seed=1)
    assert (np.diff(m.indptr) == 1).all()
    assert len(set(Q.PATTERNS)) == 5 and all(len(k) == 5 and set(k) <= {'1', 'N'} for k in Q.PATTERNS)
    assert Q.periods('N1N1N', 7) == (7, 1, 7, 1, 7)
    assert Q.N_SIZES == (1, 63, 64, 65, 257, 1025) and Q.B_SIZES == (1, 3) and Q.T_SIZES == (1, 2, 3, 5)


# ------------------------------------------------------------------------------------------------ the header, the table, the source
def test_prototypes_against_the_header():
    from brainevent_amd import _abi
    counts = {'be_lif_rec_sg_forward_params': 34, 'be_lif_rec_sg_backward_params': 43}
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
    names = lambda name: [a.split()[-1].lstrip('*') for a in re.findall(rf'\b{name}\(([^)]*)\);', header)[0].split(',')]
    five = ['syn_decay', 'sd_period', 'beta', 'beta_period', 'v_th', 'vth_period', 'rho', 'rho_period', 'kappa', 'kappa_period']
    slots = ['g_sd_slot', 'g_beta_slot', 'g_vth_slot', 'g_rho_slot', 'g_kappa_slot']
    # §2.24's argument lists with §2.22's additions: the matrix and s0, B, scale_exp, g_s0
    syn_f, rec_f = names('be_lif_syn_sg_forward_params'), names('be_lif_rec_sg_forward_params')
    assert syn_f[4:14] == five
    assert rec_f == ['x', 'w', 'indices', 'indptr', 's0'] + syn_f[1:23] + ['B'] + syn_f[23:27] + ['scale_exp', 'stream']
    syn_b, rec_b = names('be_lif_syn_sg_backward_params'), names('be_lif_rec_sg_backward_params')
    assert syn_b[10:20] == five and syn_b[24:29] == slots
    assert rec_b == syn_b[:5] + ['w', 'indices', 'indptr'] + syn_b[5:24] + ['g_s0'] + slots + ['T', 'B'] + syn_b[30:]
    assert len(re.findall(r'#define (BE_LIF_\w+) (\d+)', HEADER.read_text())) == 5            # no new numeric code
    doc = HEADER.read_text()
    for line in ('param[period == 1 ? 0 : i]', 'acc_sd    = acc_sd    + (g_c * c_prev)', 'acc_rho   = acc_rho   + (ca_in * a_in)',
                 'a period that is neither 1 nor N'):
        assert line in doc, line


def test_the_source_holds_the_new_model_in_the_one_kernel_pair():
    text = SOURCE.read_text()
    assert text.count('__global__') == 2 and text.count('template <bool HARD, bool ADAPT, bool PARAMS>') == 1
    assert text.count('template <bool HARD, int SG, bool ADAPT, bool PARAMS>') == 1
    assert text.count('be_allow_lds(') == 2 and text.count('hipLaunchKernelGGL(') == 2          # one launch site per direction
    assert 'be_lif_rec_sg_forward_params' in text and 'be_lif_rec_sg_backward_params' in text
    design = DESIGN.read_text()
    assert '### 2.25' in design and 'be_lif_rec_sg_forward_params' in design and '358 exported symbols' in design


# ------------------------------------------------------------------------------------------------ refusals that need no device
def test_refusals_without_a_device(be, monkeypatch):
    from brainevent_amd import _neuron_rec_sg

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron_rec_sg, 'call', no_call)
    monkeypatch.setattr(_neuron_rec_sg.A, 'stream_ptr', lambda: None)
    fake = FakeDevice.wrap
    B, N = 3, 4
    x = fake(torch.zeros(5, B, N))
    c, v, a, s0 = (fake(torch.zeros(B, N)) for _ in range(4))
    rec = fake_csr(be, N)
    per = lambda value=0.9, n=N: fake(torch.full((n,), value))
    kw = dict(syn_decay=0.8, beta=per(), scale_exp=20)
    run = be.parametric_recurrent_lif_sequence

    def refused(error, match, x=x, rec=rec, state=(c, v), s0=s0, **over):
        with pytest.raises(error, match=match):
            run(x, rec, state, s0, **{**kw, **over})

    # the parameters: [B, N] is refused with the reason, as is any other shape, dtype or a CPU tensor
    for name in ('syn_decay', 'beta', 'v_th'):
        refused(ValueError, 'same neurons in every sample', **{name: fake(torch.full((B, N), 0.9))})
        refused(ValueError, 'same neurons in every sample', **{name: fake(torch.full((1, N), 0.9))})
        refused(ValueError, 'one element or the shape', **{name: per(n=N + 1)})
        refused(ValueError, 'one element or the shape', **{name: per(n=B)})
        refused(TypeError, 'must be float32', **{name: per().to(torch.float64)})
        refused(TypeError, 'must be float32', **{name: per().to(torch.float16)})
        refused(ValueError, 'must be a device tensor', **{name: torch.full((N,), 0.9)})
        refused(TypeError, 'Python number', **{name: 'x'})
    for k in (0, 1):
        pair = lambda t: (t, 0.3) if k == 0 else (0.95, t)
        refused(ValueError, 'same neurons in every sample', state=(c, v, a), adapt=pair(fake(torch.full((B, N), 0.9))))
        refused(ValueError, 'one element or the shape', state=(c, v, a), adapt=pair(per(n=N + 1)))
        refused(TypeError, 'must be float32', state=(c, v, a), adapt=pair(per().to(torch.float64)))
        refused(ValueError, 'must be a device tensor', state=(c, v, a), adapt=pair(torch.full((N,), 0.9)))
    for name in ('v_reset', 'alpha'):                                          # these two stay numbers
        refused(TypeError, 'syn_decay, beta, v_th, rho and kappa may be tensors', **{name: per()})
    # everything recurrent_lif_sequence refuses
    for bad in (None, torch.zeros(N, N), object.__new__(be.CSC), object.__new__(be.PlannedMatrix)):
        refused(TypeError, 'rec must be a CSR', rec=bad)
    refused(ValueError, 'square', rec=fake_csr(be, N, shape=(N, N + 1)))
    refused(ValueError, "size of x's last axis", rec=fake_csr(be, N + 1))
    refused(TypeError, 'weights of rec must be float32', rec=fake_csr(be, N, dtype=torch.float64))
    refused(ValueError, 'one shared weight is not built', rec=fake_csr(be, N, data=torch.zeros(1)))
    refused(TypeError, 'indptr of rec must be int32', rec=fake_csr(be, N, indptr_dtype=torch.int64))
    big = _neuron_rec_sg.MAX_N + 1
    refused(ValueError, 'the limit is 8192', x=fake(torch.zeros(1, 1, big)), rec=fake_csr(be, big, nse=0), state=None, s0=None,
            beta=per(n=big))
    for bad in (fake(torch.zeros(N)), fake(torch.zeros(2, 2, B, N)), fake(torch.zeros(()))):
        refused(ValueError, r'\[T, B, N\] or \[T, N\]', x=bad, state=None, s0=None)
    refused(ValueError, 'shape of a step', s0=fake(torch.zeros(N)))
    refused(ValueError, 'shape of a step', state=(c, fake(torch.zeros(N))))
    for dtype in (torch.float64, torch.float16, torch.bool):
        refused(TypeError, 'float32', s0=s0.to(dtype))
        refused(TypeError, 'float32', x=x.to(dtype))
        refused(TypeError, 'float32', state=(c.to(dtype), v))
    for bad in (20.0, '20', True):
        refused(TypeError, 'scale_exp must be None or an int', scale_exp=bad)
    for bad in (-91, 151):
        refused(ValueError, 'scale_exp', scale_exp=bad)
    for over, match in ((dict(reset='none'), 'reset'), (dict(surrogate='relu'), 'surrogate'), (dict(alpha=0.0), 'alpha')):
        refused(ValueError, match, **over)
    for bad, error in ((0.95, TypeError), ((0.95,), ValueError)):
        refused(error, 'adapt', state=(c, v, a), adapt=bad)
    refused(ValueError, r'without adapt it is \(c, v\)', state=(c, v, a))
    refused(ValueError, r'takes \(c, v, a\)', adapt=(0.95, 0.3))
    refused(ValueError, 'device tensor', x=torch.zeros(5, B, N))
    refused(ValueError, 'device tensor', s0=torch.zeros(B, N))
    # recurrent_lif_sequence itself still takes numbers only, with the words the earlier tests pin
    with pytest.raises(TypeError, match='learnable parameters exist for lif_step only'):
        be.recurrent_lif_sequence(x, rec, syn_decay=0.8, beta=per(), scale_exp=20)
    # ... and what is accepted passes every check: the first thing it reaches is the device call
    zero_d = fake(torch.tensor(0.9))
    for args, k in (((x, rec), kw), ((x, rec, None, s0), dict(kw, adapt=(per(0.95), 0.3))), ((x, rec, (None, v)), dict(kw, v_th=zero_d)),
                    ((x, rec, [c, None, a], s0), dict(kw, beta=0.9, adapt=(0.95, fake(torch.full((1,), 0.3))))),
                    ((fake(torch.zeros(5, N)), rec, (fake(torch.zeros(N)), None)), dict(beta=per(), scale_exp=-90)),
                    ((x, fake_csr(be, N, nse=0)), dict(beta=zero_d))):
        with pytest.raises(AssertionError, match='reached the device call'):
            run(*args, **k)


def test_the_calls(be, monkeypatch):
    """Spied on, not run: all numbers reach ``be_lif_rec_sg_forward``; a tensor reaches ``be_lif_rec_sg_forward_params`` with the five
    pointers and periods, numbers beside it as one-element tensors."""
    from brainevent_amd import _neuron_rec_sg
    calls = []
    monkeypatch.setattr(_neuron_rec_sg, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(_neuron_rec_sg.A, 'stream_ptr', lambda: None)
    made = []
    real_full = torch.full
    monkeypatch.setattr(torch, 'full', lambda *a, **k: made.append(real_full(*a, **{**k, 'device': None})) or made[-1])
    fake = FakeDevice.wrap
    B, N = 3, 4
    x, s0 = fake(torch.zeros(5, B, N)), fake(torch.zeros(B, N))
    rec = fake_csr(be, N)
    be.parametric_recurrent_lif_sequence(x, rec, syn_decay=0.5, beta=0.25, v_th=2, reset='soft', adapt=(0.75, 0.125), scale_exp=-3)
    assert [n for n, _ in calls] == ['be_lif_rec_sg_forward'] and not made
    assert calls[0][1][15:27] == (5, B, N, 0.5, 0.25, 2.0, 0.0, 0.75, 0.125, 1, 1, -3)
    calls.clear()
    beta, kappa = fake(torch.full((N,), 0.9)), fake(torch.tensor(0.3))
    made.clear()
    s, v_seq, last = be.parametric_recurrent_lif_sequence(x, rec, None, s0, syn_decay=0.5, beta=beta, adapt=(0.75, kappa), v_reset=-0.25,
                                                          return_v=True, scale_exp=7)
    assert s.shape == v_seq.shape == (5, B, N) and len(last) == 3 and all(t.shape == (B, N) for t in last)
    (name, a), = calls
    assert name == 'be_lif_rec_sg_forward_params' and len(a) == 34
    assert [float(t) for t in made] == [0.5, 1.0, 0.75] and all(t.shape == (1,) and t.dtype == torch.float32 for t in made)
    assert [a[k] for k in (9, 11, 13, 15, 17)] == [1, N, 1, 1, 1]
    assert a[10].value == beta.data_ptr() and a[16].value == kappa.data_ptr() and a[8].value == made[0].data_ptr()
    assert a[26:33] == (5, B, N, -0.25, 0, 1, 7)
    # no state, nothing requires grad: c0, v0, a0, h_save, c_save, a_save are NULL; s0 and v_seq are given
    assert [i for i, t in enumerate(a[:26]) if hasattr(t, 'value') and t.value is None] == [5, 6, 7, 20, 21, 22]
