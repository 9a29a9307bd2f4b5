"""The fused recurrent spiking layer without a device: the numpy restatement the GPU tests compare with
(tests/lif_rec_sg_cases.py) is held to torch's CPU autograd of the plain composition — ``s_prev @ W_dense`` plus the plain formula
of the synaptic neuron — and, with an empty matrix, to the restatement of the feed-forward neuron (tests/lif_syn_sg_cases.py);
the constants the GPU sizes come from are held to the text of csrc/be_neuron_sg_rec.hip, the prototypes to the header, and the
refusals that need no device are raised.

The weights of the comparison with autograd are multiples of 2**-6: their sums are exact in f32 in any order and in fixed point at
the chosen exponent, so forward values must be EQUAL.  Gradients — of ``x``, the state, ``s0`` and the weights — are compared
within the propagated bound of ``lif_rec_sg_cases.backward(with_bound=True)`` / ``weight_grad``."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lif_rec_sg_cases as C
import lif_syn_sg_cases as S
from lif_rec_sg_cases import F
from test_lif_syn_sg_cpu import FakeDevice, Spike

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron_sg_rec.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'
DESIGN = ROOT / 'DESIGN.md'
EXP = 40                                     # the dyadic weights are exact from 6 on; 2**40 * (a column's |w|) stays far below 2**62


def plain(x, w, m, s0, c0, v0, a0, p):
    """The plain composition in torch: ``(s [T, B, N], v_seq, c_last, v_last, a_last)``; ``w`` holds one weight per stored entry."""
    syn_decay, beta, v_th, v_reset, rho, kappa = (torch.tensor(F(k)) for k in (p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa))
    rows, cols = torch.tensor(C.rows_of(m)), torch.tensor(m.indices.astype(np.int64))
    W = torch.zeros(m.n, m.n).index_put((rows, cols), w, accumulate=True)
    c, v, a, sp, ss, vs = c0, v0, a0, s0, [], []
    for t in range(x.shape[0]):
        xin = x[t] + sp @ W
        c = syn_decay * c + xin
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


def case(T, B, N, seed):
    m = C.dyadic_matrix(N, seed)
    assert ((m.w * 64) == np.round(m.w * 64)).all() and np.abs(m.w).max() <= 1
    return (m,) + C.inputs(T, B, N, seed)


@pytest.mark.parametrize('T', (1, 2, 5))
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', C.MODES)
def test_restatement_against_cpu_autograd(reset, surrogate, detach, adaptive, T):
    p = S.mode_params(reset, surrogate, detach, adaptive)
    B, N = 2, 97
    m, x, s0, state, grads = case(T, B, N, seed=T)
    ref = C.forward(x, m, s0, *state, p, EXP)
    # the inputs are doing something: a plausible rate, and recurrent input at every step (step 0: from s0)
    assert 0.05 < ref.s_out.mean() < 0.6
    assert all(np.count_nonzero(ref.r[t]) > 0 for t in range(T))
    leaves = [torch.tensor(a, requires_grad=True) for a in (x, m.w, s0) + state]
    s, v_seq, c_last, v_last, a_last = plain(leaves[0], leaves[1], m, *leaves[2:], p)
    for got, want in ((s, ref.s_out), (v_seq, ref.v_seq), (c_last, ref.c_last), (v_last, ref.v_last)):
        assert np.array_equal(got.detach().numpy(), want)
    if adaptive:
        assert np.array_equal(a_last.detach().numpy(), ref.a_last)
    else:
        assert ref.th_save is None and ref.a_last is None
    n_in = 6 if adaptive else 5
    for which, use in S.GRAD_SETS.items():
        if which == 'g_alast' and not adaptive:
            continue
        given = S.pick(grads, use, p)
        outs = [o for o, g in zip((s, v_seq, c_last, v_last, a_last), given) if g is not None]
        got = torch.autograd.grad(outs, leaves[:n_in], [torch.tensor(g) for g in given if g is not None], retain_graph=True,
                                  allow_unused=True)
        got = [np.zeros(l.shape, F) if g is None else g.numpy() for g, l in zip(got, leaves)]
        r, b = C.backward(ref.h_save, ref.th_save, m, *given, p, with_bound=True)
        g_w, b_w = C.weight_grad(m, ref.s_out, s0, r.g_x, b.g_x)
        wants = [('g_x', r.g_x, b.g_x), ('g_w', g_w, b_w), ('g_s0', r.g_s0, b.g_s0), ('g_c0', r.g_c0, b.g_c0), ('g_v0', r.g_v0, b.g_v0),
                 ('g_a0', r.g_a0, b.g_a0)]
        for g, (name, want, bound) in zip(got, wants):
            err = np.abs(g.astype(np.float64) - want)
            print(f'{which} {name}: max |autograd - ref| {err.max():.3e} (bound there {bound.flat[err.argmax()]:.3e})')
            assert (err <= bound).all(), (which, name)
        assert np.abs(r.g_x).max() > 1e-3
        assert b.g_x.max() < 1e-3 * b.terms.max()                      # the bound is a rounding bound, not a tolerance
        assert np.abs(g_w).max() > 1e-3 and b_w.max() < 1e-3 * np.abs(g_w).max()


def test_the_comparison_can_fail():
    """Outside the bound: a backward pass without the recurrent term, one whose gather uses weights off by a part in a thousand,
    and a weight gradient that starts one step late."""
    p = S.Params(adaptive=True)
    T, B, N = 5, 2, 97
    m, x, s0, state, grads = case(T, B, N, seed=5)
    ref = C.forward(x, m, s0, *state, p, EXP)
    r, b = C.backward(ref.h_save, ref.th_save, m, *grads, p, with_bound=True)
    outside = lambda got: any((np.abs(g.astype(np.float64) - want) > bound).any() for g, want, bound in zip(got, r, b))
    assert not outside(r)
    assert outside(C.backward(ref.h_save, ref.th_save, C.empty_matrix(N), *grads, p))
    off = C.Matrix((m.w * F(1.001)).astype(F), m.indices, m.indptr, m.n)
    assert outside(C.backward(ref.h_save, ref.th_save, off, *grads, p))
    g_w, b_w = C.weight_grad(m, ref.s_out, s0, r.g_x, b.g_x)
    late = C.weight_grad(m, ref.s_out, None, r.g_x)
    assert (np.abs(late.astype(np.float64) - g_w) > b_w).any()


@pytest.mark.parametrize('adaptive', (False, True))
def test_an_empty_matrix_is_the_feed_forward_neuron(adaptive):
    """nse = 0: r = +0 at every step and g_rec = +0, so both passes are tests/lif_syn_sg_cases.py's over B * N slots (the inputs
    hold no negative zero, which x + 0 would turn into a positive one)."""
    p = S.Params(adaptive=adaptive, reset='soft', surrogate='atan')
    T, B, N = 4, 3, 65
    x, s0, state, grads = C.inputs(T, B, N, seed=2)
    m = C.empty_matrix(N)
    f = C.forward(x, m, s0, *state, p, 0)
    flat = lambda a: None if a is None else a.reshape(a.shape[:a.ndim - 2] + (B * N,))
    f0 = S.forward(flat(x), *(flat(a) for a in state[:3 if adaptive else 2]), *((None,) * (0 if adaptive else 1)), p)
    assert not f.r.any() and not np.signbit(f.r).any()
    for a, b in zip(f[:7], f0):
        assert (a is None and b is None) or C.same_bits(flat(a), b)
    r = C.backward(f.h_save, f.th_save, m, *grads, p)
    r0 = S.backward(f0.h_save, f0.th_save, *(flat(g) for g in grads), p)
    for a, b in zip(r[:4], r0):
        assert (a is None and b is None) or C.same_bits(flat(a), b)
    assert not r.g_s0.any() and C.weight_grad(m, f.s_out, s0, r.g_x).size == 0


def test_restatement_edges():
    """The fixed-point encoding; duplicates, self-loops and the long row of the crafted matrix; a NaN stays in its sample."""
    w = np.array([0.0, 1.0, -1.0, 0.5, -0.015625, 3.0 * 2.0 ** -20], F)
    assert C.fixed_from_f32(w, 20).tolist() == [0, 1 << 20, -(1 << 20), 1 << 19, -(1 << 14), 3]
    assert C.fixed_from_f32(w[:5], 40).tolist() == [0, 1 << 40, -(1 << 40), 1 << 39, -(1 << 34)]
    m = C.crafted_matrix()
    n = np.diff(m.indptr)
    assert n[0] == 0 and n[3] == 600 > m.n == 300 and (n[4::4] == 0).all() and m.indices[m.indptr[1]] == 1
    assert m.indices[m.indptr[2]:m.indptr[3]].tolist() == [7, 7, 2, 7, 7, 7]
    e = C.exponent(m)
    active = np.zeros(m.n, bool)
    active[2] = True
    r = C.recurrent_input(m, C.fixed_from_f32(m.w, e), active, e)
    row = m.w[m.indptr[2]:m.indptr[3]].astype(np.float64)
    assert np.count_nonzero(r) == 2 and abs(r[7] - (row.sum() - row[2])) < 1e-7 and abs(r[2] - row[2]) < 1e-8
    # every row active: the restatement is the dense product to f32 accuracy (and the exponent's worst case does not wrap)
    r = C.recurrent_input(m, C.fixed_from_f32(m.w, e), np.ones(m.n, bool), e)
    assert np.abs(r - C.dense(m).sum(axis=0)).max() < 1e-6
    x, s0, state, grads = C.inputs(3, 2, m.n, seed=1)
    p = S.Params(adaptive=True)
    clean = C.forward(x, m, s0, *state, p, e)
    x = x.copy()
    x[1, 0, 4] = np.nan
    f = C.forward(x, m, s0, *state, p, e)
    assert all(C.same_bits(a[..., 1, :], b[..., 1, :]) for a, b in zip(f[:7], clean[:7]))
    assert np.isnan(f.v_seq[1:, 0, 4]).all() and np.isnan(f.h_save[:, 1]).sum() == 0


# ------------------------------------------------------------------------------------------------ the constants and the source
PATTERNS = {
    'kRecThreads': r'constexpr int kRecThreads = (\d+);',
    'kRecMaxN': r'constexpr int kRecMaxN = (\d+);',
    'kRecRowLanes': r'constexpr int kRecRowLanes = (\d+);',
    'kRecUnroll': r'constexpr int kRecUnroll = (\d+);',
}

SOURCE_TEXT = [
    ('constexpr int kRecPerThread = kRecMaxN / kRecThreads;', 1),
    ('__launch_bounds__(kRecThreads)', 2),
    ('#pragma clang fp contract(off)', 3),
    ('if (N > kRecMaxN || B > 0x7fffffffll) {', 1),
    ('const int lds = (int)be_align_up(N * 12, 16);', 1),
    ('const int lds = (int)be_align_up(N * 8, 16);', 1),
    ('if (col[q] >= 0) atomicAdd(&acc[col[q]], fixed_from_f32(wk[q], scale));', 1),
    ('k += kRecUnroll * kRecRowLanes) {', 2),
    ('dim3((unsigned)B), dim3(kRecThreads), lds, st,', 2),
]


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    found = re.findall(PATTERNS[key], SOURCE.read_text())
    assert len(found) == 1 and int(found[0]) == C.CONSTS[key], (f'{key}: be_neuron_sg_rec.hip says {found}, '
                                                               f'tests/lif_rec_sg_cases.py assumes {C.CONSTS[key]}')


def test_sizes_follow_the_constants():
    from brainevent_amd import _neuron_rec_sg
    text = SOURCE.read_text()
    for line, times in SOURCE_TEXT:
        assert text.count(line) == times, f'be_neuron_sg_rec.hip holds {line!r} {text.count(line)} times, not {times}'
    k = C.CONSTS
    assert _neuron_rec_sg.MAX_N == k['kRecMaxN'] and k['kRecMaxN'] % k['kRecThreads'] == 0
    # 8 B of sums and 4 B of ids per neuron: 96 KB of the 160 KB at the limit
    assert k['kRecMaxN'] * 12 == 96 * 1024
    # the sizes: below, at and past a wave; past a quarter of the workgroup; one neuron past it (a second neuron per thread)
    assert {1, 63, 64, 65} <= set(C.N_SIZES) and k['kRecThreads'] + 1 in C.N_SIZES and max(C.N_SIZES) < k['kRecMaxN']
    # the crafted matrix's long row is longer than the workgroup's row lanes can take in one trip, and than N
    m = C.crafted_matrix()
    assert np.diff(m.indptr).max() == 600 > k['kRecRowLanes'] and m.n == 300
    trip = k['kRecUnroll'] * k['kRecRowLanes']
    assert np.diff(m.indptr)[5:7].tolist() == [trip + 1, trip] and 600 > 2 * trip
    # no float atomics, no global atomics: the one read-modify-write is the LDS integer add
    assert text.count('atomicAdd') == 1 and '__hip_atomic' not in text and 'atomicAdd(&acc[' in text
    assert 'unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem_raw);' in text
    # DESIGN.md §2.22 names the limit and the entry points
    design = DESIGN.read_text()
    assert '### 2.22' in design and 'kRecMaxN = 8192' in design and 'be_lif_rec_sg_forward' in design


def test_prototypes_against_the_header():
    from brainevent_amd import _abi, _neuron_rec_sg, _neuron_syn_sg
    counts = {'be_lif_rec_sg_forward': 28, 'be_lif_rec_sg_backward': 30}
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
    # §2.21's order: after x come w, indices, indptr, s0; B and N in place of N; scale_exp; backwards g_s0
    syn_f, rec_f = names('be_lif_syn_sg_forward'), names('be_lif_rec_sg_forward')
    assert rec_f == ['x', 'w', 'indices', 'indptr', 's0'] + syn_f[1:12] + ['B'] + syn_f[12:21] + ['scale_exp', 'stream']
    syn_b, rec_b = names('be_lif_syn_sg_backward'), names('be_lif_rec_sg_backward')
    assert rec_b == syn_b[:2] + ['w', 'indices', 'indptr'] + syn_b[2:11] + ['g_s0', 'T', 'B'] + syn_b[12:]
    assert len(re.findall(r'#define (BE_LIF_\w+) (\d+)', HEADER.read_text())) == 5            # no new numeric code
    assert _neuron_rec_sg._Params is _neuron_syn_sg._Params
    doc = HEADER.read_text()
    for line in ('r[j] = (float)((double)(int64)R[j] * inv)', 'xin  = x[t][b][j] + r[j]', 'if t < T-1: g_sp = g_sp + g_rec',
                 'g_s0[b][i] = sum over row i of w[k] * g_x[0][b][indices[k]]'):
        assert line in doc, line


# ------------------------------------------------------------------------------------------------ refusals that need no device
def fake_csr(be, n, nse=None, dtype=torch.float32, indptr_dtype=torch.int32, shape=None, data=None):
    """A CSR container around CPU tensors (its constructor needs a device): what the checks read."""
    nse = 2 * n if nse is None else nse
    rec = object.__new__(be.CSR)
    rec.data = torch.zeros(nse, dtype=dtype) if data is None else data
    rec.indices = torch.zeros(nse, dtype=torch.int32)
    rec.indptr = torch.linspace(0, nse, n + 1).to(indptr_dtype)
    rec.shape = (n, n) if shape is None else shape
    return rec


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
    kw = dict(syn_decay=0.8, beta=0.9, scale_exp=20)
    ad = dict(kw, adapt=(0.95, 0.3))
    run = be.recurrent_lif_sequence

    def refused(error, match, x=x, rec=rec, state=(c, v), s0=s0, **over):
        with pytest.raises(error, match=match):
            run(x, rec, state, s0, **{**kw, **over})

    # the matrix
    for bad in (None, torch.zeros(N, N), (rec.data, rec.indices, rec.indptr), object.__new__(be.CSC), object.__new__(be.PlannedMatrix)):
        refused(TypeError, 'rec must be a CSR', rec=bad)
    refused(ValueError, 'square', rec=fake_csr(be, N, shape=(N, N + 1)))
    refused(ValueError, "size of x's last axis", rec=fake_csr(be, N + 1))
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        refused(TypeError, 'weights of rec must be float32', rec=fake_csr(be, N, dtype=dtype))
    refused(ValueError, 'one shared weight is not built', rec=fake_csr(be, N, data=torch.zeros(1)))
    refused(TypeError, 'indptr of rec must be int32', rec=fake_csr(be, N, indptr_dtype=torch.int64))
    big = _neuron_rec_sg.MAX_N + 1
    refused(ValueError, 'the limit is 8192', x=fake(torch.zeros(1, 1, big)), rec=fake_csr(be, big, nse=0), state=None, s0=None)
    # ranks and shapes
    for bad in (fake(torch.zeros(N)), fake(torch.zeros(2, 2, B, N)), fake(torch.zeros(()))):
        refused(ValueError, r'\[T, B, N\] or \[T, N\]', x=bad, state=None, s0=None)
    refused(ValueError, 'shape of a step', s0=fake(torch.zeros(N)))
    refused(ValueError, 'shape of a step', s0=fake(torch.zeros(B, N + 1)))
    refused(ValueError, 'shape of a step', state=(c, fake(torch.zeros(N))))
    refused(ValueError, 'shape of a step', x=fake(torch.zeros(5, N)), state=(c, v), s0=None)
    for dtype in (torch.float64, torch.float16, torch.bool, torch.int32):
        refused(TypeError, 'float32', s0=s0.to(dtype))
        refused(TypeError, 'float32', x=x.to(dtype))
        refused(TypeError, 'float32', state=(c.to(dtype), v))
    refused(TypeError, 'Tensor', s0=np.zeros((B, N), F))
    refused(TypeError, 'Tensor', x=[[0.0]])
    # the exponent
    for bad in (20.0, '20', True, fake(torch.tensor(20))):
        refused(TypeError, 'scale_exp must be None or an int', scale_exp=bad)
    for bad in (-91, 151, 1 << 40):
        refused(ValueError, 'scale_exp', scale_exp=bad)
    # everything the synaptic neuron refuses
    for over, match in ((dict(reset='none'), 'reset'), (dict(surrogate='relu'), 'surrogate'), (dict(alpha=0.0), 'alpha'),
                        (dict(alpha=float('nan')), 'alpha')):
        refused(ValueError, match, **over)
    for name in ('syn_decay', 'beta', 'v_th', 'v_reset', 'alpha'):
        refused(TypeError, 'learnable parameters exist for lif_step only', **{name: fake(torch.full((N,), 0.9))})
        refused(TypeError, 'Python number', **{name: 'x'})
    for bad, error in ((0.95, TypeError), ((0.95,), ValueError), ((0.95, None), TypeError)):
        refused(error, 'adapt', state=(c, v, a), adapt=bad)
    refused(ValueError, r'without adapt it is \(c, v\)', state=(c, v, a))
    refused(ValueError, r'takes \(c, v, a\)', adapt=(0.95, 0.3))
    refused(TypeError, 'tuple', state=c)
    # CPU tensors: there is no CPU implementation
    cpu = torch.zeros(B, N)
    refused(ValueError, 'device tensor', x=torch.zeros(5, B, N))
    refused(ValueError, 'device tensor', s0=cpu)
    refused(ValueError, 'device tensor', state=(c, cpu))
    with pytest.raises(TypeError):                                             # beta has no default
        run(x, rec, syn_decay=0.8)
    # ... and what is accepted passes every check: the first thing it reaches is the device call
    for args, k in (((x, rec), kw), ((x, rec, None, s0), ad), ((x, rec, (None, v)), kw), ((x, rec, [c, None, a], s0), ad),
                    ((fake(torch.zeros(5, N)), rec, (fake(torch.zeros(N)), None)), dict(beta=0.9, scale_exp=-90)),
                    ((x, fake_csr(be, N, nse=0)), dict(beta=0.9, scale_exp=np.int64(150)))):
        with pytest.raises(AssertionError, match='reached the device call'):
            run(*args, **k)
    with pytest.raises(AssertionError, match='reached the device call'):       # an empty matrix needs no exponent
        run(x, fake_csr(be, N, nse=0), beta=0.9)


def test_the_call(be, monkeypatch):
    """Spied on, not run: the arguments the forward entry point gets."""
    from brainevent_amd import _neuron_rec_sg
    calls = []
    monkeypatch.setattr(_neuron_rec_sg, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(_neuron_rec_sg.A, 'stream_ptr', lambda: None)
    fake = FakeDevice.wrap
    B, N = 3, 4
    x, v, s0 = fake(torch.zeros(5, B, N)), fake(torch.zeros(B, N)), fake(torch.zeros(B, N))
    rec = fake_csr(be, N)
    s, (c_last, v_last) = be.recurrent_lif_sequence(x, rec, beta=0.9, scale_exp=20)
    s, v_seq, last = be.recurrent_lif_sequence(x[:, 0], rec, (None, v[0], v[0]), s0[0], syn_decay=0.5, beta=0.25, v_th=2, reset='soft',
                                               adapt=(0.75, 0.125), return_v=True, scale_exp=-3)
    assert s.shape == v_seq.shape == (5, N) and len(last) == 3 and all(t.shape == (N,) for t in last)
    assert [n for n, _ in calls] == ['be_lif_rec_sg_forward'] * 2
    (_, a), (_, b) = calls
    assert len(a) == len(b) == 28
    assert a[15:27] == (5, B, N, 0.0, 0.9, 1.0, 0.0, 0.0, 0.0, 0, 0, 20)
    assert b[15:27] == (5, 1, N, 0.5, 0.25, 2.0, 0.0, 0.75, 0.125, 1, 1, -3)
    # no s0, no state, no adaptation, nothing requires grad: s0, c0, v0, a0, v_seq, h_save, th_save, a_last are NULL
    assert [i for i, q in enumerate(a[:15]) if q.value is None] == [4, 5, 6, 7, 9, 10, 11, 14]
    assert [i for i, q in enumerate(b[:15]) if q.value is None] == [5, 10, 11]
    assert a[1].value == rec.data.data_ptr() and a[2].value == rec.indices.data_ptr() and a[3].value == rec.indptr.data_ptr()
