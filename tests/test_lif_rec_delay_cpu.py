"""The recurrent spiking layer with synaptic delays without a device: the numpy restatement the GPU tests compare with
(tests/lif_rec_delay_cases.py) is held to torch's CPU autograd of the dense formulation — ``sum over d of sp(t - 1 - d) @ W_d`` plus
the plain formula of the synaptic neuron —; deliberately wrong variants must fall outside its bound; without delays it is
tests/lif_rec_sg_cases.py bit for bit; the constants and the limit rule are held to the text of csrc/be_neuron_sg_rec_delay.hip,
the prototypes to the header, and the refusals that need no device are raised.

The weights of the comparison with autograd are multiples of 2**-6: their sums are exact in f32 in any order and in fixed point at
the chosen exponent, so forward values must be EQUAL.  Gradients — of ``x``, the state, the history and the stacked weights — are
compared within the propagated bound of ``lif_rec_delay_cases.backward(with_bound=True)`` / ``weight_grad``."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lif_rec_delay_cases as D
import lif_rec_sg_cases as R
import lif_syn_sg_cases as S
from lif_rec_delay_cases import F
from test_lif_rec_sg_cpu import fake_csr
from test_lif_syn_sg_cpu import FakeDevice, Spike

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron_sg_rec_delay.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'
DESIGN = ROOT / 'DESIGN.md'
EXP = 40                                     # the dyadic weights are exact from 6 on; 2**40 * (a column's |w|) stays far below 2**62


def plain(x, w, dl, s_hist, c0, v0, a0, p):
    """The dense formulation in torch: ``(s [T, B, N], v_seq, c_last, v_last, a_last)``; ``w`` holds one weight per stacked entry,
    ``s_hist`` is ``[A, B, N]`` (``A`` may be 0)."""
    syn_decay, beta, v_th, v_reset, rho, kappa = (torch.tensor(F(k)) for k in (p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa))
    n, st = dl.m.n, dl.stacked
    rows, cols = torch.tensor(D.stacked_rows(dl)), torch.tensor(st.indices.astype(np.int64))
    W = torch.zeros(dl.depth * n, n).index_put((rows, cols), w, accumulate=True).reshape(dl.depth, n, n)
    c, v, a, ss, vs = c0, v0, a0, [], []
    for t in range(x.shape[0]):
        r = torch.zeros_like(x[t])               # (the dyadic sums are exact in any order: x[t] + r is the one rounded addition)
        for d in range(dl.depth):
            tau = t - 1 - d
            if tau >= 0:
                r = r + ss[tau] @ W[d]
            elif -1 - tau < s_hist.shape[0]:
                r = r + s_hist[-1 - tau] @ W[d]
        xin = x[t] + r
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
    return torch.stack(ss), torch.stack(vs), c, v, a


def case(T, B, N, depth, A, seed, kind='random'):
    m = R.dyadic_matrix(N, seed)
    assert ((m.w * 64) == np.round(m.w * 64)).all() and np.abs(m.w).max() <= 1
    dl = D.split(m, D.delays_for(kind, m, depth, seed + 100), depth)
    x, _, state, grads = D.inputs(T, B, N, seed)
    return dl, x, D.history(A, B, N, seed + 200), state, grads


def contribution_of_delay(dl, f, s_hist, d, e):
    """Whether some step receives a non-zero recurrent input through the synapses of delay ``d``."""
    sub = D.of_delay(dl, d)
    fixed = D.fixed_from_f32(sub.w, e)
    T, B, _ = f.s_out.shape
    return any(R.recurrent_input(sub, fixed, D.spikes_at(f.s_out, s_hist, t - 1 - d)[b], e).any() for t in range(T) for b in range(B))


SHAPES = sorted({(T, depth, A) for T in (1, 2, 5) for depth in (1, 2, 3, 7) for A in (0, 1, depth)})


@pytest.mark.parametrize('T,depth,A', SHAPES)
@pytest.mark.parametrize('reset,surrogate,detach,adaptive', D.R.MODES)
def test_restatement_against_cpu_autograd(reset, surrogate, detach, adaptive, T, depth, A):
    p = S.mode_params(reset, surrogate, detach, adaptive)
    B, N = 2, 61
    dl, x, s_hist, state, grads = case(T, B, N, depth, A, seed=T)
    ref = D.forward(x, dl, s_hist, *state, p, EXP)
    # the inputs are doing something: a plausible rate, recurrent input at every step that can have one, and every delay that can
    # act within T steps and A past ones does (sp(t - 1 - d) exists for -A <= t - 1 - d <= T - 2: the delays d < T - 1 + A)
    assert 0.05 < ref.s_out.mean() < 0.6
    assert all(np.count_nonzero(ref.r[t]) > 0 for t in range(1, T))
    for d in range(min(depth, T - 1 + A)):
        assert contribution_of_delay(dl, ref, s_hist, d, EXP), d
    hist = np.zeros((0, B, N), F) if s_hist is None else s_hist
    leaves = [torch.tensor(a, requires_grad=True) for a in (x, dl.stacked.w, hist) + state]
    s, v_seq, c_last, v_last, a_last = plain(leaves[0], leaves[1], dl, *leaves[2:], p)
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
        r, b = D.backward(ref.h_save, ref.th_save, dl, *given, p, hist_ages=A, with_bound=True)
        g_w, b_w = D.weight_grad(dl, ref.s_out, s_hist, r.g_x, b.g_x)
        wants = [('g_x', r.g_x, b.g_x), ('g_w', g_w, b_w), ('g_s_hist', r.g_s_hist, b.g_s_hist), ('g_c0', r.g_c0, b.g_c0),
                 ('g_v0', r.g_v0, b.g_v0), ('g_a0', r.g_a0, b.g_a0)]
        for g, (name, want, bound) in zip(got, wants):
            if want.size == 0:
                continue
            err = np.abs(g.astype(np.float64) - want)
            assert (err <= bound).all(), (which, name, err.max(), bound.flat[err.argmax()])
        assert np.abs(r.g_x).max() > 1e-3
        assert b.g_x.max() < 1e-3 * b.terms.max()                      # the bound is a rounding bound, not a tolerance
        if T - 1 + A > 0:
            assert np.abs(g_w).max() > 1e-3 and b_w.max() < 1e-3 * np.abs(g_w).max()
        else:
            assert not g_w.any()


def test_the_comparison_can_fail():
    """Outside the bound: delays off by one, a history whose ages above 0 are ignored, a weight gradient that starts one step
    late, and a history gradient without its ``d > a`` terms."""
    p = S.Params(adaptive=True)
    T, B, N, depth, A = 5, 2, 61, 3, 3
    dl, x, s_hist, state, grads = case(T, B, N, depth, A, seed=5)
    ref = D.forward(x, dl, s_hist, *state, p, EXP)
    r, b = D.backward(ref.h_save, ref.th_save, dl, *grads, p, hist_ages=A, with_bound=True)
    outside = lambda got: any((np.abs(g.astype(np.float64) - want) > bound).any() for g, want, bound in zip(got, r, b))
    assert not outside(r)
    # d + 1 for d
    off = D.split(dl.m, dl.delays + 1, depth + 1)
    assert outside(D.backward(ref.h_save, ref.th_save, off, *grads, p, hist_ages=A))
    assert not np.array_equal(D.forward(x, off, s_hist, *state, p, EXP).s_out, ref.s_out)
    # the ages above 0 of the history ignored: other spikes forwards, another weight gradient
    assert not np.array_equal(D.forward(x, dl, s_hist[:1], *state, p, EXP).s_out, ref.s_out)
    g_w, b_w = D.weight_grad(dl, ref.s_out, s_hist, r.g_x, b.g_x)
    assert not (np.abs(D.weight_grad(dl, ref.s_out, s_hist, r.g_x).astype(np.float64) - g_w) > b_w).any()
    assert (np.abs(D.weight_grad(dl, ref.s_out, s_hist[:1], r.g_x).astype(np.float64) - g_w) > b_w).any()
    # the weight gradient started a step late
    assert (np.abs(D.weight_grad(dl, ref.s_out, s_hist, r.g_x, late=1).astype(np.float64) - g_w) > b_w).any()
    # g_s_hist without its d > a terms
    own = D.backward(ref.h_save, ref.th_save, dl, *grads, p, hist_ages=A, own_age_only=True)
    assert (np.abs(own.g_s_hist.astype(np.float64) - r.g_s_hist) > b.g_s_hist).any()
    assert all(R.same_bits(u, v) for u, v in zip(own[:4], r[:4]))


@pytest.mark.parametrize('adaptive', (False, True))
def test_without_delays_it_is_the_recurrent_layer(adaptive):
    """depth = 1, every delay 0: the stacked matrix is the matrix, and forwards every output has tests/lif_rec_sg_cases.py's bits
    (N(0, 0.05) weights at the exponent's own value: nothing is exact here but the integer sums)."""
    p = S.Params(adaptive=adaptive, reset='soft', surrogate='atan')
    T, B, N = 4, 3, 65
    x, s0, state, grads = D.inputs(T, B, N, seed=2)
    m = R.random_matrix(N, 3)
    dl = D.split(m, np.zeros(len(m.w), np.int32), 1)
    assert np.array_equal(dl.stacked.indptr, m.indptr) and np.array_equal(dl.perm, np.arange(len(m.w)))
    e = D.exponent(m)
    assert e == D.exponent(dl.stacked)
    f, f0 = D.forward(x, dl, s0[None], *state, p, e), R.forward(x, m, s0, *state, p, e)
    assert f0.r.any()
    for u, v in zip(f, f0):
        assert (u is None and v is None) or R.same_bits(u, v)
    r, r0 = D.backward(f.h_save, f.th_save, dl, *grads, p, hist_ages=1), R.backward(f0.h_save, f0.th_save, m, *grads, p)
    for u, v in zip(r[:4] + (r.g_s_hist[0],), r0):
        assert (u is None and v is None) or R.same_bits(u, v)
    assert R.same_bits(D.weight_grad(dl, f.s_out, s0[None], r.g_x), R.weight_grad(m, f0.s_out, s0, r0.g_x))


def test_restatement_edges():
    """Parallel synapses count once each; the aged mask is the spike trains shifted by d steps; the split's masks and order."""
    m = D.parallel_matrix(40, 1, dyadic=True)
    n_rows = np.diff(m.indptr)
    assert (n_rows[::3] == 0).all() and n_rows.max() >= 4
    dl = D.split(m, D.delays_for('random', m, 7, 2), 7)
    assert np.array_equal(D.to_original(dl, dl.stacked.w), m.w)
    pairs = {}
    for row, col, d in zip(R.rows_of(m), m.indices, dl.delays):
        pairs.setdefault((row, col), set()).add(int(d))
    assert max(len(v) for v in pairs.values()) >= 2                    # the same (row, col) with different delays
    lens = np.diff(dl.stacked.indptr).reshape(7, 40)
    from delay_cases import unpack_words_np
    assert all(np.array_equal(unpack_words_np(dl.row_mask[d], 40)[:40], lens[d] > 0) for d in range(7)) and (lens == 0).any()
    # one presynaptic spike, alone: its entries arrive delay by delay
    T, B, N = 9, 1, 40
    pre = int(np.flatnonzero(n_rows >= 4)[0])
    hist = np.zeros((1, B, N), F)
    hist[0, 0, pre] = 1
    p = S.Params(v_th=1e9)                                              # nobody fires: the only spike is the history's
    f = D.forward(np.zeros((T, B, N), F), dl, hist, None, None, None, p, EXP)
    want = np.zeros((T, N))
    for k in range(m.indptr[pre], m.indptr[pre + 1]):
        want[dl.delays[k], m.indices[k]] += m.w[k]
    assert not f.s_out.any() and np.array_equal(f.r[:, 0], want.astype(F)) and np.count_nonzero(want.any(axis=1)) >= 2
    # the aged mask, bit by bit
    s_out = (np.random.default_rng(3).random((5, 3, N)) < 0.3).astype(F)
    s_hist = D.history(2, 3, N, 4)
    mask = D.aged_mask(s_out, s_hist, 7)
    assert mask.shape == (7 * N, 1) and mask.dtype == np.uint32
    for d, i, t, b in ((0, 5, 0, 1), (0, 5, 1, 1), (1, 7, 0, 2), (2, 7, 0, 0), (3, 9, 4, 2), (6, 0, 4, 0), (6, 39, 4, 2)):
        tau = t - 1 - d
        on = s_out[tau, b, i] if tau >= 0 else (s_hist[-1 - tau, b, i] if -1 - tau < 2 else 0)
        assert (mask[d * N + i, 0] >> (t * 3 + b)) & 1 == int(on != 0)
    assert not (mask >> 15).any()                                       # the bits past T * B are 0


# ------------------------------------------------------------------------------------------------ the constants and the source
PATTERNS = {
    'kDelThreads': r'constexpr int kDelThreads = (\d+);',
    'kDelMaxN': r'constexpr int kDelMaxN = (\d+);',
    'kDelMaxDepth': r'constexpr int kDelMaxDepth = (\d+);',
    'kDelRowLanes': r'constexpr int kDelRowLanes = (\d+);',
    'kDelUnroll': r'constexpr int kDelUnroll = (\d+);',
    'kDelMinIds': r'constexpr int kDelMinIds = (\d+);',
}

SOURCE_TEXT = [
    ('#include "be_sg_lane.h"', 1),
    ('constexpr int kDelPerThread = kDelMaxN / kDelThreads;', 1),
    ('constexpr int kDelLdsBytes = 160 * 1024 - 1024;', 1),
    ('__launch_bounds__(kDelThreads)', 2),
    ('__global__', 3),
    ('hipLaunchKernelGGL(', 3),
    ('#pragma clang fp contract(off)', 3),
    ('inline int64_t del_fixed_lds(int64_t N, int64_t depth) { return 8 * N + 8 * depth * ((N + 63) / 64); }', 1),
    ('if (N > kDelMaxN || B > 0x7fffffffll || del_fixed_lds(N, depth) + 4 * kDelMinIds > kDelLdsBytes) {', 1),
    ('return BE_ERR_RANGE;', 1),
    ('if (col[q] >= 0) atomicAdd(&acc[col[q]], fixed_from_f32(wk[q], scale));', 1),
    ('dim3((unsigned)B), dim3(kDelThreads), lds, st,', 2),
    ('template <bool HARD, bool ADAPT>', 1),
    ('template <bool HARD, int SG, bool ADAPT>', 1),
]


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    found = re.findall(PATTERNS[key], SOURCE.read_text())
    assert len(found) == 1 and int(found[0]) == D.CONSTS[key], (f'{key}: be_neuron_sg_rec_delay.hip says {found}, '
                                                               f'tests/lif_rec_delay_cases.py assumes {D.CONSTS[key]}')


def test_limits_follow_the_constants():
    from brainevent_amd import _neuron_rec_sg
    text = SOURCE.read_text()
    for line, times in SOURCE_TEXT:
        assert text.count(line) == times, f'be_neuron_sg_rec_delay.hip holds {line!r} {text.count(line)} times, not {times}'
    k = D.CONSTS
    assert (_neuron_rec_sg.MAX_N, _neuron_rec_sg.MAX_DEPTH, _neuron_rec_sg.DELAY_MIN_IDS, _neuron_rec_sg.DELAY_LDS_BYTES) == \
        (k['kDelMaxN'], k['kDelMaxDepth'], k['kDelMinIds'], D.LDS_BYTES)
    # what must be accepted is, by the rule as the source, the Python mirror and the cases state it
    for n, depth in ((8192, 16), (8192, 1), (2048, 256), (1, 256), (8191, 16), (2047, 256), (1025, 7)):
        assert D.fits(n, depth) and _neuron_rec_sg.delay_fits(n, depth), (n, depth)
    assert all(D.fits(n, 16) for n in range(1, 8193, 13)) and all(D.fits(n, 256) for n in range(1, 2049, 7))
    for n, depth in ((8193, 1), (8192, 256), (4096, 256), (100, 257), (100, 0)):
        assert not D.fits(n, depth) and not _neuron_rec_sg.delay_fits(n, depth), (n, depth)
    assert all(D.fits(n, d) == _neuron_rec_sg.delay_fits(n, d) for n in range(1, 8300, 97) for d in (1, 16, 17, 64, 255, 256))
    # the GPU sizes: a second neuron per thread, more than one 64-bit history word, an odd number of 32-bit mask words
    assert k['kDelThreads'] + 1 in D.N_SIZES and 65 in D.N_SIZES and 257 in D.N_SIZES and (2, 256) in D.T_DEPTHS
    # no float atomics, no global atomics, no cooperative launch: the one read-modify-write is the LDS integer add
    assert text.count('atomicAdd') == 1 and '__hip_atomic' not in text and 'atomicAdd(&acc[' in text and 'Cooperative' not in text
    assert 'unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem_raw);' in text
    design = DESIGN.read_text()
    assert '### 2.26' in design and 'be_lif_rec_delay_sg_forward' in design and 'kDelMaxN = 8192' in design
    assert '358 exported symbols' in design


def test_prototypes_against_the_header():
    from brainevent_amd import _abi
    counts = {'be_lif_rec_delay_sg_forward': 31, 'be_lif_rec_delay_sg_backward': 33, 'be_grad_pack_activity_aged': 9}
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
    # §2.22's order: row_mask and depth after the matrix; s_hist, hist_ages in the place of s0; g_s_hist, hist_ages in that of g_s0
    rec_f, del_f = names('be_lif_rec_sg_forward'), names('be_lif_rec_delay_sg_forward')
    assert del_f == rec_f[:4] + ['row_mask', 'depth', 's_hist', 'hist_ages'] + rec_f[5:]
    rec_b, del_b = names('be_lif_rec_sg_backward'), names('be_lif_rec_delay_sg_backward')
    assert del_b == rec_b[:5] + ['row_mask', 'depth'] + rec_b[5:14] + ['g_s_hist', 'hist_ages'] + rec_b[15:]
    assert names('be_grad_pack_activity_aged') == ['s', 's_hist', 'N', 'B', 'T', 'depth', 'hist_ages', 'mask', 'stream']
    assert len(re.findall(r'#define (BE_LIF_\w+) (\d+)', HEADER.read_text())) == 5            # no new numeric code
    doc = HEADER.read_text()
    for line in ('stacked row d * N + i is', 'g_rec = g_rec + (sum over the entries k of stacked row d * N + i of w[k] * g_x[t + 1 + d][b][indices[k]])',
                 'if t < T-1: g_sp = g_sp + g_rec', '8 * N + 8 * depth * ceil(N / 64) + 16384 <= 162816',
                 'g_x is a REQUIRED output', 'be_grad_mask_bytes(depth * N, T * B) bytes'):
        assert line in doc, line


# ------------------------------------------------------------------------------------------------ refusals that need no device
def fake_delayed(be, n, depth, nse=None, dtype=torch.float32, indptr_dtype=torch.int32, shape=None, data=None):
    """A DelayedCSR container around CPU tensors (its constructor needs a device): what the checks read."""
    nse = 2 * n if nse is None else nse
    rec = object.__new__(be.DelayedCSR)
    st = object.__new__(be.CSR)
    st.data = torch.zeros(nse, dtype=dtype) if data is None else data
    st.indices = torch.zeros(nse, dtype=torch.int32)
    st.indptr = torch.linspace(0, nse, depth * n + 1).to(indptr_dtype)
    st.shape = (depth * n, n)
    rec.stacked, rec.depth = st, depth
    rec.shape = (n, n) if shape is None else shape
    rec.row_mask = torch.zeros((depth, (n + 31) // 32), dtype=torch.int32)
    return rec


def test_refusals_without_a_device(be, monkeypatch):
    from brainevent_amd import _neuron_rec_sg

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron_rec_sg, 'call', no_call)
    monkeypatch.setattr(_neuron_rec_sg.A, 'stream_ptr', lambda: None)
    fake = FakeDevice.wrap
    B, N, depth = 3, 4, 5
    x = fake(torch.zeros(5, B, N))
    c, v, a = (fake(torch.zeros(B, N)) for _ in range(3))
    s0 = fake(torch.zeros(2, B, N))
    rec = fake_delayed(be, N, depth)
    kw = dict(syn_decay=0.8, beta=0.9, scale_exp=20)
    run = be.recurrent_lif_sequence

    def refused(error, match, x=x, rec=rec, state=(c, v), s0=s0, **over):
        with pytest.raises(error, match=match):
            run(x, rec, state, s0, **{**kw, **over})

    refused(ValueError, 'square', rec=fake_delayed(be, N, depth, shape=(N, N + 1)))
    refused(ValueError, "size of x's last axis", rec=fake_delayed(be, N + 1, depth))
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        refused(TypeError, 'weights of rec must be float32', rec=fake_delayed(be, N, depth, dtype=dtype))
    refused(ValueError, 'one shared weight is not built', rec=fake_delayed(be, N, depth, data=torch.zeros(1)))
    refused(TypeError, 'indptr of rec must be int32.*int64 indptr.*not built', rec=fake_delayed(be, N, depth, indptr_dtype=torch.int64))
    big = _neuron_rec_sg.MAX_N + 1
    refused(ValueError, 'the limit is 8192', x=fake(torch.zeros(1, 1, big)), rec=fake_delayed(be, big, 1, nse=0), state=None, s0=None)
    for n, d in ((8192, 256), (4096, 256), (8192, 17 * 8)):
        refused(ValueError, f'{n} neurons at depth {d} do not fit.*several workgroups is not built', x=fake(torch.zeros(1, 1, n)),
                rec=fake_delayed(be, n, d, nse=0), state=None, s0=None)
    # the history: a step of x, or A past steps with 1 <= A <= depth
    for bad in ((N,), (B, N + 1), (0, B, N), (depth + 1, B, N), (2, B + 1, N), (1, 2, B, N)):
        refused(ValueError, r'hold A past steps.*1 <= A <= depth = 5', s0=fake(torch.zeros(bad)))
    refused(ValueError, 'hold A past steps', x=fake(torch.zeros(5, N)), state=None, s0=fake(torch.zeros(B, 1, N)))
    for dtype in (torch.float64, torch.bool):
        refused(TypeError, 'float32', s0=s0.to(dtype))
    refused(ValueError, 'device tensor', s0=torch.zeros(2, B, N))
    for bad in (20.0, True):
        refused(TypeError, 'scale_exp must be None or an int', scale_exp=bad)
    refused(ValueError, 'scale_exp', scale_exp=151)
    refused(TypeError, 'learnable parameters exist for lif_step only', beta=fake(torch.full((N,), 0.9)))
    # learnable parameters with delays: all numbers delegate, a tensor is not built
    par = be.parametric_recurrent_lif_sequence
    for over in (dict(beta=fake(torch.tensor(0.9))), dict(beta=0.9, v_th=fake(torch.ones(N))),
                 dict(beta=0.9, adapt=(fake(torch.tensor(0.9)), 0.3))):
        with pytest.raises(NotImplementedError, match='together with synaptic delays are not built'):
            par(x, rec, (c, v, a) if 'adapt' in over else (c, v), s0, scale_exp=20, **over)
    with pytest.raises(AssertionError, match='reached the device call'):
        par(x, rec, (c, v), s0, **kw)
    # ... and what is accepted passes every check: the first thing it reaches is the device call
    for args, k in (((x, rec), kw), ((x, rec, None, s0), kw), ((x, rec, (None, v), fake(torch.zeros(B, N))), kw),
                    ((x, rec, [c, None, a], fake(torch.zeros(depth, B, N))), dict(kw, adapt=(0.95, 0.3))),
                    ((fake(torch.zeros(5, N)), rec, None, fake(torch.zeros(N))), kw),
                    ((fake(torch.zeros(5, N)), rec, None, fake(torch.zeros(3, N))), kw),
                    ((fake(torch.zeros(1, 1, 8192)), fake_delayed(be, 8192, 16, nse=0)), kw),
                    ((fake(torch.zeros(1, 1, 2048)), fake_delayed(be, 2048, 256, nse=0)), kw),
                    ((x, fake_delayed(be, N, depth, nse=0)), dict(beta=0.9))):              # an empty matrix needs no exponent
        with pytest.raises(AssertionError, match='reached the device call'):
            run(*args, **k)


def test_the_calls(be, monkeypatch):
    """Spied on, not run: a DelayedCSR reaches the delayed entry point with the stacked arrays; a plain CSR takes today's path."""
    from brainevent_amd import _neuron_rec_sg
    calls = []
    monkeypatch.setattr(_neuron_rec_sg, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(_neuron_rec_sg.A, 'stream_ptr', lambda: None)
    fake = FakeDevice.wrap
    B, N, depth = 3, 4, 5
    x, v = fake(torch.zeros(5, B, N)), fake(torch.zeros(B, N))
    rec = fake_delayed(be, N, depth)
    s, (c_last, v_last) = be.recurrent_lif_sequence(x, rec, beta=0.9, scale_exp=20)
    s, v_seq, last = be.recurrent_lif_sequence(x[:, 0], rec, (None, v[0], v[0]), fake(torch.zeros(2, N)), syn_decay=0.5, beta=0.25, v_th=2,
                                               reset='soft', adapt=(0.75, 0.125), return_v=True, scale_exp=-3)
    assert s.shape == v_seq.shape == (5, N) and len(last) == 3 and all(t.shape == (N,) for t in last)
    be.recurrent_lif_sequence(x, rec, None, v, beta=0.9, scale_exp=20)          # s0 [B, N]: one age
    be.recurrent_lif_sequence(x, fake_csr(be, N), None, v, beta=0.9, scale_exp=20)
    be.parametric_recurrent_lif_sequence(x, fake_csr(be, N), None, v, beta=0.9, scale_exp=20)
    assert [n for n, _ in calls] == ['be_lif_rec_delay_sg_forward'] * 3 + ['be_lif_rec_sg_forward'] * 2
    (_, a), (_, b), (_, c), (_, d), _ = calls
    assert len(a) == len(b) == 31 and len(d) == 28
    assert a[18:30] == (5, B, N, 0.0, 0.9, 1.0, 0.0, 0.0, 0.0, 0, 0, 20)
    assert b[18:30] == (5, 1, N, 0.5, 0.25, 2.0, 0.0, 0.75, 0.125, 1, 1, -3)
    st = rec.stacked
    for q in (a, b, c):
        assert (q[1].value, q[2].value, q[3].value, q[4].value, q[5]) == (st.data.data_ptr(), st.indices.data_ptr(), st.indptr.data_ptr(),
                                                                        rec.row_mask.data_ptr(), depth)
    assert (a[6].value, a[7]) == (None, 0) and b[6].value is not None and b[7] == 2 and c[6].value == v.data_ptr() and c[7] == 1
    # no state, no adaptation, nothing requires grad: c0, v0, a0, v_seq, h_save, th_save, a_last are NULL
    assert [i for i, q in enumerate(a[8:18], 8) if q.value is None] == [8, 9, 10, 12, 13, 14, 17]
    assert [i for i, q in enumerate(b[8:18], 8) if q.value is None] == [8, 13, 14]
