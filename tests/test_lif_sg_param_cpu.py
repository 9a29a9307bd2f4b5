"""The LIF neuron with learnable, per-neuron ``beta`` / ``v_th`` without a device: the numpy restatement the GPU tests compare with
(tests/lif_sg_param_cases.py) is held to torch's CPU autograd of the plain formula with the two parameters as leaf tensors, the
reduce's reference to ``math.fsum``, the constants the GPU sizes come from to the text of csrc/be_neuron_sg.hip (the lane kernels) and
csrc/be_neuron_sg_reduce.hip (the reduce), and the refusals that need no device are raised.

Forward values must be equal.  ``g_x`` / ``g_v0`` are compared within the bound of tests/lif_sg_cases.py.  A parameter's gradient
is a sum of ``n = T * N / P`` terms that autograd forms and adds in an order that is not ours to fix; it is compared within
``sum (what the difference carried by a term's factors becomes in it) + (n + 1) 2**-23 sum |terms|`` — twice the first-order bound
of an n-term f32 sum of rounded products in any order."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lif_sg_cases as C
import lif_sg_param_cases as PC
from lif_sg_cases import F

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron_sg.hip'
REDUCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron_sg_reduce.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'


class Spike(torch.autograd.Function):
    """Heaviside of ``h - th`` forwards; backwards the surrogate's derivative, to ``h`` and (negated) to ``th``."""

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
        return g * sg, -(g * sg), None


def plain(x, v0, beta, v_th, p):
    """The plain formula in torch on ``[T, R, n]``: ``(s, v_seq, v_last)``; ``beta`` / ``v_th`` broadcast (``[1]`` or ``[n]``)."""
    v_reset = torch.tensor(F(p.v_reset))
    v, ss, vs = v0, [], []
    for t in range(x.shape[0]):
        h = beta * v + x[t]
        s = Spike.apply(h, v_th.expand_as(h), p)
        sr = s.detach() if p.detach_reset else s
        v = h * (1 - sr) + v_reset * sr if p.reset == 'hard' else h - sr * v_th
        ss.append(s)
        vs.append(v)
    return torch.stack(ss), torch.stack(vs), v


N_NEURONS = 37


def restated(T, R, shared, p, seed, use=(True, True, True)):
    """One case: the inputs, the restatement's results and its bounds."""
    N = R * N_NEURONS
    x, v0, g_s, g_vseq, g_vlast = C.inputs(T, N, seed)
    P = 1 if shared else N_NEURONS
    beta, v_th = PC.param_inputs(P, P, seed)
    fw = PC.forward(x, v0, beta, v_th, p)
    bw = PC.backward(fw[2], v0, g_s if use[0] else None, g_vseq if use[1] else None, g_vlast if use[2] else None, beta, v_th, p,
                     with_bound=True)
    return (x, v0, g_s, g_vseq, g_vlast, beta, v_th), fw, bw, P


def autograd_grads(arrays, R, p, use):
    x, v0, g_s, g_vseq, g_vlast, beta, v_th = arrays
    T = x.shape[0]
    shape = (R, N_NEURONS)
    xt = torch.tensor(x.reshape((T,) + shape), requires_grad=True)
    vt = torch.tensor(v0.reshape(shape), requires_grad=True)
    bt, tt = torch.tensor(beta, requires_grad=True), torch.tensor(v_th, requires_grad=True)
    s, v_seq, v_last = plain(xt, vt, bt, tt, p)
    outs = [o for o, u in zip((s, v_seq, v_last), use) if u]
    grads = [torch.tensor(g.reshape(o.shape)) for (g, o), u in zip(((g_s, s), (g_vseq, v_seq), (g_vlast, v_last)), use) if u]
    got = torch.autograd.grad(outs, [xt, vt, bt, tt], grads, allow_unused=True)
    zeros = (np.zeros_like(x), np.zeros_like(v0), np.zeros_like(beta), np.zeros_like(v_th))
    got = [z if g is None else g.numpy().reshape(z.shape) for g, z in zip(got, zeros)]
    return (s.detach().numpy().reshape(T, -1), v_seq.detach().numpy().reshape(T, -1), v_last.detach().numpy().reshape(-1)), got


def param_bounds(info, P):
    """name -> (sum |terms|, the bound) per element of the parameter."""
    out = {}
    for name in ('beta', 'vth'):
        terms, carried = info[f'{name}_terms'], info[f'{name}_carried']
        total = np.abs(terms).reshape(-1, P).sum(axis=0)
        out[name] = (total, carried.reshape(-1, P).sum(axis=0) + PC.any_order_bound(terms, P))
    return out


@pytest.mark.parametrize('T', (1, 2, 5))
@pytest.mark.parametrize('R', (1, 3))
@pytest.mark.parametrize('shared', (True, False))
@pytest.mark.parametrize('reset,surrogate,detach', C.MODES)
def test_restatement_against_cpu_autograd(reset, surrogate, detach, shared, R, T):
    p = C.Params(reset=reset, surrogate=surrogate, detach_reset=detach, v_reset=-0.25, alpha=2.0 if surrogate == 'triangle' else 10.0)
    use = (True, True, True)
    arrays, (s_ref, vseq_ref, h_ref, vlast_ref), (rx, rv0, slot_b, slot_t, info), P = restated(T, R, shared, p, seed=10 * T + R)
    assert 0.1 < s_ref.mean() < 0.9
    (s, v_seq, v_last), (gx, gv0, gb, gt) = autograd_grads(arrays, R, p, use)
    assert np.array_equal(s, s_ref) and np.array_equal(v_seq, vseq_ref) and np.array_equal(v_last, vlast_ref)
    ex, ev0 = np.abs(gx.astype(np.float64) - rx), np.abs(gv0.astype(np.float64) - rv0)
    assert np.abs(rx).max() > 1e-3 and (ex <= info['g_x']).all() and (ev0 <= info['g_v0']).all()
    assert info['g_x'].max() < 1e-3 * max(1.0, np.abs(rx).max())
    bounds = param_bounds(info, P)
    for name, got, slot in (('beta', gb, slot_b), ('vth', gt, slot_t)):
        ref = PC.reduce_exact(slot, P)
        total, bound = bounds[name]
        err = np.abs(got.astype(np.float64) - ref)
        print(f'{name}: max |grad - ref| {err.max():.3e} (bound there {bound[err.argmax()]:.3e}, sum |terms| {total[err.argmax()]:.3e})')
        assert total.max() > 0 and (bound <= 1e-3 * total).all(), name        # a rounding bound, not a tolerance
        assert (err <= bound + PC.reduce_bound(slot, P)).all(), name


def test_the_comparison_can_fail():
    """A gradient off by a part in a thousand is outside the bound, and so is a v_th gradient without the soft reset's direct
    term — for the shared and for the per-neuron parameter.  (T = 2: the shared parameter's sum has 222 terms, whose any-order
    bound, 2.7e-5 of their absolute sum, is well under a thousandth of the gradient unless the terms cancel to under 3 %.)"""
    p = C.Params(reset='soft', v_reset=-0.25)
    for shared in (True, False):
        arrays, fw, (rx, rv0, slot_b, slot_t, info), P = restated(2, 3, shared, p, seed=53)
        bounds = param_bounds(info, P)
        for name, slot in (('beta', slot_b), ('vth', slot_t)):
            ref = PC.reduce_exact(slot, P)
            bound = bounds[name][1] + PC.reduce_bound(slot, P)
            assert (np.abs(ref * 1.001 - ref) > bound).any(), (name, shared)
            assert (np.abs(ref.astype(F).astype(np.float64) - ref) <= bound).all()
        # without the direct term: a_th = - sum g_sp * sg alone (the hard reset's formula on the soft reset's quantities)
        x, v0, g_s, g_vseq, g_vlast, beta, v_th = arrays
        h, N = fw[2], fw[2].shape[1]
        th = PC.expand(v_th, N)
        b = PC.expand(beta, N)
        carry, without = g_vlast.copy(), np.zeros(N, np.float64)
        for t in range(h.shape[0] - 1, -1, -1):
            g_vo = carry + g_vseq[t]
            sg = C.surrogate(h[t] - th, p)
            gs = (g_s[t] - g_vo * th) * sg
            without -= gs
            carry = b * (gs + g_vo)
        ref = PC.reduce_exact(slot_t, P)
        bound = bounds['vth'][1] + PC.reduce_bound(slot_t, P)
        assert (np.abs(without.reshape(-1, P).sum(axis=0) - ref) > bound).any(), shared


def test_restatement_edges():
    """Period 1 equals lif_sg_cases with the same constants; h == th_i spikes per neuron; v0 None is zeros; unused gradients are
    zeros; the accumulators of a detached hard reset without g_s are -0 + ... = what the formulas say."""
    p = C.Params(beta=0.9, v_th=1.0, v_reset=-0.25, reset='soft', surrogate='atan')
    x, v0, g_s, g_vseq, g_vlast = C.inputs(5, 24, seed=2)
    one_b, one_t = np.array([0.9], F), np.array([1.0], F)
    fw_old, fw_new = C.forward(x, v0, p), PC.forward(x, v0, one_b, one_t, p)
    assert all(C.same_bits(a, b) for a, b in zip(fw_old, fw_new))
    bw_old = C.backward(fw_old[2], g_s, g_vseq, g_vlast, p)
    bw_new = PC.backward(fw_new[2], v0, g_s, g_vseq, g_vlast, one_b, one_t, p)
    assert C.same_bits(bw_old[0], bw_new[0]) and C.same_bits(bw_old[1], bw_new[1])
    # thresholds that differ across neurons, each met exactly
    th = np.array([0.5, 1.0, 1.5, 2.0], F)
    hit = PC.forward(th[None].copy(), None, one_b, th, C.Params())
    miss = PC.forward(np.nextafter(th, F(0))[None], None, one_b, th, C.Params())
    assert hit[0].tolist() == [[1.0] * 4] and miss[0].tolist() == [[0.0] * 4]
    # the period: slot i reads param[i % P]
    assert PC.expand(np.array([1, 2, 3], F), 6).tolist() == [1, 2, 3, 1, 2, 3]
    a = PC.backward(fw_new[2], None, g_s, None, None, one_b, one_t, p)
    b = PC.backward(fw_new[2], np.zeros_like(v0), g_s, np.zeros_like(g_vseq), np.zeros_like(g_vlast), one_b, one_t, p)
    assert all(C.same_bits(i, j) for i, j in zip(a, b))


# ------------------------------------------------------------------------------------------------ the reduce's reference
def test_reduce_reference_is_fsum_and_a_running_f32_sum_is_outside():
    for R, P in ((33, 3), (33, 65), (PC.CONSTS['kSgpRedTile'] + 1, 1)):
        slot = PC.cancelling(R, P, seed=R + P)
        E = PC.reduce_exact(slot, P)
        cols = slot.reshape(R, P)
        for q in range(P):
            assert E[q] == math.fsum(float(v) for v in cols[:, q])
        A = np.abs(cols.astype(np.float64)).sum(axis=0)
        assert (np.abs(E) < 1e-4 * A).all()                                  # heavy cancellation
        assert PC.within_reduce_bound(PC.reduce_ref(slot, P), slot, P)
        assert PC.within_reduce_bound(cols.astype(np.float64).sum(axis=0).astype(F), slot, P)         # an f64 sum in another order
        running = np.zeros(P, F)
        for r in range(R):
            running = running + cols[r]
        assert running.dtype == F and not PC.within_reduce_bound(running, slot, P)
    assert not PC.within_reduce_bound(np.zeros(3, np.float64), np.zeros(6, F), 3)      # the dtype is part of the comparison
    assert PC.within_reduce_bound(np.array([3.0], F), np.array([1.0, 2.0], F), 1)
    assert not PC.within_reduce_bound(np.array([3.0 + 2.0 ** -21], F), np.array([1.0, 2.0], F), 1)


# ------------------------------------------------------------------------------------------------ the constants and the source
PATTERNS = {key: rf'constexpr int {key} = (\d+);' for key in PC.CONSTS}

SOURCE_TEXT = [
    # which kernel a call takes, and how many blocks
    ('const bool vec = (N % kSgVec == 0) && lane::all_aligned16(x, v0, s_out, v_seq, h_save, v_last) && param_vec(beta, beta_period) &&\n'
     '                   param_vec(v_th, vth_period);', 1),
    ('const float* v0_read = g_beta_slot != nullptr ? v0 : nullptr;', 1),
    ('const bool vec = (N % kSgVec == 0) && lane::all_aligned16(h_save, v0_read, g_s, g_vseq, g_vlast, g_x, g_v0, g_beta_slot, g_vth_slot) &&\n'
     '                   param_vec(beta, beta_period) && param_vec(v_th, vth_period);', 1),
    ('return period == 1 || (period % kSgVec == 0 && lane::aligned16(p));', 1),
    ('constexpr int S = decltype(V)::value ? kSgVec : 1;', 2),
    ('dim3(lane_grid(N, S)),', 2),
    ('return (int)std::min<int64_t>((groups + kSgThreads - 1) / kSgThreads, kSgGridCap);', 1),
    ('__launch_bounds__(kSgThreads)', 2),
    # the ring
    ('for (int64_t t0 = 0; t0 < T; t0 += kSgPrefetch) {', 1),
    ('for (int64_t k0 = 0; k0 < T; k0 += kSgPrefetch) {', 1),
    ('if (t + kSgPrefetch < T) ring[r] = lane::load<S>(x + (t + kSgPrefetch) * N + i);', 1),
    ('if (k + kSgPrefetch < T) {', 1),
    ('const V hp = ring_h[(r + 1) % kSgPrefetch];', 1),
    ('#pragma clang fp contract(off)', 2),
]

REDUCE_TEXT = [
    ('return (int)std::min<int64_t>((N + kSgpRedTile - 1) / kSgpRedTile, kSgpRedGridCap);', 1),
    ('for (int64_t base = (int64_t)blockIdx.x * kSgpRedTile; base < N; base += (int64_t)gridDim.x * kSgpRedTile) {', 1),
    ('const int64_t blocks = (P + kSgpRedCols - 1) / kSgpRedCols;', 1),
    ('constexpr int kRows = kSgpRedThreads / kSgpRedCols;', 1),
    ('__launch_bounds__(kSgpRedThreads)', 3),
]


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    source = REDUCE if key.startswith('kSgpRed') else SOURCE
    found = re.findall(PATTERNS[key], source.read_text())
    assert len(found) == 1 and int(found[0]) == PC.CONSTS[key], (f'{key}: {source.name} says {found}, '
                                                                f'tests/lif_sg_param_cases.py assumes {PC.CONSTS[key]}')


def test_sizes_follow_the_constants():
    text, reduce = SOURCE.read_text(), REDUCE.read_text()
    for source, held, lines in ((SOURCE, text, SOURCE_TEXT), (REDUCE, reduce, REDUCE_TEXT)):
        for line, times in lines:
            assert held.count(line) == times, f'{source.name} holds {line!r} {held.count(line)} times, not {times}'
    k = PC.CONSTS
    scalar, vector = PC.N_PAST_ONE_PASS
    assert scalar % k['kSgVec'] != 0 and scalar == k['kSgThreads'] * k['kSgGridCap'] + 1
    assert vector % k['kSgVec'] == 0 and vector // k['kSgVec'] == k['kSgThreads'] * k['kSgGridCap'] + 1
    assert {k['kSgPrefetch'] - 1, k['kSgPrefetch'], k['kSgPrefetch'] + 1, 1, 2, 25} == set(PC.T_SIZES)
    assert any(n % k['kSgVec'] for n in PC.N_SIZES) and any(n % k['kSgVec'] == 0 for n in PC.N_SIZES)
    assert max(PC.REDUCE_N_SHARED) == k['kSgpRedTile'] * k['kSgpRedGridCap'] + 1 and k['kSgpRedTile'] + 1 in PC.REDUCE_N_SHARED
    assert k['kSgpRedThreads'] + 1 in PC.REDUCE_N_SHARED and k['kSgpRedGridCap'] <= k['kSgpRedThreads']
    rows = k['kSgpRedThreads'] // k['kSgpRedCols']
    assert {k['kSgpRedCols'], k['kSgpRedCols'] + 1} <= set(PC.REDUCE_PERIODS) and min(PC.REDUCE_PERIODS) < k['kSgpRedCols']
    assert min(PC.REDUCE_ROWS) < rows < max(PC.REDUCE_ROWS) and max(PC.REDUCE_ROWS) % rows != 0
    # deterministic sums: no atomic read-modify-write in the lane kernels or in the reduce; LDS in the reduce alone
    for held in (text, reduce):
        assert 'atomicAdd' not in held and '__hip_atomic' not in held and 'atomic_' not in held
    assert '__shared__' not in text and '__shared__' in reduce


def test_abi_and_codes():
    from brainevent_amd import _abi
    counts = {'be_lif_sg_forward_params': 15, 'be_lif_sg_backward_params': 21, 'be_lif_sg_reduce_slots': 7,
              'be_lif_sg_reduce_slots_workspace_bytes': 2}
    header = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    for name, n in counts.items():
        assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name][1]) == n, name
        args, = re.findall(rf'\b{name}\(([^)]*)\);', header)
        assert len(args.split(',')) == n, name
    assert _abi.PROTOTYPES['be_lif_sg_reduce_slots_workspace_bytes'][0] is ctypes.c_int64
    assert _abi.PROTOTYPES['be_lif_sg_forward_params'][1][3] is ctypes.c_int64          # the periods are int64
    # no new numeric code: the five of the float path are reused
    assert len(re.findall(r'#define (BE_LIF_\w+) (\d+)', HEADER.read_text())) == 5


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
    from brainevent_amd import _neuron_sg

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron_sg, 'call', no_call)
    monkeypatch.setattr(_neuron_sg, 'fn', no_call)
    monkeypatch.setattr(_neuron_sg.A, 'stream_ptr', lambda: None)               # (evaluated before the call it is an argument of)
    fake = FakeDevice.wrap
    v, x, seq = fake(torch.zeros(2, 3, 4)), fake(torch.zeros(2, 3, 4)), fake(torch.zeros(5, 2, 3, 4))
    good = fake(torch.full((4,), 0.9))
    for name in ('beta', 'v_th'):
        def both(value, error, match):
            kw = {'beta': 0.9, name: value}
            with pytest.raises(error, match=match):
                be.lif_step(v, x, **kw)
            with pytest.raises(error, match=match):
                be.lif_sequence(seq, v, **kw)
            with pytest.raises(error, match=match):
                be.lif_sequence(seq, **{**{'beta': good, 'v_th': good}, name: value})
        for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
            both(fake(torch.ones(4, dtype=dtype)), TypeError, f'tensor {name} must be float32')
            both(fake(torch.ones((), dtype=dtype)), TypeError, f'tensor {name} must be float32')
        both(torch.ones(4), ValueError, f'tensor {name} must be a device tensor')
        both(torch.ones(()), ValueError, f'tensor {name} must be a device tensor')
        for shape in ((3,), (2,), (5,), (4, 3), (2, 4), (1, 4), (4, 1), (1, 1), (2, 3, 4, 1), (1, 2, 3, 4), (5, 2, 3, 4), (0,)):
            both(fake(torch.ones(shape)), ValueError, 'shape of the last dimensions')
    # lif_sequence: the shape is a STEP's
    with pytest.raises(ValueError, match='shape of the last dimensions'):
        be.lif_sequence(seq, v, beta=fake(torch.ones(5, 2, 3, 4)))
    # the accepted shapes pass every check: the first thing they reach is the device call
    for ok in (fake(torch.ones(())), fake(torch.ones(1)), good, fake(torch.ones(3, 4)), fake(torch.ones(2, 3, 4))):
        with pytest.raises(AssertionError, match='reached the device call'):
            be.lif_step(v, x, beta=ok)
        with pytest.raises(AssertionError, match='reached the device call'):
            be.lif_sequence(seq, v, beta=0.9, v_th=ok)
    # the checks of the float path come first and are unchanged
    with pytest.raises(ValueError, match='device tensor'):
        be.lif_step(torch.zeros(4), torch.zeros(4), beta=good)
    with pytest.raises(ValueError, match='reset'):
        be.lif_step(v, x, beta=good, reset='none')


def test_two_floats_take_the_unchanged_path(be, monkeypatch):
    """Spied on, not run: two Python numbers reach be_lif_sg_forward with the doubles; a tensor reaches the params entry point."""
    from brainevent_amd import _neuron_sg
    calls = []

    def spy(name, *args):
        calls.append((name, args))
    monkeypatch.setattr(_neuron_sg, 'call', spy)
    monkeypatch.setattr(_neuron_sg.A, 'stream_ptr', lambda: None)
    fake = FakeDevice.wrap
    v, x, seq = fake(torch.zeros(3, 4)), fake(torch.zeros(3, 4)), fake(torch.zeros(5, 3, 4))
    be.lif_step(v, x, beta=0.9, v_th=1.25)
    be.lif_sequence(seq, v, beta=np.float32(0.5), v_th=2)
    assert [c[0] for c in calls] == ['be_lif_sg_forward', 'be_lif_sg_forward']
    (_, a), (_, b) = calls
    assert a[6:11] == (1, 12, 0.9, 1.25, 0.0) and b[6:11] == (5, 12, 0.5, 2.0, 0.0) and len(a) == 13
    calls.clear()
    be.lif_sequence(seq, v, beta=fake(torch.full((4,), 0.9)), v_th=fake(torch.ones(())))
    (name, args), = calls
    assert name == 'be_lif_sg_forward_params' and len(args) == 15
    assert (args[3], args[5]) == (4, 1) and args[10:12] == (5, 12) and args[8].value is None      # periods, T, N; no h_save
    # one file defines both entry points, each once; two floats allocate and copy nothing on their way to the kernel
    text = SOURCE.read_text()
    for entry in ('be_lif_sg_forward', 'be_lif_sg_forward_params'):
        assert len(re.findall(rf'^int {entry}\(', text, flags=re.M)) == 1, entry
    assert 'hipMalloc' not in text and 'hipMemcpy' not in text
