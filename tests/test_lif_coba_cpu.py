"""The fused COBA / CUBA neuron step without a device: the numpy restatement the GPU tests compare with (tests/lif_coba_cases.py) is
held to the same formulas written as torch CPU elementwise ops (bit for bit) and to an f64 evaluation of the header's formulas
(within a derived rounding bound), the constants the GPU sizes come from are held to the text of csrc/be_neuron.hip, and the
conditions the GPU cases rely on are asserted on the restatement alone.

The one tolerance here, of the f64 comparison: every f32 operation adds ``u |result| + 2**-150`` (``u = 2**-24 (1 + 2**-12)``: half
an ulp, the factor absorbing the second-order terms of the at most 13 operations in a chain; the absolute term is the rounding of
a subnormal result) to the error its operands carry, which passes through a sum as it is and through a product times the other
factor's magnitude."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lif_coba_cases as C
from lif_coba_cases import F, same_bits

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'brainevent_amd' / 'csrc' / 'be_neuron.hip'
HEADER = ROOT / 'include' / 'brainevent_amd.h'


# ------------------------------------------------------------------------------------------------ the constants and the source
def test_constants_match_the_source():
    text = SOURCE.read_text()
    bounds = re.findall(r'__launch_bounds__\((\d+)\)', text)
    blocks = re.findall(r'dim3\(grid\), dim3\((\d+)\)', text)
    grids = re.findall(r'const int grid = \(int\)std::min<int64_t>\(\(n \+ (\d+)\) / (\d+), (\d+)\);', text)
    t, cap = C.CONSTS['threads'], C.CONSTS['grid_cap']
    assert bounds == [str(t)] and blocks == [str(t)] and grids == [(str(t - 1), str(t), str(cap))], (bounds, blocks, grids)
    assert text.count('hipLaunchKernelGGL(') == 1 and text.count('__global__') == 1          # one kernel, one launch site
    assert C.FULL_PASS == t * cap == 524288
    # a word's first lane writes it: the grid stride must be a multiple of the wave, the block of the word
    assert C.FULL_PASS % 64 == 0 and t % 32 == 0
    assert text.count('#pragma clang fp contract(off)') == 1


def test_sizes_follow_the_constants():
    one_word, two_words = C.N_PAST_ONE_PASS
    assert one_word - C.FULL_PASS == 33 and two_words - C.FULL_PASS == 65          # a whole word (two) and a one-bit word
    t = C.CONSTS['threads']
    assert {1, 31, 32, 33, 63, 64, 65, t - 1, t, t + 1} <= set(C.N_SIZES) and max(C.N_SIZES) < C.FULL_PASS
    assert sum(n % 32 != 0 for n in C.N_SIZES) >= 6 and C.MULTI_N % 32 != 0 and C.EDGE_N % 32 != 0 and C.EDGE_N > 32


def test_header_states_the_order_restated():
    """The lines of the header the restatement follows, as they stand there."""
    text = HEADER.read_text()
    for line in ('g_exc = g_exc * decay_exc + in_exc;   g_inh = g_inh * decay_inh + in_inh',
                 'i_syn = (g_exc * (e_exc - v) + g_inh * (e_inh - v)) * syn_scale',
                 'dv    = (-(v - v_rest) + i_syn + i_ext) * (dt / tau_m)',
                 "active = refractory <= 0;  v' = active ? v + dv : v;  spike = active && v' >= v_th",
                 "v = spike ? v_reset : v';  refractory = spike ? t_ref : refractory - dt;",
                 'i_syn = (g_exc + g_inh) * syn_scale',
                 'g = g * decay + in * in_scale, each operation rounded separately'):
        assert text.count(line) == 1, line


def test_params_are_rounded_once():
    p = C.params(dt=0.1, tau_m=20.0, tau_exc=5.0, tau_inh=10.0)
    assert p.f['dt_over_tau'] == F(0.1 / 20.0) and p.f['dt'] == F(0.1) and set(p.f) == set(p.d) - {'tau_m', 'tau_exc', 'tau_inh'} | {'dt_over_tau'}
    assert p.d['decay_exc'] == np.exp(-0.1 / 5.0) and p.f['decay_exc'] == F(np.exp(-0.1 / 5.0))
    assert all(v.dtype == F for v in p.f.values()) and all(isinstance(v, float) for v in p.d.values())
    q = p.scaled(0.6, 6.7)
    assert q.f['in_scale_exc'] == F(0.6) and q.f['in_scale_inh'] == F(6.7) and q.d['dt'] == p.d['dt']
    with pytest.raises(AssertionError):
        C.params(tau=1.0)


# ------------------------------------------------------------------------------------------------ against torch CPU ops
def torch_step(state, in_exc, in_inh, d, current_based):
    """One step as separate torch CPU tensor ops with Python doubles for the constants (examples/cuba_2005.py ``elementwise_step``,
    the loop of test_fused_neuron_step_reproduces_the_elementwise_formulation_bit_for_bit), the inputs given."""
    V, ge, gi, refr = state
    ge = ge * d['decay_exc'] + in_exc * d['in_scale_exc']
    gi = gi * d['decay_inh'] + in_inh * d['in_scale_inh']
    if current_based:
        I_syn = (ge + gi) * d['syn_scale']
    else:
        I_syn = (ge * (d['e_exc'] - V) + gi * (d['e_inh'] - V)) * d['syn_scale']
    dV = (-(V - d['v_rest']) + I_syn + d['i_ext']) * (d['dt'] / d['tau_m'])
    active = refr <= 0
    V = torch.where(active, V + dV, V)
    spk = active & (V >= d['v_th'])
    V = torch.where(spk, torch.full_like(V, d['v_reset']), V)
    refr = torch.where(spk, torch.full_like(refr, d['t_ref']), refr - d['dt'])
    return (V, ge, gi, refr), spk


@pytest.mark.parametrize('current_based,dt', C.MULTI_CASES)
def test_restatement_equals_torch_cpu_ops(current_based, dt):
    p, state, drive = C.multi_step_case(current_based, dt)
    ref = C.run(state, drive, p, current_based)
    t_state = tuple(torch.tensor(a) for a in state)
    for t, ((in_exc, in_inh), (r_state, r_spikes)) in enumerate(zip(drive, ref)):
        t_state, spk = torch_step(t_state, torch.tensor(in_exc), torch.tensor(in_inh), p.d, current_based)
        assert all(a.dtype == torch.float32 for a in t_state) and spk.dtype == torch.bool
        assert np.array_equal(spk.numpy(), r_spikes), t
        for name, got, want in zip(('v', 'g_exc', 'g_inh', 'refractory'), t_state, r_state):
            assert same_bits(got.numpy(), want), (name, t)


@pytest.mark.parametrize('current_based', (0, 1))
def test_edge_slots_equal_torch_cpu_ops(current_based):
    p, state, in_exc, in_inh = C.edge_inputs()
    r_state, r_spikes = C.step(state, in_exc, in_inh, p, current_based)
    t_state, spk = torch_step(tuple(torch.tensor(a) for a in state), torch.tensor(in_exc), torch.tensor(in_inh), p.d, current_based)
    assert np.array_equal(spk.numpy(), r_spikes)
    for name, got, want in zip(('v', 'g_exc', 'g_inh', 'refractory'), t_state, r_state):
        assert same_bits(got.numpy(), want), name


# ------------------------------------------------------------------------------------------------ against f64
U = 2.0 ** -24 * (1 + 2.0 ** -12)
TINY_HALF = 2.0 ** -150


class Tracked:
    """An f64 value and a bound on what the f32 evaluation of the same expression may differ from it by."""

    def __init__(self, value, err=None, rounded=False):
        self.v = np.asarray(value, np.float64)
        self.e = np.zeros_like(self.v) if err is None else err
        if rounded:
            self.e = self.e + U * np.abs(self.v) + TINY_HALF

    def __add__(self, o):
        return Tracked(self.v + o.v, self.e + o.e, rounded=True)

    def __sub__(self, o):
        return Tracked(self.v - o.v, self.e + o.e, rounded=True)

    def __mul__(self, o):
        return Tracked(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e, rounded=True)

    def __neg__(self):
        return Tracked(-self.v, self.e)


def f64_step(state, in_exc, in_inh, p, current_based):
    """The header's formulas in f64 on the f32 constants: ``(g_exc, g_inh, v', spike)``, the first three Tracked."""
    v, ge, gi, r = (Tracked(a) for a in state)
    c = {k: Tracked(np.float64(x)) for k, x in p.f.items()}
    g_e = ge * c['decay_exc'] + Tracked(in_exc) * c['in_scale_exc']
    g_i = gi * c['decay_inh'] + Tracked(in_inh) * c['in_scale_inh']
    if current_based:
        i_syn = (g_e + g_i) * c['syn_scale']
    else:
        i_syn = (g_e * (c['e_exc'] - v) + g_i * (c['e_inh'] - v)) * c['syn_scale']
    dv = (-(v - c['v_rest']) + i_syn + c['i_ext']) * c['dt_over_tau']
    active = r.v <= 0
    stepped = v + dv
    v_new = Tracked(np.where(active, stepped.v, v.v), np.where(active, stepped.e, 0.0))
    return g_e, g_i, v_new, active & (v_new.v >= c['v_th'].v)


@pytest.mark.parametrize('current_based,dt', C.MULTI_CASES)
def test_one_step_within_the_f64_bound(current_based, dt):
    p = C.multi_step_case(current_based, dt)[0]
    state, in_exc, in_inh = C.inputs(4000, seed=3)
    (_, g_exc, g_inh, _), spikes, detail = C.step(state, in_exc, in_inh, p, current_based, detail=True)
    e_exc, e_inh, e_v, e_spikes = f64_step(state, in_exc, in_inh, p, current_based)
    same = spikes == e_spikes
    assert (~same).mean() <= 0.01 and 0.02 < spikes.mean() < 0.98
    for name, got, want in (('g_exc', g_exc, e_exc), ('g_inh', g_inh, e_inh), ('v_new', detail['v_new'], e_v)):
        err = np.abs(got.astype(np.float64) - want.v)[same]
        bound = want.e[same]
        print(f'{name}: max error {err.max():.3e}, bound there {bound[err.argmax()]:.3e}, largest bound {bound.max():.3e}')
        assert (err <= bound).all(), name
        assert bound.max() < 1e-5 * max(1.0, np.abs(want.v).max())          # a rounding bound, not a tolerance


def test_the_f64_comparison_can_fail():
    """A membrane a part in a million off is outside the bound."""
    p = C.multi_step_case(0, 0.1)[0]
    state, in_exc, in_inh = C.inputs(4000, seed=3)
    want = f64_step(state, in_exc, in_inh, p, 0)
    off = C.step((state[0] * F(1 + 1e-6), *state[1:]), in_exc, in_inh, p, 0, detail=True)[2]['v_new']
    assert (np.abs(off.astype(np.float64) - want[2].v) > want[2].e).any()


# ------------------------------------------------------------------------------------------------ what the GPU cases rely on
@pytest.mark.parametrize('current_based,dt', C.MULTI_CASES)
def test_multi_step_case_exercises_the_branches(current_based, dt):
    p, state, drive = C.multi_step_case(current_based, dt)
    out = C.run(state, drive, p, current_based)
    rates = [float(s.mean()) for _, s in out]
    assert all(0 <= r < 1 for r in rates) and sum(0 < r < 1 for r in rates) >= len(rates) / 2
    total = sum(s.astype(np.int64) for _, s in out)
    assert (total >= 2).sum() >= C.MULTI_N / 2
    assert (out[-1][0][3] < 0).any()                                          # a timer that ran on below zero
    # the timers a step read (after the first: what earlier steps wrote) and whether the neuron moved on them
    after = [st[3] for st, _ in out[:-1]]
    came_down = [(a == 0) & (np.signbit(a) == 0) for a in after]
    near_zero = [(a != 0) & (np.abs(a) < 1e-6) for a in after]
    if dt == 0.5:              # t_ref and dt are dyadic: a timer comes down to +0 exactly, and `r <= 0` lets the neuron go on
        assert p.d['t_ref'] / p.d['dt'] == 4.0 and sum(int(z.sum()) for z in came_down) >= C.MULTI_N
        moved = [(out[t + 1][0][0] != out[t][0][0]) & came_down[t] for t in range(len(after))]
        assert sum(int(m.sum()) for m in moved) >= C.MULTI_N / 2
    else:                      # dt = 0.1f is not: the timers pass zero at a few 1e-8 on either side, decided by f32 rounding
        seen = np.concatenate([a[z] for a, z in zip(after, near_zero)])
        assert (seen > 0).any() and (seen < 0).any() and not any(z.any() for z in came_down)
    # the input scales matter: other scales, other spikes
    other = C.run(state, drive, p.scaled(1.0, 1.0), current_based)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(out, other)) or not same_bits(out[-1][0][1], other[-1][0][1])


@pytest.mark.parametrize('current_based', (0, 1))
def test_each_edge_slot_takes_its_branch(current_based):
    p, state, in_exc, in_inh = C.edge_inputs()
    (v, g_exc, g_inh, r), spikes, d = C.step(state, in_exc, in_inh, p, current_based, detail=True)
    k = {name: i for i, name in enumerate(C.EDGE_SLOTS)}
    assert len(k) == len(C.EDGE_SLOTS) == 14 and state[0].size == C.EDGE_N and set(C.EDGE_NON_FINITE) <= set(k)
    v_th, v_reset, t_ref = p.f['v_th'], p.f['v_reset'], p.f['t_ref']
    i = k['on_threshold']
    assert d['v_new'][i] == v_th and spikes[i] and v[i] == v_reset and r[i] == t_ref
    i = k['ulp_under_threshold']
    assert d['v_new'][i] == np.nextafter(v_th, F(-np.inf)) and not spikes[i] and v[i] == d['v_new'][i] and r[i] == F(-0.5)
    for name in ('r_plus_zero', 'r_minus_zero', 'r_negative'):                 # active: the membrane moved
        i = k[name]
        assert d['active'][i] and v[i] != state[0][i] and not spikes[i], name
    assert np.signbit(state[3][k['r_minus_zero']]) and state[3][k['r_minus_zero']] == 0 and r[k['r_negative']] == F(-0.75)
    for name in ('r_subnormal', 'r_inf', 'r_nan'):                             # inactive: it did not, whatever dv is
        i = k[name]
        assert not d['active'][i] and v[i] == state[0][i] and not spikes[i], name
    assert 0 < state[3][k['r_subnormal']] < C.MIN_NORMAL and r[k['r_subnormal']] == F(-0.5)
    assert r[k['r_inf']] == np.inf and np.isnan(r[k['r_nan']])
    i = k['v_nan']
    assert d['active'][i] and np.isnan(v[i]) and not spikes[i] and r[i] == F(-0.5) and np.isfinite(g_exc[i])
    i = k['in_exc_inf']                                                         # the membrane goes to +inf: a spike, and a reset
    assert g_exc[i] == np.inf and d['v_new'][i] == np.inf and spikes[i] and v[i] == v_reset
    i = k['in_inh_nan']
    assert np.isnan(g_inh[i]) and np.isnan(v[i]) and not spikes[i] and np.isfinite(g_exc[i])
    for name in ('g_exc_subnormal', 'g_exc_decays_to_subnormal'):
        i = k[name]
        assert 0 < g_exc[i] < C.MIN_NORMAL and g_exc[i] == F(np.float64(state[1][i]) * np.float64(p.f['decay_exc'])), name
    assert state[1][k['g_exc_subnormal']] < C.MIN_NORMAL <= state[1][k['g_exc_decays_to_subnormal']]
    i = k['in_minus_zero']
    assert p.f['in_scale_exc'] == 1 and g_exc[i] == 0 and np.signbit(g_exc[i])
    # the NaNs and infinities stay in their slots, on the host as well
    q, q_state, q_exc, q_inh = C.edge_inputs(without_non_finite=True)
    (qv, qe, qi, qr), q_spikes = C.step(q_state, q_exc, q_inh, q, current_based)
    keep = np.ones(C.EDGE_N, bool)
    keep[[k[name] for name in C.EDGE_NON_FINITE]] = False
    assert np.isfinite(np.concatenate([qv, qe, qi, qr])).all()
    assert all(same_bits(a[keep], b[keep]) for a, b in zip((v, g_exc, g_inh, r), (qv, qe, qi, qr)))
    assert np.array_equal(spikes[keep], q_spikes[keep])


def test_pack_is_the_inverse_of_unpackbits():
    rng = np.random.default_rng(0)
    for n in C.N_SIZES + (C.MULTI_N, C.EDGE_N, 70001):
        spikes = rng.random(n) < 0.3
        words = C.pack(spikes)
        assert words.dtype == np.uint32 and words.shape == (-(-n // 32),)
        bits = np.unpackbits(words.view(np.uint8), bitorder='little')
        assert np.array_equal(bits[:n].astype(bool), spikes) and not bits[n:].any()
    assert C.pack(np.array([True] + [False] * 30 + [True, True])).tolist() == [0x80000001, 1]
    assert C.pack(np.zeros(0, bool)).shape == (0,)


def test_same_bits_tells_zeros_apart_and_nans_not():
    assert not same_bits(np.array([0.0], F), np.array([-0.0], F)) and same_bits(np.array([np.nan], F), -np.array([np.nan], F))
    assert not same_bits(np.array([1.0], F), np.array([np.nan], F))


# ------------------------------------------------------------------------------------------------ refusals that need no device
def test_refusals_without_a_device(be, monkeypatch):
    from brainevent_amd import _neuron

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron, 'call', no_call)
    z = [torch.zeros(8) for _ in range(6)]
    for step in (be.lif_coba_step, be.lif_cuba_step):
        with pytest.raises(ValueError, match='device tensors'):                # host tensors: there is no CPU implementation
            step(*z, torch.zeros(8, dtype=torch.bool))
