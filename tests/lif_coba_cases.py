"""Shared by tests/test_lif_coba_cpu.py and tests/test_lif_coba_gpu.py: a numpy restatement of the fused COBA / CUBA neuron step
(include/brainevent_amd.h, be_lif_coba_step ... be_lif_step_scaled_packed; csrc/be_neuron.hip), the CONSTS table the GPU sizes are
taken from (the CPU test holds it against the source text), and the inputs of the cases.

The restatement works on ``np.float32`` arrays with ``np.float32`` constants, one operation per statement in the header's order:
every one of them (add, subtract, multiply, negate, compare, select) is correctly rounded in IEEE 754 binary32 on the host and
on the device, subnormal operands and results included, so the device results are compared with it as equalities
(:func:`same_bits`: any NaN stands for any NaN, everything else bit for bit, signed zeros included)."""
import math

import numpy as np

from lif_sg_cases import F, same_bits  # noqa: F401  (same_bits: re-exported to the two test modules)

#: the launch shape of csrc/be_neuron.hip: blocks of ``threads`` lanes, at most ``grid_cap`` of them, a grid-stride loop beyond
CONSTS = {'threads': 256, 'grid_cap': 2048}
#: the neurons one trip of the capped grid covers
FULL_PASS = CONSTS['threads'] * CONSTS['grid_cap']
#: the second trip holds one whole word and a one-bit word / two whole words and a one-bit word
N_PAST_ONE_PASS = (FULL_PASS + 33, FULL_PASS + 64 + 1)
N_SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4000)

#: the scalar arguments of a call in the C order (be_lif_step_scaled_packed has them all; decay_* = exp(-dt / tau_*))
DEFAULTS = dict(dt=0.1, tau_m=20.0, v_rest=-60.0, v_th=-50.0, v_reset=-60.0, t_ref=5.0, e_exc=0.0, e_inh=-80.0, tau_exc=5.0,
                tau_inh=10.0, i_ext=20.0, syn_scale=1e-3, in_scale_exc=1.0, in_scale_inh=1.0)


class Params:
    """``d``: the host doubles a caller passes (``decay_*`` formed in double by the caller); ``f``: the f32 constants the kernel
    works with, derived as ``lif_step<CUBA>`` derives them: ``dt / tau_m`` formed in double and rounded once, every other one a
    single ``(float)`` cast."""

    def __init__(self, **kw):
        assert set(kw) <= set(DEFAULTS), sorted(set(kw) - set(DEFAULTS))
        d = {k: float(v) for k, v in {**DEFAULTS, **kw}.items()}
        d['decay_exc'] = math.exp(-d['dt'] / d['tau_exc'])
        d['decay_inh'] = math.exp(-d['dt'] / d['tau_inh'])
        self.d = d
        self.f = {k: F(d[k]) for k in ('dt', 'v_rest', 'v_th', 'v_reset', 't_ref', 'e_exc', 'e_inh', 'decay_exc', 'decay_inh', 'i_ext',
                                       'syn_scale', 'in_scale_exc', 'in_scale_inh')}
        self.f['dt_over_tau'] = F(d['dt'] / d['tau_m'])

    def scaled(self, in_scale_exc, in_scale_inh):
        """The same call with other input scales."""
        return Params(**{**{k: self.d[k] for k in DEFAULTS}, 'in_scale_exc': in_scale_exc, 'in_scale_inh': in_scale_inh})

    def __repr__(self):
        return f'Params({ {k: self.d[k] for k in DEFAULTS if self.d[k] != DEFAULTS[k]} })'


def params(**kw):
    return Params(**kw)


def step(state, in_exc, in_inh, p, current_based, detail=False):
    """``state = (v, g_exc, g_inh, refractory)``, f32 ``[n]`` each -> ``(state', spikes bool[n])``; nothing is changed in place.
    ``detail``: also the dict of the intermediates (``v_new``: the membrane before the reset)."""
    v, ge, gi, r = state
    assert all(a.dtype == F and a.shape == v.shape and a.ndim == 1 for a in (v, ge, gi, r, in_exc, in_inh))
    c = p.f
    with np.errstate(all='ignore'):
        ge_d = ge * c['decay_exc']
        ie_s = in_exc * c['in_scale_exc']
        g_e = ge_d + ie_s
        gi_d = gi * c['decay_inh']
        ii_s = in_inh * c['in_scale_inh']
        g_i = gi_d + ii_s
        if current_based:
            g_sum = g_e + g_i
            i_syn = g_sum * c['syn_scale']
            parts = (g_sum,)
        else:
            d_e = c['e_exc'] - v
            d_i = c['e_inh'] - v
            p_e = g_e * d_e
            p_i = g_i * d_i
            p_sum = p_e + p_i
            i_syn = p_sum * c['syn_scale']
            parts = (d_e, d_i, p_e, p_i, p_sum)
        d_rest = v - c['v_rest']
        leak = -d_rest
        a_syn = leak + i_syn
        a_ext = a_syn + c['i_ext']
        dv = a_ext * c['dt_over_tau']
        active = r <= F(0)
        v_step = v + dv
        v_new = np.where(active, v_step, v)
        spike = active & (v_new >= c['v_th'])
        v_out = np.where(spike, c['v_reset'], v_new)
        r_less = r - c['dt']
        r_out = np.where(spike, c['t_ref'], r_less)
    every = (ge_d, ie_s, g_e, gi_d, ii_s, g_i, i_syn, d_rest, leak, a_syn, a_ext, dv, v_step, v_new, v_out, r_less, r_out) + parts
    assert all(a.dtype == F for a in every) and active.dtype == spike.dtype == np.bool_
    out = ((v_out, g_e, g_i, r_out), spike)
    if detail:
        return out + (dict(g_exc=g_e, g_inh=g_i, i_syn=i_syn, dv=dv, active=active, v_new=v_new),)
    return out


def run(state, drive, p, current_based):
    """``drive``: a list of ``(in_exc, in_inh)``, one per step -> the list of ``(state', spikes)`` after every step."""
    out = []
    for in_exc, in_inh in drive:
        state, spikes = step(state, in_exc, in_inh, p, current_based)
        out.append((state, spikes))
    return out


def pack(spikes):
    """bool ``[n]`` -> uint32 ``[ceil(n / 32)]``: bit ``i % 32`` of word ``i // 32``, zero past ``n``."""
    spikes = np.asarray(spikes)
    assert spikes.dtype == np.bool_ and spikes.ndim == 1
    words = -(-spikes.size // 32)
    padded = np.zeros(words * 32, np.uint32)
    padded[:spikes.size] = spikes
    return (padded.reshape(words, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)


def inputs(n, seed):
    """Seeded ``(state, in_exc, in_inh)``: membranes on both sides of where one step reaches the threshold, conductances in (0, 1), a
    fifth of the neurons refractory, the inputs small integer counts."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-62.0, -49.5, n).astype(F)
    g_exc, g_inh = rng.uniform(0.0, 1.0, n).astype(F), rng.uniform(0.0, 1.0, n).astype(F)
    refractory = np.where(rng.random(n) < 0.2, F(1), F(0)).astype(F)
    return (v, g_exc, g_inh, refractory), rng.integers(0, 6, n).astype(F), rng.integers(0, 3, n).astype(F)


# ---------------------------------------------------------------------------------------------------- the multi-step case
MULTI_N = 257
#: dt -> (t_ref, steps): 0.5 and 2.0 are dyadic, a refractory timer then comes down to exactly 0; 0.1 is not
MULTI_DT = {0.5: (2.0, 24), 0.1: (0.5, 72)}
#: the CUBA network's inhibitory weight is -9.0 in the reference's example; under this drive that silences most neurons after their
#: first spike, so the case weakens it (at -1.0 a neuron spikes the moment it is active again: no timer stays negative)
MULTI_CUBA_W_INH = -3.0


def multi_step_case(current_based, dt):
    """``(p, state, drive)``: a fast membrane (tau_m = 2 ms) under the networks' drive, so that a neuron spikes, sits out its
    refractory period and spikes again within the case; the inputs are counts, the weights are the input scales."""
    t_ref, steps = MULTI_DT[dt]
    if current_based:
        p = params(dt=dt, tau_m=2.0, t_ref=t_ref, v_rest=-49.0, syn_scale=1.0, in_scale_exc=1.62, in_scale_inh=MULTI_CUBA_W_INH)
    else:
        p = params(dt=dt, tau_m=2.0, t_ref=t_ref, in_scale_exc=0.6, in_scale_inh=6.7)
    state, _, _ = inputs(MULTI_N, seed=11 + int(current_based))
    rng = np.random.default_rng(100 + int(current_based))
    drive = [(rng.integers(0, 6, MULTI_N).astype(F), rng.integers(0, 3, MULTI_N).astype(F)) for _ in range(steps)]
    return p, state, drive


MULTI_CASES = [(cb, dt) for cb in (0, 1) for dt in MULTI_DT]


# ---------------------------------------------------------------------------------------------------- edge values
#: the parameters of the edge case: dt / tau_m = 0.25 and in_scale = 1.0 exactly; one set for COBA and CUBA (a slot without
#: conductance and input has i_syn = 0 in both)
EDGE_PARAMS = dict(dt=0.5, tau_m=2.0, t_ref=2.0)
EDGE_SLOTS = ('on_threshold', 'ulp_under_threshold', 'r_plus_zero', 'r_minus_zero', 'r_subnormal', 'r_negative', 'r_inf', 'r_nan',
              'v_nan', 'in_exc_inf', 'in_inh_nan', 'g_exc_subnormal', 'g_exc_decays_to_subnormal', 'in_minus_zero')
#: the slots that hold a NaN or an infinity (a run with these put back to the plain slot leaves every other slot as it was)
EDGE_NON_FINITE = ('r_inf', 'r_nan', 'v_nan', 'in_exc_inf', 'in_inh_nan')
EDGE_N = 37          # the named slots, then plain ones: two words, the second one partial
TINY = F(2.0 ** -149)           # the smallest positive subnormal
MIN_NORMAL = F(2.0 ** -126)


def _membrane_reaching(target, p):
    """The f32 membrane from which one step without conductance or input lands on ``target`` exactly: ``v' = v + (-(v - v_rest) +
    0 + i_ext) * dt_over_tau`` rises by about 0.75 ulp per ulp of v, so every f32 near the threshold is reached by some v."""
    c = p.f
    guess = (float(target) - float(c['dt_over_tau']) * (float(c['v_rest']) + float(c['i_ext']))) / (1.0 - float(c['dt_over_tau']))
    v = np.full(65, F(guess), F)
    for k in range(32):
        v[33 + k] = np.nextafter(v[32 + k], F(np.inf))
        v[31 - k] = np.nextafter(v[32 - k], F(-np.inf))
    zeros = np.zeros(65, F)
    landed = step((v, zeros, zeros, zeros), zeros, zeros, p, 0, detail=True)[2]['v_new']
    hit = np.flatnonzero(landed == target)
    assert hit.size, (target, guess)
    return v[hit[0]]


def edge_inputs(without_non_finite=False):
    """``(p, state, in_exc, in_inh)`` of EDGE_N slots: slot ``EDGE_SLOTS.index(name)`` is the one named, the others are plain (active,
    finite, below the threshold)."""
    p = params(**EDGE_PARAMS)
    n = EDGE_N
    v, g_exc, g_inh, r = np.full(n, F(-55), F), np.full(n, F(0.3), F), np.full(n, F(0.2), F), np.zeros(n, F)
    in_exc, in_inh = np.ones(n, F), np.zeros(n, F)
    v[len(EDGE_SLOTS):] = np.linspace(-59.0, -52.0, n - len(EDGE_SLOTS)).astype(F)
    k = {name: i for i, name in enumerate(EDGE_SLOTS)}

    def quiet(i):          # no conductance, no input: i_syn = 0
        g_exc[i] = g_inh[i] = in_exc[i] = in_inh[i] = 0
    for name, target in (('on_threshold', p.f['v_th']), ('ulp_under_threshold', np.nextafter(p.f['v_th'], F(-np.inf)))):
        quiet(k[name])
        v[k[name]] = _membrane_reaching(target, p)
    r[k['r_plus_zero']], r[k['r_minus_zero']], r[k['r_subnormal']], r[k['r_negative']] = F(0.0), F(-0.0), TINY, F(-0.25)
    r[k['r_inf']], r[k['r_nan']] = F(np.inf), F(np.nan)
    v[k['v_nan']] = F(np.nan)
    in_exc[k['in_exc_inf']] = F(np.inf)
    in_inh[k['in_inh_nan']] = F(np.nan)
    quiet(k['g_exc_subnormal'])
    g_exc[k['g_exc_subnormal']] = F(2.0 ** -140) * F(3)
    quiet(k['g_exc_decays_to_subnormal'])
    g_exc[k['g_exc_decays_to_subnormal']] = MIN_NORMAL * F(1.0625)
    quiet(k['in_minus_zero'])
    g_exc[k['in_minus_zero']] = in_exc[k['in_minus_zero']] = F(-0.0)
    if without_non_finite:
        for name in EDGE_NON_FINITE:
            i = k[name]
            v[i], r[i], in_exc[i], in_inh[i] = F(-55), F(0), F(1), F(0)
    return p, (v, g_exc, g_inh, r), in_exc, in_inh
