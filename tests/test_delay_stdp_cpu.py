"""Plasticity of delayed synapses without a device: the stacked restatement of tests/delay_stdp_cases.py against a brute-force
loop over the entries, the refusals of ``ValueRing`` and ``DelayedCSR.update_on_pre`` / ``update_on_post`` that are promised before
the first device call, the public names, and the tile constants of ``k_value_ring_push`` that the GPU cases are sized by."""
import re
from pathlib import Path

import numpy as np
import pytest

import delay_cases as DC
import delay_stdp_cases as SC

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['f32', 'f64', 'f16', 'bf16'])
@pytest.mark.parametrize('n_pre,n_post,depth,ring_depth,max_row,steps', [
    (9, 14, 3, 3, 6, 7),            # steps > depth
    (40, 25, 7, 9, 20, 16),         # a ring deeper than the matrix, parallel synapses
    (1, 5, 1, 1, 4, 3),
    (12, 6, 5, 5, 8, 2),            # steps < depth: part of the history is still silent / zero
])
def test_restatement_matches_the_brute_force(n_pre, n_post, depth, ring_depth, max_row, steps, name):
    case = SC.stdp_case(7, n_pre, n_post, depth, max_row, name)
    data, indices, indptr, delays = case
    rows = np.repeat(np.arange(n_pre), np.diff(indptr))
    if n_pre == 40:
        assert len(set(zip(rows.tolist(), indices.tolist()))) < indices.size          # parallel synapses are really there
        assert (np.diff(indptr) == 0).any()                                           # ... and empty rows
    rng = np.random.default_rng(11)
    ring, hist = DC.ring_np(n_pre, ring_depth), SC.value_ring_np(n_pre, ring_depth, name)
    w = data
    for t in range(steps):
        ring.push(rng.random(n_pre) < (0.0 if t == 0 else 0.4))                       # (a silent first step)
        hist.push(rng.normal(size=n_pre))
        post_trace, post_spike = rng.normal(size=n_post), rng.random(n_post) < 0.5
        lo, hi = (None, None) if t % 3 == 0 else ((-0.5, None) if t % 3 == 1 else (-0.5, 0.75))
        a = SC.stacked_on_pre(w, indices, indptr, delays, n_pre, depth, ring, post_trace, name, lo, hi)
        b = SC.brute_on_pre(w, indices, indptr, delays, ring, post_trace, name, lo, hi)
        assert a.dtype == b.dtype == SC.DTYPES[name] and np.array_equal(a, b)
        w = a
        a = SC.stacked_on_post(w, indices, indptr, delays, n_pre, depth, hist, post_spike, name, lo, hi)
        b = SC.brute_on_post(w, indices, indptr, delays, hist, post_spike, name, lo, hi)
        assert np.array_equal(a, b)
        w = a
    assert not np.array_equal(w, data)


def test_value_ring_restatement():
    hist = SC.value_ring_np(4, 3, 'f16')
    assert not hist.by_age().any()
    vs = [np.array([1.0, 2.0, 3.0, 4.0]) * (k + 1) + 1e-4 for k in range(5)]
    for k, v in enumerate(vs):
        hist.push(v)
        assert hist.head == (k + 1) % 3
        for a in range(3):
            want = vs[k - a].astype(np.float32).astype(np.float16) if a <= k else np.zeros(4, np.float16)
            assert np.array_equal(hist.age(a), want)
            assert np.array_equal(hist.aged(np.full(4, a), np.arange(4)), want)          # the device layout agrees with the list
    assert hist.by_age().dtype == np.float16
    assert np.array_equal(SC.to_dtype_np(np.array([1.0 + 2.0 ** -9]), 'bf16'), [1.0]) and SC.to_dtype_np([1.0], 'bf16').dtype == np.float32


def test_add_and_clip_rounds_once():
    w, t = np.array([1.0, 1.0, 0.5], np.float16), np.array([2.0 ** -11, 3 * 2.0 ** -12, 9.0], np.float16)
    # 1 + 2^-11 is a tie in f16 (to even: 1); 1 + 0.75 * 2^-10 rounds up; the third entry is not touched
    got = SC.add_clip_np(w, t, np.array([True, True, False]), 'f16')
    assert np.array_equal(got, np.array([1.0, 1.0 + 2.0 ** -10, 0.5], np.float16))
    got = SC.add_clip_np(np.array([0.25, 0.5], np.float32), np.array([1.0, 1.0], np.float32), np.array([True, False]), 'f32', 0.3, 0.9)
    assert np.array_equal(got, np.array([0.9, 0.5], np.float32))
    got = SC.add_clip_np(np.array([0.25, 0.1], np.float32), np.array([1.0, 1.0], np.float32), np.array([True, False]), 'f32', 0.3)
    assert np.array_equal(got, np.array([1.25, 0.3], np.float32))                        # the clip is over the WHOLE array


def test_gradient_model():
    case = SC.stdp_case(3, 6, 5, 3, 4)
    _, indices, indptr, delays = case
    ring = DC.ring_np(6, 3)
    rng = np.random.default_rng(0)
    for _ in range(4):
        ring.push(rng.random(6) < 0.5)
    g = rng.integers(-64, 65, 5) / 64.0
    grad = SC.brute_grad(indices, indptr, delays, ring, g)
    # the derivative of <g, ring @ D> in w_e, by finite differences of the (linear) product
    w = np.zeros(indices.size)
    for e in range(indices.size):
        w[:] = 0.0
        w[e] = 1.0
        assert grad[e] == g @ DC.delayed_currents_np(w, indices, indptr, delays, ring, 5)


# ---------------------------------------------------------------------------------------------------------------------------
# the package: names and eager validation
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_names(be):
    assert be.ValueRing.__module__ == 'brainevent_amd._delay'
    for name in ('push', 'value', 'by_age', 'reset'):
        assert callable(getattr(be.ValueRing, name))
    for name in ('update_on_pre', 'update_on_post', 'stacked_to_original'):
        assert callable(getattr(be.DelayedCSR, name))
    assert isinstance(be.DelayedCSR.plastic_state, property)
    doc = be.DelayedCSR.__doc__
    assert 'Gradients, STDP on delayed synapses' not in doc


def test_value_ring_refusals_need_no_device(be):
    import torch
    with pytest.raises(ValueError, match='n must be >= 1'):
        be.ValueRing(0, 4)
    with pytest.raises(ValueError, match='depth must be >= 1'):
        be.ValueRing(10, 0)
    with pytest.raises(ValueError, match='below 2\\^31'):
        be.ValueRing(1 << 27, 16)
    with pytest.raises(TypeError, match='dtype'):
        be.ValueRing(10, 4, dtype=torch.int32)


class _Ring:
    """What the methods look at before they touch the device (a ring cannot be built without one)."""

    def __init__(self, cls, n, depth, dtype=None):
        self.__class__ = cls
        self.n, self.depth, self.dtype = n, depth, dtype


def _delayed(be, n_pre=3, n_post=4, depth=2, shared=False):
    """A ``DelayedCSR`` as far as the eager checks look at it: shape, depth, dtype, the shape of the weights."""
    import torch
    D = object.__new__(be.DelayedCSR)
    D.shape, D.depth = (n_pre, n_post), depth
    D.delays = torch.zeros(5, dtype=torch.int32)
    D._data_shape = (1,) if shared else (5,)

    class _St:
        data = torch.zeros(1 if shared else 5, dtype=torch.float32)
        plastic_state = None
    D.stacked = _St()
    return D


def test_update_refusals_need_no_device(be):
    """Every refusal below comes before the first device call: this test runs where there is no GPU."""
    import torch
    D = _delayed(be)
    spikes, hist = _Ring(be.SpikeRing, 3, 2), _Ring(be.ValueRing, 3, 2, torch.float32)
    trace, post = np.zeros(4, np.float32), np.zeros(4, bool)
    # on-pre
    with pytest.raises(TypeError, match='SpikeRing'):
        D.update_on_pre(np.zeros(3, bool), trace)
    with pytest.raises(ValueError, match='4 neurons.*3 rows'):
        D.update_on_pre(_Ring(be.SpikeRing, 4, 2), trace)
    with pytest.raises(ValueError, match='remembers 1 steps.*depth 2'):
        D.update_on_pre(_Ring(be.SpikeRing, 3, 1), trace)
    with pytest.raises(ValueError, match=r'post_trace must have shape \(4,\)'):
        D.update_on_pre(spikes, np.zeros(5, np.float32))
    with pytest.raises(ValueError, match='w_min must be'):
        D.update_on_pre(spikes, trace, w_min='low')
    with pytest.raises(ValueError, match='homogeneous'):
        _delayed(be, shared=True).update_on_pre(spikes, trace)
    # on-post
    with pytest.raises(ValueError, match='holds 4 neurons.*3 rows'):
        D.update_on_post(_Ring(be.ValueRing, 4, 2, torch.float32), post)
    with pytest.raises(ValueError, match='remembers 1 steps.*depth 2'):
        D.update_on_post(_Ring(be.ValueRing, 3, 1, torch.float32), post)
    with pytest.raises(TypeError, match='float16.*float32'):
        D.update_on_post(_Ring(be.ValueRing, 3, 2, torch.float16), post)
    with pytest.raises(ValueError, match=r'must have shape \(2, 3\)'):
        D.update_on_post(np.zeros((3, 3), np.float32), post)
    with pytest.raises(ValueError, match=r'must have shape \(2, 3\)'):
        D.update_on_post(np.zeros(6, np.float32), post)
    with pytest.raises(ValueError, match=r'post_spike must have shape \(4,\)'):
        D.update_on_post(hist, np.zeros(3, bool))
    with pytest.raises(ValueError, match='w_max must be'):
        D.update_on_post(hist, post, w_max=[1.0, 2.0])
    with pytest.raises(ValueError, match='homogeneous'):
        _delayed(be, shared=True).update_on_post(hist, post)
    assert D.plastic_state is None


def test_push_refusals_need_no_device(be):
    import torch
    hist = _Ring(be.ValueRing, 5, 3, torch.float32)
    with pytest.raises(NotImplementedError, match='1-D'):
        hist.push(np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError, match='6 values for a ring of 5'):
        hist.push(np.zeros(6, np.float32))
    with pytest.raises(TypeError, match='float'):
        hist.push(np.zeros(5, np.int32))
    with pytest.raises(TypeError, match='float'):
        hist.push(torch.zeros(5, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'age must lie in \[0, 3\)'):
        hist.value(3)


# ---------------------------------------------------------------------------------------------------------------------------
# the tile constants of k_value_ring_push
# ---------------------------------------------------------------------------------------------------------------------------
PATTERNS = {
    'kValueThreads': r'constexpr\s+int\s+kValueThreads\s*=\s*(\d+)',
    'kValuePer': r'constexpr\s+int\s+kValueThreads\s*=\s*\d+\s*,\s*kValuePer\s*=\s*(\d+)',
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(SC.PUSH_TILES)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_push_constant_matches_the_source(key):
    text = (CSRC / 'be_delay.hip').read_text()
    found = re.findall(PATTERNS[key], text)
    assert found, f"{key}: be_delay.hip no longer holds /{PATTERNS[key]}/ — the GPU cases sized by it need a look"
    assert {int(v) for v in found} == {SC.PUSH_TILES[key]}, f"{key}: be_delay.hip says {found}, tests/delay_stdp_cases.py assumes {SC.PUSH_TILES[key]}"


def test_push_tile_is_derived_as_the_cases_assume():
    text = (CSRC / 'be_delay.hip').read_text()
    assert re.search(r'kValueTile\s*=\s*kValueThreads\s*\*\s*kValuePer\s*;', text)
    assert re.search(r'k_value_ring_push<S, D>\)\s*,\s*dim3\(\(unsigned\)\(\(n \+ kValueTile - 1\) / kValueTile\)\)\s*,\s*dim3\(kValueThreads\)',
                     text)
    assert SC.VALUE_TILE == 4096


def test_aged_kernel_shares_the_walk_of_the_plain_one():
    """One ``k_plast_rows``: the aged update is an instantiation of it (a trace policy), not a copy."""
    text = (CSRC / 'be_plasticity.hip').read_text()
    assert len(re.findall(r'__global__[^;{]*\bk_plast_rows\b', text)) == 1
    assert 'struct TracePlain' in text and 'struct TraceAged' in text and 'be_plasticity_rows_aged' in text
