"""The fused COBA / CUBA neuron step (csrc/be_neuron.hip, brainevent_amd/_neuron.py) on the device, by direct C calls with every
output pre-filled with a sentinel.  State, byte spikes, packed words and counts are compared with the numpy restatement of
tests/lif_coba_cases.py as EQUALITIES, bit for bit (``same_bits``); nothing here is compared with torch's device kernels, and there
is no tolerance.  tests/test_lif_coba_cpu.py holds the restatement to torch's CPU ops and to f64, and the sizes used here to the
kernel's source."""
import functools

import numpy as np
import pytest
import torch

import lif_coba_cases as C
from lif_coba_cases import F, same_bits

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
STATE = ('v', 'g_exc', 'g_inh', 'refractory')
REQUIRED = STATE + ('in_exc', 'in_inh')
BYTE_SENTINEL, COUNT_START, EXTRA_WORDS = 7, 3.0, 2
#: entry point -> (current_based, takes spike_bits_out, takes the input scales and the flag)
ENTRY_POINTS = {'be_lif_coba_step': (0, False, False), 'be_lif_coba_step_packed': (0, True, False),
                'be_lif_cuba_step': (1, False, False), 'be_lif_cuba_step_packed': (1, True, False),
                'be_lif_step_scaled_packed': (None, True, True)}


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()          # (a copy: the shared inputs are read-only)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def n_words(n):
    return -(-n // 32)


@functools.lru_cache(maxsize=None)
def case(n, seed):
    state, in_exc, in_inh = C.inputs(n, seed)
    for a in state + (in_exc, in_inh):
        a.setflags(write=False)
    return state, in_exc, in_inh


def device(state, in_exc, in_inh, spikes_dtype=torch.uint8):
    """The arguments of a call as device tensors: copies of the state and the inputs, and the three outputs pre-filled — the byte
    spikes with 7, the words (two more than ceil(n / 32)) with -1, the counts with 3."""
    n = state[0].size
    a = {name: dev(x) for name, x in zip(REQUIRED, state + (in_exc, in_inh))}
    a['spikes'] = torch.full((n,), BYTE_SENTINEL, dtype=torch.uint8, device='cuda').view(spikes_dtype)
    a['bits'] = torch.full((n_words(n) + EXTRA_WORDS,), -1, dtype=torch.int32, device='cuda')
    a['count'] = torch.full((n,), COUNT_START, device='cuda')
    return a


def c_step(name, a, p, current_based=None, n=None, use=('spikes', 'bits', 'count'), **over):
    """Call entry point ``name`` on the tensors of ``a``; the outputs not named in ``use`` go in as NULL.  ``over``: a required
    pointer replaced (``v=None``: NULL), a host double replaced (``dt=0.0``)."""
    from brainevent_amd import _array as A, _lib
    cb, packed, scaled = ENTRY_POINTS[name]
    assert (current_based is not None) == scaled and set(over) <= set(REQUIRED) | set(p.d)
    assert scaled or (p.d['in_scale_exc'] == p.d['in_scale_inh'] == 1.0)
    cb = current_based if scaled else cb
    d = {**p.d, **{k: v for k, v in over.items() if k in p.d}}
    ptrs = [A.ptr(over[k] if k in over else a[k]) for k in REQUIRED]
    outs = [A.ptr(a[k] if k in use else None) for k in (('spikes', 'bits', 'count') if packed else ('spikes', 'count'))]
    reversal = [d['e_exc'], d['e_inh']] if (scaled or not cb) else []
    scalars = [d[k] for k in ('dt', 'tau_m', 'v_rest', 'v_th', 'v_reset', 't_ref')] + reversal + \
              [d[k] for k in ('decay_exc', 'decay_inh', 'i_ext', 'syn_scale')]
    lead, scales = ([int(cb)], [d['in_scale_exc'], d['in_scale_inh']]) if scaled else ([], [])
    n = a['v'].numel() if n is None else n
    return _lib.fn(name)(*lead, *ptrs, *scales, *outs, n, *scalars, A.stream_ptr())


def check(a, ref_state, ref_spikes, use=('spikes', 'bits', 'count'), count_before=None, what=None):
    """The tensors of ``a`` after a call against the restatement; an output that was not given kept its sentinel."""
    n = ref_spikes.size
    for name, ref in zip(STATE, ref_state):
        assert same_bits(host(a[name]), ref), (name, what)
    spikes = host(a['spikes'].view(torch.uint8))
    assert np.array_equal(spikes, ref_spikes.astype(np.uint8) if 'spikes' in use else np.full(n, BYTE_SENTINEL, np.uint8)), ('spikes', what)
    words = host(a['bits']).view(np.uint32)
    kept = words if 'bits' not in use else words[n_words(n):]
    assert words.size == n_words(n) + EXTRA_WORDS and (kept == 0xFFFFFFFF).all(), ('the words past ceil(n / 32)', what)
    if 'bits' in use:              # the bits past n in the last word are 0: pack() leaves them so
        assert np.array_equal(words[:n_words(n)], C.pack(ref_spikes)), ('bits', what)
    before = np.full(n, F(COUNT_START)) if count_before is None else count_before
    after = before + ref_spikes.astype(F) if 'count' in use else before
    assert same_bits(host(a['count']), after), ('count', what)
    return after


def fast(current_based, **kw):
    """The parameters of the multi-step case (a fast membrane: a quarter of the neurons of ``inputs`` spike in one step)."""
    p = C.multi_step_case(current_based, 0.5)[0]
    return C.params(**{**{k: p.d[k] for k in C.DEFAULTS}, **kw})


def packed_name(current_based):
    return 'be_lif_cuba_step_packed' if current_based else 'be_lif_coba_step_packed'


# ======================================================================================================== sizes
@pytest.mark.parametrize('i,n', list(enumerate(C.N_SIZES)))
def test_sizes(i, n):
    """One lane, a word less one, a word, a word and one, the same around a wave and a block, and 4000: bytes and words together.
    The last word's bits past n are 0 and the two words after it keep their sentinel."""
    current_based = i % 2
    p = fast(current_based)
    state, in_exc, in_inh = case(n, seed=n)
    ref_state, ref_spikes = C.step(state, in_exc, in_inh, p, current_based)
    a = device(state, in_exc, in_inh)
    assert c_step('be_lif_step_scaled_packed', a, p, current_based) == OK
    check(a, ref_state, ref_spikes, what=(n, current_based))
    assert n < 255 or 0.05 < ref_spikes.mean() < 0.95


@pytest.mark.parametrize('n', C.N_PAST_ONE_PASS)
@pytest.mark.parametrize('current_based', (0, 1))
def test_past_one_pass_of_the_capped_grid(current_based, n):
    """A second trip of the grid-stride loop, in which the ballot runs with most lanes of the wave out of the loop; two steps, so that
    the state the second trip wrote is read again."""
    assert n > C.FULL_PASS and (n - C.FULL_PASS) % 32 == 1
    p = fast(current_based)
    state, in_exc, in_inh = case(n, seed=5)
    a = device(state, in_exc, in_inh)
    count = None
    for t in range(2):
        state, spikes = C.step(state, in_exc, in_inh, p, current_based)
        a['spikes'].fill_(BYTE_SENTINEL)
        a['bits'].fill_(-1)
        assert c_step('be_lif_step_scaled_packed', a, p, current_based) == OK
        count = check(a, state, spikes, count_before=count, what=(n, current_based, t))
        assert 0.05 < spikes.mean() < 0.95 and spikes[C.FULL_PASS:].any() and not spikes[C.FULL_PASS:].all()


# ======================================================================================================== output forms
@pytest.mark.parametrize('current_based', (0, 1))
def test_output_forms_and_entry_points(current_based):
    """Bytes only, words only, both, with and without the counts, through each entry point that can state the call: the same state
    from the same start, and an output that was not asked for is not written."""
    n = 257
    p = fast(current_based, in_scale_exc=1.0, in_scale_inh=1.0)
    state, in_exc, in_inh = case(n, seed=8)
    ref = C.step(state, in_exc, in_inh, p, current_based)
    assert 0.05 < ref[1].mean() < 0.95
    plain, packed = ('be_lif_cuba_step', 'be_lif_cuba_step_packed') if current_based else ('be_lif_coba_step', 'be_lif_coba_step_packed')
    forms = [('spikes',), ('bits',), ('spikes', 'bits')]
    calls = [(plain, None, ('spikes',))] + [(packed, None, f) for f in forms] + [('be_lif_step_scaled_packed', current_based, f) for f in forms]
    for name, flag, form in calls:
        for counted in (True, False):
            use = form + (('count',) if counted else ())
            a = device(state, in_exc, in_inh)
            assert c_step(name, a, p, flag, use=use) == OK
            check(a, *ref, use=use, what=(name, use))
    # current_based = 1 ignores the reversal potentials
    if current_based:
        a = device(state, in_exc, in_inh)
        assert c_step('be_lif_step_scaled_packed', a, p, 1, e_exc=float('nan'), e_inh=float('nan')) == OK
        check(a, *ref, what='e_exc = e_inh = NaN')
    else:
        assert not same_bits(C.step(state, in_exc, in_inh, fast(0, in_scale_exc=1.0, in_scale_inh=1.0, e_inh=-70.0), 0)[0][0], ref[0][0])
    # the two inputs may be one array
    a = device(state, in_exc, in_inh)
    assert c_step(packed, a, p, in_inh=a['in_exc']) == OK
    check(a, *C.step(state, in_exc, in_exc, p, current_based), what='in_inh is in_exc')


@pytest.mark.parametrize('current_based', (0, 1))
def test_python_wrapper_bool_and_uint8_spikes(current_based):
    """be.lif_coba_step / be.lif_cuba_step with the spikes as uint8 and as bool, with words, without bytes, with input scales."""
    import brainevent_amd as be
    n = 257
    p = fast(current_based)
    assert p.d['in_scale_exc'] != 1.0 and p.d['in_scale_inh'] != 1.0
    kw = {k: p.d[k] for k in C.DEFAULTS if not (current_based and k in ('e_exc', 'e_inh'))}
    step = be.lif_cuba_step if current_based else be.lif_coba_step
    state, in_exc, in_inh = case(n, seed=9)
    ref = C.step(state, in_exc, in_inh, p, current_based)
    for dtype, use in ((torch.uint8, ('spikes', 'bits', 'count')), (torch.bool, ('spikes', 'bits', 'count')), (torch.bool, ('spikes',)),
                       (torch.uint8, ('bits', 'count'))):
        a = device(state, in_exc, in_inh, spikes_dtype=dtype)
        step(*(a[k] for k in REQUIRED), a['spikes'] if 'spikes' in use else None, a['count'] if 'count' in use else None,
             spike_bits=a['bits'] if 'bits' in use else None, **kw)
        check(a, *ref, use=use, what=(dtype, use))


# ======================================================================================================== several steps
@pytest.mark.parametrize('current_based,dt', C.MULTI_CASES)
def test_several_steps(current_based, dt):
    """The multi-step case (every neuron spikes, sits out its refractory period and spikes again; at dt = 0.5 the timers come down to
    exactly 0): state, spikes and words after every step, the counts as the running sum, with the weights as input scales — and with
    the inputs multiplied by the weights on the host in f32 and a scale of 1, which is the same bits."""
    p, state, drive = C.multi_step_case(current_based, dt)
    ref = C.run(state, drive, p, current_based)
    unit = p.scaled(1.0, 1.0)
    a = device(state, *drive[0])
    b = device(state, *drive[0])
    count = np.zeros(C.MULTI_N, F)
    a['count'].zero_()
    b['count'].zero_()
    for t, ((in_exc, in_inh), (r_state, r_spikes)) in enumerate(zip(drive, ref)):
        a['in_exc'].copy_(dev(in_exc))
        a['in_inh'].copy_(dev(in_inh))
        b['in_exc'].copy_(dev(in_exc * p.f['in_scale_exc']))
        b['in_inh'].copy_(dev(in_inh * p.f['in_scale_inh']))
        assert c_step('be_lif_step_scaled_packed', a, p, current_based) == OK
        assert c_step(packed_name(current_based), b, unit) == OK
        check(a, r_state, r_spikes, count_before=count, what=('scaled', t))
        count = check(b, r_state, r_spikes, count_before=count, what=('pre-multiplied', t))
    assert count.max() >= 2 and count.sum() == sum(int(s.sum()) for _, s in ref)


# ======================================================================================================== edge values
@pytest.mark.parametrize('current_based', (0, 1))
def test_edge_values(current_based):
    """v' exactly on the threshold and one ulp under it; a refractory timer of +0, -0, the smallest subnormal, a negative, +inf and
    NaN; a NaN membrane; an infinite and a NaN input; subnormal conductances (the device keeps them: no flush); -0.  Every slot
    equals the restatement's, and the NaNs and infinities leave every other slot, and every other bit of the words, as it is
    without them."""
    p, state, in_exc, in_inh = C.edge_inputs()
    ref = C.step(state, in_exc, in_inh, p, current_based)
    a = device(state, in_exc, in_inh)
    assert c_step(packed_name(current_based), a, p) == OK
    check(a, *ref, what='edge slots')
    k = {name: i for i, name in enumerate(C.EDGE_SLOTS)}
    got = host(a['spikes'])
    assert got[k['on_threshold']] == 1 and got[k['ulp_under_threshold']] == 0 and got[k['in_exc_inf']] == 1
    g_exc = host(a['g_exc'])
    assert 0 < g_exc[k['g_exc_subnormal']] < C.MIN_NORMAL and 0 < g_exc[k['g_exc_decays_to_subnormal']] < C.MIN_NORMAL
    q, q_state, q_exc, q_inh = C.edge_inputs(without_non_finite=True)
    b = device(q_state, q_exc, q_inh)
    assert c_step(packed_name(current_based), b, q) == OK
    check(b, *C.step(q_state, q_exc, q_inh, q, current_based), what='edge slots without the NaNs and infinities')
    keep = np.ones(C.EDGE_N, bool)
    keep[[k[name] for name in C.EDGE_NON_FINITE]] = False
    for name in STATE + ('count',):
        assert same_bits(host(a[name])[keep], host(b[name])[keep]), name
    assert np.array_equal(got[keep], host(b['spikes'])[keep])
    mask = C.pack(keep)
    assert np.array_equal(host(a['bits']).view(np.uint32)[:2] & mask, host(b['bits']).view(np.uint32)[:2] & mask)


# ======================================================================================================== downstream
@pytest.mark.parametrize('current_based', (0, 1))
def test_packed_spikes_feed_a_scatter(current_based):
    """The words as they are written, as the operand of ``@ csr``: equal to the byte spikes' product bit for bit, and both to the host
    product of the restatement's spikes (dyadic weights: the sums are exact in any order)."""
    import brainevent_amd as be
    n, k, n_conn = 70001, 513, 3
    p = fast(current_based)
    state, in_exc, in_inh = case(n, seed=13)
    ref_state, ref_spikes = C.step(state, in_exc, in_inh, p, current_based)
    rng = np.random.default_rng(14)
    indices = rng.integers(0, k, n * n_conn).astype(np.int32)
    weights = (rng.integers(1, 9, n * n_conn) / 8.0).astype(F)
    csr = be.CSR((dev(weights), dev(indices), torch.arange(n + 1, dtype=torch.int32, device='cuda') * n_conn), shape=(n, k))
    a = device(state, in_exc, in_inh, spikes_dtype=torch.bool)
    a['bits'] = torch.full((n_words(n),), -1, dtype=torch.int32, device='cuda')
    assert c_step('be_lif_step_scaled_packed', a, p, current_based) == OK
    assert np.array_equal(host(a['spikes']), ref_spikes) and np.array_equal(host(a['bits']).view(np.uint32), C.pack(ref_spikes))
    from_words = be.BitPackedBinary.from_packed(a['bits'], n) @ csr
    from_bytes = be.BinaryArray(a['spikes']) @ csr
    want = np.zeros(k, np.float64)
    np.add.at(want, indices.reshape(n, n_conn)[ref_spikes].reshape(-1), weights.reshape(n, n_conn)[ref_spikes].reshape(-1).astype(np.float64))
    assert want.max() * 8 < 2 ** 24 and 0.05 < ref_spikes.mean() < 0.95
    assert same_bits(host(from_words), want.astype(F)) and same_bits(host(from_bytes), want.astype(F))


# ======================================================================================================== C error codes
@pytest.mark.parametrize('name', sorted(ENTRY_POINTS))
def test_c_error_codes_then_a_clean_call(name):
    """Every refusal returns BE_ERR_INVALID under the name of the entry point that was called and writes nothing; n = 0 is BE_OK
    whatever the pointers; the call after them is clean."""
    from brainevent_amd import _lib
    cb, packed, scaled = ENTRY_POINTS[name]
    flag = 1 if scaled else None
    current_based = 1 if scaled else cb
    n = 37
    p = fast(current_based, in_scale_exc=1.0, in_scale_inh=1.0)
    state, in_exc, in_inh = case(n, seed=2)
    a = device(state, in_exc, in_inh)
    bad_calls = [dict(n=-1)] + [{k: None} for k in REQUIRED] + [dict(use=('count',))]
    if packed:
        bad_calls += [dict(use=())]
    for key in ('dt', 'tau_m'):
        bad_calls += [{key: 0.0}, {key: -0.0}, {key: -1.0}, {key: float('nan')}]
    for bad in bad_calls:
        assert c_step(name, a, p, flag, **bad) == INVALID, bad
        assert _lib.last_error().startswith(name + ': '), (bad, _lib.last_error())
    messages = set()
    for bad in (dict(n=-1), dict(v=None), dict(dt=0.0)):
        c_step(name, a, p, flag, **bad)
        messages.add(_lib.last_error())
    assert messages == {name + ': n < 0', name + ': null pointer', name + ': dt and tau_m must be positive'}
    # nothing to do: BE_OK and nothing written, whatever the pointers and the scalars
    assert c_step(name, a, p, flag, n=0) == OK
    assert c_step(name, a, p, flag, n=0, use=(), dt=0.0, **{k: None for k in REQUIRED}) == OK
    torch.cuda.synchronize()
    check(a, state, np.zeros(n, bool), use=(), what='after the refusals')
    use = ('spikes', 'bits', 'count') if packed else ('spikes', 'count')
    assert c_step(name, a, p, flag, use=use) == OK
    check(a, *C.step(state, in_exc, in_inh, p, current_based), use=use, what='the clean call')


# ======================================================================================================== Python refusals
def test_python_refusals(monkeypatch):
    import brainevent_amd as be
    from brainevent_amd import _neuron

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron, 'call', no_call)
    n = 64
    for step in (be.lif_coba_step, be.lif_cuba_step):
        def good():
            return ([torch.zeros(n, device='cuda') for _ in REQUIRED],
                    dict(spikes=torch.zeros(n, dtype=torch.bool, device='cuda'), spike_count=torch.zeros(n, device='cuda'),
                         spike_bits=torch.zeros(2, dtype=torch.int32, device='cuda')))

        def refused(match, args, kw):
            with pytest.raises(ValueError, match=match):
                step(*args, **kw)
        for i in range(len(REQUIRED)):
            for wrong in (torch.zeros(n, dtype=torch.float64, device='cuda'), torch.zeros(n, dtype=torch.float16, device='cuda'),
                          torch.zeros(n), torch.zeros(n + 1, device='cuda'), torch.zeros(n - 1, device='cuda'),
                          torch.zeros(2 * n, device='cuda')[::2], torch.zeros(n, 2, device='cuda')[:, 0]):
                args, kw = good()
                args[i] = wrong
                refused('contiguous f32 device tensors of one length', args, kw)
        for key, match, wrongs in (
                ('spikes', 'spikes must be a contiguous bool / uint8 device tensor',
                 (torch.zeros(n, dtype=torch.int32, device='cuda'), torch.zeros(n, dtype=torch.int8, device='cuda'),
                  torch.zeros(n, device='cuda'), torch.zeros(n - 1, dtype=torch.bool, device='cuda'),
                  torch.zeros(n + 1, dtype=torch.uint8, device='cuda'), torch.zeros(n, dtype=torch.bool),
                  torch.zeros(2 * n, dtype=torch.bool, device='cuda')[::2])),
                ('spike_bits', 'spike_bits must be a contiguous int32 device tensor',
                 (torch.zeros(1, dtype=torch.int32, device='cuda'), torch.zeros(2, dtype=torch.int64, device='cuda'),
                  torch.zeros(8, dtype=torch.uint8, device='cuda'), torch.zeros(2, device='cuda'), torch.zeros(2, dtype=torch.int32),
                  torch.zeros(4, dtype=torch.int32, device='cuda')[::2])),
                ('spike_count', 'spike_count must be a contiguous f32 device tensor',
                 (torch.zeros(n, dtype=torch.float64, device='cuda'), torch.zeros(n, dtype=torch.int32, device='cuda'),
                  torch.zeros(n + 1, device='cuda'), torch.zeros(n), torch.zeros(n, 2, device='cuda')[:, 0],       # a column: its base
                  torch.zeros(2 * n, device='cuda')[::2]))):                       # pointer is the matrix's, the kernel would add there
            for wrong in wrongs:
                args, kw = good()
                kw[key] = wrong
                refused(match, args, kw)
        args, kw = good()
        refused('give spikes, spike_bits or both', args, dict(spike_count=kw['spike_count']))
        refused('give spikes, spike_bits or both', args, {})
        # 65 neurons need three words
        refused('spike_bits must', [torch.zeros(n + 1, device='cuda') for _ in REQUIRED], dict(spike_bits=good()[1]['spike_bits']))


def test_a_contiguous_slice_of_the_counts_is_taken():
    """What the refusal of a strided spike_count leaves: a contiguous slice is added into where it lies, and nowhere else."""
    import brainevent_amd as be
    n = 37
    p = fast(0)
    state, in_exc, in_inh = case(n, seed=2)
    ref_state, ref_spikes = C.step(state, in_exc, in_inh, p, 0)
    a = device(state, in_exc, in_inh)
    counts = torch.full((3, n), COUNT_START, device='cuda')
    be.lif_coba_step(*(a[k] for k in REQUIRED), None, counts[1], spike_bits=a['bits'], **{k: p.d[k] for k in C.DEFAULTS})
    want = np.full((3, n), F(COUNT_START))
    want[1] += ref_spikes
    assert ref_spikes.any() and same_bits(host(counts), want)
    a['count'] = counts[1]
    check(a, ref_state, ref_spikes, use=('bits', 'count'))
