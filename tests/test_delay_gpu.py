"""Synaptic delays on the device (csrc/be_delay.hip through ``SpikeRing`` / ``DelayedCSR``) against the numpy restatement of
tests/delay_cases.py, which tests/test_delay_cpu.py holds to a brute-force dense evaluation.

The split and the ring are compared exactly (integers).  The products are compared exactly too: the generator's weights are
multiples of 1/64 (small integers for f16) whose partial sums are exact in the weight dtype in any order — see the docstring of
tests/delay_cases.py — so every ``assert_equal`` below is an equality, on the direct route (float atomics) as on the fixed-point
routes.  Sizes follow ``delay_cases.TILES``: 64-entry chunks and the 256-entry step of a split workgroup, 8192 bits per ring
workgroup, 16384 rows per pass of the split's grid."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
import brainevent_amd._csr as C
import delay_cases as DC

pytestmark = pytest.mark.gpu

RING_SIZES = [1, 31, 32, 33, DC.RING_TILE_BITS, DC.RING_TILE_BITS + 1]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def build(case, shape, depth, indptr_dtype=np.int32):
    data, indices, indptr, delays = case
    return be.DelayedCSR((dev(data), dev(indices), dev(indptr.astype(indptr_dtype)), dev(delays)), shape=shape, depth=depth)


def check_split(D, indices, indptr, delays, m, depth, want_dtype=torch.int32):
    indptr_s, perm, row_mask = DC.split_by_delay_np(indptr, delays, m, depth)
    st = D.stacked
    assert st.shape == (depth * m, D.shape[1]) and st.indptr.dtype == want_dtype and D.perm.dtype == want_dtype
    np.testing.assert_array_equal(host(st.indptr), indptr_s)
    np.testing.assert_array_equal(host(D.perm), perm)
    np.testing.assert_array_equal(host(st.indices), np.asarray(indices).reshape(-1)[perm])
    np.testing.assert_array_equal(host(D.row_mask).view(np.uint32), row_mask)
    np.testing.assert_array_equal(host(D.delays), np.asarray(delays).reshape(-1))


# ---------------------------------------------------------------------------------------------------------------------------
# split
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', ['random', 'equal', 'ends', 'sorted', 'reversed'])
@pytest.mark.parametrize('depth', [1, 2, 7, 256])
def test_split_is_the_stable_sort(depth, pattern):
    lens, indptr = DC.row_lengths_case(11)
    assert set(lens) >= {0, 1, 63, 64, 65, 257, 2 * DC.SPLIT_TILE + 3}
    m, n_post = len(lens), 1000
    nnz = int(indptr[-1])
    rng = np.random.default_rng(depth)
    indices = rng.integers(0, n_post, nnz).astype(np.int32)
    data = (rng.integers(-64, 65, nnz) / 64.0).astype(np.float32)
    delays = DC.delay_pattern(pattern, 17 + depth, indptr, depth)
    for dt, want in ((np.int32, torch.int32), (np.int64, torch.int64)):
        D = build((data, indices, indptr, delays), (m, n_post), depth, indptr_dtype=dt)
        check_split(D, indices, indptr, delays, m, depth, want)
        np.testing.assert_array_equal(host(D.stacked.data), data[DC.split_by_delay_np(indptr, delays, m, depth)[1]])
        np.testing.assert_array_equal(host(D.data), data)            # ... and back in the original order


def test_split_of_fixed_length_rows_and_of_one_row():
    rng = np.random.default_rng(3)
    n_pre, K, n_post, depth = 37, 65, 400, 7
    indices = rng.integers(0, n_post, (n_pre, K)).astype(np.int32)
    data = (rng.integers(-64, 65, (n_pre, K)) / 64.0).astype(np.float32)
    delays = rng.integers(0, depth, (n_pre, K)).astype(np.int32)
    indptr = np.arange(n_pre + 1) * K
    for D in (be.DelayedCSR((dev(data), dev(indices), None, dev(delays)), shape=(n_pre, n_post), depth=depth),
              be.FixedNumPerPre((dev(data), dev(indices)), shape=(n_pre, n_post)).with_delays(dev(delays.astype(np.int64)), depth)):
        assert isinstance(D.stacked, be.CSR)
        check_split(D, indices, indptr, delays, n_pre, depth)
        np.testing.assert_array_equal(host(D.data), data)
    # m = 1: one row, longer than two workgroup steps
    L = 2 * DC.SPLIT_TILE + 3
    indptr1 = np.array([0, L], np.int32)
    idx1, d1 = rng.integers(0, n_post, L).astype(np.int32), DC.delay_pattern('reversed', 4, indptr1, 5)
    D = be.CSR((dev(np.ones(L, np.float32)), dev(idx1), dev(indptr1)), shape=(1, n_post)).with_delays(d1.astype(np.int16), 5)
    check_split(D, idx1, indptr1, d1, 1, 5)


def test_split_past_one_pass_of_its_grid():
    """More rows than the split's (and the row-mask kernel's) grid covers at once: the grid-stride loops come round."""
    rng = np.random.default_rng(8)
    m, n_post, depth = DC.SPLIT_ROWS_PER_PASS + 5, 64, 3
    lens = rng.integers(0, 4, m)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(indptr[-1])
    indices, delays = rng.integers(0, n_post, nnz).astype(np.int32), rng.integers(0, depth, nnz).astype(np.int32)
    D = build((np.ones(1, np.float32), indices, indptr, delays), (m, n_post), depth)
    check_split(D, indices, indptr, delays, m, depth)
    assert D.stacked.data.numel() == 1                   # one shared weight stays shared


def test_delay_out_of_range_is_refused_and_the_flag_does_not_stick():
    lens, indptr = DC.row_lengths_case(2)
    m, n_post, depth = len(lens), 50, 7
    nnz = int(indptr[-1])
    rng = np.random.default_rng(1)
    indices, data = rng.integers(0, n_post, nnz).astype(np.int32), np.ones(nnz, np.float32)
    good = DC.delay_pattern('random', 5, indptr, depth)
    for pos, value in ((nnz - 3, -1), (200, depth), (0, 1000)):
        bad = good.copy()
        bad[pos] = value
        with pytest.raises(ValueError, match=rf'delays\[{pos}\] = {value} '):
            build((data, indices, indptr, bad), (m, n_post), depth)
    bad = good.copy()
    bad[[700, 90, 400]] = [-5, depth, depth + 1]
    with pytest.raises(ValueError, match=r'delays\[90\]'):            # the first offending position
        build((data, indices, indptr, bad), (m, n_post), depth)
    check_split(build((data, indices, indptr, good), (m, n_post), depth), indices, indptr, good, m, depth)


# ---------------------------------------------------------------------------------------------------------------------------
# ring: push, events
# ---------------------------------------------------------------------------------------------------------------------------
def _spike_vector(rng, n, kind):
    s = rng.random(n) < 0.3
    if kind == 'bool':
        return s, dev(s)
    if kind == 'float':          # negatives and zeros are inactive
        v = np.where(s, rng.random(n) + 0.25, -rng.random(n) * (rng.random(n) < 0.5)).astype(np.float32)
        return s, dev(v)
    nw = (n + 31) // 32          # packed words with every bit past n SET: the push has to clear them
    full = np.ones(nw * 32, bool)
    full[:n] = s
    words = dev(DC.pack_rows_np(full)[0].view(np.int32))
    return s, be.BitPackedBinary.from_packed(words, n)


@pytest.mark.parametrize('kind', ['bool', 'float', 'packed'])
@pytest.mark.parametrize('n', RING_SIZES)
def test_push_and_events(n, kind):
    depth = 3
    rng = np.random.default_rng(n)
    ring, ref = be.SpikeRing(n, depth), DC.ring_np(n, depth)
    assert ring.bits.dtype == torch.int32 and tuple(ring.bits.shape) == (depth, (n + 31) // 32) and not ring.bits.any()
    assert ring.head.dtype == torch.int32 and tuple(ring.head.shape) == (1,) and ring.head.device == ring.bits.device
    for a in range(depth):                                   # history before the first push is silent
        assert not host(ring.events(a).value).any()
    for t in range(depth + 3):
        s, payload = _spike_vector(rng, n, kind)
        ring.push(payload)
        ref.push(s)
        assert int(ring.head) == (t + 1) % depth
        for a in range(depth):
            np.testing.assert_array_equal(host(ring.events(a).value).astype(bool), ref.age(a))
        for slot in host(ring.bits):
            assert not DC.unpack_words_np(slot, n)[n:].any()          # bits past n stay zero in every slot
    ring.reset()
    assert not ring.bits.any() and int(ring.head) == 0


def test_push_takes_the_library_containers_and_numpy():
    n, depth = 100, 4
    rng = np.random.default_rng(0)
    ring, ref = be.SpikeRing(n, depth), DC.ring_np(n, depth)
    s = [rng.random(n) < 0.5 for _ in range(4)]
    for payload, v in ((s[0], s[0]), (be.BinaryArray(dev(s[1])), s[1]), (be.BitPackedBinary(dev(s[2])), s[2]),
                       (be.BinaryArray(s[3].astype(np.int8)), s[3])):
        ring.push(payload)
        ref.push(v)
    for a in range(depth):
        np.testing.assert_array_equal(host(ring.events(a).value).astype(bool), ref.age(a))
    with pytest.raises(ValueError):
        ring.push(np.zeros(n + 1, bool))
    with pytest.raises(NotImplementedError):
        ring.push(np.zeros((2, n), bool))


# ---------------------------------------------------------------------------------------------------------------------------
# ring: compaction
# ---------------------------------------------------------------------------------------------------------------------------
def _ids_of(op):
    c = int(op.count)
    return np.sort(host(op.ids)[:c].astype(np.int64)), c


@pytest.mark.parametrize('masked', [False, True], ids=['all', 'masked'])
@pytest.mark.parametrize('depth', [1, 3, 256])
@pytest.mark.parametrize('n', RING_SIZES)
def test_compaction(n, depth, masked):
    rng = np.random.default_rng(1000 * depth + n)
    ring, ref = be.SpikeRing(n, depth), DC.ring_np(n, depth)
    nw = (n + 31) // 32
    mask_np = rng.integers(0, 2 ** 32, (depth, nw), dtype=np.uint64).astype(np.uint32) if masked else None
    mask = dev(mask_np.view(np.int32)) if masked else None
    ids, c = _ids_of(ring.ids(row_mask=mask))
    assert c == 0                                               # a silent ring
    for _ in range(depth + 2):
        s = rng.random(n) < 0.3
        ring.push(dev(s))
        ref.push(s)
    op = ring.ids(row_mask=mask)
    assert op.n == depth * n and op.ids.dtype == torch.int32 and op.ids.numel() == depth * n
    ids, c = _ids_of(op)
    want = ref.ids(row_mask=mask_np)
    np.testing.assert_array_equal(ids, want)                    # each id once, none missing, all < depth * n
    ids2, c2 = _ids_of(ring.ids(row_mask=mask))                 # no push in between: count was re-armed
    assert c2 == c
    np.testing.assert_array_equal(ids2, want)
    assert ring.ids(row_mask=mask) is op                        # steady state: the same operand over the same buffers
    if depth > 1:                                               # fewer ages than the ring remembers
        np.testing.assert_array_equal(_ids_of(ring.ids(ages=depth - 1, row_mask=mask))[0], ref.ids(depth - 1, mask_np))
    for _ in range(depth):
        ring.push(dev(np.ones(n, bool)))
    ids, c = _ids_of(ring.ids())
    assert c == depth * n
    np.testing.assert_array_equal(ids, np.arange(depth * n))


# ---------------------------------------------------------------------------------------------------------------------------
# product
# ---------------------------------------------------------------------------------------------------------------------------
N_PRE, N_POST, DEPTH, RATE = 70, 300, 7, 0.2
WEIGHTS = {'f32': dict(dtype=np.float32), 'f64': dict(dtype=np.float64), 'shared': dict(dtype=np.float32, homo=True),
           'f16': dict(dtype=np.float16)}


def _route(D, route):
    """``direct``: nothing prepared, a matrix this small takes the direct kernel; ``prepared``: ``D.prepare()``, the router's
    choice; ``plan`` / ``binned``: that workspace installed, as tests/test_event_encodings_gpu.py does for a plain CSR."""
    st = D.stacked
    if route == 'prepared':
        assert D.prepare() is D and 'scatter_plan' in st.buffers
    elif route == 'plan':
        st.buffers['scatter_plan'] = C.ScatterPlan.build(st.data, st.indices, st.indptr, shape=st.shape)
    elif route == 'binned':
        st.buffers['scatter_plan'] = C.BinnedScatter(st.data, st.shape[0], st.shape[1], st.nse, indices=st.indices,
                                                     indptr=st.indptr)
    return D


def _run_and_compare(D, case, n_pre, n_post, depth, steps, seed=9, rate=RATE):
    data, indices, indptr, delays = case
    rng = np.random.default_rng(seed)
    ring, ref = be.SpikeRing(n_pre, depth), DC.ring_np(n_pre, depth)
    for t in range(steps):
        s = rng.random(n_pre) < rate
        ring.push(dev(s))
        ref.push(s)
        got = ring @ D
        assert isinstance(got, torch.Tensor) and got.dtype == D.dtype and tuple(got.shape) == (n_post,)
        want = DC.delayed_currents_np(data, indices, indptr, delays, ref, n_post)
        np.testing.assert_array_equal(host(got).astype(np.float64), want, err_msg=f'step {t}')
    return ring, ref


@pytest.mark.parametrize('route', ['direct', 'prepared'])
@pytest.mark.parametrize('weights', sorted(WEIGHTS))
def test_product_every_weight_kind(weights, route):
    case = DC.exact_case(21, N_PRE, N_POST, DEPTH, 32, parallel=True, **WEIGHTS[weights])
    D = _route(build(case, (N_PRE, N_POST), DEPTH), route)
    assert D.stacked.data.numel() == (1 if weights == 'shared' else case[1].size)
    ring, _ = _run_and_compare(D, case, N_PRE, N_POST, DEPTH, 2 * DEPTH + 1)
    # no id of an empty stacked row reaches the scatter
    ids, _ = _ids_of(ring.ids(ages=DEPTH, row_mask=D.row_mask))
    ptr = host(D.stacked.indptr)
    assert ids.size and (ptr[ids + 1] > ptr[ids]).all()
    unmasked, _ = _ids_of(ring.ids(ages=DEPTH))
    assert set(ids) <= set(unmasked) and ids.size < unmasked.size          # the rows of 0 entries fired too


@pytest.mark.parametrize('route', ['plan', 'binned'])
@pytest.mark.parametrize('weights', ['f32', 'shared'])
def test_product_on_the_fixed_point_routes(weights, route):
    case = DC.exact_case(22, N_PRE, N_POST, DEPTH, 32, parallel=True, **WEIGHTS[weights])
    D = _route(build(case, (N_PRE, N_POST), DEPTH), route)
    _run_and_compare(D, case, N_PRE, N_POST, DEPTH, 2 * DEPTH + 1)
    assert isinstance(D.stacked.buffers['scatter_plan'], C.ScatterPlan if route == 'plan' else C.BinnedScatter)


def test_numpy_in_numpy_out():
    case = DC.exact_case(23, N_PRE, N_POST, DEPTH, 32)
    D = be.DelayedCSR(case, shape=(N_PRE, N_POST), depth=DEPTH)
    rng = np.random.default_rng(2)
    ring, ref = be.SpikeRing(N_PRE, DEPTH), DC.ring_np(N_PRE, DEPTH)
    for _ in range(DEPTH + 1):
        s = rng.random(N_PRE) < RATE
        ring.push(s)
        ref.push(s)
        got = ring @ D
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        np.testing.assert_array_equal(got.astype(np.float64), DC.delayed_currents_np(*case, ref, N_POST))
    ring.push(dev(s))                                       # a device tensor anywhere: a tensor comes back
    assert isinstance(ring @ D, torch.Tensor)


@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_product_past_65536_stacked_rows(route):
    n_pre, n_post, depth = 4100, 500, 16
    assert depth * n_pre > 1 << 16
    case = DC.exact_case(24, n_pre, n_post, depth, 3, fixed_len=3)
    D = _route(build(case, (n_pre, n_post), depth), route)
    _run_and_compare(D, case, n_pre, n_post, depth, depth + 2, rate=0.1)


def test_depth_one_is_the_undelayed_product():
    case = DC.exact_case(25, N_PRE, N_POST, 1, 32)
    data, indices, indptr, delays = case
    D = build(case, (N_PRE, N_POST), 1)
    csr = be.CSR((dev(data), dev(indices), dev(indptr)), shape=(N_PRE, N_POST))
    ring = be.SpikeRing(N_PRE, 1)
    rng = np.random.default_rng(4)
    for _ in range(3):
        s = dev(rng.random(N_PRE) < RATE)
        ring.push(s)
        assert torch.equal(ring @ D, be.BinaryArray(s) @ csr)


def test_one_delay_for_a_whole_projection():
    """``ring.events(a) @ csr``: the homogeneous delay, with a container that knows nothing of delays."""
    case = DC.exact_case(26, N_PRE, N_POST, 1, 32)
    data, indices, indptr, _ = case
    csr = be.CSR((dev(data), dev(indices), dev(indptr)), shape=(N_PRE, N_POST))
    depth = 5
    ring, ref = be.SpikeRing(N_PRE, depth), DC.ring_np(N_PRE, depth)
    rng = np.random.default_rng(6)
    for _ in range(depth + 2):
        s = rng.random(N_PRE) < RATE
        ring.push(dev(s))
        ref.push(s)
        for a in range(depth):
            assert torch.equal(ring.events(a) @ csr, be.BinaryArray(dev(ref.age(a))) @ csr)


@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_new_weights(route):
    case = DC.exact_case(27, N_PRE, N_POST, DEPTH, 32)
    data, indices, indptr, delays = case
    rng = np.random.default_rng(12)
    w2 = (rng.integers(-64, 65, data.size) / 64.0).astype(np.float32)
    w3 = (rng.integers(-64, 65, data.size) / 64.0).astype(np.float32)
    D = _route(build(case, (N_PRE, N_POST), DEPTH), route)
    _run_and_compare(D, case, N_PRE, N_POST, DEPTH, 3)
    D2 = _route(D.with_data(dev(w2)), route)
    assert D2 is not D and D2.perm is D.perm and D2.stacked.indices is D.stacked.indices and D2.stacked.indptr is D.stacked.indptr
    _run_and_compare(D2, (w2, indices, indptr, delays), N_PRE, N_POST, DEPTH, DEPTH + 2)
    _run_and_compare(D, case, N_PRE, N_POST, DEPTH, 3)                       # the original is untouched
    assert D.set_data_(dev(w3)) is D                                         # in place: a cached plan refreshes by itself
    np.testing.assert_array_equal(host(D.data), w3)
    _run_and_compare(D, (w3, indices, indptr, delays), N_PRE, N_POST, DEPTH, DEPTH + 2)
    with pytest.raises(ValueError):
        D.with_data(dev(w2[:-1]))


def test_refusals_on_the_device():
    case = DC.exact_case(28, N_PRE, N_POST, DEPTH, 8)
    D = build(case, (N_PRE, N_POST), DEPTH)
    with pytest.raises(ValueError, match='71 neurons'):
        be.SpikeRing(N_PRE + 1, DEPTH) @ D
    with pytest.raises(ValueError, match='remembers 6 steps'):
        be.SpikeRing(N_PRE, DEPTH - 1) @ D
    ring = be.SpikeRing(N_PRE, DEPTH + 2).push(np.ones(N_PRE, bool))         # a deeper ring serves a shallower matrix
    want = DC.ring_np(N_PRE, DEPTH + 2)
    want.push(np.ones(N_PRE, bool))
    np.testing.assert_array_equal(host(ring @ D).astype(np.float64), DC.delayed_currents_np(*case, want, N_POST))
    with pytest.raises(NotImplementedError):
        D @ ring
    with pytest.raises(NotImplementedError):
        be.BinaryArray(torch.zeros((2, N_PRE), dtype=torch.bool, device='cuda')) @ D          # a batch of vectors
    with pytest.raises(NotImplementedError):
        ring @ be.CSR((dev(case[0]), dev(case[1]), dev(case[2])), shape=(N_PRE, N_POST))


# ---------------------------------------------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_captured_steps_replay_with_the_head_on_the_device(route):
    """Three steps per replay (``repeat=3``) against a ring of depth 7: every replay starts at another head, which only a head
    read on the device gets right."""
    repeat = 3
    case = DC.exact_case(29, N_PRE, N_POST, DEPTH, 32)
    D = _route(build(case, (N_PRE, N_POST), DEPTH), route)
    rng = np.random.default_rng(31)
    spikes = [[rng.random(N_PRE) < RATE for _ in range(repeat)] for _ in range(DEPTH)]        # 3 * depth steps
    # eager loop
    ring = be.SpikeRing(N_PRE, DEPTH)
    eager = []
    for trio in spikes:
        for s in trio:
            ring.push(dev(s))
            eager.append((ring @ D).clone())
    # captured: sub-step k of a replay reads bufs[k] and writes outs[k]
    ring2 = be.SpikeRing(N_PRE, DEPTH)
    bufs = torch.zeros((repeat, N_PRE), dtype=torch.bool, device='cuda')
    outs = torch.zeros((repeat, N_POST), dtype=D.dtype, device='cuda')
    k = [0]

    def step():
        i = k[0] % repeat
        k[0] += 1
        ring2.push(bufs[i])
        outs[i].copy_(ring2 @ D)
        return outs

    graphed = be.capture_step(step, warmup=repeat, repeat=repeat)
    ring2.reset()                                               # (the warm-up pushed)
    got = []
    for trio in spikes:
        bufs.copy_(dev(np.stack(trio)))
        graphed()
        torch.cuda.synchronize()
        got.extend(outs.clone())
    assert int(ring2.head) == (repeat * DEPTH) % DEPTH
    ref = DC.ring_np(N_PRE, DEPTH)
    for t, (g, e) in enumerate(zip(got, eager)):
        ref.push(spikes[t // repeat][t % repeat])
        assert torch.equal(g, e), f'step {t}'
        np.testing.assert_array_equal(host(g).astype(np.float64), DC.delayed_currents_np(*case, ref, N_POST), err_msg=f'step {t}')
