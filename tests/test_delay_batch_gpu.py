"""Batched spike rings on the device (``SpikeRing(n, depth, batch=B)``, ``be_spike_ring_push_batch``,
``be_spike_ring_unroll`` and ``ring @ D`` for a batch of histories) against the numpy restatement of tests/delay_batch_cases.py,
which tests/test_delay_batch_cpu.py holds to a brute-force per-bit loop.

The ring and the unrolled words are compared exactly, padding bits included.  The products are equalities too: the generator of
tests/delay_cases.py draws weights ``k / 64`` (small integers for f16) whose partial sums are exact in the weight dtype in any
order, so a batched result equals, bit for bit, what ``B`` one-sample rings fed row by row give through the existing
``ring_b @ D`` — on the direct route (float atomics) as on the fixed-point routes.  The gradient is exact for the same reason:
output gradients ``k / 64``, at most ``3 * 33`` of them per weight.

Sizes: 8192 bits per workgroup of the push (``delay_cases.RING_TILE_BITS``) and of the unroll (256 words), and the largest batch,
65535: the batch row is the second grid dimension of both kernels, which neither strides over — a larger batch is refused
(tests/test_delay_batch_cpu.py), so the bound itself is the case.  The stacked row counts ``7 * 33`` and ``7 * 70`` are no multiples
of 32: with ``B > 1`` and packed words the direct and the binned batch entry points are reached from Python for the first time
here."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
import brainevent_amd._csr as C
import delay_cases as DC
import delay_batch_cases as BC

pytestmark = pytest.mark.gpu

SMALL = [1, 31, 32, 33]
RING_SIZES = SMALL + [63, 64, 65, DC.RING_TILE_BITS - 1, DC.RING_TILE_BITS, DC.RING_TILE_BITS + 1]
BATCHES = [1, 2, 33]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def words_of(t):
    return host(t).view(np.uint32)


def build(case, shape, depth):
    data, indices, indptr, delays = case
    return be.DelayedCSR((dev(data), dev(indices), dev(indptr), dev(delays)), shape=shape, depth=depth)


def _route(D, route):
    """``direct``: nothing prepared, a matrix this small takes the direct kernel; ``prepared``: ``D.prepare()``, the router's
    choice; ``plan`` / ``binned``: that workspace installed (as tests/test_delay_gpu.py forces them)."""
    st = D.stacked
    if route == 'prepared':
        assert D.prepare() is D and 'scatter_plan' in st.buffers
    elif route == 'plan':
        st.buffers['scatter_plan'] = C.ScatterPlan.build(st.data, st.indices, st.indptr, shape=st.shape)
    elif route == 'binned':
        st.buffers['scatter_plan'] = C.BinnedScatter(st.data, st.shape[0], st.shape[1], st.nse, indices=st.indices,
                                                     indptr=st.indptr)
    return D


def _workspace_is(D, route):
    ws = D.stacked.buffers.get('scatter_plan')
    if route == 'direct':
        return ws is None
    return isinstance(ws, {'plan': C.ScatterPlan, 'binned': C.BinnedScatter}[route])


# ---------------------------------------------------------------------------------------------------------------------------
# push and unroll
# ---------------------------------------------------------------------------------------------------------------------------
def _payload(rng, batch, n, kind, rate=0.3):
    """``(bool [B, n], what to push, how)``: a bool tensor, a float tensor (negatives and zeros inactive), or packed words with
    every bit past ``n`` SET (the push has to clear them)."""
    s = rng.random((batch, n)) < rate
    if kind == 'bool':
        return s, dev(s), 'push'
    if kind == 'float':
        v = np.where(s, rng.random((batch, n)) + 0.25, -rng.random((batch, n)) * (rng.random((batch, n)) < 0.5)).astype(np.float32)
        return s, dev(v), 'push'
    full = np.ones((batch, ((n + 31) // 32) * 32), bool)
    full[:, :n] = s
    return s, dev(DC.pack_rows_np(full).view(np.int32)), 'push_packed'


def _check_ring(ring, ref, masks):
    """``bits``, ``head`` and the unrolled words (every age and one fewer; with and without a mask), padding bits included."""
    n, depth = ref.n, ref.depth
    np.testing.assert_array_equal(words_of(ring.bits), ref.bits())
    assert int(ring.head) == ref.head
    for ages in sorted({depth, max(1, depth - 1)}):
        for mask_np, mask in masks:
            got = ring.stacked_bits(ages=ages, row_mask=mask)
            assert got.dtype == torch.int32 and tuple(got.shape) == (ref.batch, (ages * n + 31) // 32)
            np.testing.assert_array_equal(words_of(got), ref.stacked_words(ages, mask_np), err_msg=f'ages {ages}')


@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('n,depth', [(n, d) for n in RING_SIZES for d in (1, 3)] + [(n, 256) for n in SMALL])
def test_push_and_unroll(n, depth, batch):
    rng = np.random.default_rng(100000 * batch + 1000 * depth + n)
    ring, ref = be.SpikeRing(n, depth, batch=batch), BC.batch_ring_np(n, depth, batch)
    nw = (n + 31) // 32
    assert ring.batch == batch and ring.shape == (batch, n) and ring.ndim == 2
    assert ring.bits.dtype == torch.int32 and tuple(ring.bits.shape) == (depth, batch, nw) and not ring.bits.any()
    assert ring.head.dtype == torch.int32 and tuple(ring.head.shape) == (1,)
    mask_np = BC.random_mask(rng, depth, n)
    masks = [(None, None), (mask_np, dev(mask_np.view(np.int32)))]
    _check_ring(ring, ref, masks)                                # a silent ring: every word is written, all zero
    steps = 2 * depth + 1                                        # head wraps twice
    look = set(range(steps)) if depth <= 3 else {0, depth - 2, depth - 1, depth, steps - 1}
    for t in range(steps):
        s, payload, how = _payload(rng, batch, n, ('bool', 'float', 'packed')[t % 3])
        assert getattr(ring, how)(payload) is ring
        ref.push(s)
        if t in look:
            _check_ring(ring, ref, masks)
    a = ring.stacked_bits()
    first = a.clone()
    b = ring.stacked_bits()                                      # no push in between: the same words, in the same buffer
    assert b.data_ptr() == a.data_ptr() and torch.equal(b, first)
    for _ in range(depth):                                       # a full ring
        ring.push(dev(np.ones((batch, n), bool)))
        ref.push(np.ones((batch, n), bool))
    _check_ring(ring, ref, masks)
    full = DC.unpack_words_np(words_of(ring.stacked_bits()).reshape(-1), 0).reshape(batch, -1)
    assert full[:, :depth * n].all() and not full[:, depth * n:].any()
    assert ring.reset() is ring and not ring.bits.any() and int(ring.head) == 0
    assert not ring.stacked_bits().any()


def test_the_largest_batch():
    """``batch = 65535``: the last row of the grid's second dimension, in the push and in the unroll."""
    n, depth, batch = 33, 2, BC.MAX_BATCH
    rng = np.random.default_rng(5)
    ring, ref = be.SpikeRing(n, depth, batch=batch), BC.batch_ring_np(n, depth, batch)
    mask_np = BC.random_mask(rng, depth, n)
    for kind in ('float', 'packed', 'bool'):
        s, payload, how = _payload(rng, batch, n, kind)
        getattr(ring, how)(payload)
        ref.push(s)
    _check_ring(ring, ref, [(None, None), (mask_np, dev(mask_np.view(np.int32)))])


def test_push_takes_numpy_and_a_binary_array():
    n, depth, batch = 100, 3, 4
    rng = np.random.default_rng(0)
    ring, ref = be.SpikeRing(n, depth, batch=batch), BC.batch_ring_np(n, depth, batch)
    s = [rng.random((batch, n)) < 0.5 for _ in range(4)]
    for payload, v in ((s[0], s[0]), (be.BinaryArray(dev(s[1])), s[1]), (be.BinaryArray(s[2].astype(np.int8)), s[2]),
                       (dev(s[3].astype(np.int64) * 7), s[3])):                  # (another dtype: as spikes_to_device treats it)
        ring.push(payload)
        ref.push(v)
    np.testing.assert_array_equal(words_of(ring.bits), ref.bits())
    ring.push_packed(DC.pack_rows_np(s[0]).view(np.int32))                       # numpy words
    ref.push(s[0])
    np.testing.assert_array_equal(words_of(ring.stacked_bits()), ref.stacked_words())


# ---------------------------------------------------------------------------------------------------------------------------
# identity with the ring without a batch
# ---------------------------------------------------------------------------------------------------------------------------
N_POST, DEPTH, RATE = 300, 7, 0.2
WEIGHTS = {'f32': dict(dtype=np.float32), 'f64': dict(dtype=np.float64), 'shared': dict(dtype=np.float32, homo=True),
           'f16': dict(dtype=np.float16)}


@pytest.mark.parametrize('route', ['direct', 'plan', 'binned'])
def test_batch_of_one_is_the_ring_without_a_batch(route):
    n_pre = 70
    case = DC.exact_case(41, n_pre, N_POST, DEPTH, 32, parallel=True)
    D = _route(build(case, (n_pre, N_POST), DEPTH), route)
    one, many = be.SpikeRing(n_pre, DEPTH), be.SpikeRing(n_pre, DEPTH, batch=1)
    rng = np.random.default_rng(3)
    for _ in range(2 * DEPTH + 1):
        s = dev(rng.random(n_pre) < RATE)
        one.push(s)
        many.push(s.reshape(1, -1))
        assert torch.equal(many.bits.reshape(one.bits.shape), one.bits) and torch.equal(many.head, one.head)
        y1, yb = one @ D, many @ D
        assert tuple(yb.shape) == (1, N_POST) and yb.dtype == y1.dtype and torch.equal(yb[0], y1)
    assert _workspace_is(D, route)


# ---------------------------------------------------------------------------------------------------------------------------
# products: a batched ring against B one-sample rings
# ---------------------------------------------------------------------------------------------------------------------------
def _run_and_compare(D, n_pre, n_post, depth, batch, steps, seed=9, rate=RATE, ring_depth=None):
    ring_depth = depth if ring_depth is None else ring_depth
    rng = np.random.default_rng(seed)
    ring = be.SpikeRing(n_pre, ring_depth, batch=batch)
    singles = [be.SpikeRing(n_pre, ring_depth) for _ in range(batch)]
    seen = False
    for t in range(steps):
        S = dev(rng.random((batch, n_pre)) < rate)
        ring.push(S)
        got = ring @ D
        assert isinstance(got, torch.Tensor) and got.dtype == D.dtype and tuple(got.shape) == (batch, n_post)
        for b, single in enumerate(singles):
            single.push(S[b])
            want = single @ D
            assert torch.equal(got[b], want), f'step {t}, sample {b}'
            seen = seen or bool(want.any())
    assert seen                                                  # (the comparison was not of zeros with zeros)
    return ring


@pytest.mark.parametrize('batch', BATCHES[:1] + [3, 33])
@pytest.mark.parametrize('n_pre', [33, 70])
@pytest.mark.parametrize('route', ['direct', 'prepared'])
@pytest.mark.parametrize('weights', sorted(WEIGHTS))
def test_product_every_weight_kind(weights, route, n_pre, batch):
    case = DC.exact_case(51, n_pre, N_POST, DEPTH, 32, parallel=True, **WEIGHTS[weights])
    D = _route(build(case, (n_pre, N_POST), DEPTH), route)
    assert (DEPTH * n_pre) % 32 != 0
    ptr = host(D.stacked.indptr)
    assert (ptr[1:] == ptr[:-1]).any()                           # some stacked rows are empty
    _run_and_compare(D, n_pre, N_POST, DEPTH, batch, 2 * DEPTH + 1)


@pytest.mark.parametrize('batch', [1, 3, 33])                    # 33 passes the binned route's 32 rows at a time
@pytest.mark.parametrize('n_pre', [33, 70])
@pytest.mark.parametrize('route', ['plan', 'binned'])
@pytest.mark.parametrize('weights', ['f32', 'shared'])
def test_product_on_the_fixed_point_routes(weights, route, n_pre, batch):
    case = DC.exact_case(52, n_pre, N_POST, DEPTH, 32, parallel=True, **WEIGHTS[weights])
    D = _route(build(case, (n_pre, N_POST), DEPTH), route)
    _run_and_compare(D, n_pre, N_POST, DEPTH, batch, 2 * DEPTH + 1)
    assert _workspace_is(D, route)


def test_a_deeper_ring_on_a_shallower_matrix():
    n_pre = 70
    case = DC.exact_case(53, n_pre, N_POST, DEPTH, 32, parallel=True)
    D = build(case, (n_pre, N_POST), DEPTH)
    _run_and_compare(D, n_pre, N_POST, DEPTH, 3, 2 * (DEPTH + 2) + 1, ring_depth=DEPTH + 2)


@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_product_past_65536_stacked_rows(route):
    n_pre, n_post, depth = 4100, 500, 16
    assert depth * n_pre > 1 << 16
    case = DC.exact_case(54, n_pre, n_post, depth, 3, fixed_len=3)
    D = _route(build(case, (n_pre, n_post), depth), route)
    _run_and_compare(D, n_pre, n_post, depth, 3, depth + 2, rate=0.1)


@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_new_weights_through_set_data(route):
    n_pre = 70
    case = DC.exact_case(55, n_pre, N_POST, DEPTH, 32)
    rng = np.random.default_rng(12)
    w2 = (rng.integers(-64, 65, case[0].size) / 64.0).astype(np.float32)
    D = _route(build(case, (n_pre, N_POST), DEPTH), route)
    _run_and_compare(D, n_pre, N_POST, DEPTH, 3, 3)
    assert D.set_data_(dev(w2)) is D                             # in place: a cached plan refreshes by itself
    ring = _run_and_compare(D, n_pre, N_POST, DEPTH, 3, DEPTH + 2)
    # ... and against the restatement, so that "both stale" cannot pass: the last step by the numpy loop over the entries
    ref = DC.ring_np(n_pre, DEPTH)
    bits = BC.batch_ring_np(n_pre, DEPTH, 3)
    rng2 = np.random.default_rng(9)
    for _ in range(DEPTH + 2):
        bits.push(rng2.random((3, n_pre)) < RATE)
    ref.history = [h[1] for h in bits.history]
    want = DC.delayed_currents_np(w2, case[1], case[2], case[3], ref, N_POST)
    np.testing.assert_array_equal(host(ring @ D)[1].astype(np.float64), want)


def test_numpy_in_numpy_out():
    n_pre, batch = 70, 3
    case = DC.exact_case(56, n_pre, N_POST, DEPTH, 32)
    D = be.DelayedCSR(case, shape=(n_pre, N_POST), depth=DEPTH)
    rng = np.random.default_rng(2)
    ring, ref = be.SpikeRing(n_pre, DEPTH, batch=batch), BC.batch_ring_np(n_pre, DEPTH, batch)
    for _ in range(DEPTH + 1):
        S = rng.random((batch, n_pre)) < RATE
        ring.push(S)
        ref.push(S)
    got = ring @ D
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (batch, N_POST)
    for b in range(batch):
        one = DC.ring_np(n_pre, DEPTH)
        one.history = [h[b] for h in ref.history]
        np.testing.assert_array_equal(got[b].astype(np.float64), DC.delayed_currents_np(*case, one, N_POST))
    ring.push(dev(S))                                            # a device tensor anywhere: a tensor comes back
    assert isinstance(ring @ D, torch.Tensor)


# ---------------------------------------------------------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', [3, 33])
@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_weight_gradient_is_the_sum_of_the_one_sample_gradients(route, batch):
    """Three forwards, one backward: ``dL/dw_e = sum_t sum_b g_t[b, col(e)] * s_b,row(e)(age = delays[e])``."""
    n_pre = 70
    case = DC.exact_case(61, n_pre, N_POST, DEPTH, 32, parallel=True)
    data, indices, indptr, delays = case
    rows = np.repeat(np.arange(n_pre), np.diff(indptr))
    Db, D1 = (_route(build(case, (n_pre, N_POST), DEPTH), route) for _ in range(2))
    for D in (Db, D1):
        D.stacked.data.requires_grad_(True)
    rng = np.random.default_rng(13)
    ring, ref = be.SpikeRing(n_pre, DEPTH, batch=batch), BC.batch_ring_np(n_pre, DEPTH, batch)
    singles = [be.SpikeRing(n_pre, DEPTH) for _ in range(batch)]
    for _ in range(DEPTH - 2):                                   # some history first, outside the graph
        S = rng.random((batch, n_pre)) < RATE
        ring.push(dev(S))
        ref.push(S)
        for b, single in enumerate(singles):
            single.push(dev(S[b]))
    loss_b = loss_1 = 0
    want = np.zeros(indices.size)
    for _ in range(3):
        S = rng.random((batch, n_pre)) < RATE
        G = rng.integers(-64, 65, (batch, N_POST)) / 64.0
        g = dev(G.astype(np.float32))
        ring.push(dev(S))
        ref.push(S)
        y = ring @ Db
        assert isinstance(y, torch.Tensor) and y.requires_grad and tuple(y.shape) == (batch, N_POST)
        loss_b = loss_b + (y * g).sum()
        for b, single in enumerate(singles):
            single.push(dev(S[b]))
            yb = single @ D1
            assert torch.equal(yb.detach(), y.detach()[b])
            loss_1 = loss_1 + (yb * g[b]).sum()
        by_age = np.stack([ref.age(a) for a in range(DEPTH)])                  # [depth, B, n_pre]
        want += (by_age[delays, :, rows] * G[:, indices].T).sum(axis=1)
    loss_b.backward()
    loss_1.backward()
    gb, g1 = Db.stacked.data.grad, D1.stacked.data.grad
    assert gb is not None and gb.dtype == torch.float32 and gb.shape == Db.stacked.data.shape
    assert torch.equal(gb, g1)
    orig = Db.stacked_to_original(gb)
    assert tuple(orig.shape) == data.shape and torch.equal(orig, D1.stacked_to_original(g1))
    np.testing.assert_array_equal(host(orig).astype(np.float64), want)
    assert np.abs(want).max() > 0
    assert _workspace_is(Db, route)


def test_shared_weight_gradient():
    n_pre, batch = 33, 3
    case = DC.exact_case(62, n_pre, N_POST, DEPTH, 32, homo=True)
    Db, D1 = (build(case, (n_pre, N_POST), DEPTH) for _ in range(2))
    for D in (Db, D1):
        D.stacked.data.requires_grad_(True)
    rng = np.random.default_rng(14)
    ring, singles = be.SpikeRing(n_pre, DEPTH, batch=batch), [be.SpikeRing(n_pre, DEPTH) for _ in range(batch)]
    loss_b = loss_1 = 0
    for _ in range(3):
        S = dev(rng.random((batch, n_pre)) < RATE)
        g = dev((rng.integers(-64, 65, (batch, N_POST)) / 64.0).astype(np.float32))
        ring.push(S)
        loss_b = loss_b + ((ring @ Db) * g).sum()
        for b, single in enumerate(singles):
            single.push(S[b])
            loss_1 = loss_1 + ((single @ D1) * g[b]).sum()
    loss_b.backward()
    loss_1.backward()
    assert Db.stacked.data.grad.shape == (1,) and torch.equal(Db.stacked.data.grad, D1.stacked.data.grad)
    assert float(Db.stacked.data.grad) != 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_captured_steps_replay_with_the_head_on_the_device(route):
    """Three steps per replay (``repeat=3``) against a ring of depth 7: every replay starts at another head.  Nothing on this path
    is zeroed by a memset node — the unroll writes every word of its buffer itself (tests/test_delay_batch_cpu.py reads that from
    the source) — and the replays show it as the existing capture tests do: each starts clean and equals the eager step, with
    the unrolled buffer still holding the previous sub-step's words."""
    repeat, n_pre, batch = 3, 70, 3
    case = DC.exact_case(71, n_pre, N_POST, DEPTH, 32, parallel=True)
    D = _route(build(case, (n_pre, N_POST), DEPTH), route)
    rng = np.random.default_rng(31)
    spikes = [[rng.random((batch, n_pre)) < RATE for _ in range(repeat)] for _ in range(DEPTH)]      # 3 * depth steps
    ring = be.SpikeRing(n_pre, DEPTH, batch=batch)
    eager = []
    for trio in spikes:
        for s in trio:
            ring.push(dev(s))
            eager.append((ring @ D).clone())
    ring2 = be.SpikeRing(n_pre, DEPTH, batch=batch)
    bufs = torch.zeros((repeat, batch, n_pre), dtype=torch.bool, device='cuda')
    outs = torch.zeros((repeat, batch, N_POST), dtype=D.dtype, device='cuda')
    k = [0]

    def step():
        i = k[0] % repeat
        k[0] += 1
        ring2.push(bufs[i])
        outs[i].copy_(ring2 @ D)
        return outs

    graphed = be.capture_step(step, warmup=repeat, repeat=repeat)
    ring2.reset()                                                # (the warm-up pushed)
    got = []
    for trio in spikes:
        bufs.copy_(dev(np.stack(trio)))
        graphed()
        torch.cuda.synchronize()
        got.extend(outs.clone())
    assert int(ring2.head) == (repeat * DEPTH) % DEPTH
    assert torch.equal(ring2.bits, ring.bits)
    singles = [be.SpikeRing(n_pre, DEPTH) for _ in range(batch)]
    for t, (g, e) in enumerate(zip(got, eager)):
        assert torch.equal(g, e), f'step {t}'
        for b, single in enumerate(singles):
            single.push(dev(spikes[t // repeat][t % repeat][b]))
            assert torch.equal(g[b], single @ D), f'step {t}, sample {b}'
    assert any(bool(g.any()) for g in got)


# ---------------------------------------------------------------------------------------------------------------------------
# events and refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [33, 64, 70])
def test_events_of_every_age(n):
    depth, batch = 5, 3
    rng = np.random.default_rng(n)
    ring, ref = be.SpikeRing(n, depth, batch=batch), BC.batch_ring_np(n, depth, batch)
    for t in range(depth + 3):
        for a in range(depth):
            ev = ring.events(a)
            assert isinstance(ev, be.BinaryArray) and ev.value.dtype == torch.bool and tuple(ev.value.shape) == (batch, n)
            np.testing.assert_array_equal(host(ev.value), ref.age(a), err_msg=f'step {t}, age {a}')
        S = rng.random((batch, n)) < 0.3
        ring.push(dev(S))
        ref.push(S)


def test_one_delay_for_a_whole_projection():
    n_pre, depth, batch = 70, 5, 3
    data, indices, indptr, _ = DC.exact_case(81, n_pre, N_POST, 1, 32)
    csr = be.CSR((dev(data), dev(indices), dev(indptr)), shape=(n_pre, N_POST))
    ring, ref = be.SpikeRing(n_pre, depth, batch=batch), BC.batch_ring_np(n_pre, depth, batch)
    rng = np.random.default_rng(6)
    for _ in range(depth + 2):
        S = rng.random((batch, n_pre)) < RATE
        ring.push(dev(S))
        ref.push(S)
    got = ring.events(2) @ csr
    assert tuple(got.shape) == (batch, N_POST) and got.any()
    for b in range(batch):
        assert torch.equal(got[b], be.BinaryArray(dev(ref.age(2)[b])) @ csr)


def test_refusals_on_the_device():
    n_pre, batch = 70, 3
    case = DC.exact_case(82, n_pre, N_POST, DEPTH, 8)
    D = build(case, (n_pre, N_POST), DEPTH)
    ring = be.SpikeRing(n_pre, DEPTH, batch=batch)
    before = ring.bits.clone()
    for bad in (torch.zeros(n_pre, dtype=torch.bool, device='cuda'), torch.zeros((batch + 1, n_pre), dtype=torch.bool, device='cuda'),
                torch.zeros((batch, n_pre + 1), dtype=torch.bool, device='cuda')):
        with pytest.raises(ValueError):
            ring.push(bad)
    with pytest.raises(ValueError):
        ring.push_packed(torch.zeros((batch, 4), dtype=torch.int32, device='cuda'))
    with pytest.raises(TypeError):
        ring.push(be.BitPackedBinary(torch.zeros(n_pre, dtype=torch.bool, device='cuda')))
    assert torch.equal(ring.bits, before) and int(ring.head) == 0              # nothing was pushed
    with pytest.raises(NotImplementedError):
        ring.ids()
    with pytest.raises(NotImplementedError, match='one sample'):
        D.update_on_pre(ring, torch.zeros(N_POST, device='cuda'))
    with pytest.raises(ValueError, match='71 neurons'):
        be.SpikeRing(n_pre + 1, DEPTH, batch=batch) @ D
    with pytest.raises(ValueError, match='remembers 6 steps'):
        be.SpikeRing(n_pre, DEPTH - 1, batch=batch) @ D
    with pytest.raises(NotImplementedError):
        D @ ring
    with pytest.raises(NotImplementedError):
        be.BinaryArray(torch.zeros((batch, n_pre), dtype=torch.bool, device='cuda')) @ D
    with pytest.raises(NotImplementedError):
        ring @ be.CSR((dev(case[0]), dev(case[1]), dev(case[2])), shape=(n_pre, N_POST))
    with pytest.raises(NotImplementedError):                                   # a ring without a batch keeps its rule
        be.SpikeRing(n_pre, DEPTH).push(torch.zeros((batch, n_pre), dtype=torch.bool, device='cuda'))
