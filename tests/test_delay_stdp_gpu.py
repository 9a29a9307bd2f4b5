"""Plasticity and weight gradients of delayed synapses on the device (``ValueRing``, ``DelayedCSR.update_on_pre`` / ``update_on_post``,
autograd through ``ring @ D``; csrc/be_delay.hip, csrc/be_plasticity.hip) against the numpy restatement of
tests/delay_stdp_cases.py, which tests/test_delay_stdp_cpu.py holds to a brute-force loop over the entries.

One call adds at most one value to an entry, so every weight comparison is an equality for arbitrary float inputs; the products
after updates and the gradients use multiples of 1/64, whose sums are exact on every route (see the docstring of the cases
module).  Sizes follow ``delay_stdp_cases.PUSH_TILES`` and the THRESHOLDS table of tests/test_update_kernels_at_scale_gpu.py: 4096
elements per push workgroup, 2048 entries per tile of the update kernel, 16384 active rows per pass of the offsets scan, 4096
tiles per grid stride."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
import brainevent_amd._csr as C
from brainevent_amd import _plasticity as P
import delay_cases as DC
import delay_stdp_cases as SC
from test_plasticity_gpu import encode
from test_update_kernels_at_scale_gpu import THRESHOLDS

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
NAMES = sorted(TORCH)
N_PRE, N_POST, DEPTH, RATE = 70, 50, 6, 0.3
TILE = THRESHOLDS['plast.kRowThreads'] * THRESHOLDS['plast.kRowPer']
SCAN_PASS = THRESHOLDS['plast.kScanThreads'] * THRESHOLDS['plast.kScanPer']
GRID_CAP = THRESHOLDS['plast.rows_grid_cap']
assert (TILE, SCAN_PASS, GRID_CAP) == (2048, 16384, 4096)
CLIPS = [(None, None), (-0.5, None), (-0.5, 0.75)]


def dev(x, name=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if name is None else t.to(TORCH[name])


def host(t):
    t = t.detach().cpu()
    return t.float().numpy() if t.dtype == torch.bfloat16 else t.numpy()


def on_device(x):
    return torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x


def build(case, shape, depth, name='f32', indptr_dtype=np.int32):
    data, indices, indptr, delays = case
    ptr = None if indptr is None else dev(indptr.astype(indptr_dtype))
    return be.DelayedCSR((dev(data, name), dev(indices), ptr, dev(delays)), shape=shape, depth=depth)


def assert_weights(D, want, name, msg=''):
    got = host(D.data).reshape(-1)
    assert got.dtype == SC.DTYPES[name]
    np.testing.assert_array_equal(got, want, err_msg=msg)           # (NaN-free inputs: an equality of values is one of bits)
    assert not (np.signbit(got) != np.signbit(want)).any(), msg


def shares_structure(Dn, D):
    return (Dn is not D and Dn.perm is D.perm and Dn.delays is D.delays and Dn.row_mask is D.row_mask
            and Dn.stacked.indices is D.stacked.indices and Dn.stacked.indptr is D.stacked.indptr)


# ---------------------------------------------------------------------------------------------------------------------------
# ValueRing
# ---------------------------------------------------------------------------------------------------------------------------
RING_SIZES = [1, 31, 33, SC.VALUE_TILE - 1, SC.VALUE_TILE, SC.VALUE_TILE + 1]
NP_IN = {'f32': np.float32, 'f64': np.float64, 'f16': np.float16}


@pytest.mark.parametrize('depth', [1, 3, 256])
@pytest.mark.parametrize('n', RING_SIZES)
def test_value_ring_push_value_by_age(n, depth):
    rng = np.random.default_rng(100 * depth + n)
    pool = rng.normal(size=(5, n)) * 3.0
    look = sorted({0, 1, depth - 2, depth - 1, depth, depth + 1, 2 * depth - 1, 2 * depth} & set(range(2 * depth + 1)))
    for src, name in (('f32', 'f32'), ('f64', 'f64'), ('f16', 'f16'), ('bf16', 'bf16'), ('f64', 'f32'), ('f32', 'f16')):
        hist, ref = be.ValueRing(n, depth, dtype=TORCH[name]), SC.value_ring_np(n, depth, name)
        assert hist.values.dtype == TORCH[name] and tuple(hist.values.shape) == (depth, n) and not hist.values.any()
        assert hist.head.dtype == torch.int32 and tuple(hist.head.shape) == (1,) and hist.head.device == hist.values.device
        assert not hist.by_age().any()                                      # history before the first push is zero
        xs = SC.to_dtype_np(pool, src)                                      # values of the INPUT dtype
        xs_d = dev(xs, src)
        for t in range(2 * depth + 1):
            x = xs_d[t % 5]
            hist.push(x.clone() if t % 2 else x)        # a fresh (aligned) tensor, or a row of the pool (aligned when n * size allows)
            ref.push(xs[t % 5])
            if t in look:
                assert int(hist.head) == (t + 1) % depth
                got = hist.by_age()
                assert got.dtype == TORCH[name] and tuple(got.shape) == (depth, n)
                np.testing.assert_array_equal(host(got), ref.by_age(), err_msg=f'{src}->{name} push {t}')
                for a in sorted({0, depth // 2, depth - 1}):
                    np.testing.assert_array_equal(host(hist.value(a)), ref.age(a), err_msg=f'{src}->{name} push {t} age {a}')
        assert hist.reset() is hist and not hist.values.any() and int(hist.head) == 0
        hist.push(xs[0].astype(NP_IN[src]) if src in NP_IN else xs_d[0])   # numpy in (bf16 has no numpy dtype)
        ref = SC.value_ring_np(n, depth, name)
        ref.push(xs[0])
        np.testing.assert_array_equal(host(hist.by_age()), ref.by_age())


def test_value_ring_refusals_on_the_device():
    hist = be.ValueRing(10, 3)
    with pytest.raises(ValueError, match='11 values'):
        hist.push(torch.zeros(11, device='cuda'))
    with pytest.raises(NotImplementedError):
        hist.push(torch.zeros((2, 10), device='cuda'))
    with pytest.raises(TypeError):
        hist.push(torch.zeros(10, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        hist.value(3)
    assert not hist.values.any() and int(hist.head) == 0                  # nothing was written


def test_value_ring_captured_pushes_replay_with_the_head_on_the_device():
    """Three pushes per replay against depth 7: every replay starts at another head."""
    n, depth, repeat = 33, 7, 3
    rng = np.random.default_rng(5)
    xs = rng.normal(size=(depth, repeat, n)).astype(np.float32)
    hist, ref = be.ValueRing(n, depth), SC.value_ring_np(n, depth)
    bufs = torch.zeros((repeat, n), device='cuda')
    outs = torch.zeros((repeat, depth, n), device='cuda')
    k = [0]

    def step():
        i = k[0] % repeat
        k[0] += 1
        hist.push(bufs[i])
        outs[i].copy_(hist.by_age())

    graphed = be.capture_step(step, warmup=repeat, repeat=repeat)
    hist.reset()
    for trio in xs:
        bufs.copy_(dev(trio))
        graphed()
        torch.cuda.synchronize()
        for i in range(repeat):
            ref.push(trio[i])
            np.testing.assert_array_equal(host(outs[i]), ref.by_age())
    assert int(hist.head) == (repeat * depth) % depth


# ---------------------------------------------------------------------------------------------------------------------------
# the two updates against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _certified_before(D, lo, hi):
    return P._certified(D.stacked, *P._bounds(lo, hi))


def _learn(case, n_pre, n_post, depth, name, *, which, inplace, steps, ring_depth=None, indptr_dtype=np.int32, seed=3, rate=RATE,
           compare_by_age=False):
    """``steps`` steps of pushes and updates (``which``: 'pre', 'post' or 'both') through the container and the restatement; the
    clip mode changes every second step, so every bounded mode is run uncertified, then certified (in place)."""
    data, indices, indptr, delays = case
    ring_depth = depth if ring_depth is None else ring_depth
    rng = np.random.default_rng(seed)
    D = build(case, (n_pre, n_post), depth, name, indptr_dtype)
    assert D.stacked.indptr.dtype == (torch.int64 if indptr_dtype == np.int64 else torch.int32)
    ring, ring_ref = be.SpikeRing(n_pre, ring_depth), DC.ring_np(n_pre, ring_depth)
    hist, hist_ref = be.ValueRing(n_pre, ring_depth, dtype=TORCH[name]), SC.value_ring_np(n_pre, ring_depth, name)
    w = np.asarray(data).reshape(-1)
    enc = ['bool', 'float', 'bitpacked', 'compact']
    certified_seen = False
    for t in range(steps):
        s, x = rng.random(n_pre) < rate, rng.normal(size=n_pre)
        ring.push(dev(s))
        ring_ref.push(s)
        hist.push(dev(x))                                                     # an f64 input into the ring's dtype
        hist_ref.push(x)
        lo, hi = CLIPS[(t // 2) % 3]
        if which in ('pre', 'both'):
            tr = rng.normal(size=n_post)
            want = SC.stacked_on_pre(w, indices, indptr, delays, n_pre, depth, ring_ref, tr, name, lo, hi)
            if inplace and t % 2 == 1 and lo is not None:
                assert _certified_before(D, lo, hi)
                certified_seen = True
            Dn = D.update_on_pre(ring, dev(tr), lo, hi, inplace=inplace)
            D, w = _after(D, Dn, w, want, name, inplace, f'on-pre step {t}')
        if which in ('post', 'both'):
            spk = rng.random(n_post) < 0.4
            want = SC.stacked_on_post(w, indices, indptr, delays, n_pre, depth, hist_ref, spk, name, lo, hi)
            if compare_by_age:
                by_age = D.update_on_post(hist.by_age()[:depth], on_device(encode(spk, 'bool')), lo, hi)
                assert shares_structure(by_age, D)
                assert_weights(by_age, want, name, f'by-age array, step {t}')
            if inplace and which == 'post' and t % 2 == 1 and lo is not None:
                assert _certified_before(D, lo, hi)
                certified_seen = True
            Dn = D.update_on_post(hist, on_device(encode(spk, enc[t % 4])), lo, hi, inplace=inplace)
            D, w = _after(D, Dn, w, want, name, inplace, f'on-post step {t} ({enc[t % 4]})')
    assert certified_seen == (inplace and steps >= 4)
    assert not np.array_equal(w, np.asarray(data).reshape(-1))               # something was learnt
    return D


def _after(D, Dn, w, want, name, inplace, msg):
    if inplace:
        assert Dn is D
    else:
        assert shares_structure(Dn, D) and Dn.depth == D.depth and Dn.shape == D.shape
        assert_weights(D, w, name, msg + ': the original')                   # untouched
        assert D.stacked.buffers.get(P.INDEX_KEY) is Dn.stacked.buffers.get(P.INDEX_KEY)
    assert_weights(Dn, want, name, msg)
    return Dn, want


@pytest.mark.parametrize('inplace', [False, True], ids=['new', 'inplace'])
@pytest.mark.parametrize('indptr_dtype', [np.int32, np.int64], ids=['i32', 'i64'])
@pytest.mark.parametrize('name', NAMES)
def test_update_on_pre(name, indptr_dtype, inplace):
    case = SC.stdp_case(41, N_PRE, N_POST, DEPTH, 32, name)
    _learn(case, N_PRE, N_POST, DEPTH, name, which='pre', inplace=inplace, steps=2 * DEPTH + 1, indptr_dtype=indptr_dtype)


@pytest.mark.parametrize('ring_depth', [DEPTH, DEPTH + 2])
@pytest.mark.parametrize('inplace', [False, True], ids=['new', 'inplace'])
@pytest.mark.parametrize('indptr_dtype', [np.int32, np.int64], ids=['i32', 'i64'])
@pytest.mark.parametrize('name', NAMES)
def test_update_on_post_through_the_value_ring(name, indptr_dtype, inplace, ring_depth):
    case = SC.stdp_case(42, N_PRE, N_POST, DEPTH, 32, name)
    _learn(case, N_PRE, N_POST, DEPTH, name, which='post', inplace=inplace, steps=2 * DEPTH + 1, indptr_dtype=indptr_dtype,
           ring_depth=ring_depth, compare_by_age=True)


@pytest.mark.parametrize('n_pre,n_post,depth,ends', [(9, 40, 256, False), (1, 20, 5, False), (33, 20, 5, False), (33, 20, 7, True)],
                         ids=['depth256', 'n_pre1', 'n_pre33', 'ends'])
def test_update_on_post_shapes(n_pre, n_post, depth, ends):
    case = SC.stdp_case(43, n_pre, n_post, depth, 32, ends=ends, fixed_len=24 if n_pre == 1 else None)
    if ends:
        assert set(case[3]) == {0, depth - 1}
    _learn(case, n_pre, n_post, depth, 'f32', which='both', inplace=True, steps=6 if depth == 256 else 2 * depth + 1,
           compare_by_age=True)


def test_depth_256_past_one_turn_of_the_ring():
    n_pre, n_post, depth = 9, 40, 256
    case = SC.stdp_case(44, n_pre, n_post, depth, 32)
    D = build(case, (n_pre, n_post), depth)
    rng = np.random.default_rng(2)
    hist, ref = be.ValueRing(n_pre, depth), SC.value_ring_np(n_pre, depth)
    xs = rng.normal(size=(depth + 5, n_pre)).astype(np.float32)
    for x in dev(xs):
        hist.push(x)
    for x in xs:
        ref.push(x)
    spk = rng.random(n_post) < 0.5
    want = SC.stacked_on_post(case[0], case[1], case[2], case[3], n_pre, depth, ref, spk, 'f32')
    assert_weights(D.update_on_post(hist, dev(spk)), want, 'f32')


def test_depth_one_is_the_undelayed_update():
    case = SC.stdp_case(45, N_PRE, N_POST, 1, 32)
    data, indices, indptr, _ = case
    D = build(case, (N_PRE, N_POST), 1)
    csr = be.CSR((dev(data), dev(indices), dev(indptr)), shape=(N_PRE, N_POST))
    rng = np.random.default_rng(6)
    ring, hist = be.SpikeRing(N_PRE, 1), be.ValueRing(N_PRE, 1)
    for t in range(3):
        s, x, tr, spk = dev(rng.random(N_PRE) < RATE), dev(rng.normal(size=N_PRE).astype(np.float32)), \
            dev(rng.normal(size=N_POST).astype(np.float32)), dev(rng.random(N_POST) < 0.4)
        ring.push(s)
        hist.push(x)
        D = D.update_on_post(hist, spk, -0.5, 0.75)
        csr = csr.update_on_post(x, spk, -0.5, 0.75)
        assert torch.equal(D.data, csr.data)
        D = D.update_on_pre(ring, tr, -0.5, 0.75)
        csr = csr.update_on_pre(s, tr, -0.5, 0.75)
        assert torch.equal(D.data, csr.data)


# ---------------------------------------------------------------------------------------------------------------------------
# loop bounds of the aged instantiation
# ---------------------------------------------------------------------------------------------------------------------------
def _sorted_csr(rows, cols, n_pre):
    order = np.argsort(rows, kind='stable')
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_pre))]).astype(np.int32)
    return order, indptr, cols[order].astype(np.int32)


def _aged_once(case, n_pre, n_post, depth, spk, seed=1, lo=None, hi=None):
    rng = np.random.default_rng(seed)
    D = build(case, (n_pre, n_post), depth)
    hist, ref = be.ValueRing(n_pre, depth + 1), SC.value_ring_np(n_pre, depth + 1)
    for _ in range(depth + 3):
        x = rng.normal(size=n_pre).astype(np.float32)
        hist.push(dev(x))
        ref.push(x)
    want = SC.stacked_on_post(case[0], case[1], case[2], case[3], n_pre, depth, ref, spk, 'f32', lo, hi)
    assert D.update_on_post(hist, dev(spk), lo, hi, inplace=True) is D
    assert_weights(D, want, 'f32')
    return D


def test_one_post_column_spanning_tiles():
    n_pre, n_post, depth = 300, 3, DEPTH
    L = 2 * TILE + 3
    rng = np.random.default_rng(9)
    rows = np.concatenate([np.arange(L) % n_pre, rng.integers(0, n_pre, 200)])
    cols = np.concatenate([np.zeros(L, np.int64), rng.integers(1, 3, 200)])
    order, indptr, indices = _sorted_csr(rows, cols, n_pre)
    delays = (rng.permutation(rows.size) % depth).astype(np.int32)
    assert set(delays[indices == 0]) == set(range(depth)) and (indices == 0).sum() == L
    data = rng.uniform(-1, 1, rows.size).astype(np.float32)
    _aged_once((data, indices, indptr, delays), n_pre, n_post, depth, np.array([True, False, False]))
    _aged_once((data, indices, indptr, delays), n_pre, n_post, depth, np.array([True, False, True]), lo=-0.5, hi=0.5)


def test_more_active_post_neurons_than_one_pass_of_the_offsets_scan():
    n_pre, depth = 33, 4
    n_post = SCAN_PASS + 5 + 64
    rng = np.random.default_rng(10)
    rows = rng.integers(0, n_pre, 2 * n_post)
    cols = np.concatenate([np.arange(n_post), rng.integers(0, n_post, n_post)])
    order, indptr, indices = _sorted_csr(rows, cols, n_pre)
    delays = rng.integers(0, depth, rows.size).astype(np.int32)
    data = rng.uniform(-1, 1, rows.size).astype(np.float32)
    spk = np.zeros(n_post, bool)
    spk[rng.permutation(n_post)[:SCAN_PASS + 5]] = True
    _aged_once((data, indices, indptr, delays), n_pre, n_post, depth, spk)


def test_one_call_past_one_grid_stride_of_tiles():
    n_pre, n_post, depth = TILE, GRID_CAP + 104, 4             # 4200 post neurons with 2048 entries each, all spiking
    assert n_post * n_pre > GRID_CAP * TILE
    rng = np.random.default_rng(12)
    indices = np.tile(np.arange(n_post, dtype=np.int32), n_pre)
    indptr = (np.arange(n_pre + 1, dtype=np.int64) * n_post).astype(np.int32)
    delays = rng.integers(0, depth, indices.size).astype(np.int32)
    data = rng.uniform(-1, 1, indices.size).astype(np.float32)
    _aged_once((data, indices, indptr, delays), n_pre, n_post, depth, np.ones(n_post, bool))


# ---------------------------------------------------------------------------------------------------------------------------
# plastic mode, capture
# ---------------------------------------------------------------------------------------------------------------------------
def _route(D, route):
    """As tests/test_delay_gpu.py: ``direct`` — nothing prepared; ``plan`` / ``binned`` — that workspace installed."""
    st = D.stacked
    if route == 'plan':
        st.buffers['scatter_plan'] = C.ScatterPlan.build(st.data, st.indices, st.indptr, shape=st.shape)
    elif route == 'binned':
        st.buffers['scatter_plan'] = C.BinnedScatter(st.data, st.shape[0], st.shape[1], st.nse, indices=st.indices,
                                                     indptr=st.indptr)
    return D


def q64(rng, n, lo, hi):
    return (rng.integers(int(lo * 64), int(hi * 64) + 1, n) / 64.0).astype(np.float32)


def _forbid_full_refresh(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError('a full refresh ran on an armed container')
    monkeypatch.setattr(C.ScatterPlan, 'refresh_weights', boom)
    monkeypatch.setattr(C.ScatterPlan, '_fill', boom)


@pytest.mark.parametrize('route', ['plan', 'binned', 'direct'])
def test_plastic_mode_keeps_the_product_current(route, monkeypatch):
    case = SC.stdp_case(51, N_PRE, N_POST, DEPTH, 32, exact=True)
    data, indices, indptr, delays = case
    D = _route(build(case, (N_PRE, N_POST), DEPTH), route)
    ws = D.stacked.buffers.get('scatter_plan')
    assert D.prepare(plastic=(0.0, 1.0)) is D
    st = D.plastic_state
    assert st is not None and st['route'].startswith(route) and (st['w_min'], st['w_max']) == (0.0, 1.0)
    assert D.stacked.buffers.get('scatter_plan') is ws
    _forbid_full_refresh(monkeypatch)
    rng = np.random.default_rng(13)
    ring, ring_ref = be.SpikeRing(N_PRE, DEPTH), DC.ring_np(N_PRE, DEPTH)
    hist, hist_ref = be.ValueRing(N_PRE, DEPTH), SC.value_ring_np(N_PRE, DEPTH)
    w = data
    for t in range(DEPTH + 2):
        s, x = rng.random(N_PRE) < RATE, q64(rng, N_PRE, -0.25, 0.25)
        tr, spk = q64(rng, N_POST, -0.25, 0.25), rng.random(N_POST) < 0.4
        ring.push(dev(s))
        ring_ref.push(s)
        hist.push(dev(x))
        hist_ref.push(x)
        w = SC.stacked_on_pre(w, indices, indptr, delays, N_PRE, DEPTH, ring_ref, tr, 'f32', 0.0, 1.0)
        assert D.update_on_pre(ring, dev(tr), 0.0, 1.0, inplace=True) is D
        assert_weights(D, w, 'f32', f'on-pre {t}')
        w = SC.stacked_on_post(w, indices, indptr, delays, N_PRE, DEPTH, hist_ref, spk, 'f32', 0.0, 1.0)
        assert D.update_on_post(hist, dev(spk), 0.0, 1.0, inplace=True) is D
        assert_weights(D, w, 'f32', f'on-post {t}')
        got = ring @ D
        fresh = be.DelayedCSR((D.data, dev(indices), dev(indptr), dev(delays)), shape=(N_PRE, N_POST), depth=DEPTH)
        assert torch.equal(got, ring @ fresh), f'step {t}'
        np.testing.assert_array_equal(host(got).astype(np.float64),
                                      DC.delayed_currents_np(w, indices, indptr, delays, ring_ref, N_POST), err_msg=f'step {t}')
    assert D.plastic_state is not None and D.stacked.buffers.get('scatter_plan') is ws


@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_captured_learning_step(route):
    """push, push, product and both updates, three steps per replay against depth 7: the replayed graph ends with the weights of
    the eager loop, bit for bit."""
    repeat, depth = 3, 7
    case = SC.stdp_case(52, N_PRE, N_POST, depth, 32, exact=True)
    rng = np.random.default_rng(14)
    n_rep = depth
    S = rng.random((n_rep, repeat, N_PRE)) < RATE
    X = q64(rng, n_rep * repeat * N_PRE, -0.25, 0.25).reshape(n_rep, repeat, N_PRE)
    T = q64(rng, n_rep * repeat * N_POST, -0.25, 0.25).reshape(n_rep, repeat, N_POST)
    K = rng.random((n_rep, repeat, N_POST)) < 0.4

    def make():
        D = _route(build(case, (N_PRE, N_POST), depth), route).prepare(plastic=(0.0, 1.0))
        return D, be.SpikeRing(N_PRE, depth), be.ValueRing(N_PRE, depth)

    def one(D, ring, hist, s, x, tr, spk, out):
        ring.push(s)
        hist.push(x)
        out.copy_(ring @ D)
        D.update_on_pre(ring, tr, 0.0, 1.0, inplace=True)
        D.update_on_post(hist, spk, 0.0, 1.0, inplace=True)

    D, ring, hist = make()
    eager = []
    for r in range(n_rep):
        for i in range(repeat):
            out = torch.zeros(N_POST, device='cuda')
            one(D, ring, hist, dev(S[r, i]), dev(X[r, i]), dev(T[r, i]), dev(K[r, i]), out)
            eager.append(out)
    # captured: sub-step i of a replay reads the i-th row of every buffer.  The buffers are zero while the graph is warmed up and
    # captured, so those runs learn nothing; the rings are reset afterwards
    D2, ring2, hist2 = make()
    sb, kb = (torch.zeros((repeat, n), dtype=torch.bool, device='cuda') for n in (N_PRE, N_POST))
    xb, tb, outs = (torch.zeros((repeat, n), device='cuda') for n in (N_PRE, N_POST, N_POST))
    k = [0]

    def step():
        i = k[0] % repeat
        k[0] += 1
        one(D2, ring2, hist2, sb[i], xb[i], tb[i], kb[i], outs[i])

    graphed = be.capture_step(step, warmup=repeat, repeat=repeat)
    ring2.reset()
    hist2.reset()
    assert torch.equal(D2.data, dev(case[0]))
    got = []
    for r in range(n_rep):
        for buf, src in ((sb, S), (xb, X), (tb, T), (kb, K)):
            buf.copy_(dev(src[r]))
        graphed()
        torch.cuda.synchronize()
        got.extend(outs.clone())
    for t, (g, e) in enumerate(zip(got, eager)):
        assert torch.equal(g, e), f'step {t}'
    assert torch.equal(D2.data, D.data) and not torch.equal(D.data, dev(case[0]))
    assert torch.equal(ring2.bits, ring.bits) and torch.equal(hist2.values, hist.values)


# ---------------------------------------------------------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['direct', 'plan'])
def test_weight_gradient_over_three_steps(route):
    """Several forwards on one ring — which reuses one id buffer — then one backward: each step's own activity counts."""
    case = SC.stdp_case(61, N_PRE, N_POST, DEPTH, 32, exact=True)
    data, indices, indptr, delays = case
    D = _route(build(case, (N_PRE, N_POST), DEPTH), route)
    leaf = D.stacked.data.requires_grad_(True)
    rng = np.random.default_rng(15)
    ring, ref = be.SpikeRing(N_PRE, DEPTH), DC.ring_np(N_PRE, DEPTH)
    loss, want = 0.0, np.zeros(indices.size)
    for _ in range(3):
        s, g = rng.random(N_PRE) < RATE, rng.integers(-64, 65, N_POST) / 64.0
        ring.push(dev(s))
        ref.push(s)
        y = ring @ D
        assert y.requires_grad
        loss = loss + (dev(g.astype(np.float32)) * y).sum()
        want += SC.brute_grad(indices, indptr, delays, ref, g)
    loss.backward()
    assert leaf.grad is not None and leaf.grad.shape == leaf.shape
    grad = D.stacked_to_original(leaf.grad)
    assert tuple(grad.shape) == data.shape and grad.dtype == torch.float32
    np.testing.assert_array_equal(host(grad).astype(np.float64), want)
    assert np.count_nonzero(want) > 0 and not np.array_equal(want, 3 * SC.brute_grad(indices, indptr, delays, ref, g))
    with torch.no_grad():                                  # no grad mode: the plain path, same bits
        assert torch.equal(ring @ D, y.detach())
    with pytest.raises(ValueError):
        D.stacked_to_original(leaf.grad[:-1])


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    case = SC.stdp_case(71, N_PRE, N_POST, DEPTH, 8)
    D = build(case, (N_PRE, N_POST), DEPTH)
    w0 = D.data.clone()
    ring, hist = be.SpikeRing(N_PRE, DEPTH), be.ValueRing(N_PRE, DEPTH)
    tr, spk = torch.zeros(N_POST, device='cuda'), torch.ones(N_POST, dtype=torch.bool, device='cuda')
    shared = build((np.ones(1, np.float32),) + case[1:], (N_PRE, N_POST), DEPTH)
    with pytest.raises(ValueError, match='homogeneous'):
        shared.update_on_pre(ring, tr)
    with pytest.raises(ValueError, match='homogeneous'):
        shared.update_on_post(hist, spk)
    with pytest.raises(ValueError, match='homogeneous'):
        shared.prepare(plastic=(0.0, 2.0))
    with pytest.raises(ValueError, match='71 neurons'):
        D.update_on_pre(be.SpikeRing(N_PRE + 1, DEPTH), tr)
    with pytest.raises(ValueError, match='remembers 5 steps'):
        D.update_on_pre(be.SpikeRing(N_PRE, DEPTH - 1), tr)
    with pytest.raises(ValueError, match='71 neurons'):
        D.update_on_post(be.ValueRing(N_PRE + 1, DEPTH), spk)
    with pytest.raises(ValueError, match='remembers 5 steps'):
        D.update_on_post(be.ValueRing(N_PRE, DEPTH - 1), spk)
    with pytest.raises(TypeError, match='float16'):
        D.update_on_post(be.ValueRing(N_PRE, DEPTH, dtype=torch.float16), spk)
    with pytest.raises(ValueError, match='by age must have shape'):
        D.update_on_post(hist.by_age()[:DEPTH - 1], spk)
    with pytest.raises(TypeError, match='SpikeRing'):
        D.update_on_pre(hist, tr)
    assert torch.equal(D.data, w0)
    # a deeper history serves a shallower matrix; a history in another dtype goes through the by-age array
    deep = be.ValueRing(N_PRE, DEPTH + 3, dtype=torch.float64).push(np.ones(N_PRE))
    got = D.update_on_post(deep.by_age()[:DEPTH], spk)
    d0 = np.asarray(case[3]) == 0
    np.testing.assert_array_equal(host(got.data), (case[0] + d0.astype(np.float32)).astype(np.float32))
