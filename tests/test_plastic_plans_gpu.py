"""Plastic mode on the device: after ``prepare(plastic=(w_min, w_max))`` every in-place STDP update keeps the container's cached
scatter workspace current itself (``be_scatter_plan_refresh_rows`` / ``be_scatter_plan_patch_entries``), so the next scatter-side
product launches no refresh — on every route, for every container, under graph capture, and past the one-pass sizes of the two
new kernels.

Weights, traces and bounds are multiples of 2^-8 and column sums stay below 2^16: every sum is exact in f32 whatever its order
(the direct route's float atomics included), so products are compared bit for bit with ``float32(exact sum)``."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _csr as C
from brainevent_amd import _plasticity as P
from brainevent_amd._error import MathError
from test_plasticity_cpu import model_cols, model_rows, row_of
from test_plasticity_gpu import assert_bit_equal, encode, host

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
KINDS = ['csr', 'csc', 'fcn_pre', 'fcn_post']
ROUTES = ['plan-d8', 'plan-u16', 'binned', 'direct']
ENC = ['bool', 'float', 'bitpacked', 'compact', 'uint8', 'binary']


# ------------------------------------------------------------------------------------------------------------ helpers
def q8(rng, n, lo=0.0, hi=1.0):
    """n multiples of 2^-8 in [lo, hi]."""
    return (rng.integers(int(lo * 256), int(hi * 256) + 1, n) / 256.0).astype(np.float32)


def ragged(rng, m, k, max_len, long_row=None):
    """rows of 0..max_len entries, empty rows, a duplicated column, optionally one long row."""
    lens = rng.integers(0, max_len + 1, m)
    lens[::7] = 0
    lens[1] = max(lens[1], 3)
    if long_row:
        lens[m // 2] = long_row
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    idx[ptr[1] + 1] = idx[ptr[1]]
    return idx, ptr


def fixed(rng, m, k, nc):
    idx = rng.integers(0, k, (m, nc)).astype(np.int32)
    idx[0, 1] = idx[0, 0]
    return idx.reshape(-1), (np.arange(m + 1) * nc).astype(np.int32)


def container(kind, w, idx, ptr, m, k, dtype=torch.float32):
    """`m` stored rows over `k` secondary ids as a container of `kind` (CSC / FixedNumPerPost store the transpose)."""
    wd = torch.tensor(w, device=DEV).to(dtype)
    idx_d = torch.tensor(idx, device=DEV)
    shape = (m, k) if kind in ('csr', 'fcn_pre') else (k, m)
    if kind in ('csr', 'csc'):
        return (be.CSR if kind == 'csr' else be.CSC)((wd, idx_d, torch.tensor(ptr, device=DEV)), shape=shape)
    nc = len(idx) // m
    return (be.FixedNumPerPre if kind == 'fcn_pre' else be.FixedNumPerPost)((wd.view(m, nc), idx_d.view(m, nc)), shape=shape)


def install(M, route, slice_width=2000, keep_order=True):
    """Put the workspace of `route` into the container's cache (arming uses a fresh cached workspace as it is)."""
    r = M._stored_rows()
    w, idx = M.data.reshape(-1), r.indices.reshape(-1)
    if route == 'plan-d8':
        ws = C.ScatterPlan.build(w, idx, r.indptr, shape=(r.m, r.k), row_len=r.row_len, slice_width=slice_width, layout='d8',
                                 keep_order=keep_order)
        assert ws.layout == C.ScatterPlan.LAYOUT_D8 and (ws.order is not None) == keep_order
    elif route == 'plan-u16':
        ws = C.ScatterPlan.build(w, idx, r.indptr, shape=(r.m, r.k), row_len=r.row_len, slice_shift=11, slice_width=slice_width,
                                 layout='u16')
        assert ws.layout == C.ScatterPlan.LAYOUT_U16
    elif route == 'binned':
        ws = C.BinnedScatter(w, r.m, r.k, int(idx.numel()), indices=idx, indptr=r.indptr, row_len=r.row_len)
    else:
        ws = None
    M.buffers['scatter_plan'] = ws
    return ws


def upd_rows(M, spk, trace, lo, hi):
    """The update whose spikes lie on the stored rows (row refresh)."""
    if M._stored_transposed:
        return M.update_on_post(trace, spk, lo, hi, inplace=True)
    return M.update_on_pre(spk, trace, lo, hi, inplace=True)


def upd_cols(M, spk, trace, lo, hi):
    """The update whose spikes lie on the secondary ids (entry patch)."""
    if M._stored_transposed:
        return M.update_on_pre(spk, trace, lo, hi, inplace=True)
    return M.update_on_post(trace, spk, lo, hi, inplace=True)


def scatter_product(M, spk_rows):
    ev = be.BinaryArray(torch.tensor(spk_rows, device=DEV))
    return (M @ ev) if M._stored_transposed else (ev @ M)


def exact_product(w, idx, ptr, spk_rows, k):
    """float64 sums of the active rows' entries per column (exact for the values used here)."""
    act = np.asarray(spk_rows, bool)[row_of(ptr)]
    wf = (w.float() if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w)).float()).numpy().astype(np.float64)
    return np.bincount(idx[act], weights=wf[act], minlength=k)


def check_product(M, w, idx, ptr, spk_rows, k, tag):
    got = scatter_product(M, spk_rows)
    want = torch.from_numpy(exact_product(w, idx, ptr, spk_rows, k).astype(np.float32)).to(M.data.dtype)
    assert_bit_equal(got, want, tag)


def forbid_full_refresh(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError('a full refresh ran on an armed container')
    monkeypatch.setattr(C.ScatterPlan, 'refresh_weights', boom)
    monkeypatch.setattr(C.ScatterPlan, '_fill', boom)
    monkeypatch.setattr(C.BinnedScatter, '_derive_exponent', boom)


def learn(M, w, idx, ptr, m, k, rng, steps, lo, hi, tag, p_rows=0.3, p_cols=0.3, after=None):
    """`steps` alternating row-side / column-side updates through the container and the host model; the product after each."""
    for t in range(steps):
        if t % 2 == 0:
            spk, tr = rng.random(m) < p_rows, q8(rng, k, -1.0, 1.0)
            upd_rows(M, encode(spk, ENC[t % len(ENC)]), tr, lo, hi)
            w = model_rows(w, idx, ptr, spk, tr, lo, hi)
        else:
            spk, tr = rng.random(k) < p_cols, q8(rng, m, -1.0, 1.0)
            upd_cols(M, encode(spk, ENC[t % len(ENC)]), tr, lo, hi)
            w = model_cols(w, idx, ptr, spk, tr, lo, hi)
        assert_bit_equal(M.data.reshape(-1), w, f'{tag}: weights after update {t}')
        if after is not None:
            after(t)
        check_product(M, w, idx, ptr, rng.random(m) < 0.4, k, f'{tag}: product after update {t}')
    return w


# ------------------------------------------------------------------------------------------------------------ 1. the blocks
@pytest.mark.parametrize('kind', ['csr', 'csc'])
@pytest.mark.parametrize('keep_order', [True, False])
def test_blocks_identical_to_a_full_refresh(kind, keep_order):
    rng = np.random.default_rng(21)
    m, k = 600, 6000
    idx, ptr = ragged(rng, m, k, 80, long_row=5000)
    w = q8(rng, len(idx))
    M = container(kind, w, idx, ptr, m, k)
    plan = install(M, 'plan-d8', slice_width=2000, keep_order=keep_order)
    assert plan.n_slices == 3
    assert bool((plan.blob == 255).any())                 # (the structure does produce escape bytes)
    M.prepare(plastic=(0.0, 1.0))
    assert M.plastic_state['route'] == 'plan-d8' and M.buffers['scatter_plan'] is plan
    twin = C.ScatterPlan(m, k, False, plan.slice_shift, plan.seg, plan.blob.clone(), plan.scale_exp, plan.weight_dtype,
                         plan.slice_width, plan.layout)
    twin.nnz, twin.row_len, twin.order = plan.nnz, plan.row_len, plan.order
    seg0 = plan.seg.clone()
    r = M._stored_rows()

    def same_blocks(t):
        assert not plan.is_stale(M.data)
        twin.refresh_weights(M.data, r.indices, r.indptr)
        assert torch.equal(plan.blob, twin.blob), f'blocks differ from a full refresh after update {t}'
        assert torch.equal(plan.seg, seg0)

    learn(M, w, idx, ptr, m, k, rng, 4, 0.0, 1.0, f'{kind}', after=same_blocks)
    assert plan.slot is not None and plan.nbytes() >= plan.blob.numel() + 2 * plan.slot.numel()
    assert M.plastic_state is not None


# ------------------------------------------------------------------------------------------------------------ 2. every route
def route_case(kind, route, dtype, monkeypatch, seed):
    rng = np.random.default_rng(seed)
    m, k = 300, 5000
    idx, ptr = ragged(rng, m, k, 60, long_row=700) if kind in ('csr', 'csc') else fixed(rng, m, k, 48)
    w = q8(rng, len(idx))
    M = container(kind, w, idx, ptr, m, k, dtype)
    ws = install(M, route, slice_width=1700)
    if route.startswith('plan'):
        assert ws.n_slices == 3
    M.prepare(plastic=(0.0, 1.0))
    st = M.plastic_state
    assert st['route'] == route and (st['w_min'], st['w_max']) == (0.0, 1.0)
    assert (st['exponent'] is None) == (route == 'direct')
    forbid_full_refresh(monkeypatch)
    w0 = host(M.data.reshape(-1))
    learn(M, w0, idx, ptr, m, k, rng, 4, 0.0, 1.0, f'{kind}/{route}/{dtype}')
    assert M.plastic_state is not None and M.buffers['scatter_plan'] is ws


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('kind', KINDS)
def test_products_on_every_route(kind, route, monkeypatch):
    route_case(kind, route, torch.float32, monkeypatch, 31)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('kind', ['csr', 'fcn_post'])
def test_half_precision_weights_on_a_plan(kind, dtype, monkeypatch):
    route_case(kind, 'plan-d8', dtype, monkeypatch, 32)


# ------------------------------------------------------------------------------------------------------------ 3. the bound
@pytest.mark.parametrize('route', ['plan-d8', 'plan-u16', 'binned'])
def test_the_exponent_bound_prevents_overflow(route, monkeypatch):
    m, k = 40, 1024                                        # every row lists every column: 40 entries per column
    idx = np.tile(np.arange(k, dtype=np.int32), m)
    ptr = (np.arange(m + 1) * k).astype(np.int32)
    w = np.full(m * k, 2.0 ** -10, np.float32)
    hi = 2.0 ** 20
    M = container('csr', w, idx, ptr, m, k)
    ws = install(M, route, slice_width=512)
    e_weights = ws.scale_exp                               # derived from the initial weights: fine for 40 * 2^-10 ...
    assert 40 * hi * 2.0 ** e_weights >= 2.0 ** 63         # ... and wraps 64-bit sums once the weights reach the bound
    M.prepare(plastic=(0.0, hi))
    st = M.plastic_state
    assert st['cmax'] == 40
    assert st['exponent'] <= P.plastic_exponent_bound(40, hi) == 36
    forbid_full_refresh(monkeypatch)
    every = np.ones(m, bool)
    check_product(M, w, idx, ptr, every, k, 'before learning')
    upd_rows(M, every, np.full(k, hi, np.float32), 0.0, hi)
    w = model_rows(w, idx, ptr, every, np.full(k, hi, np.float32), 0.0, hi)
    assert (w == hi).all()
    assert_bit_equal(M.data, w, 'weights at the bound')
    got = scatter_product(M, every)
    assert float(got.max()) == float(got.min()) == 40 * hi
    assert M.plastic_state['exponent'] == st['exponent']


def test_the_bound_itself_must_keep_its_bits():
    rng = np.random.default_rng(5)
    m, k = 64, 512
    idx, ptr = fixed(rng, m, k, 16)
    M = container('csr', np.zeros(len(idx), np.float32), idx, ptr, m, k)
    install(M, 'plan-d8', slice_width=256)
    with pytest.raises(MathError):
        M.prepare(plastic=(0.0, 0.0))                      # B == 0: no bits at any exponent
    assert M.plastic_state is None


# ------------------------------------------------------------------------------------------------------------ 4. fallbacks
def small_case(rng, kind='csr', route='plan-d8', dtype=torch.float32):
    m, k = 200, 3000
    idx, ptr = ragged(rng, m, k, 40)
    w = q8(rng, len(idx))
    M = container(kind, w, idx, ptr, m, k, dtype)
    install(M, route, slice_width=1000)
    return M, w, idx, ptr, m, k


@pytest.mark.parametrize('how', ['foreign write', 'other bounds', 'no bounds'])
@pytest.mark.parametrize('route', ['plan-d8', 'binned'])
def test_fallbacks_disarm_and_stay_correct(how, route):
    rng = np.random.default_rng(41)
    M, w, idx, ptr, m, k = small_case(rng, route=route)
    M.prepare(plastic=(0.0, 1.0))
    w = learn(M, w, idx, ptr, m, k, rng, 2, 0.0, 1.0, 'armed')
    assert M.plastic_state is not None
    lo, hi = 0.0, 1.0
    if how == 'foreign write':
        M.data[5] = 0.5
        w[5] = 0.5
    elif how == 'other bounds':
        lo, hi = 0.0, 0.75
    else:
        lo, hi = None, None
    w = learn(M, w, idx, ptr, m, k, rng, 2, lo, hi, how)          # through today's path: whole-array clip, full refresh
    assert M.plastic_state is None
    learn(M, w, idx, ptr, m, k, rng, 2, 0.0, 1.0 if how != 'other bounds' else 0.75, how + ', afterwards')
    assert M.plastic_state is None                                 # disarmed until prepare(plastic=...) is called again


@pytest.mark.parametrize('route', ['plan-u16', 'plan-d8'])
def test_rearming_after_a_full_refresh_builds_new_slots(route):
    """arm, patch, disarm, product (full refresh: a u16 fill draws every block position anew), re-arm, patch: the slot table of
    the first arming must not survive the refresh."""
    rng = np.random.default_rng(45)
    m, k = 120, 2500
    idx, ptr = ragged(rng, m, k, 900)                      # rows far above the 256 entries one pass of a u16 fill places
    assert np.diff(ptr).max() > 512
    w = q8(rng, len(idx))
    M = container('csr', w, idx, ptr, m, k)
    plan = install(M, route, slice_width=1250)
    M.prepare(plastic=(0.0, 1.0))

    def patch(w, lo=0.0, hi=1.0):
        spk, tr = rng.random(k) < 0.5, q8(rng, m, -1.0, 1.0)
        upd_cols(M, spk, tr, lo, hi)
        return model_cols(w, idx, ptr, spk, tr, lo, hi)

    w = patch(w)
    assert plan.slot is not None and M.plastic_state is not None
    check_product(M, w, idx, ptr, rng.random(m) < 0.5, k, 'armed')
    w = patch(w, 0.0, 0.75)                                # other bounds: disarms, the table is dropped
    assert M.plastic_state is None and plan.slot is None
    check_product(M, w, idx, ptr, rng.random(m) < 0.5, k, 'after the full refresh')
    assert M.buffers['scatter_plan'] is plan and not plan.is_stale(M.data)
    M.prepare(plastic=(0.0, 0.75))
    assert M.buffers['scatter_plan'] is plan and plan.slot is None
    for t in range(3):
        w = patch(w, 0.0, 0.75)
        assert M.plastic_state is not None and plan.slot is not None
        assert_bit_equal(M.data, w, f're-armed: weights {t}')
        check_product(M, w, idx, ptr, np.ones(m, bool), k, f're-armed: product {t}')
        spk, tr = rng.random(m) < 0.5, q8(rng, k, -1.0, 1.0)       # a row refresh in between moves u16 slots again
        upd_rows(M, spk, tr, 0.0, 0.75)
        w = model_rows(w, idx, ptr, spk, tr, 0.0, 0.75)
        check_product(M, w, idx, ptr, np.ones(m, bool), k, f're-armed: product after a row refresh {t}')


def test_a_fill_voids_the_slot_table():
    rng = np.random.default_rng(46)
    M, w, idx, ptr, m, k = small_case(rng, route='plan-u16')
    plan = M.buffers['scatter_plan']
    M.prepare(plastic=(0.0, 1.0))
    upd_cols(M, rng.random(k) < 0.5, q8(rng, m, -1.0, 1.0), 0.0, 1.0)
    assert plan.slot is not None
    r = M._stored_rows()
    plan.refresh_weights(M.data, r.indices, r.indptr)      # every block rewritten: positions drawn anew
    assert plan.slot is None


def test_not_inplace_returns_an_unarmed_container():
    rng = np.random.default_rng(42)
    M, w, idx, ptr, m, k = small_case(rng)
    M.prepare(plastic=(0.0, 1.0))
    spk, tr = rng.random(m) < 0.3, q8(rng, k, -1.0, 1.0)
    out = M.update_on_pre(spk, tr, 0.0, 1.0)
    assert out.plastic_state is None and M.plastic_state is not None
    assert_bit_equal(out.data, model_rows(w, idx, ptr, spk, tr, 0.0, 1.0))
    assert_bit_equal(M.data, w)


def test_arming_refuses_what_it_cannot_certify():
    rng = np.random.default_rng(43)
    M, w, idx, ptr, m, k = small_case(rng)
    w_before = M.data.clone()
    with pytest.raises(ValueError, match='clamp'):
        M.prepare(plastic=(0.0, 0.5))                      # weights reach 1.0
    with pytest.raises(ValueError, match='clamp'):
        M.prepare(plastic=(0.25, 1.0))
    assert torch.equal(M.data, w_before) and M.plastic_state is None        # never modified
    with pytest.raises(ValueError, match='host numbers'):
        M.prepare(plastic=(torch.zeros((), device=DEV), 1.0))
    with pytest.raises(ValueError, match='release_raw'):
        M.prepare(plastic=(0.0, 1.0), release_raw=True)
    idx_d, ptr_d = torch.tensor(idx, device=DEV), torch.tensor(ptr, device=DEV)
    homo = be.CSR((torch.tensor([0.5], device=DEV), idx_d, ptr_d), shape=(m, k))
    with pytest.raises(ValueError, match='heterogeneous'):
        homo.prepare(plastic=(0.0, 1.0))
    f64 = be.CSR((torch.tensor(w, device=DEV).double(), idx_d, ptr_d), shape=(m, k))
    with pytest.raises(ValueError, match='f64'):
        f64.prepare(plastic=(0.0, 1.0))
    nan = container('csr', np.where(np.arange(len(w)) == 3, np.nan, w).astype(np.float32), idx, ptr, m, k)
    with pytest.raises(ValueError, match='clamp'):
        nan.prepare(plastic=(0.0, 1.0))
    assert M.prepare(plastic=(0.0, 1.0)).plastic_state['route'] == 'plan-d8'


def test_arming_builds_a_workspace_that_keeps_its_order():
    rng = np.random.default_rng(44)
    m, k, nc = 1200, 4000, 40
    idx, ptr = fixed(rng, m, k, nc)
    assert m * nc >= C.PLAN_MIN_NNZ
    M = container('csr', q8(rng, m * nc), idx, ptr, m, k)
    st = M.prepare(plastic=(0.0, 1.0)).plastic_state
    ws = M.buffers['scatter_plan']
    if isinstance(ws, C.ScatterPlan) and ws.layout == C.ScatterPlan.LAYOUT_D8:
        assert ws.order is not None
    assert st['cmax'] == int(np.bincount(idx, minlength=k).max())
    assert st['exponent'] <= P.plastic_exponent_bound(st['cmax'], 1.0)


# ------------------------------------------------------------------------------------------------------------ 5. graph capture
def test_graph_capture_replays_a_learning_step():
    rng = np.random.default_rng(51)
    m, k, steps, warm = 400, 4500, 20, 3
    idx, ptr = ragged(rng, m, k, 60, long_row=1500)
    w = q8(rng, len(idx))
    spk_r = torch.tensor(rng.random((steps + warm, m)) < 0.2, device=DEV)
    spk_c = torch.tensor(rng.random((steps + warm, k)) < 0.2, device=DEV)
    tr_k = torch.tensor(np.stack([q8(rng, k, -1.0, 1.0) for _ in range(steps + warm)]), device=DEV)
    tr_m = torch.tensor(np.stack([q8(rng, m, -1.0, 1.0) for _ in range(steps + warm)]), device=DEV)

    def make():
        M = container('csr', w, idx, ptr, m, k)
        plan = install(M, 'plan-d8', slice_width=1500)
        assert plan.n_slices == 3
        M.prepare(plastic=(0.0, 1.0))
        io = dict(sr=torch.zeros(m, dtype=torch.bool, device=DEV), sc=torch.zeros(k, dtype=torch.bool, device=DEV),
                  tk=torch.zeros(k, device=DEV), tm=torch.zeros(m, device=DEV), out=torch.zeros(k, device=DEV))
        return M, io

    def step(M, io):
        io['out'].copy_(be.BinaryArray(io['sr']) @ M)
        M.update_on_pre(io['sr'], io['tk'], 0.0, 1.0, inplace=True)
        M.update_on_post(io['tm'], io['sc'], 0.0, 1.0, inplace=True)

    def feed(io, t):
        io['sr'].copy_(spk_r[t]); io['sc'].copy_(spk_c[t]); io['tk'].copy_(tr_k[t]); io['tm'].copy_(tr_m[t])

    Me, ie = make()
    eager = []
    for t in range(steps + warm):
        feed(ie, 0 if t < warm else t)                     # (the capture warms up with `warm` eager steps on the first inputs)
        step(Me, ie)
        eager.append(ie['out'].clone())
    Mg, ig = make()
    feed(ig, 0)
    graphed = be.capture_step(lambda: step(Mg, ig), warmup=warm)
    assert Mg.plastic_state is not None
    for t in range(warm, steps + warm):
        feed(ig, t)
        graphed()
        assert_bit_equal(ig['out'], eager[t], f'product of replay {t - warm}')
    torch.cuda.synchronize()
    assert Me.plastic_state is not None
    assert not torch.equal(Me.data, torch.tensor(w, device=DEV))
    assert_bit_equal(Mg.data, Me.data, 'weights')
    # the eager twin against the host model: the captured step is compared with something that is itself right
    wh = w
    for t in range(steps + warm):
        tt = 0 if t < warm else t
        exp = exact_product(wh, idx, ptr, spk_r[tt].cpu().numpy(), k).astype(np.float32)
        assert_bit_equal(eager[t], exp, f'eager product {t}')
        wh = model_rows(wh, idx, ptr, spk_r[tt].cpu().numpy(), tr_k[tt].cpu().numpy(), 0.0, 1.0)
        wh = model_cols(wh, idx, ptr, spk_c[tt].cpu().numpy(), tr_m[tt].cpu().numpy(), 0.0, 1.0)
    assert_bit_equal(Me.data, wh, 'eager weights')


# ------------------------------------------------------------------------------------------------------------ 6. loop bounds
# be_scatter_plan_refresh_rows: the list of active rows is walked with a grid stride — 2048 workgroups (d8), 4096 (u16);
#   a u16 row is walked 256 entries at a time; a d8 thread owns ceil(len / 1024) sorted positions (tests 1, 2, 5: rows above 1024).
# be_scatter_plan_patch_entries: the offsets of the active ids come 16384 per pass; the tiles of 2048 entries are walked with a
#   grid stride of 4096 workgroups (8 388 608 touched entries per trip).
@pytest.mark.parametrize('route, m', [('plan-d8', 2048 + 150), ('plan-u16', 4096 + 150)])
def test_more_active_rows_than_workgroups(route, m, monkeypatch):
    rng = np.random.default_rng(61)
    k = 3000
    idx, ptr = ragged(rng, m, k, 6, long_row=300)          # (300 > 256: a u16 row walked twice)
    w = q8(rng, len(idx))
    M = container('csr', w, idx, ptr, m, k)
    install(M, route, slice_width=1000)
    M.prepare(plastic=(0.0, 1.0))
    forbid_full_refresh(monkeypatch)
    learn(M, w, idx, ptr, m, k, rng, 2, 0.0, 1.0, route, p_rows=1.0, p_cols=0.5)       # every row active, then a patch


def test_patch_past_one_offsets_pass_and_one_grid_of_tiles(monkeypatch):
    rng = np.random.default_rng(62)
    m, k, nc = 2100, 16384 + 700, 4000
    assert m * nc > 4096 * 2048 and k > 16384
    idx_d = torch.randint(0, k, (m, nc), dtype=torch.int32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    w_d = torch.randint(0, 257, (m, nc), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)).float() / 256
    M = be.FixedNumPerPre((w_d.clone(), idx_d), shape=(m, k))
    install(M, 'plan-d8', slice_width=8600)
    M.prepare(plastic=(0.0, 1.0))
    forbid_full_refresh(monkeypatch)
    spk = torch.ones(k, dtype=torch.bool, device=DEV)      # every column active: every entry is touched
    tr = torch.tensor(q8(rng, m, -1.0, 1.0), device=DEV)
    M.update_on_post(tr, spk, 0.0, 1.0, inplace=True)
    w_new = (w_d + tr[:, None]).clamp_(0.0, 1.0)
    assert torch.equal(M.data, w_new)
    rows_on = torch.tensor(rng.random(m) < 0.3, device=DEV)
    got = be.BinaryArray(rows_on) @ M
    want = torch.zeros(k, dtype=torch.float64, device=DEV)
    want.index_add_(0, idx_d[rows_on].reshape(-1).long(), w_new[rows_on].reshape(-1).double())
    assert torch.equal(got, want.float())
    assert M.plastic_state is not None
