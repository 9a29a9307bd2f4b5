"""The plasticity (csrc/be_plasticity.hip) and gradient (csrc/be_grad.hip) kernels past their one-pass sizes: every
multi-pass loop, grid-stride loop and grid split of the two files is crossed by a named case and compared with the host
models of tests/test_plasticity_cpu.py / tests/test_autograd_cpu.py — bit for bit, except the shared-weight gradient with
random values (an error bound derived in `homo_bound`) and the route-independence product (the tolerance of
test_plasticity_gpu.py::test_cached_workspaces_follow_an_inplace_update).  Every case starts with host-side asserts that its
sizes really cross the loop bound it is there for; the bounds are the entries of THRESHOLDS, which
tests/test_update_kernels_thresholds_cpu.py compares with the HIP sources.

Which loop is reached where:
  k_plast_offsets, second and later scan passes (carry)       test_scan_pass_boundaries, test_sparse_plasticity_large
  k_plast_rows, tile grid-stride + clip + 4 dtypes + i32 perm  test_sparse_plasticity_large
  k_plast_rows, rows > one tile / across workgroups / equal offs test_one_huge_row_among_empty_rows, test_sparse_plasticity_large
  k_plast_dense_rows, gridDim.y > 1 and the row loop           test_dense_plasticity_pre_column_split
  k_plast_dense_cols, lane loop and block loop                 test_dense_plasticity_post_loops
  k_plast_nonzero, grid-stride loop                            test_float_spikes_above_one_grid
  k_grad_rows, tile grid-stride loop                           test_rows_gradient_large, test_fixed_number_gradient_wide_rows
  k_grad_finish > 256 partials, rows_grid at its cap           test_homo_gradient_exact, test_homo_gradient_bound
  k_grad_rows, long rows / row_on refresh                      test_rows_gradient_large
  k_grad_dense, gridDim.y > 1 and the row loop                 test_dense_gradient_column_split
  k_grad_pack / k_grad_pack_ids grid-stride loops              test_activity_packers_above_one_grid
  masked_sum / any_word with many mask words                   test_many_mask_words, test_largest_batch
  k_grad_rows above 2**31 entries                              test_gradient_above_2_31_entries
"""
import os

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _autograd as AG
from brainevent_amd import _csr as C
from brainevent_amd import _plasticity as P
from brainevent_amd._error import KernelExecutionError
from test_autograd_cpu import model_dense_dw, model_rows_dw, model_rows_homo, random_csr
from test_plasticity_cpu import model_cols, model_rows, model_update, row_of
from test_plasticity_gpu import assert_bit_equal, encode, host

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]

# The loop bounds of the two kernel files as the cases below use them (tests/test_update_kernels_thresholds_cpu.py reads the
# sources and fails when one of them moves: the cases named in the module docstring then need new sizes).
THRESHOLDS = {
    'plast.kScanThreads': 1024, 'plast.kScanPer': 16, 'plast.kRowThreads': 256, 'plast.kRowPer': 8,
    'plast.rows_grid_cap': 4096, 'plast.nonzero_grid_cap': 4096, 'plast.cols_per_y': 4096,
    'plast.dense_pre_grid': 2048, 'plast.dense_post_grid_cap': 8192,
    'grad.kRowThreads': 256, 'grad.kRowPer': 8, 'grad.rows_grid_cap': 4096, 'grad.cols_per_y': 4096,
    'grad.dense_grid': 4096, 'grad.pack_grid_cap': 8192, 'grad.pack_ids_grid_cap': 4096, 'grad.finish_threads': 256,
    'kMaxBatch': 65535,
}
T = THRESHOLDS
SCAN_SPAN = T['plast.kScanThreads'] * T['plast.kScanPer']                 # active rows one scan pass covers
P_TILE = T['plast.kRowThreads'] * T['plast.kRowPer']
P_STRIDE = T['plast.rows_grid_cap'] * P_TILE                             # active entries one sweep of the grid covers
NONZERO_SPAN = 256 * T['plast.nonzero_grid_cap']
G_TILE = T['grad.kRowThreads'] * T['grad.kRowPer']
G_STRIDE = T['grad.rows_grid_cap'] * G_TILE
PACK_SPAN = 256 * T['grad.pack_grid_cap']
PACK_IDS_SPAN = 256 * T['grad.pack_ids_grid_cap']


def free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def dev(x, dtype=None):
    return torch.as_tensor(x, dtype=dtype).to(DEV)


def zero_bits(t: torch.Tensor) -> bool:
    """every element is +0.0 (a -0.0 or a denormal would not pass)."""
    return int(torch.count_nonzero(t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]))) == 0


# =========================================================================================================== structures
def ragged_csr(rng, m=60000, k=50000, max_len=400, huge=70000):
    """Rows of 0..max_len entries, every 7th row empty, the first and the last rows empty, one row of `huge` entries, one
    duplicated column; columns drawn with replacement."""
    lens = rng.integers(0, max_len + 1, m)
    lens[::7] = 0
    lens[:5] = 0
    lens[-4:] = 0
    big = m // 3 + 1
    lens[big] = huge
    lens[8] = max(lens[8], 3)
    assert big % 7 != 0 and lens[big] == huge
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    idx[ptr[8] + 1] = idx[ptr[8]]
    return idx, ptr.astype(np.int32), big


_RAGGED = {}


def the_ragged():
    """One instance for the whole module (host arrays only)."""
    if not _RAGGED:
        idx, ptr, big = ragged_csr(np.random.default_rng(20240))
        _RAGGED.update(idx=idx, ptr=ptr, big=big, m=len(ptr) - 1, k=50000, rows=row_of(ptr))
    return _RAGGED


def rand_w(rng, n, dtype):
    """weights in [0, 1) as values of `dtype`."""
    return torch.tensor(rng.random(n), dtype=torch.float64).to(dtype).to(DEV)


def spikes_with(rng, n, p, on=(), off=()):
    s = rng.random(n) < p
    s[list(on)] = True
    s[list(off)] = False
    return s


def certified_for(M, lo, hi) -> bool:
    cert = M.buffers.get(P.CLIP_KEY)
    return cert is not None and cert[0] == C.weights_stamp(M.data) and (cert[1], cert[2]) == (lo, hi)


def to_np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def step(M, stored_is_pre, idx, ptr, w_host, pre, spk, how, trace, lo, hi, tag, certified=None):
    """One in-place container update + the host model of it; returns the model's new weights."""
    if certified is not None:          # which path runs: the kernel's clip of the touched entries, or the whole-array clamp
        assert certified_for(M, lo, hi) == certified, f"{tag}: certificate {'missing' if certified else 'unexpected'}"
    upd = M.update_on_pre if pre else M.update_on_post
    args = (encode(spk, how), trace) if pre else (trace, encode(spk, how))
    assert upd(*args, lo, hi, inplace=True) is M
    f = model_rows if stored_is_pre == pre else model_cols
    w_new = f(w_host, idx, ptr, spk, trace, lo, hi)
    assert_bit_equal(M.data, w_new, tag)
    return w_new


def trace_for(rng, n):
    return (rng.random(n) - 0.5).astype(np.float32)


# =========================================================================================================== sparse plasticity
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_sparse_plasticity_large(dtype, oracle):
    """CSR 60 000 x 50 000, ~10 M entries, 95 % of the rows (columns) active: the tile grid-stride loop of k_plast_rows (more
    active entries than 4096 tiles), three scan passes, a row of 70 000 entries across ~35 workgroups, both directions (row
    walk, int32 permutation), without clip, with the whole-array clamp and with the kernel's own clip (certified state).
    f32 also checks one product per direction afterwards (plan / index caches follow the large update)."""
    S = the_ragged()
    idx, ptr, m, k, big = S['idx'], S['ptr'], S['m'], S['k'], S['big']
    rng = np.random.default_rng(100 + DTYPES.index(dtype))
    w = rand_w(rng, len(idx), dtype)
    M = be.CSR((w, dev(idx), dev(ptr)), shape=(m, k))
    pre_s = [spikes_with(rng, m, 0.95, on=(big, 0, 7, m - 1)) for _ in range(3)]
    post_s = [spikes_with(rng, k, 0.95) for _ in range(2)]
    lens = np.diff(ptr.astype(np.int64))
    for s in pre_s:
        assert int(lens[s].sum()) > P_STRIDE, "pre: the active entries must exceed one sweep of the grid"
        assert int(s.sum()) > 2 * SCAN_SPAN, "pre: three scan passes"
    for s in post_s:
        assert int(s[idx].sum()) > P_STRIDE and int(s.sum()) > 2 * SCAN_SPAN
    assert lens[big] > 4 * P_TILE and lens[0] == 0 and lens[m - 1] == 0
    if dtype == torch.float32:       # cached products before the update (the plan of the scatter direction)
        spk_r, spk_c = rng.random(m) < 0.05, rng.random(k) < 0.05
        before_s = to_np(be.BinaryArray(spk_r) @ M).copy()
        before_g = to_np(M @ be.BinaryArray(spk_c)).copy()
    wh = host(w)
    wh = step(M, True, idx, ptr, wh, True, pre_s[0], 'bool', trace_for(rng, k), None, None, f'{dtype} pre unclipped')
    wh = step(M, True, idx, ptr, wh, False, post_s[0], 'compact', trace_for(rng, m), None, None, f'{dtype} post unclipped')
    assert M.buffers[P.INDEX_KEY][2].dtype == torch.int32
    wh = step(M, True, idx, ptr, wh, True, pre_s[1], 'float', trace_for(rng, k), 0.1, 0.8, f'{dtype} pre clamp', certified=False)
    wh = step(M, True, idx, ptr, wh, True, pre_s[2], 'bitpacked', trace_for(rng, k), 0.1, 0.8, f'{dtype} pre kernel clip',
              certified=True)
    wh = step(M, True, idx, ptr, wh, False, post_s[1], 'bool', trace_for(rng, m), 0.1, 0.8, f'{dtype} post kernel clip',
              certified=True)
    if dtype == torch.float32:
        ref_s = oracle.binary_csrmv(wh.astype(np.float64), idx, ptr, spk_r, (m, k), True)
        ref_g = oracle.binary_csrmv(wh.astype(np.float64), idx, ptr, spk_c, (m, k), False)
        assert np.abs(ref_s - before_s).max() > 100 * 1e-5 * np.abs(ref_s).max()
        assert np.abs(ref_g - before_g).max() > 100 * 1e-5 * np.abs(ref_g).max()
        np.testing.assert_allclose(to_np(be.BinaryArray(spk_r) @ M), ref_s, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(to_np(M @ be.BinaryArray(spk_c)), ref_g, rtol=1e-5, atol=1e-5)
    del M, w
    free()


@pytest.mark.parametrize('kind', ['csc', 'fcn_pre', 'fcn_post'])
def test_other_containers_cross_the_tile_stride(kind):
    """CSC (the ragged structure read as columns), FixedNumPerPre with n_conn > 2048 and FixedNumPerPost, each with more
    active entries than one sweep of the grid, in both directions (fixed rows: RowPtr without indptr)."""
    rng = np.random.default_rng(200 + ['csc', 'fcn_pre', 'fcn_post'].index(kind))
    if kind == 'csc':
        S = the_ragged()
        idx, ptr, n_rows, upper = S['idx'], S['ptr'], S['m'], S['k']
        dtype = torch.float32
        M = be.CSC((rand_w(rng, len(idx), dtype), dev(idx), dev(ptr)), shape=(upper, n_rows))
    else:
        n_rows, nc, upper = (4200, 2100, 30000) if kind == 'fcn_pre' else (9000, 1000, 7000)
        dtype = torch.float16 if kind == 'fcn_pre' else torch.bfloat16
        idx2 = rng.integers(0, upper, (n_rows, nc)).astype(np.int32)
        idx2[0, 1] = idx2[0, 0]
        idx, ptr = idx2.reshape(-1), (np.arange(n_rows + 1, dtype=np.int64) * nc)
        if kind == 'fcn_pre':
            assert nc > P_TILE
            M = be.FixedNumPerPre((rand_w(rng, n_rows * nc, dtype).reshape(n_rows, nc), dev(idx2)), shape=(n_rows, upper))
        else:
            M = be.FixedNumPerPost((rand_w(rng, n_rows * nc, dtype).reshape(n_rows, nc), dev(idx2)), shape=(upper, n_rows))
    stored_is_pre = kind == 'fcn_pre'
    n_pre, n_post = M.shape
    lens = np.diff(np.asarray(ptr, dtype=np.int64))
    wh = host(M.data.reshape(-1))
    for i, (rows_dir, lo, hi, how, cert) in enumerate([(True, 0.1, 0.8, 'bool', False), (True, 0.1, 0.8, 'compact', True),
                                                       (False, None, None, 'float', None)]):
        pre = rows_dir == stored_is_pre
        n_spk, n_tr = (n_pre, n_post) if pre else (n_post, n_pre)
        spk = spikes_with(rng, n_spk, 0.97)
        active_entries = int(lens[spk].sum()) if rows_dir else int(spk[idx].sum())
        assert active_entries > P_STRIDE, (kind, i, active_entries)
        wh = step(M, stored_is_pre, idx, ptr, wh, pre, spk, how, trace_for(rng, n_tr), lo, hi, f'{kind} step {i}', certified=cert)
    del M
    free()


@pytest.mark.parametrize('n_active', [SCAN_SPAN, SCAN_SPAN + 1, 2 * SCAN_SPAN + 1])
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_scan_pass_boundaries(n_active, dtype):
    """Exactly 16 384 (one full pass), 16 385 (one row in the second pass) and 32 769 (one row in the third) active rows,
    empty active rows mixed in, rows of one or two entries; both directions, every encoding, with and without bounds."""
    assert SCAN_SPAN == 16384
    rng = np.random.default_rng([n_active, DTYPES.index(dtype)])
    n = 40000
    lens = rng.integers(0, 3, n)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, n, int(ptr[-1])).astype(np.int32)
    M = be.CSR((rand_w(rng, len(idx), dtype), dev(idx), dev(ptr)), shape=(n, n))
    wh = host(M.data)
    plan = [(True, 'bool', None, None, None), (False, 'compact', None, None, None), (True, 'float', 0.1, 0.8, False),
            (False, 'bitpacked', 0.1, 0.8, True), (True, 'uint8', 0.1, 0.8, True), (False, 'binary', 0.7, 0.2, False),
            (True, 'compact', 0.7, 0.2, True)]
    for i, (pre, how, lo, hi, cert) in enumerate(plan):
        spk = np.zeros(n, bool)
        spk[rng.choice(n, n_active, replace=False)] = True
        assert int(spk.sum()) == n_active
        if pre:
            assert (lens[spk] == 0).any() and (lens[spk] > 0).any()
        wh = step(M, True, idx, ptr, wh, pre, spk, how, trace_for(rng, n), lo, hi, f'n_active {n_active} {dtype} step {i}',
                  certified=cert)


def test_float_spikes_above_one_grid():
    """Float spikes over 1 100 000 rows of one entry: the grid-stride loop of k_plast_nonzero (negative values are spikes)."""
    n, k = 1_100_000, 1000
    assert n > NONZERO_SPAN
    rng = np.random.default_rng(300)
    ptr = np.arange(n + 1, dtype=np.int32)
    idx = rng.integers(0, k, n).astype(np.int32)
    M = be.CSR((rand_w(rng, n, torch.float32), dev(idx), dev(ptr)), shape=(n, k))
    wh = host(M.data)
    spk = spikes_with(rng, n, 0.5, on=(0, n - 1, NONZERO_SPAN, NONZERO_SPAN + 1), off=(1, NONZERO_SPAN - 1))
    assert int(spk.sum()) > SCAN_SPAN
    wh = step(M, True, idx, ptr, wh, True, spk, 'float', trace_for(rng, k), None, None, 'float spikes')
    spk2 = spikes_with(rng, n, 0.01, on=(n - 1,), off=(0,))
    step(M, True, idx, ptr, wh, True, spk2, 'float', trace_for(rng, k), 0.2, 0.7, 'float spikes, sparse')
    del M
    free()


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_one_huge_row_among_empty_rows(dtype):
    """All rows active; one row holds more than four tiles and every other row is empty (runs of equal offsets on both sides of
    the binary search), then the mirror image: thousands of active empty rows around one row of three entries."""
    rng = np.random.default_rng(400 + DTYPES.index(dtype))
    m, k = 5000, 3000
    for long_len in (4 * P_TILE + 1808, 3):
        lens = np.zeros(m, np.int64)
        lens[2500] = long_len
        if long_len > 3:
            assert long_len > 4 * P_TILE and long_len % T['plast.kRowThreads'] != 0
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
        M = be.CSR((rand_w(rng, len(idx), dtype), dev(idx), dev(ptr)), shape=(m, k))
        wh = host(M.data)
        every = np.ones(m, bool)
        assert int(every.sum()) - 1 > 4000                      # the empty active rows around the one with entries
        wh = step(M, True, idx, ptr, wh, True, every, 'bool', trace_for(rng, k), None, None, f'{long_len} all rows')
        wh = step(M, True, idx, ptr, wh, True, every, 'compact', trace_for(rng, k), 0.1, 0.8, f'{long_len} clamp', certified=False)
        wh = step(M, True, idx, ptr, wh, True, every, 'bitpacked', trace_for(rng, k), 0.1, 0.8, f'{long_len} clip', certified=True)
        some = spikes_with(rng, m, 0.5, off=(2500,))           # the only row with entries is inactive: nothing may change
        wh2 = step(M, True, idx, ptr, wh, True, some, 'bool', trace_for(rng, k), 0.1, 0.8, f'{long_len} none', certified=True)
        assert_bit_equal(wh2, wh)
        step(M, True, idx, ptr, wh2, False, np.ones(k, bool), 'bool', trace_for(rng, m), 0.1, 0.8, f'{long_len} post', certified=True)


# =========================================================================================================== dense plasticity
def dense_step(D, wh, pre, spk, how, trace, lo, hi, tag, certified=None):
    if certified is not None:
        assert certified_for(D, lo, hi) == certified, tag
    n_pre, n_post = D.shape
    if pre:
        assert D.update_on_pre(encode(spk, how), trace, lo, hi, inplace=True) is D
        pos = (np.nonzero(spk)[0][:, None] * n_post + np.arange(n_post)[None, :]).reshape(-1)
        tidx = pos % n_post
    else:
        assert D.update_on_post(trace, encode(spk, how), lo, hi, inplace=True) is D
        pos = (np.arange(n_pre)[:, None] * n_post + np.nonzero(spk)[0][None, :]).reshape(-1)
        tidx = pos // n_post
    flat = wh.reshape(-1)
    new = model_update(flat, pos, tidx, trace, lo, hi).reshape(n_pre, n_post)
    assert_bit_equal(D.data, new, tag)
    return new


@pytest.mark.parametrize('n_cols,n_rows', [(4096, 2600), (4097, 1300), (9000, 800)])
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_dense_plasticity_pre_column_split(n_cols, n_rows, dtype):
    """n_cols = 4096 (gridDim.y = 1, the last full split), 4097 (a second split of one column), 9000 (three), with more active
    rows than the grid has workgroups along x (the row loop)."""
    gy = -(-n_cols // T['plast.cols_per_y'])
    assert gy == {4096: 1, 4097: 2, 9000: 3}[n_cols]
    rng = np.random.default_rng([n_cols, DTYPES.index(dtype)])
    D = be.Dense(rand_w(rng, n_rows * n_cols, dtype).reshape(n_rows, n_cols))
    wh = host(D.data)
    plan = [('bool', None, None, None), ('float', 0.1, 0.8, False), ('compact', 0.1, 0.8, True)]
    if n_cols == 4097:
        plan += [('bitpacked', 0.7, 0.2, False), ('bool', 0.7, 0.2, True)]
    for i, (how, lo, hi, cert) in enumerate(plan):
        spk = spikes_with(rng, n_rows, 0.9, on=(0, n_rows - 1), off=(1,))
        assert int(spk.sum()) > T['plast.dense_pre_grid'] // gy
        wh = dense_step(D, wh, True, spk, how, trace_for(rng, n_cols), lo, hi, f'{n_cols} {dtype} step {i}', certified=cert)
    del D
    free()


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_dense_plasticity_post_loops(dtype):
    """More than 256 active columns (the lane loop) and more than 8192 rows (the block loop)."""
    n_pre, n_post = 8300, 700
    assert n_pre > T['plast.dense_post_grid_cap']
    rng = np.random.default_rng(500 + DTYPES.index(dtype))
    D = be.Dense(rand_w(rng, n_pre * n_post, dtype).reshape(n_pre, n_post))
    wh = host(D.data)
    for i, (how, lo, hi, cert) in enumerate([('bool', None, None, None), ('compact', 0.1, 0.8, False), ('float', 0.1, 0.8, True),
                                             ('bitpacked', 0.7, 0.2, False), ('uint8', 0.7, 0.2, True)]):
        spk = spikes_with(rng, n_post, 0.5, on=(0, n_post - 1))
        assert int(spk.sum()) > 256
        wh = dense_step(D, wh, False, spk, how, trace_for(rng, n_pre), lo, hi, f'post {dtype} step {i}', certified=cert)
    del D
    free()


# =========================================================================================================== gradients
def grad_vals(rng, shape, dtype, ternary=False):
    v = rng.integers(-1, 2, shape).astype(np.float64) if ternary else rng.standard_normal(shape)
    return torch.tensor(v, dtype=torch.float64).to(dtype).to(DEV)


def poison_next_alloc(n, dtype):
    """Leave NaN in the block the allocator hands out next for `n` elements of `dtype` (the gradient buffer is torch.empty)."""
    t = torch.full((n,), float('nan'), dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    del t


def csr_backward(w, idx_d, ptr_d, s_bm, nb, m, k, transpose, g):
    """functional product + backward; s_bm [nb or 1, n] bool (host); g: the output gradient (device) or None for ones."""
    w.grad = None
    if nb is None:
        y = be.binary_csrmv(w, idx_d, ptr_d, dev(s_bm[0]), shape=(m, k), transpose=transpose)
    else:
        y = be.binary_csrmm(w, idx_d, ptr_d, dev(s_bm.T.copy()), shape=(m, k), transpose=transpose)
    poison_next_alloc(w.numel(), w.dtype)
    y.backward(g)
    return w.grad


def g_bm_of(g, nb):
    a = g.detach().double().cpu().numpy()
    return a.reshape(1, -1) if nb is None else a.T


LARGE_GRAD = [(torch.float32, True), (torch.float32, False), (torch.float64, True), (torch.float64, False),
              (torch.float16, True), (torch.bfloat16, False)]


@pytest.mark.parametrize('dtype,transpose', LARGE_GRAD, ids=lambda v: str(v))
def test_rows_gradient_large(dtype, transpose):
    """The ragged structure (nse > 4096 tiles: the tile grid-stride loop; a row of 70 000 entries across workgroups; empty rows
    at both ends): per-entry gradient bit-exact, nb None with int32 indptr and nb 3 with int64 indptr.  Half of the rows are
    active, so lanes walk from active to inactive rows and back (the row_on refresh); the entries of inactive rows are +0 over
    NaN-poisoned memory, also after a second call with the activity inverted; two runs agree bit for bit."""
    S = the_ragged()
    idx, ptr, rows, m, k, big = S['idx'], S['ptr'], S['rows'], S['m'], S['k'], S['big']
    nse = len(idx)
    assert nse > G_STRIDE and nse < 2**31
    lens = np.diff(ptr.astype(np.int64))
    assert lens[big] > 4 * G_TILE
    rng = np.random.default_rng([7, DTYPES.index(dtype), int(transpose)])
    idx_d = dev(idx)
    n_spk, n_out = (m, k) if transpose else (k, m)
    for nb, ptr_dtype in ((None, torch.int32), (3, torch.int64)):
        ptr_d = dev(ptr).to(ptr_dtype)
        w = torch.zeros(nse, dtype=dtype, device=DEV, requires_grad=True)
        s = rng.random((1 if nb is None else nb, n_spk)) < 0.5
        if transpose:
            s[:, big] = True
            s[:, big + 1] = False
        g = grad_vals(rng, (n_out,) if nb is None else (n_out, nb), dtype)
        got = csr_backward(w, idx_d, ptr_d, s, nb, m, k, transpose, g).clone()
        want = model_rows_dw(idx, rows, transpose, s, g_bm_of(g, nb), dtype)
        assert torch.equal(got.cpu(), want), (nb, (got.cpu() != want).nonzero()[:5].reshape(-1).tolist())
        assert not torch.isnan(got).any()
        again = csr_backward(w, idx_d, ptr_d, s, nb, m, k, transpose, g)
        assert_bit_equal(again, got, 'two runs')
        if transpose:            # inactive rows: exact zeros, now and after the activity is inverted
            off = dev(~s.any(axis=0)[rows])
            assert off.any() and zero_bits(got[off])
            s2 = ~s
            got2 = csr_backward(w, idx_d, ptr_d, s2, nb, m, k, transpose, g)
            off2 = dev(~s2.any(axis=0)[rows])
            assert zero_bits(got2[off2])
            if nb is None:       # one batch row: the two activities partition the entries, g itself where active
                on2 = ~off2
                assert torch.equal(got2[on2], g[dev(idx.astype(np.int64))][on2])
                assert zero_bits(got[int(ptr[big + 1]):int(ptr[big + 2])]) and zero_bits(got2[int(ptr[big]):int(ptr[big + 1])])
        del w, got, again
    free()


def test_fixed_number_gradient_wide_rows():
    """FixedNumPerPre with n_conn = 2100 (> one tile: `e / rp.fixed` with several tiles per row) and nse above one sweep of the
    grid; both operand orders, bit-exact."""
    n_rows, nc, upper = 4200, 2100, 30000
    assert nc > G_TILE and n_rows * nc > G_STRIDE
    rng = np.random.default_rng(600)
    idx2 = rng.integers(0, upper, (n_rows, nc)).astype(np.int32)
    frows = np.repeat(np.arange(n_rows), nc)
    w = torch.zeros((n_rows, nc), dtype=torch.float32, device=DEV, requires_grad=True)
    M = be.FixedNumPerPre((w, dev(idx2)), shape=(n_rows, upper))
    for left in (True, False):
        M.data.grad = None
        n_spk = n_rows if left else upper
        s = rng.random((1, n_spk)) < 0.5
        ev = be.BinaryArray(dev(s[0]))
        y = ev @ M if left else M @ ev
        g = grad_vals(rng, tuple(y.shape), torch.float32)
        poison_next_alloc(n_rows * nc, torch.float32)
        y.backward(g)
        want = model_rows_dw(idx2, frows, left, s, g_bm_of(g, None), torch.float32).reshape(n_rows, nc)
        assert torch.equal(M.data.grad.cpu(), want), left
    del M, w
    free()


def test_activity_packers_above_one_grid():
    """2 200 000 stored rows of at most one entry: k_grad_pack's grid-stride loop (n * nw above 256 * 8192) with byte spikes and
    k_grad_pack_ids' with a CompactBinary of more than 1 048 576 active ids."""
    m, k = 2_200_000, 1000
    assert m > PACK_SPAN
    rng = np.random.default_rng(700)
    lens = (rng.random(m) < 0.9).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    rows = row_of(ptr)
    w = torch.zeros(len(idx), dtype=torch.float32, device=DEV, requires_grad=True)
    M = be.CSR((w, dev(idx), dev(ptr.astype(np.int32))), shape=(m, k))
    s = spikes_with(rng, m, 0.6, on=(0, m - 1, PACK_SPAN, PACK_IDS_SPAN), off=(1, PACK_SPAN - 1, PACK_IDS_SPAN - 1))
    assert int(s.sum()) > PACK_IDS_SPAN
    comp = be.CompactBinary.from_array(dev(s))
    assert comp._ids_operand() is not None
    for name, ev in (('bool', be.BinaryArray(dev(s))), ('compact', comp), ('float', be.BinaryArray(dev(s).float()))):
        M.data.grad = None
        y = ev @ M
        g = grad_vals(rng, tuple(y.shape), torch.float32)
        poison_next_alloc(len(idx), torch.float32)
        y.backward(g)
        want = model_rows_dw(idx, rows, True, s[None, :], g_bm_of(g, None), torch.float32)
        assert torch.equal(M.data.grad.cpu(), want), name
    del M, w
    free()


@pytest.mark.parametrize('transpose', [True, False])
def test_many_mask_words(transpose):
    """nb = 1025: 33 mask words per neuron (masked_sum / any_word loop over words; bit 0 of the last word alone)."""
    nb = 1025
    assert -(-nb // 32) >= 33
    rng = np.random.default_rng(800 + transpose)
    m, k = 67, 93
    indices, indptr, rows = random_csr(rng, m, k, 0.2)
    n_spk, n_out = (m, k) if transpose else (k, m)
    s = rng.random((nb, n_spk)) < 0.02
    s[:, 3] = False
    s[-1, 3] = True                                 # active only through the single bit of the 33rd word
    s[:, 4] = False
    for dtype in DTYPES:
        w = torch.zeros(indices.size, dtype=dtype, device=DEV, requires_grad=True)
        g = grad_vals(rng, (n_out, nb), dtype)
        got = csr_backward(w, dev(indices), dev(indptr), s, nb, m, k, transpose, g)
        assert torch.equal(got.cpu(), model_rows_dw(indices, rows, transpose, s, g_bm_of(g, nb), dtype)), dtype
        # shared weight: derived bound
        wh = torch.ones(1, dtype=dtype, device=DEV, requires_grad=True)
        goth = csr_backward(wh, dev(indices), dev(indptr), s, nb, m, k, transpose, g)
        check_homo_bound(goth, indices, rows, transpose, s, g_bm_of(g, nb), dtype)
        # dense
        W = torch.zeros((m, k), dtype=dtype, device=DEV, requires_grad=True)
        y = be.binary_densemm(W, dev(s.T.copy()), transpose=transpose)
        y.backward(g)
        assert torch.equal(W.grad.cpu(), model_dense_dw(transpose, s, g_bm_of(g, nb), dtype)), dtype


@pytest.mark.parametrize('transpose', [True, False])
def test_largest_batch(transpose):
    """nb = kMaxBatch = 65535 (2048 mask words) on a 5 x 4 structure, bit-exact; one more column is refused with the library's
    error before any kernel runs."""
    nb = T['kMaxBatch']
    m, k = 5, 4
    indices = np.array([0, 3, 1, 1, 2, 0, 3], np.int32)
    indptr = np.array([0, 2, 2, 4, 5, 7], np.int64)
    rows = row_of(indptr)
    rng = np.random.default_rng(900 + transpose)
    n_spk, n_out = (m, k) if transpose else (k, m)
    s = rng.random((nb, n_spk)) < 0.01
    s[-1, 0] = True
    w = torch.zeros(indices.size, dtype=torch.float32, device=DEV, requires_grad=True)
    g = grad_vals(rng, (n_out, nb), torch.float32)
    got = csr_backward(w, dev(indices), dev(indptr), s, nb, m, k, transpose, g)
    assert torch.equal(got.cpu(), model_rows_dw(indices, rows, transpose, s, g_bm_of(g, nb), torch.float32))
    too_many = torch.zeros((n_spk, nb + 1), dtype=torch.bool, device=DEV)
    w.grad = None
    with pytest.raises(KernelExecutionError, match='n_batch|out of range'):
        be.binary_csrmm(w, dev(indices), dev(indptr), too_many, shape=(m, k), transpose=transpose)
    with pytest.raises(KernelExecutionError, match='n_batch|out of range'):
        AG.activity(too_many, 'nm')
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- shared weight
def homo_depth(nse, nb, dtype):
    """The longest chain of additions behind the shared-weight gradient: a lane adds nb values for each of its kRowPer entries of
    each of its ceil(tiles / grid) tiles, the wave reduction adds 6 levels, the workgroup 4 waves; the finish kernel: a lane adds
    ceil(grid / 256) partials, then 6 levels and 4 waves."""
    tiles = -(-nse // G_TILE)
    grid = max(1, min(tiles, T['grad.rows_grid_cap']))
    return nb * T['grad.kRowPer'] * -(-tiles // grid) + 6 + 4 + -(-grid // T['grad.finish_threads']) + 6 + 4


MANT = {torch.float32: 23, torch.float64: 52, torch.float16: 10, torch.bfloat16: 7}


def homo_bound(nse, nb, dtype, sum_abs, want):
    """|got - model| <= depth * u * sum|a * g| + half an ulp of the weight dtype, u = 2**-24 (f32 accumulation: f32, f16 and
    bf16 weights) or 2**-53 (f64): each addition of a chain of `depth` additions adds at most u times the magnitude of its
    partial sum, which sum|a * g| bounds.  The final rounding to the weight dtype costs half an ulp, taken at the largest
    magnitude the accumulated value can have."""
    u = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    acc = homo_depth(nse, nb, dtype) * u * sum_abs
    top = abs(want) + acc
    half_ulp = 0.0 if top == 0 else 2.0 ** (np.floor(np.log2(top)) - MANT[dtype]) / 2
    if dtype == torch.float16:
        half_ulp = max(half_ulp, 2.0 ** -25)       # f16 subnormal spacing 2**-24
    return acc + half_ulp


def check_homo_bound(got, indices, rows, transpose, s, g_bm, dtype):
    indices = np.asarray(indices).reshape(-1)
    want = model_rows_homo(indices, rows, transpose, s, g_bm)
    sidx, gidx = (rows, indices.astype(np.int64)) if transpose else (indices.astype(np.int64), rows)
    sum_abs = 0.0
    for b in range(s.shape[0]):                    # sum|a * g| in f64 from the model's operands, one batch row at a time
        sum_abs += float(np.abs(np.asarray(g_bm[b], np.float64)[gidx[s[b, sidx]]]).sum())
    bound = homo_bound(indices.size, s.shape[0], dtype, sum_abs, want)
    err = abs(float(got.double().reshape(-1)[0]) - want)
    print(f"homo {dtype} transpose={transpose} nse={indices.size} nb={s.shape[0]}: got-model {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound, want)


def small_homo_structure(rng):
    """nse just above 256 tiles: 257 per-workgroup partials."""
    m, k = 3000, 2500
    lens = rng.integers(100, 260, m)
    lens[::11] = 0
    target = T['grad.finish_threads'] * G_TILE + 37
    lens[-1] += target - int(lens.sum())
    assert lens[-1] >= 0
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    return idx, ptr, m, k


def homo_cases(size):
    if size == 'small':
        idx, ptr, m, k = small_homo_structure(np.random.default_rng(1000))
        nse = len(idx)
        assert T['grad.finish_threads'] * G_TILE < nse < T['grad.finish_threads'] * G_TILE + G_TILE
        assert -(-nse // G_TILE) == T['grad.finish_threads'] + 1
        return idx, ptr, row_of(ptr), m, k
    S = the_ragged()
    assert len(S['idx']) >= T['grad.rows_grid_cap'] * G_TILE        # the grid at its cap, two tiles per workgroup and more
    return S['idx'], S['ptr'], S['rows'], S['m'], S['k']


@pytest.mark.parametrize('size,dtype', [('small', d) for d in DTYPES] + [('large', torch.float32), ('large', torch.float64),
                                                                         ('large', torch.bfloat16)], ids=lambda v: str(v))
@pytest.mark.parametrize('transpose', [True, False])
def test_homo_gradient_exact(size, dtype, transpose):
    """Gradient values in {-1, 0, 1}, one batch row: every partial sum is an integer below 2**24, so every f32 (f64) addition
    is exact in any order and the result is the f64 model rounded once to the weight dtype, bit for bit.  Two runs agree."""
    idx, ptr, rows, m, k = homo_cases(size)
    nse = len(idx)
    assert nse < 2**24
    rng = np.random.default_rng([11, int(transpose), DTYPES.index(dtype)])
    n_spk, n_out = (m, k) if transpose else (k, m)
    s = rng.random((1, n_spk)) < 0.6
    g = grad_vals(rng, (n_out,), dtype, ternary=True)
    w = torch.ones(1, dtype=dtype, device=DEV, requires_grad=True)
    got = csr_backward(w, dev(idx), dev(ptr), s, None, m, k, transpose, g).clone()
    want = model_rows_homo(idx, rows, transpose, s, g_bm_of(g, None))
    assert want == int(want) and abs(want) < 2**24
    assert_bit_equal(got, torch.tensor([want], dtype=torch.float64).to(dtype), f'{size} {dtype} {transpose}: {float(got)} vs {want}')
    again = csr_backward(w, dev(idx), dev(ptr), s, None, m, k, transpose, g)
    assert_bit_equal(again, got, 'two runs')


@pytest.mark.parametrize('size,dtype,nb', [('small', torch.float32, None), ('small', torch.float64, 3), ('small', torch.float16, 3),
                                           ('small', torch.bfloat16, None), ('large', torch.float32, 3),
                                           ('large', torch.float64, None), ('large', torch.float16, None)], ids=lambda v: str(v))
@pytest.mark.parametrize('transpose', [True, False])
def test_homo_gradient_bound(size, dtype, nb, transpose):
    """Random normal gradients: within the derived bound of `homo_bound` of the f64 model, and equal between two runs."""
    idx, ptr, rows, m, k = homo_cases(size)
    rng = np.random.default_rng([13, int(transpose), DTYPES.index(dtype)])
    n_spk, n_out = (m, k) if transpose else (k, m)
    s = rng.random((1 if nb is None else nb, n_spk)) < 0.6
    g = grad_vals(rng, (n_out,) if nb is None else (n_out, nb), dtype)
    w = torch.ones(1, dtype=dtype, device=DEV, requires_grad=True)
    got = csr_backward(w, dev(idx), dev(ptr), s, nb, m, k, transpose, g).clone()
    check_homo_bound(got, idx, rows, transpose, s, g_bm_of(g, nb), dtype)
    again = csr_backward(w, dev(idx), dev(ptr), s, nb, m, k, transpose, g)
    assert_bit_equal(again, got, 'two runs')


# ----------------------------------------------------------------------------------------------------------- dense
@pytest.mark.parametrize('n_cols,n_rows', [(4097, 2100), (9000, 1400)])
@pytest.mark.parametrize('transpose', [True, False])
def test_dense_gradient_column_split(n_cols, n_rows, transpose):
    """n_cols = 4097 / 9000 (gridDim.y = 2 / 3) with more rows than the grid has workgroups along x; nb None (four dtypes) and
    33 (f32); inactive rows of `s @ W` are +0 over NaN-poisoned memory."""
    gy = -(-n_cols // T['grad.cols_per_y'])
    assert gy > 1 and n_rows > T['grad.dense_grid'] // gy
    rng = np.random.default_rng([17, n_cols, int(transpose)])
    n_spk, n_out = (n_rows, n_cols) if transpose else (n_cols, n_rows)
    for dtype, nb in [(torch.float32, None), (torch.float32, 33), (torch.float64, None), (torch.float16, None),
                      (torch.bfloat16, None)]:
        W = torch.zeros((n_rows, n_cols), dtype=dtype, device=DEV, requires_grad=True)
        s = rng.random((1 if nb is None else nb, n_spk)) < (0.5 if nb is None else 0.03)
        s[:, 0] = False
        s[0, n_spk - 1] = True
        if nb is None:
            y = be.binary_densemv(W, dev(s[0]), transpose=transpose)
        else:
            y = be.binary_densemm(W, dev(s.T.copy()), transpose=transpose)
        g = grad_vals(rng, tuple(y.shape), dtype)
        poison_next_alloc(n_rows * n_cols, dtype)
        y.backward(g)
        want = model_dense_dw(transpose, s, g_bm_of(g, nb), dtype)
        assert torch.equal(W.grad.cpu(), want), (dtype, nb)
        off = dev(~s.any(axis=0))
        assert off.any()
        assert zero_bits(W.grad[off] if transpose else W.grad[:, off])
        del W, y
    free()


# ----------------------------------------------------------------------------------------------------------- above 2**31
def test_gradient_above_2_31_entries():
    """The autograd twin of test_plasticity_gpu.py::test_above_2_31_entries: 2**31 + 2**17 entries in regular rows, int64
    indptr, then the same entries as a fixed-number structure (no indptr: `e / rp.fixed` on a 64-bit entry index).  Both
    directions, one batch row, f32, against a torch expression on the device in row chunks (with one batch row the sum has one
    term: g where active, +0 elsewhere).  Runs the autograd layer's own device calls (`activity`, `rows_weight_grad`: what
    RowsProduct.backward runs) on the structure; no product of that size is formed."""
    m, L, k = 1 << 17, (1 << 14) + 1, 50000
    nse = m * L
    assert nse > 2**31 and L > G_TILE
    gen = torch.Generator(device=DEV).manual_seed(1)
    idx = torch.randint(0, k, (nse,), dtype=torch.int32, device=DEV, generator=gen)
    ptr = torch.arange(m + 1, dtype=torch.int64, device=DEV) * L
    act_r = torch.rand(m, device=DEV, generator=gen) < 0.5
    act_c = torch.rand(k, device=DEV, generator=gen) < 0.5
    act_r[m - 1] = True
    g_c = torch.randn(k, device=DEV, generator=gen)
    g_r = torch.randn(m, device=DEV, generator=gen)
    I = idx.view(m, L)
    for fixed in (False, True):
        for transpose in (True, False):
            mask, nb = AG.activity(act_r if transpose else act_c, 'vec')
            assert nb == 1
            g = (g_c if transpose else g_r).reshape(-1, 1)
            poison_next_alloc(nse, torch.float32)
            if fixed:
                dw = AG.rows_weight_grad(((m, L), torch.float32), idx.view(m, L), None, L, m, transpose, mask, nb, g)
            else:
                dw = AG.rows_weight_grad(((nse,), torch.float32), idx, ptr, -1, m, transpose, mask, nb, g)
            D = dw.view(m, L)
            for r0 in range(0, m, 8192):
                r1 = min(m, r0 + 8192)
                if transpose:
                    ref = g_c[I[r0:r1].long()] * act_r[r0:r1, None].float()
                else:
                    ref = g_r[r0:r1, None] * act_c[I[r0:r1].long()].float()
                assert torch.equal(D[r0:r1], ref), (fixed, transpose, r0)
                if transpose:
                    assert zero_bits(D[r0:r1][~act_r[r0:r1]]), (fixed, r0)
                del ref
            del dw, D, mask
            free()
    del idx, ptr, I
    free()


# =========================================================================================================== randomized
@pytest.mark.parametrize('seed', range(int(os.environ.get('BE_STRESS_SEEDS', 8))))
def test_randomized_structures_cross_a_bound(seed):
    """Random shape, row-length law, activity and dtype; each law is biased so that at least one loop bound is crossed (asserted):
    0 many short active rows (scan passes), 1 a few rows longer than a tile among short ones, 2 more entries than one sweep of
    the grid, 3 regular rows wider than a tile.  Plasticity in both directions (kernel clip included) and the per-entry
    gradient in both directions, bit-exact."""
    rng = np.random.default_rng(5000 + seed)
    law = seed % 4
    dtype = DTYPES[int(rng.integers(0, 4))]
    if law == 0:
        m, k = int(rng.integers(40000, 90000)), int(rng.integers(1000, 60000))
        lens = rng.integers(0, 4, m)
        n_on = int(rng.integers(SCAN_SPAN + 1, m))
    elif law == 1:
        m, k = int(rng.integers(500, 3000)), int(rng.integers(100, 40000))
        lens = rng.integers(0, 6, m)
        longs = rng.choice(m, 3, replace=False)
        n_on = int(rng.integers(3, m))
    elif law == 2:
        m, k = int(rng.integers(20000, 50000)), int(rng.integers(5000, 60000))
        top = int(2.6 * P_STRIDE / m) + 1
        lens = rng.integers(0, top + 1, m)
        n_on = m - int(rng.integers(0, m // 50))
    else:
        m, k = int(rng.integers(600, 2500)), int(rng.integers(3000, 40000))
        lens = np.full(m, int(rng.integers(P_TILE + 1, 4000)))
        n_on = int(rng.integers(m // 2, m))
    lens[rng.random(m) < 0.1] = 0 if law != 3 else lens[0]
    if law == 1:
        lens[longs] = rng.integers(P_TILE + 1, 30000, 3)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    rows = row_of(ptr)
    pre_s = np.zeros(m, bool)
    pre_s[rng.choice(m, n_on, replace=False)] = True
    if law == 1:
        pre_s[longs] = True
    post_s = rng.random(k) < rng.uniform(0.3, 1.0)
    active_entries = int(lens[pre_s].sum())
    crossed = {'scan': int(pre_s.sum()) > SCAN_SPAN, 'long row': bool((lens[pre_s] > P_TILE).any()),
               'tile stride': active_entries > P_STRIDE, 'grad stride': len(idx) > G_STRIDE}
    assert crossed[['scan', 'long row', 'tile stride', 'long row'][law]], (seed, crossed)
    if law == 2:
        assert crossed['grad stride']
    ptr_d = dev(ptr if rng.random() < 0.5 else ptr.astype(np.int32))
    M = be.CSR((rand_w(rng, len(idx), dtype), dev(idx), ptr_d), shape=(m, k))
    wh = host(M.data)
    lo, hi = (0.1, 0.8) if rng.random() < 0.7 else (0.7, 0.2)
    hows = ['bool', 'uint8', 'float', 'binary', 'bitpacked', 'compact']
    pick = lambda: hows[int(rng.integers(0, len(hows)))]
    tag = f'seed {seed} law {law} {dtype} m={m} k={k} nse={len(idx)}'
    wh = step(M, True, idx, ptr, wh, True, pre_s, pick(), trace_for(rng, k), None, None, tag + ' pre')
    wh = step(M, True, idx, ptr, wh, False, post_s, pick(), trace_for(rng, m), lo, hi, tag + ' post clamp', certified=False)
    wh = step(M, True, idx, ptr, wh, True, pre_s, pick(), trace_for(rng, k), lo, hi, tag + ' pre clip', certified=True)
    wh = step(M, True, idx, ptr, wh, False, post_s, pick(), trace_for(rng, m), lo, hi, tag + ' post clip', certified=True)
    for transpose in (True, False):
        nb = None if rng.random() < 0.5 else 2
        n_spk, n_out = (m, k) if transpose else (k, m)
        s = np.stack([pre_s if transpose else post_s] * (1 if nb is None else nb))
        if nb is not None:
            s[1] = rng.random(n_spk) < 0.2
        w = torch.zeros(len(idx), dtype=dtype, device=DEV, requires_grad=True)
        g = grad_vals(rng, (n_out,) if nb is None else (n_out, nb), dtype)
        got = csr_backward(w, M.indices, M.indptr, s, nb, m, k, transpose, g)
        want = model_rows_dw(idx, rows, transpose, s, g_bm_of(g, nb), dtype)
        assert torch.equal(got.cpu(), want), tag + f' grad transpose={transpose} nb={nb}'
    del M
    free()
