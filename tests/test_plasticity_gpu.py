"""Spike-triggered plasticity on the MI355X: every container x both directions x the four weight dtypes x the spike encodings
x the bounds, bit-exact against the host model of tests/test_plasticity_cpu.py; the whole-array clip, the clip certificate,
cached workspaces after an in-place update, graph capture, and a structure above 2**31 entries.
The sizes past one pass of every loop of the kernels are in tests/test_update_kernels_at_scale_gpu.py."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _csr as C
from brainevent_amd import _plasticity as P
from test_plasticity_cpu import model_cols, model_rows, model_update, row_of

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
BOUNDS = [(None, None), (0.1, None), (None, 0.8), (0.1, 0.8), (0.7, 0.2)]
ENCODINGS = ['bool', 'uint8', 'float', 'binary', 'bitpacked', 'compact']


def host(w: torch.Tensor):
    """device weights -> host model operand (numpy, bf16: CPU torch)."""
    w = w.detach().cpu()
    return w if w.dtype == torch.bfloat16 else w.numpy()


def bits(x):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_bit_equal(got, exp, msg=''):
    g, e = bits(got).reshape(-1), bits(exp).reshape(-1)
    assert g.shape == e.shape, msg
    bad = (g != e).nonzero()
    assert bad.numel() == 0, f"{msg}: {bad.numel()} entries differ, first at {bad[:5].reshape(-1).tolist()}"


def encode(spk: np.ndarray, how: str):
    b = spk != 0
    if how == 'bool':
        return b
    if how == 'uint8':
        return torch.tensor(b.astype(np.uint8), device=DEV)
    if how == 'float':            # any nonzero value is a spike, negative ones included
        return np.where(b, np.where(np.arange(len(b)) % 2 == 0, 1.0, -2.5), 0.0).astype(np.float32)
    t = torch.tensor(b, device=DEV)
    if how == 'binary':
        return be.BinaryArray(t)
    if how == 'bitpacked':
        return be.BitPackedBinary(t)
    if how == 'compact':
        c = be.CompactBinary.from_array(t)
        assert c._ids_operand() is not None           # the device id list is consumed as it is
        return c
    raise ValueError(how)


def random_csr(rng, m, k, max_len=9):
    """rows of 0..max_len entries (empty rows included), columns drawn with replacement (duplicates included)."""
    lens = rng.integers(0, max_len + 1, m)
    lens[::7] = 0
    lens[1] = max(lens[1], 3)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    idx[ptr[1] + 1] = idx[ptr[1]]                         # a column listed twice in row 1
    return idx, ptr


# the containers as (stored rows, stored indices, n_pre, n_post) + which model each direction uses
def make_container(kind, rng, dtype, n_pre=45, n_post=37):
    if kind == 'dense':
        w = torch.tensor(rng.random((n_pre, n_post)), dtype=dtype, device=DEV)
        return be.Dense(w), None, None
    if kind in ('fcn_pre', 'fcn_post'):
        n_rows, upper = (n_pre, n_post) if kind == 'fcn_pre' else (n_post, n_pre)
        idx = rng.integers(0, upper, (n_rows, 5)).astype(np.int32)
        idx[0, 1] = idx[0, 0]
        w = torch.tensor(rng.random((n_rows, 5)), dtype=dtype, device=DEV)
        cls = be.FixedNumPerPre if kind == 'fcn_pre' else be.FixedNumPerPost
        M = cls((w, torch.tensor(idx, device=DEV)), shape=(n_pre, n_post))
        return M, idx.reshape(-1), (np.arange(n_rows + 1) * 5).astype(np.int32)
    n_rows, upper = (n_pre, n_post) if kind == 'csr' else (n_post, n_pre)
    idx, ptr = random_csr(rng, n_rows, upper)
    w = torch.tensor(rng.random(len(idx)), dtype=dtype, device=DEV)
    cls = be.CSR if kind == 'csr' else be.CSC
    return cls((w, torch.tensor(idx, device=DEV), torch.tensor(ptr, device=DEV)), shape=(n_pre, n_post)), idx, ptr


def expected(kind, pre, w0, idx, ptr, spk, trace, lo, hi):
    """host model of one update on a container of `kind` (stored-row view for the sparse ones)."""
    if kind == 'dense':
        w = host(w0)
        n_pre, n_post = w0.shape
        if pre:
            pos = np.nonzero(np.repeat(spk != 0, n_post))[0]
            tidx = pos % n_post
        else:
            pos = np.nonzero(np.tile(spk != 0, n_pre))[0]
            tidx = pos // n_post
        flat = w.reshape(-1)
        return model_update(flat, pos, tidx, trace, lo, hi).reshape(tuple(w0.shape))
    stored_is_pre = kind in ('csr', 'fcn_pre')
    f = model_rows if stored_is_pre == pre else model_cols
    return f(host(w0).reshape(-1), idx, ptr, spk, trace, lo, hi).reshape(tuple(w0.shape))


def functional(kind, pre, M, spk, trace, lo, hi):
    n_pre, n_post = M.shape
    if kind == 'dense':
        return (be.update_dense_on_binary_pre(M.data, spk, trace, lo, hi) if pre
                else be.update_dense_on_binary_post(M.data, trace, spk, lo, hi))
    if kind == 'csr':
        if pre:
            return be.update_csr_on_binary_pre(M.data, M.indices, M.indptr, spk, trace, lo, hi, shape=M.shape)
        t_ptr, t_rows, perm = be.csr_to_csc_index(M.indptr, M.indices, shape=M.shape)
        return be.update_csr_on_binary_post(M.data, t_rows, t_ptr, perm, trace, spk, lo, hi, shape=M.shape)
    if kind == 'csc':
        return (be.update_csc_on_binary_pre(M.data, M.indices, M.indptr, spk, trace, lo, hi, shape=M.shape) if pre
                else be.update_csc_on_binary_post(M.data, M.indices, M.indptr, trace, spk, lo, hi, shape=M.shape))
    if kind == 'fcn_pre' and pre:
        return be.update_fixed_post_conn_on_binary_pre(M.data, M.indices, spk, trace, lo, hi, shape=M.shape)
    if kind == 'fcn_post' and not pre:
        return be.update_fixed_pre_conn_on_binary_post(M.data, M.indices, trace, spk, lo, hi, shape=M.shape)
    return None          # (the reference has no functional form of the unfavourable fixed-number directions)


KINDS = ['csr', 'csc', 'dense', 'fcn_pre', 'fcn_post']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_sweep_bit_exact(kind, dtype):
    rng = np.random.default_rng(10 * KINDS.index(kind) + DTYPES.index(dtype))
    for pre in (True, False):
        for pattern in ('random', 'none', 'all'):
            for how in ENCODINGS:
                for lo, hi in BOUNDS:
                    M, idx, ptr = make_container(kind, rng, dtype)
                    n_spk, n_tr = (M.shape[0], M.shape[1]) if pre else (M.shape[1], M.shape[0])
                    spk = {'random': rng.random(n_spk) < 0.4, 'none': np.zeros(n_spk, bool),
                           'all': np.ones(n_spk, bool)}[pattern]
                    trace = (rng.random(n_tr) - 0.5).astype(np.float32)
                    w0 = M.data.clone()
                    exp = expected(kind, pre, w0, idx, ptr, spk, trace, lo, hi)
                    tag = f"{kind} {'pre' if pre else 'post'} {dtype} {pattern} {how} [{lo}, {hi}]"
                    got = functional(kind, pre, M, encode(spk, how), trace, lo, hi)
                    if got is not None:
                        assert_bit_equal(got, exp, 'functional ' + tag)
                        assert_bit_equal(M.data, w0, 'functional leaves its input ' + tag)
                    upd = M.update_on_pre if pre else M.update_on_post
                    args = (encode(spk, how), trace) if pre else (trace, encode(spk, how))
                    new = upd(*args, lo, hi)
                    assert new is not M and type(new) is type(M)
                    assert_bit_equal(new.data, exp, 'method ' + tag)
                    assert_bit_equal(M.data, w0, 'inplace=False leaves the container ' + tag)
                    if kind not in ('dense',):
                        assert new.indices is M.indices
                    args = (encode(spk, how), trace) if pre else (trace, encode(spk, how))
                    assert upd(*args, lo, hi, inplace=True) is M
                    assert_bit_equal(M.data, exp, 'inplace ' + tag)


@pytest.mark.parametrize('i64', [False, True])
def test_reference_kats_on_device(i64):
    dt = np.int64 if i64 else np.int32
    got = be.update_csr_on_binary_pre(np.array([1., 2., 3., 4.], np.float32), np.array([0, 2, 1, 2], np.int32),
                                      np.array([0, 2, 4], dt), np.array([True, False]), np.array([0.5, 1.5, 2.5], np.float32),
                                      shape=(2, 3))
    np.testing.assert_array_equal(got, np.array([1.5, 4.5, 3.0, 4.0], np.float32))
    got = be.update_csr_on_binary_post(np.array([1., 2., 3., 4.], np.float32), np.array([0, 1, 0, 1], np.int32),
                                       np.array([0, 2, 4], dt), np.array([0, 2, 1, 3], dt), np.array([0.5, 1.5], np.float32),
                                       np.array([False, True]), shape=(2, 2))
    np.testing.assert_array_equal(got, np.array([1.0, 2.5, 3.0, 5.5], np.float32))
    M = be.CSR((np.array([1., 2., 3., 4.], np.float32), np.array([0, 2, 1, 2], np.int32), np.array([0, 2, 4], dt)), shape=(2, 3))
    np.testing.assert_array_equal(M.update_on_pre(np.array([True, False]), np.array([0.5, 1.5, 2.5], np.float32)).data.cpu().numpy(),
                                  np.array([1.5, 4.5, 3.0, 4.0], np.float32))


def test_whole_array_clip_and_nan():
    rng = np.random.default_rng(5)
    idx, ptr = random_csr(rng, 40, 30)
    w = rng.random(len(idx)).astype(np.float32)
    spk = np.zeros(40, bool)
    spk[3] = True
    untouched = int(ptr[10])                           # row 10 is not active
    assert ptr[11] > ptr[10]
    w[untouched] = 7.0                                 # out of range, never touched
    w[untouched + 1 if ptr[11] - ptr[10] > 1 else int(ptr[12])] = np.nan
    trace = (rng.random(30) - 0.5).astype(np.float32)
    got = be.update_csr_on_binary_pre(w, idx, ptr, spk, trace, 0.0, 1.0, shape=(40, 30))
    exp = model_rows(w, idx, ptr, spk, trace, 0.0, 1.0)
    assert got[untouched] == 1.0
    assert np.isnan(got).sum() == 1
    assert_bit_equal(got, exp)
    M = be.CSR((w, idx, ptr), shape=(40, 30))
    M.update_on_pre(spk, trace, 0.0, 1.0, inplace=True)
    assert_bit_equal(M.data, exp)


@pytest.mark.parametrize('pre', [True, False])
def test_certificate_is_voided_by_a_foreign_write(pre):
    rng = np.random.default_rng(7)
    idx, ptr = random_csr(rng, 60, 50)
    M = be.CSR((rng.random(len(idx)).astype(np.float32), idx, ptr), shape=(60, 50))
    n_spk, n_tr = (60, 50) if pre else (50, 60)
    upd = (lambda s, t, **k: M.update_on_pre(s, t, 0.2, 0.9, **k)) if pre else (lambda s, t, **k: M.update_on_post(t, s, 0.2, 0.9, **k))
    model = (lambda w, s, t: model_rows(w, idx, ptr, s, t, 0.2, 0.9)) if pre else (lambda w, s, t: model_cols(w, idx, ptr, s, t, 0.2, 0.9))
    w = M.data.cpu().numpy()
    for _ in range(3):
        s, t = rng.random(n_spk) < 0.3, (rng.random(n_tr) - 0.5).astype(np.float32)
        upd(s, t, inplace=True)
        w = model(w, s, t)
        assert_bit_equal(M.data, w)
    assert M.buffers[P.CLIP_KEY][0] == C.weights_stamp(M.data)            # certified
    s = np.zeros(n_spk, bool)
    s[0] = True
    touched = np.nonzero((s[row_of(ptr)]) if pre else s[idx])[0]
    victim = int(np.setdiff1d(np.arange(len(idx)), touched)[0])
    M.data[victim] = 5.0                                                    # a write the certificate did not see
    w[victim] = 5.0
    t = (rng.random(n_tr) - 0.5).astype(np.float32)
    upd(s, t, inplace=True)
    w = model(w, s, t)
    assert float(M.data[victim]) == np.float32(0.9)
    assert_bit_equal(M.data, w)


@pytest.mark.parametrize('route', ['plan', 'binned', 'mirror'])
def test_cached_workspaces_follow_an_inplace_update(route):
    from oracle import oracle_np
    rng = np.random.default_rng(11)
    m, k, nc = 2000, 1500, 40
    ptr = (np.arange(m + 1) * nc).astype(np.int32)
    idx = rng.integers(0, k, m * nc).astype(np.int32)
    w = rng.random(m * nc).astype(np.float32)
    assert m * nc >= C.PLAN_MIN_NNZ
    M = be.CSR((w, idx, ptr), shape=(m, k))
    if route == 'mirror':
        M.prepare(mirror=True)
    else:
        M.buffers['scatter_plan'] = C.make_scatter_workspace(route, M.data, M.indices, M.indptr, m, k, M.nse)
        assert isinstance(M.buffers['scatter_plan'], C.ScatterPlan if route == 'plan' else C.BinnedScatter)
    spk_r, spk_c = rng.random(m) < 0.05, rng.random(k) < 0.05
    before_s = (be.BinaryArray(spk_r) @ M).copy()
    before_g = (M @ be.BinaryArray(spk_c)).copy()
    pre_s, post_s = rng.random(m) < 0.5, rng.random(k) < 0.5
    M.update_on_pre(pre_s, np.full(k, 3.0, np.float32), inplace=True)
    M.update_on_post(np.full(m, 2.0, np.float32), post_s, inplace=True)
    w_new = model_cols(model_rows(w, idx, ptr, pre_s, np.full(k, 3.0, np.float32)), idx, ptr, post_s, np.full(m, 2.0, np.float32))
    assert_bit_equal(M.data, w_new)
    ref_s = oracle_np.binary_csrmv(w_new.astype(np.float64), idx, ptr, spk_r, (m, k), True)
    ref_g = oracle_np.binary_csrmv(w_new.astype(np.float64), idx, ptr, spk_c, (m, k), False)
    assert np.abs(ref_s - before_s).max() > 100 * 1e-5 * np.abs(ref_s).max()       # the update is far above the tolerance
    assert np.abs(ref_g - before_g).max() > 100 * 1e-5 * np.abs(ref_g).max()
    np.testing.assert_allclose(be.BinaryArray(spk_r) @ M, ref_s, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(M @ be.BinaryArray(spk_c), ref_g, rtol=1e-5, atol=1e-5)


def test_graph_capture_matches_eager():
    """product (gather over a CSC: deterministic sums), lif_coba_step, trace decay, both updates in place."""
    rng = np.random.default_rng(13)
    n, steps = 300, 50
    idx, ptr = random_csr(rng, n, n, max_len=30)         # CSC of W (n_pre = n_post = n): stored rows = post neurons
    w0 = torch.tensor(rng.uniform(0.2, 0.8, len(idx)).astype(np.float32), device=DEV)
    ext = torch.tensor(rng.random((steps + 8, n)) < 0.05, device=DEV)

    def make():
        M = be.CSC((w0.clone(), torch.tensor(idx, device=DEV), torch.tensor(ptr, device=DEV)), shape=(n, n))
        st = dict(v=torch.full((n,), -60.0, device=DEV), ge=torch.zeros(n, device=DEV), gi=torch.zeros(n, device=DEV),
                  ref=torch.zeros(n, device=DEV), spk=torch.zeros(n, dtype=torch.uint8, device=DEV),
                  xpre=torch.zeros(n, device=DEV), xpost=torch.zeros(n, device=DEV), ext=torch.zeros(n, dtype=torch.bool, device=DEV))
        return M, st

    def step(M, st):
        drive = be.BinaryArray(st['ext']) @ M                       # gather: the input each post neuron receives
        be.lif_coba_step(st['v'], st['ge'], st['gi'], st['ref'], drive * 5.0, torch.zeros_like(drive), st['spk'], dt=1.0)
        st['xpre'].mul_(0.95).add_(st['ext'].float())
        st['xpost'].mul_(0.95).add_(st['spk'].float())
        M.update_on_pre(st['ext'], st['xpost'] * 0.01, 0.0, 1.0, inplace=True)
        M.update_on_post(st['xpre'] * -0.012, st['spk'], 0.0, 1.0, inplace=True)

    Me, se = make()
    for t in range(steps):
        se['ext'].copy_(ext[t])
        step(Me, se)
    Mg, sg = make()
    keep = {k: v.clone() for k, v in sg.items()}
    graphed = be.capture_step(lambda: step(Mg, sg))
    Mg.data.copy_(w0)
    for k, v in keep.items():
        sg[k].copy_(v)
    for t in range(steps):
        sg['ext'].copy_(ext[t])
        graphed()
    torch.cuda.synchronize()
    assert not torch.equal(Me.data, w0)          # post neurons fired: both rules moved weights
    assert_bit_equal(Mg.data, Me.data, 'weights')
    assert_bit_equal(sg['v'], se['v'], 'membrane')


def test_above_2_31_entries():
    """CSR of 2**31 + 2**17 entries (int64 indptr, int64 perm): both directions against a torch model on the device."""
    m, L, k = 1 << 17, (1 << 14) + 1, 50000
    nnz = m * L
    assert nnz > 2**31
    g = torch.Generator(device=DEV).manual_seed(0)
    idx = torch.randint(0, k, (nnz,), dtype=torch.int32, device=DEV, generator=g)
    ptr = torch.arange(m + 1, dtype=torch.int64, device=DEV) * L
    w = torch.rand(nnz, device=DEV, generator=g)
    M = be.CSR._from_parts(w, idx, ptr, shape=(m, k))
    act_r = torch.rand(m, device=DEV, generator=g) < 0.03
    act_c = torch.rand(k, device=DEV, generator=g) < 0.03
    tr_c = torch.rand(k, device=DEV, generator=g) - 0.5
    tr_r = torch.rand(m, device=DEV, generator=g) - 0.5
    w0 = w.clone()
    M.update_on_pre(act_r, tr_c, inplace=True)
    M.update_on_post(tr_r, act_c, inplace=True)
    assert M.buffers[P.INDEX_KEY][2].dtype == torch.int64
    W, I, W0 = M.data.view(m, L), idx.view(m, L), w0.view(m, L)
    for r0 in range(0, m, 8192):                  # w + trace[idx] * active (exact for active in {0, 1}), in row chunks
        r1 = min(m, r0 + 8192)
        ref = W0[r0:r1] + tr_c[I[r0:r1].long()] * act_r[r0:r1, None].float()
        ref = ref + tr_r[r0:r1, None] * act_c[I[r0:r1].long()].float()
        assert torch.equal(W[r0:r1], ref), r0
