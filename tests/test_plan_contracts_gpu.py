"""Contracts of the per-matrix scatter workspace (the role of the reference's cached task workspace,
``brainevent/_csr/main.py:58-88``, ``:148-161``): sizing of the partial sums, in-place weight updates, workspace lifetime
under graph capture, and the C ABI's own checks of what the Python layer normally guards.

Oracle: ``oracle/oracle_np.py`` (numpy restatement of ``_csr/binary.py:387-489`` / ``_fcn/binary.py:156-253``).
Tolerance: f32 accumulated currents rtol = atol = 1e-5; homogeneous counts exact.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-5


def _fixed_rows(rng, m, k, row, homo):
    idx = rng.integers(0, k, m * row).astype(np.int32)
    ptr = (np.arange(m + 1) * row).astype(np.int32)
    w = np.ones(1, np.float32) if homo else rng.uniform(0.1, 1.0, m * row).astype(np.float32)
    return w, idx, ptr


@pytest.mark.parametrize('width', [32769, 32770, 32771, 39998])
def test_h8_partial_sums_fit_the_sized_workspace(be, oracle, width):
    """h8 slices wider than 2^15 whose width is not a multiple of 4: a task's partial sums are (width + 3) & ~3 counters
    wide, which the workspace query has to cover (it used to size for width + 1).  A canary behind the workspace the
    query asked for must survive the call."""
    from brainevent_amd._csr import ScatterPlan, _plan_call
    from brainevent_amd import _array as A
    from brainevent_amd._lib import fn
    rng = np.random.default_rng(width)
    m, k, row, parts = 300, 2 * width, 700, 10
    w, idx, ptr = _fixed_rows(rng, m, k, row, homo=True)
    plan = ScatterPlan.build(w, idx, torch.tensor(ptr), shape=(m, k), slice_width=width, layout='h8')
    assert plan.layout == ScatterPlan.LAYOUT_H8 and plan.slice_width == width and plan.n_slices == 2
    f = fn('be_binary_csrmm_t_plan_workspace_bytes', ctypes.c_int64,
           [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int])
    nbytes = int(f(m, k, 1, plan.slice_shift, plan.slice_width, parts, 1))
    big = torch.full((nbytes + 4096,), 0xAB, dtype=torch.uint8, device='cuda')
    big[:1024].zero_()                                   # spike counters: zero on entry
    plan._ws[(parts, 1)] = big[:nbytes]
    v = rng.random(m) < 0.5
    spikes, sd = A.spikes_to_device(v)
    out = torch.empty(k, dtype=torch.float32, device='cuda')
    _plan_call(plan, A.to_device(w), spikes, sd, out, parts=parts)
    torch.cuda.synchronize()
    assert bool((big[nbytes:] == 0xAB).all()), "the planned step wrote past the workspace the library asked for"
    ref = np.zeros(k, np.int64)
    np.add.at(ref, idx.reshape(m, row)[v].reshape(-1), 1)
    np.testing.assert_array_equal(out.cpu().numpy().astype(np.int64), ref)


def test_plan_follows_in_place_weight_updates(be, oracle, monkeypatch):
    """The plan embeds heterogeneous weights; the containers notice ``data`` modified in place (``_version``) and refresh the
    blocks — the reference's workspace is weight independent (``_csr/main.py:58-88``), so the same code is legal there."""
    import brainevent_amd._csr as C
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1000)
    rng = np.random.default_rng(3)
    m, k, row = 500, 30000, 300
    w, idx, ptr = _fixed_rows(rng, m, k, row, homo=False)
    data = torch.tensor(w, device='cuda')
    csr = be.CSR((data, torch.tensor(idx, device='cuda'), torch.tensor(ptr, device='cuda')), shape=(m, k))
    v = rng.random(m) < 0.2
    spk = be.BinaryArray(torch.tensor(v, device='cuda'))
    y0 = (spk @ csr).cpu().numpy()
    plan = csr.buffers['scatter_plan']
    assert isinstance(plan, C.ScatterPlan) and not plan.is_stale(csr.data)
    np.testing.assert_allclose(y0, oracle.binary_csrmv(w.astype(np.float64), idx, ptr, v, (m, k), True), rtol=RTOL, atol=ATOL)
    blob_ptr, e0 = plan.blob.data_ptr(), plan.scale_exp
    # plasticity-style update: scale some weights, overwrite others
    data.mul_(0.5)
    data[::3] = torch.tensor(rng.uniform(-1, 1, len(w[::3])).astype(np.float32), device='cuda')
    w1 = data.cpu().numpy()
    assert plan.is_stale(csr.data)
    y1 = (spk @ csr).cpu().numpy()
    assert csr.buffers['scatter_plan'] is plan and plan.blob.data_ptr() == blob_ptr, "refresh must reuse the blocks"
    assert plan.scale_exp == e0, "the exponent is kept while it still cannot overflow (captured graphs hold it)"
    np.testing.assert_allclose(y1, oracle.binary_csrmv(w1.astype(np.float64), idx, ptr, v, (m, k), True), rtol=RTOL, atol=ATOL)
    # much larger weights: the kept exponent would overflow, a new one is derived
    data.mul_(1e6)
    y2 = (spk @ csr).cpu().numpy()
    assert plan.scale_exp < e0
    np.testing.assert_allclose(y2, oracle.binary_csrmv(data.cpu().numpy().astype(np.float64), idx, ptr, v, (m, k), True),
                               rtol=RTOL, atol=ATOL * 1e6)
    # weights the fixed-point sums cannot hold: the container falls back to the direct route instead of a wrong answer
    data[0] = float('inf')
    y3 = (spk @ csr).cpu().numpy()
    assert csr.buffers['scatter_plan'] is None
    ref3 = oracle.binary_csrmv(data.cpu().numpy().astype(np.float64), idx, ptr, v, (m, k), True)
    np.testing.assert_allclose(y3, ref3, rtol=RTOL, atol=ATOL * 1e6)


def test_mirror_and_fixed_num_follow_in_place_weight_updates(be, oracle, monkeypatch):
    import brainevent_amd._csr as C
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1000)
    rng = np.random.default_rng(4)
    m, k, row = 400, 20000, 256
    w, idx, ptr = _fixed_rows(rng, m, k, row, homo=False)
    data = torch.tensor(w, device='cuda')
    csr = be.CSR((data, torch.tensor(idx, device='cuda'), torch.tensor(ptr, device='cuda')), shape=(m, k)).prepare(mirror=True)
    v2 = rng.random(k) < 0.05
    g0 = (csr @ be.BinaryArray(torch.tensor(v2, device='cuda'))).cpu().numpy()
    np.testing.assert_allclose(g0, oracle.binary_csrmv(w.astype(np.float64), idx, ptr, v2, (m, k), False), rtol=RTOL, atol=ATOL)
    data.add_(0.25)
    g1 = (csr @ be.BinaryArray(torch.tensor(v2, device='cuda'))).cpu().numpy()
    np.testing.assert_allclose(g1, oracle.binary_csrmv((w + np.float32(0.25)).astype(np.float64), idx, ptr, v2, (m, k), False),
                               rtol=RTOL, atol=ATOL)
    # FixedNumPerPre: same contract
    fdata = torch.tensor(w.reshape(m, row), device='cuda')
    fcn = be.FixedNumPerPre((fdata, torch.tensor(idx.reshape(m, row), device='cuda')), shape=(m, k))
    v = rng.random(m) < 0.3
    spk = be.BinaryArray(torch.tensor(v, device='cuda'))
    f0 = (spk @ fcn).cpu().numpy()
    assert isinstance(fcn.buffers['scatter_plan'], C.ScatterPlan)
    np.testing.assert_allclose(f0, oracle.binary_csrmv(w.astype(np.float64), idx, ptr, v, (m, k), True), rtol=RTOL, atol=ATOL)
    fdata.mul_(-2.0)
    f1 = (spk @ fcn).cpu().numpy()
    np.testing.assert_allclose(f1, oracle.binary_csrmv((w * np.float32(-2)).astype(np.float64), idx, ptr, v, (m, k), True),
                               rtol=RTOL, atol=ATOL)


def test_binned_route_follows_in_place_weight_updates(be, oracle):
    from brainevent_amd._csr import BinnedScatter
    rng = np.random.default_rng(5)
    m, k, row = 300, 200000, 64
    w, idx, ptr = _fixed_rows(rng, m, k, row, homo=False)
    data = torch.tensor(w, device='cuda')
    tidx, tptr = torch.tensor(idx, device='cuda'), torch.tensor(ptr, device='cuda')
    ws = BinnedScatter(data, m, k, m * row, indices=tidx)
    v = rng.random(m) < 0.3
    e0 = ws.scale_exp
    data.mul_(1e5)
    assert ws.is_stale(data)
    from brainevent_amd._csr import fresh_scatter_workspace
    assert fresh_scatter_workspace(ws, data, tidx, tptr) is ws and ws.scale_exp < e0
    got = be.binary_csrmv(data, tidx, tptr, torch.tensor(v, device='cuda'), shape=(m, k), transpose=True, workspace=ws)
    ref = oracle.binary_csrmv(data.cpu().numpy().astype(np.float64), idx, ptr, v, (m, k), True)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=RTOL, atol=ATOL * 1e5)


def test_plan_keeps_every_workspace_it_handed_out(be):
    """A captured graph keeps the raw pointer of the workspace it was recorded with: a later call with another
    (parts, n_batch) must not free it."""
    from brainevent_amd._csr import ScatterPlan
    rng = np.random.default_rng(6)
    m, k, row = 200, 5000, 100
    w, idx, ptr = _fixed_rows(rng, m, k, row, homo=True)
    plan = ScatterPlan.build(w, idx, torch.tensor(ptr), shape=(m, k), slice_shift=10)
    a = plan.workspace(3, 1)
    b = plan.workspace(2, 4)
    c = plan.workspace(3, 1)
    assert a.data_ptr() == c.data_ptr() and a.data_ptr() != b.data_ptr()
    assert len(plan._ws) == 2


def test_c_abi_refuses_rows_the_delta_layouts_cannot_sort(be):
    """``be_scatter_plan_count`` with BE_PLAN_D8 / BE_PLAN_H8 and a real indptr checks the row lengths on the device:
    a 20000-entry row is BE_ERR_RANGE at the boundary, not a silently truncated row."""
    from brainevent_amd._lib import fn, lib
    c_i64, c_int, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    rng = np.random.default_rng(8)
    m, k = 64, 100000
    lens = np.full(m, 50, np.int64)
    lens[17] = 20000
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device='cuda')
    idx = torch.tensor(rng.integers(0, k, int(lens.sum())).astype(np.int32), device='cuda')
    f_scr = fn('be_scatter_plan_scratch_bytes', c_i64, [c_i64, c_i64, c_int, c_int])
    f_cnt = fn('be_scatter_plan_count', c_int,
               [c_vp, c_vp, c_int, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, c_vp, c_vp, c_i64, ctypes.POINTER(c_i64), c_vp])
    for layout, homo, shift in ((1, 0, 14), (2, 1, 15)):
        width = 1 << shift
        n_slices = -(-k // width)
        seg = torch.zeros(n_slices * m * 2, dtype=torch.int32, device='cuda')
        scratch = torch.empty(int(f_scr(m, k, shift, width)), dtype=torch.uint8, device='cuda')
        blob_bytes = c_i64(-1)
        rc = f_cnt(idx.data_ptr(), ptr.data_ptr(), 0, -1, m, k, shift, width, homo, layout, seg.data_ptr(), scratch.data_ptr(),
                   scratch.numel(), ctypes.byref(blob_bytes), None)
        assert rc == -4, rc                                     # BE_ERR_RANGE
        assert b'20000' in lib().be_last_error()
        # the uint16 layout takes the same matrix
        rc = f_cnt(idx.data_ptr(), ptr.data_ptr(), 0, -1, m, k, shift, width, homo, 0, seg.data_ptr(), scratch.data_ptr(),
                   scratch.numel(), ctypes.byref(blob_bytes), None)
        assert rc == 0 and blob_bytes.value > 0
    # and the Python layer still routes such a matrix to the uint16 layout by itself
    from brainevent_amd._csr import ScatterPlan
    plan = ScatterPlan.build(np.ones(1, np.float32), idx, ptr, shape=(m, k))
    assert plan.layout == ScatterPlan.LAYOUT_U16


@pytest.mark.parametrize('homo', [True, False])
def test_binned_route_is_bitwise_reproducible_with_one_workgroup_per_slice(be, oracle, homo):
    """include/brainevent_amd.h, binned scatter, "Reproducibility": more than 128 slices and no overflowing region ->
    integer sums converted once, identical bits on every call; an overflowing region switches that run to float atomics
    (still within tolerance)."""
    from brainevent_amd._csr import BinnedScatter
    rng = np.random.default_rng(21)
    m, k, row = 3000, 5_000_000, 400                   # 306 slices of 2^14 (153 of 2^15 counted)
    w, idx, ptr = _fixed_rows(rng, m, k, row, homo)
    if not homo:
        w = rng.normal(0, 1, w.shape).astype(np.float32)
    wd, idd, ptd = torch.tensor(w, device='cuda'), torch.tensor(idx, device='cuda'), torch.tensor(ptr, device='cuda')
    v = torch.tensor(rng.random(m) < 0.3, device='cuda')
    ws = BinnedScatter(wd, m, k, idx.size, max_active_fraction=0.5, indices=idd)
    assert ws.n_slices > 128
    outs = [be.binary_csrmv(wd, idd, ptd, v, shape=(m, k), transpose=True, workspace=ws) for _ in range(4)]
    for o in outs[1:]:
        assert torch.equal(outs[0], o), 'binned route with one workgroup per slice must be bitwise reproducible'
    ref = oracle.binary_csrmv(w.astype(np.float64), idx, ptr, v.cpu().numpy(), (m, k), True)
    np.testing.assert_allclose(outs[0].cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
    # regions sized far too small: overflowing runs are delivered by float atomics — correct, order dependent in the last bit
    tiny = BinnedScatter(wd, m, k, idx.size, max_active_fraction=1e-4, indices=idd)
    got = be.binary_csrmv(wd, idd, ptd, v, shape=(m, k), transpose=True, workspace=tiny)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=RTOL, atol=1e-4)


# ---------------------------------------------------------------------------------------------------
# the dtype / shape matrix of the reference's scatter variants (f64 / f16 / bf16 weights, batched operands:
# brainevent/_csr/binary_csrmv_hybrid.cu:789-821, binary_csrmm_hybrid.cu:469-530) on the fast routes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('homo', [True, False])
@pytest.mark.parametrize('layout', [None, 'u16'])
def test_f64_weights_take_the_planned_route(be, oracle, monkeypatch, homo, layout):
    """Per-entry f64 weights are stored as two f32 entries (hi + lo), summed exactly as 64-bit integers and scaled once in
    f64: 1e-10 relative, the bar of the f64 tests; one f64 weight is a count times the weight in f64."""
    import brainevent_amd._csr as C
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1000)
    rng = np.random.default_rng(31)
    m, k, row = 700, 40000, 300
    idx = rng.integers(0, k, m * row).astype(np.int32)
    ptr = (np.arange(m + 1) * row).astype(np.int64)
    w = np.asarray([0.37], np.float64) if homo else rng.normal(0, 1, m * row) * np.exp(rng.uniform(-3, 3, m * row))
    data = torch.tensor(w, device='cuda')
    tidx, tptr = torch.tensor(idx, device='cuda'), torch.tensor(ptr, device='cuda')
    if layout is None:
        csr = be.CSR((data, tidx, tptr), shape=(m, k)).prepare()
        plan = csr.buffers['scatter_plan']
    else:
        csr = be.CSR((data, tidx, tptr), shape=(m, k))
        plan = csr.buffers['scatter_plan'] = C.ScatterPlan.build(data, tidx, tptr, shape=(m, k), layout=layout)
    assert isinstance(plan, C.ScatterPlan) and plan.split_f64 == (not homo)
    for fire in (0.1, 1.0):
        v = rng.random(m) < fire
        got = be.BinaryArray(torch.tensor(v, device='cuda')) @ csr
        assert got.dtype == torch.float64
        ref = oracle.binary_csrmv(w, idx, ptr, v, (m, k), True)
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-10, atol=1e-10 * max(1.0, float(np.abs(ref).max())))
    B = rng.random((3, m)) < 0.3                               # batched
    gotB = be.BinaryArray(torch.tensor(B, device='cuda')) @ csr
    refB = np.stack([oracle.binary_csrmv(w, idx, ptr, B[b], (m, k), True) for b in range(3)])
    np.testing.assert_allclose(gotB.cpu().numpy(), refB, rtol=1e-10, atol=1e-10 * max(1.0, float(np.abs(refB).max())))
    if not homo:                                               # in-place update of f64 weights: the split blocks follow
        data.mul_(-0.5)
        v = rng.random(m) < 0.5
        got = be.BinaryArray(torch.tensor(v, device='cuda')) @ csr
        assert csr.buffers['scatter_plan'] is plan
        np.testing.assert_allclose(got.cpu().numpy(), oracle.binary_csrmv(w * -0.5, idx, ptr, v, (m, k), True), rtol=1e-10, atol=1e-9)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize('homo', [True, False])
def test_binned_route_half_precision_and_batches(be, oracle, monkeypatch, dtype, homo):
    """Sparse rows over many outputs (the binned route) with f16 / bf16 weights and with a batch of spike vectors: the bins carry
    f32, sums are exact integers, the output is rounded once."""
    import brainevent_amd._csr as C
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1000)
    rng = np.random.default_rng(32)
    n_pre, n_post, K = 3000, 400_000, 24                   # 24 entries over 25 slices: the binned route
    idx = rng.integers(0, n_post, (n_pre, K)).astype(np.int32)
    w32 = np.asarray([0.75], np.float32) if homo else rng.uniform(0.1, 1.0, (n_pre, K)).astype(np.float32)
    data = torch.tensor(w32, device='cuda').to(dtype)
    wref = data.float().cpu().numpy().astype(np.float64)
    conn = be.FixedNumPerPre((data, torch.tensor(idx, device='cuda')), shape=(n_pre, n_post))
    tol = {torch.float32: 1e-5, torch.float16: 2e-3, torch.bfloat16: 1.6e-2}[dtype]
    v = rng.random(n_pre) < 0.2
    got = be.BinaryArray(torch.tensor(v, device='cuda')) @ conn
    assert isinstance(conn.buffers['scatter_plan'], C.BinnedScatter) and got.dtype == dtype
    ptr = (np.arange(n_pre + 1) * K).astype(np.int64)
    ref = oracle.binary_csrmv(wref.reshape(-1), idx.reshape(-1), ptr, v, (n_pre, n_post), True)
    np.testing.assert_allclose(got.float().cpu().numpy(), ref, rtol=tol, atol=tol)
    B = rng.random((4, n_pre)) < 0.2
    gotB = be.BinaryArray(torch.tensor(B, device='cuda')) @ conn
    refB = np.stack([oracle.binary_csrmv(wref.reshape(-1), idx.reshape(-1), ptr, B[b], (n_pre, n_post), True) for b in range(4)])
    assert gotB.shape == (4, n_post)
    np.testing.assert_allclose(gotB.float().cpu().numpy(), refB, rtol=tol, atol=tol)


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('layout,homo', [('d8', False), ('u16', False), ('u16', True), ('h8', True)])
def test_fused_step_lists_its_rows_in_the_kernel_and_spills_to_the_workspace(be, oracle, layout, homo, packed):
    """The planned step lists the active rows of each part inside the accumulate kernel when LDS has room behind the
    accumulators (be_csr_plan.hip: build_part_list).  Dense firing over many rows makes a part's list outgrow that room:
    it is then written to the part's region of the workspace.  Bit-packed and 1-byte spikes, every layout, a row count that
    is not a multiple of the 1024-row stripes; results against the oracle, bitwise equal between the two spike encodings."""
    from brainevent_amd._csr import ScatterPlan, _plan_call
    from brainevent_amd import _array as A
    rng = np.random.default_rng(77)
    m, row = 200_123, 6
    width = 18000 if layout != 'u16' else (16000 if not homo else 30000)
    k = 2 * width
    w, idx, ptr = _fixed_rows(rng, m, k, row, homo)
    if not homo:
        w = rng.normal(0, 1, w.shape).astype(np.float32)
    plan = ScatterPlan.build(w, idx, torch.tensor(ptr), shape=(m, k), slice_width=width, layout=layout)
    outs = []
    for fire in (1.0, 0.5, 0.001):
        v = rng.random(m) < fire
        ev = be.BinaryArray(torch.tensor(v, device='cuda'))
        spikes, sd = A.spikes_to_device(A.PackedSpikes(ev.bitpack().packed[0], m) if packed else ev.value)
        assert sd == (A.BE_SPIKE_BITS if packed else A.BE_SPIKE_BOOL)
        out = torch.empty(k, dtype=torch.float32, device='cuda')
        _plan_call(plan, A.to_device(w), spikes, sd, out, parts=4)
        ref = oracle.binary_csrmv(w.astype(np.float64), idx, ptr, v, (m, k), True)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=RTOL, atol=ATOL * max(1.0, float(np.abs(ref).max())))
        outs.append(out.clone())
    assert len(outs) == 3


def test_plan_that_does_not_fit_memory_falls_back_to_the_binned_route(be, oracle, monkeypatch):
    """A scatter plan costs 128 bytes per (row, slice) block; when it does not fit the free device memory the container
    takes the binned route (no per-matrix layout) instead of failing — simulated by an out-of-memory error in the build."""
    from brainevent_amd import _csr as C
    rng = np.random.default_rng(8)
    m, k, row = 3000, 40000, 60
    idx = rng.integers(0, k, (m, row)).astype(np.int32)
    w = rng.random((m, row)).astype(np.float32)
    oom = getattr(torch, 'OutOfMemoryError', RuntimeError)

    def no_room(*a, **kw):
        raise oom('HIP out of memory (simulated)')
    monkeypatch.setattr(C.ScatterPlan, 'build', classmethod(lambda cls, *a, **kw: no_room()))
    monkeypatch.setattr(C, 'choose_scatter_route', lambda *a, **kw: 'plan')
    conn = be.FixedNumPerPre((w, idx), shape=(m, k)).prepare()
    assert isinstance(conn.buffers['scatter_plan'], C.BinnedScatter)
    spk = rng.random(m) < 0.1
    ptr = (np.arange(m + 1) * row).astype(np.int32)
    got = be.BinaryArray(spk) @ conn
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, oracle.binary_csrmv(w.reshape(-1), idx.reshape(-1), ptr, spk, (m, k), True), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('homo', [False, True])
@pytest.mark.parametrize('enc', ['bool', 'float', 'bits'])
def test_binned_batch_reads_the_rows_once_for_the_whole_batch(be, oracle, homo, enc):
    """be_binary_csrmm_t_binned: the rows with a spike in any batch row are streamed once, every entry appended once per batch
    row that has its row active (virtual bins = batch row x bin).  Against the oracle per batch row (the reference's batched
    scatter is a loop over the columns, brainevent/_fcn/binary_fcnmm.cu:486-529), ragged CSR rows including empty ones, batch
    sizes on both sides of the 32 rows one pass takes, all three spike encodings, bitwise equal between them."""
    from brainevent_amd._csr import BinnedScatter, binned_batch
    from brainevent_amd import _array as A
    rng = np.random.default_rng(5 + int(homo))
    m, k = 20_000, 300_000
    lens = rng.integers(0, 40, m)
    lens[::7] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    w = np.asarray([1.5], np.float32) if homo else rng.uniform(-1.0, 1.0, idx.size).astype(np.float32)
    wd, idd, ptd = (torch.tensor(x, device='cuda') for x in (w, idx, ptr))
    ws = BinnedScatter(wd, m, k, idx.size, max_active_fraction=0.3, indices=idd)
    for nb in (2, 8, 37):
        S = rng.random((nb, m)) < 0.1
        S[1, :] = False                                    # a batch row without a spike
        if enc == 'bool':
            sp, sd = torch.tensor(S, device='cuda'), A.BE_SPIKE_BOOL
        elif enc == 'float':
            sp, sd = torch.tensor(np.where(S, 0.5, -1.0).astype(np.float32), device='cuda'), A.BE_SPIKE_FLOAT
        else:
            words = np.packbits(np.pad(S, ((0, 0), (0, (-m) % 32))), axis=1, bitorder='little').view(np.uint32)
            sp, sd = torch.tensor(words.view(np.int32), device='cuda'), A.BE_SPIKE_BITS
        out = torch.full((nb, k), 7.0, dtype=torch.float32, device='cuda')      # every output has to be written
        binned_batch(ws, wd, idd, ptd, -1, sp, sd, out)
        ref = np.stack([oracle.binary_csrmv(w.astype(np.float64), idx, ptr, S[b], (m, k), True) for b in range(nb)])
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
        out2 = torch.empty_like(out)
        binned_batch(ws, wd, idd, ptd, -1, sp, sd, out2)
        # (fewer than 129 virtual bins: several workgroups of pass C share a bin and merge through float atomics, see the header)
        np.testing.assert_allclose(out2.cpu().numpy(), out.cpu().numpy(), rtol=1e-6, atol=1e-6)
        if nb >= 32:          # the first pass takes 32 batch rows: 16 bins each = 512 virtual bins, one workgroup per bin
            assert torch.equal(out[:32], out2[:32]), 'integer sums converted once: bitwise reproducible'



@pytest.mark.parametrize('layout,homo', [('d8', False), ('h8', True)])
def test_stored_row_order_builds_and_refreshes_the_same_blocks(be, oracle, layout, homo):
    """The sorted layouts keep the rows' column order from the count pass (`be_scatter_plan_*_ordered`): a build that reads it
    back in the fill, a build without it, and a weight refresh through the kept order (a gather-copy) or without it (a
    re-sort) produce the same segment table and bit-identical products; rows are ragged, some empty, some already ascending,
    columns repeat."""
    from brainevent_amd._csr import ScatterPlan
    rng = np.random.default_rng(77)
    m, k = 700, 90_000
    lens = rng.integers(0, 900, m)
    lens[::50] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, k, ptr[-1]).astype(np.int32)
    for r in range(0, m, 7):                            # canonical rows: no sort happens, the order is the identity
        idx[ptr[r]:ptr[r + 1]] = np.sort(idx[ptr[r]:ptr[r + 1]])
    idx[ptr[3]:ptr[3] + 5] = idx[ptr[3]]                # repeated columns inside a row
    w = np.ones(1, np.float32) if homo else rng.uniform(0.1, 1.0, ptr[-1]).astype(np.float32)
    wd, idd, ptd = torch.tensor(w, device='cuda'), torch.tensor(idx, device='cuda'), torch.tensor(ptr, device='cuda')
    plans = {ko: ScatterPlan.build(wd, idd, ptd, shape=(m, k), layout=layout, keep_order=ko) for ko in (True, False, None)}
    assert plans[False].order is None and (plans[True].order is not None) == (not homo)
    assert (plans[None].order is not None) == (not homo)          # small next to the plan: kept by default (weighted plans only)
    spikes = [torch.tensor(rng.random(m) < p, device='cuda') for p in (0.3, 1.1, 0.02)]        # (1.1: every row)

    def same_products(wt):       # (the blocks' unwritten alignment padding differs from build to build: compare what they compute)
        outs = {ko: [be.binary_csrmv(wt, idd, ptd, sv, shape=(m, k), transpose=True, workspace=plans[ko]) for sv in spikes]
                for ko in plans}
        for ko in (False, None):
            assert torch.equal(plans[True].seg, plans[ko].seg)
            assert all(torch.equal(a, b) for a, b in zip(outs[True], outs[ko])), ko
    same_products(wd)
    v = spikes[0]
    ref = oracle.binary_csrmv(np.broadcast_to(w, idx.shape).astype(np.float64), idx, ptr, v.cpu().numpy(), (m, k), True)
    out = be.binary_csrmv(wd, idd, ptd, v, shape=(m, k), transpose=True, workspace=plans[True])
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
    if homo:
        return
    order = plans[True].order.cpu().numpy().view(np.uint16)
    for r in (1, 2, 8, 14, m - 1):                      # the stored order sorts every row's columns
        seg = idx[ptr[r]:ptr[r + 1]][order[ptr[r]:ptr[r + 1]]]
        assert np.all(np.diff(seg) >= 0) and sorted(order[ptr[r]:ptr[r + 1]]) == list(range(ptr[r + 1] - ptr[r]))
    w2 = rng.uniform(0.1, 1.0, ptr[-1]).astype(np.float32)
    w2d = torch.tensor(w2, device='cuda')
    for ko in plans:
        plans[ko].refresh_weights(w2d, idd, ptd)
    same_products(w2d)
    out = be.binary_csrmv(w2d, idd, ptd, v, shape=(m, k), transpose=True, workspace=plans[True])
    ref2 = oracle.binary_csrmv(w2.astype(np.float64), idx, ptr, v.cpu().numpy(), (m, k), True)
    np.testing.assert_allclose(out.cpu().numpy(), ref2, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('layout', ['d8', 'u16'])
def test_plan_exponent_from_its_own_blocks_matches_the_entry_pass(be, oracle, layout):
    """`be_scatter_plan_exponent` (column statistics from the plan's blocks: a planned step over |w| with every row active)
    against `be_fixed_point_exponent` (global atomics over the raw entries): the same exponent — or one step HIGHER where the
    largest column sum lies within 0.1 % under a power of two: the plan's bound is the sum itself (addends rounded up), the
    entry pass adds a margin of 1.001; never lower (tests/exponent_cases.py derives it, tests/test_exponent_exact_gpu.py builds
    the case in that band) — over weight scales, signs, repeated columns and blocks of more than 256 items; the same refusal
    of weights the sums cannot resolve; keep_exp honoured."""
    from brainevent_amd._csr import ScatterPlan, fixed_point_exponent, MathError
    rng = np.random.default_rng(5)
    m, k = 900, 60_000
    lens = rng.integers(0, 1500, m)
    lens[0] = 4000                                    # ~1300 items per (row, slice): several 64-lane-group passes per block
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, k, ptr[-1]).astype(np.int32)
    idx[ptr[5]:ptr[5] + 300] = 77                     # one column listed 300 times in a row: column sums are not bounded by rows x max
    idd, ptd = torch.tensor(idx, device='cuda'), torch.tensor(ptr, device='cuda')
    for scale, signed in ((1.0, False), (1e-3, True), (4096.0, True), (2.0 ** -20, False)):
        w = (rng.uniform(0.25, 1.0, ptr[-1]) * scale).astype(np.float32)
        if signed:
            w *= rng.choice([-1.0, 1.0], w.size).astype(np.float32)
        wd = torch.tensor(w, device='cuda')
        plan = ScatterPlan.build(wd, idd, ptd, shape=(m, k), layout=layout)
        e_ref = fixed_point_exponent(wd, idd, k)
        assert plan.scale_exp in (e_ref, e_ref + 1), (plan.scale_exp, e_ref, scale)
        # no column can overflow at the chosen exponent with every row active
        colsum = np.zeros(k)
        np.add.at(colsum, idx, np.abs(w.astype(np.float64)))
        assert colsum.max() * 2.0 ** plan.scale_exp < 2.0 ** 62
        v = torch.ones(m, dtype=torch.bool, device='cuda')
        out = be.binary_csrmv(wd, idd, ptd, v, shape=(m, k), transpose=True, workspace=plan)
        ref = oracle.binary_csrmv(w.astype(np.float64), idx, ptr, np.ones(m, bool), (m, k), True)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=RTOL, atol=ATOL * scale)
        # a refresh with smaller weights keeps the exponent (it still cannot overflow); larger ones that would overflow move it
        e0 = plan.scale_exp
        plan.refresh_weights(wd * 0.5, idd, ptd)
        assert plan.scale_exp == e0
        plan.refresh_weights(wd * 64.0, idd, ptd)
        assert plan.scale_exp <= e0 - 5
    # a column whose only weights the sums cannot resolve next to huge ones elsewhere: refused like the entry pass refuses it
    w = rng.uniform(0.5, 1.0, ptr[-1]).astype(np.float32)
    w[idx == idx[ptr[9]]] = 1e-30
    w[ptr[20]] = 1e30 if idx[ptr[20]] != idx[ptr[9]] else w[ptr[20]]
    wd = torch.tensor(w, device='cuda')
    with pytest.raises(MathError):
        fixed_point_exponent(wd, idd, k)
    with pytest.raises(MathError):
        ScatterPlan.build(wd, idd, ptd, shape=(m, k), layout=layout)


@pytest.mark.parametrize('layout,homo', [('d8', False), ('u16', False), ('h8', True), ('u16', True)])
def test_plan_built_from_row_blocks_equals_the_resident_build(be, oracle, layout, homo):
    """`ScatterPlan.build_from_blocks` (the raw arrays resident one block of rows at a time: `be_scatter_plan_begin / _count_rows /
    _scan`, the fill per block) gives the plan `build` gives for the whole matrix — same segment table, same exponent, bit-identical
    products — and `PlannedMatrix` serves `events @ M` from the plan alone: vectors, batches, packed words; ragged rows with
    int32 / int64 row pointers and fixed-length rows; uneven last block."""
    from brainevent_amd._csr import ScatterPlan, PlannedMatrix
    rng = np.random.default_rng(123)
    m, k = 1000, 70_000
    for fixed in (False, True):
        lens = np.full(m, 300) if fixed else rng.integers(0, 700, m)
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        idx = rng.integers(0, k, ptr[-1]).astype(np.int32)
        w = np.full(1, 0.75, np.float32) if homo else rng.normal(0, 1, ptr[-1]).astype(np.float32)
        wd, idd = torch.tensor(w, device='cuda'), torch.tensor(idx, device='cuda')
        ptd = torch.tensor(ptr.astype(np.int32), device='cuda')
        whole = ScatterPlan.build(wd, idd, None if fixed else ptd, shape=(m, k), row_len=300 if fixed else -1, layout=layout)
        calls = []

        def get_block(r0, r1, _ptr_dtype=[torch.int32, torch.int64]):
            calls.append((r0, r1))
            lo, hi = int(ptr[r0]), int(ptr[r1])
            pb = None if fixed else torch.tensor(ptr[r0:r1 + 1] - ptr[r0], device='cuda').to(_ptr_dtype[len(calls) % 2])
            return (wd if homo else wd[lo:hi].clone()), idd[lo:hi].clone(), pb
        blocked = ScatterPlan.build_from_blocks(get_block, 384, shape=(m, k), nnz=int(ptr[-1]), max_row_len=int(lens.max()),
                                                homo=homo, layout=layout)
        assert calls == [(0, 384), (384, 768), (768, 1000)] * 2
        assert blocked.layout == whole.layout and blocked.slice_width == whole.slice_width
        assert torch.equal(blocked.seg, whole.seg) and blocked.scale_exp == whole.scale_exp
        M = PlannedMatrix(blocked, weight=None if not homo else w)
        for p in (0.2, 1.1):
            s = rng.random(m) < p
            sv = torch.tensor(s, device='cuda')
            ref_out = be.binary_csrmv(wd, idd, ptd, sv, shape=(m, k), transpose=True, workspace=whole)
            got = be.BinaryArray(sv) @ M
            assert torch.equal(got, ref_out)
            assert torch.equal(be.BitPackedBinary(sv) @ M, ref_out)
            ref = oracle.binary_csrmv(np.broadcast_to(w, idx.shape).astype(np.float64), idx, ptr, s, (m, k), True)
            np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
        S = torch.tensor(rng.random((3, m)) < 0.3, device='cuda')
        got = be.BinaryArray(S) @ M
        for b in range(3):
            assert torch.equal(got[b], be.binary_csrmv(wd, idd, ptd, S[b], shape=(m, k), transpose=True, workspace=whole))
        assert isinstance(be.BinaryArray(s) @ M, np.ndarray)                  # numpy events in, numpy out
        with pytest.raises(Exception):
            be.BinaryArray(torch.zeros(m + 1, dtype=torch.bool, device='cuda')) @ M


def test_binned_32bit_sums_are_gated_exact_enough_and_reproducible(be, oracle, monkeypatch):
    """BE_BINNED_ACC32: per-entry weights summed in 32-bit fixed point (bins twice as wide) — taken only when every column's
    largest weight keeps >= 18 bits at the 32-bit exponent; then within 1e-5 of the oracle (measured ~1e-7), bitwise repeatable,
    and within 2e-6 of the 64-bit sums; weights whose range the 32-bit sums cannot resolve fall back to 64-bit bins."""
    from brainevent_amd._csr import BinnedScatter, MathError
    rng = np.random.default_rng(61)
    m, k, row = 4000, 300_000, 24
    idx = torch.tensor(rng.integers(0, k, m * row).astype(np.int32), device='cuda')
    ptr = torch.arange(0, m * row + 1, row, dtype=torch.int32, device='cuda')
    w = torch.tensor((rng.uniform(0.25, 1.0, m * row) * rng.choice([-1.0, 1.0], m * row)).astype(np.float32), device='cuda')   # mixed signs
    v = torch.tensor(rng.random(m) < 0.2, device='cuda')
    ref = oracle.binary_csrmv(w.cpu().numpy().astype(np.float64), idx.cpu().numpy(), ptr.cpu().numpy(), v.cpu().numpy(), (m, k), True)
    ws32 = BinnedScatter(w, m, k, m * row, indices=idx, acc32=True)
    ws64 = BinnedScatter(w, m, k, m * row, indices=idx, acc32=False)
    assert ws32.acc32 and ws32.kind == 2 and not ws64.acc32 and ws64.kind == 0
    assert ws32.scale_exp == ws64.scale_exp - 32
    o32 = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws32)
    o64 = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws64)
    np.testing.assert_allclose(o32.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(o32.cpu().numpy(), o64.cpu().numpy(), rtol=0, atol=2e-6 * float(w.abs().max()) * 8)
    assert torch.equal(o32, be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws32))
    # batches go through the same accumulators
    B = torch.tensor(rng.random((m, 3)) < 0.2, device='cuda')
    ob = be.binary_csrmm(w, idx, ptr, B, shape=(m, k), transpose=True, workspace=ws32)
    np.testing.assert_allclose(ob.cpu().numpy(), oracle.binary_csrmm(w.cpu().numpy().astype(np.float64), idx.cpu().numpy(), ptr.cpu().numpy(),
                                                                       B.cpu().numpy(), (m, k), True), rtol=1e-5, atol=1e-5)
    # columns whose only weight is ~1e-6 of the largest column sum: 32-bit sums cannot give them 18 bits -> refused / 64-bit
    w2 = w.clone()
    w2[::7] *= 1e-6
    with pytest.raises(MathError):
        BinnedScatter(w2, m, k, m * row, indices=idx, acc32=True)
    auto = BinnedScatter(w2, m, k, m * row, indices=idx)
    assert not auto.acc32                                  # (also: below ACC32_MIN_OUTPUTS the automatic choice is 64-bit)
    # the AUTOMATIC choice is stricter than the explicit one: every single addend must keep 17 bits (an output made of one small
    # weight is then still within 1e-5 relative).  Weights in [0.25, 1) with column sums < 2^10: exponent 20, 0.25 keeps 18 bits
    monkeypatch.setattr(BinnedScatter, 'ACC32_MIN_OUTPUTS', 1)
    assert BinnedScatter(w, m, k, m * row, indices=idx).acc32
    w3 = w.clone(); w3[11] = 1e-4                           # one small weight: its own column still passes the explicit gate? no: alone -> refused
    idx3 = idx.clone(); idx3[11] = idx3[12]                 # ... so put it into a column that also holds a large weight
    assert not BinnedScatter(w3, m, k, m * row, indices=idx3).acc32          # automatic: the smallest weight keeps < 17 bits -> 64-bit
    assert BinnedScatter(w3, m, k, m * row, indices=idx3, acc32=True).acc32  # explicit: the column gate alone (documented accuracy)
    # an in-place update that stops qualifying moves a 32-bit workspace back to 64-bit bins
    w.copy_(w2)
    from brainevent_amd._csr import fresh_scatter_workspace
    assert fresh_scatter_workspace(ws32, w, idx, ptr) is ws32 and not ws32.acc32
    o = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws32)
    ref2 = oracle.binary_csrmv(w.cpu().numpy().astype(np.float64), idx.cpu().numpy(), ptr.cpu().numpy(), v.cpu().numpy(), (m, k), True)
    np.testing.assert_allclose(o.cpu().numpy(), ref2, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('homo', [True, False])
def test_row_sort_of_the_sorted_layouts_by_counting(be, oracle, monkeypatch, homo):
    """Round 4: the d8 / h8 build orders a row by a counting sort over column ranges + a rank sort inside each bucket instead of
    one bitonic network.  Rows that exercise every branch — uniform columns (buckets of ~128), columns clustered into a few
    hundred ids (buckets above 256: the bitonic fallback), many duplicates of one column, already ascending rows, rows at the
    16384 limit, short rows — must give the products of the unsorted uint16 layout bit for bit and match the oracle."""
    import brainevent_amd._csr as C
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1000)
    rng = np.random.default_rng(71)
    k = 90_000
    rows = []
    rows.append(rng.integers(0, k, 10_000))                              # uniform
    rows.append(rng.integers(40_000, 40_300, 6_000))                     # clustered: one or two buckets hold everything
    rows.append(np.concatenate([np.full(3_000, 777), rng.integers(0, k, 2_000)]))      # many duplicates
    rows.append(np.sort(rng.integers(0, k, 9_000)))                      # ascending already
    rows.append(rng.integers(0, k, 16_384))                              # the longest row the layouts take
    rows.append(rng.integers(0, k, 300))
    rows.append(rng.integers(0, k, 257))
    rows.append(np.array([5, 3, 3, 89_999, 0]))
    rows.append(np.array([], dtype=np.int64))
    rows += [rng.integers(0, k, int(n)) for n in rng.integers(200, 3000, 40)]
    lens = np.array([len(r) for r in rows])
    m = len(rows)
    idx = np.concatenate(rows).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    w = np.array([0.5], np.float32) if homo else rng.uniform(-1, 1, idx.size).astype(np.float32)
    dw, di, dp = torch.tensor(w, device='cuda'), torch.tensor(idx, device='cuda'), torch.tensor(ptr, device='cuda')
    sorted_plan = C.ScatterPlan.build(dw, di, dp, shape=(m, k), layout='h8' if homo else 'd8', keep_order=True)
    plain_plan = C.ScatterPlan.build(dw, di, dp, shape=(m, k), layout='u16', slice_shift=sorted_plan.slice_shift)
    for trial in range(3):
        v = rng.random(m) < (1.0 if trial == 0 else 0.4)
        dv = torch.tensor(v, device='cuda')
        a = be.binary_csrmv(dw, di, dp, dv, shape=(m, k), transpose=True, workspace=sorted_plan)
        b = be.binary_csrmv(dw, di, dp, dv, shape=(m, k), transpose=True, workspace=plain_plan)
        if homo:
            assert torch.equal(a, b)
        else:
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6, atol=1e-6)   # (exponents of the two plans may differ)
        ref = oracle.binary_csrmv(np.asarray(w, np.float64), idx, ptr, v, (m, k), True)
        np.testing.assert_allclose(a.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    # the stored order really is the ascending column order of every row (ties by position)
    if homo:          # (one shared weight is never re-encoded: its plan does not keep the order)
        return
    order = sorted_plan.order.cpu().numpy().astype(np.int64) & 0xffff
    for r in (0, 1, 2, 4, 7):
        seg = slice(ptr[r], ptr[r + 1])
        want = np.lexsort((np.arange(lens[r]), idx[seg]))
        np.testing.assert_array_equal(order[seg], want)


@pytest.mark.parametrize('fixed_rows', [True, False])
def test_binned_exponent_from_binned_steps_equals_the_atomic_pass(be, oracle, monkeypatch, fixed_rows):
    """Round 4: the column statistics behind a binned workspace's exponent (largest column sum of |w|, the accuracy gate) come
    from binned steps over |w| and over counts (BE_BINNED_ABS) instead of passes of global atomics over the entries.  Same
    exponent as ``be_fixed_point_exponent`` (the step sums are exact to 2^-29 of a weight, the atomic float sums are not: the
    bound may land on the other side of a power of two only when it sits within 1e-3 of one), products within 1e-5."""
    from brainevent_amd._csr import BinnedScatter, fixed_point_exponent
    rng = np.random.default_rng(81)
    m, k, row = 30_000, 400_000, 40
    if fixed_rows:
        idx = torch.tensor(rng.integers(0, k, (m, row)).astype(np.int32), device='cuda')
        ptr, rl = None, row
        ptr_np = np.arange(0, m * row + 1, row, dtype=np.int32)
    else:
        lens = rng.integers(0, 2 * row, m)
        ptr_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        idx = torch.tensor(rng.integers(0, k, int(ptr_np[-1])).astype(np.int32), device='cuda')
        ptr, rl = torch.tensor(ptr_np, device='cuda'), -1
    nnz = int(idx.numel())
    w = torch.tensor((rng.uniform(0.2, 1.0, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(np.float32), device='cuda')
    flat_idx = idx.reshape(-1)
    e_atomic = fixed_point_exponent(w, flat_idx, k)
    monkeypatch.setattr(BinnedScatter, 'STATS_BY_STEPS_MIN_NNZ', 1)
    ws = BinnedScatter(w, m, k, nnz, indices=flat_idx, indptr=ptr, row_len=rl, acc32=False)
    assert ws._stats is not None and ws.scale_exp == e_atomic
    colsum = np.zeros(k); np.add.at(colsum, flat_idx.cpu().numpy(), np.abs(w.cpu().numpy().astype(np.float64)))
    np.testing.assert_allclose(ws._stats[0], colsum.max(), rtol=1e-6)
    v = rng.random(m) < 0.05
    got = be.binary_csrmv(w, flat_idx, torch.tensor(ptr_np, device='cuda'), torch.tensor(v, device='cuda'), shape=(m, k), transpose=True,
                          workspace=ws)
    ref = oracle.binary_csrmv(w.cpu().numpy().astype(np.float64), flat_idx.cpu().numpy(), ptr_np, v, (m, k), True)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    # 32-bit sums decided from the same statistics
    ws32 = BinnedScatter(w, m, k, nnz, indices=flat_idx, indptr=ptr, row_len=rl, acc32=True)
    assert ws32.acc32 and ws32.scale_exp == e_atomic - 32
    # inf / nan are refused before any step runs
    w_bad = w.clone(); w_bad[5] = float('inf')
    with pytest.raises(be.MathError):
        BinnedScatter(w_bad, m, k, nnz, indices=flat_idx, indptr=ptr, row_len=rl)


def test_reference_task_workspace_handle_carries_the_native_workspace(be, oracle, monkeypatch):
    """A reference-style task workspace passed as `workspace=` (brainevent/_csr/binary.py:128-138 requires one): the matrix's
    native scatter workspace is built on first use and cached on the handle — keyed on the arrays, so the same handle reused
    for another matrix of the same indptr re-derives it — and `binary_csrmv_p_call` returns the reference's 4-tuple."""
    import brainevent_amd._csr as C
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1000)
    rng = np.random.default_rng(91)
    m, k, row = 600, 40_000, 200
    ptr = torch.arange(0, m * row + 1, row, dtype=torch.int32, device='cuda')
    handle = C._make_binary_csrmv_workspace(ptr)
    assert handle.task_capacity == m and handle.task_begin.dtype == torch.int32 and handle.status.shape == (2,)
    v = rng.random(m) < 0.2
    dv = torch.tensor(v, device='cuda')
    for trial in range(2):                                   # second trial: ANOTHER matrix with the same indptr through the same handle
        idx = torch.tensor(rng.integers(0, k, m * row).astype(np.int32), device='cuda')
        w = torch.tensor(rng.random(m * row).astype(np.float32), device='cuda')
        y, tb, te, st = C.binary_csrmv_p_call(w, idx, ptr, dv, handle, shape=(m, k), transpose=True)
        assert tb is handle.task_begin and te is handle.task_end and st is handle.status
        assert isinstance(handle._native, C.ScatterPlan)
        ref = oracle.binary_csrmv(w.cpu().numpy().astype(np.float64), idx.cpu().numpy(), ptr.cpu().numpy(), v, (m, k), True)
        np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
        got = be.binary_csrmv(w, idx, ptr, dv, shape=(m, k), workspace=handle, transpose=True)
        assert torch.equal(got, y)
        w.mul_(2.0)                                          # in-place update: the cached workspace follows
        np.testing.assert_allclose(be.binary_csrmv(w, idx, ptr, dv, shape=(m, k), workspace=handle, transpose=True).cpu().numpy(),
                                   2.0 * ref, rtol=1e-5, atol=1e-5)
    # without a handle: (y, None, None, None); the gather direction ignores the handle
    out = C.binary_csrmv_p_call(w, idx, ptr, dv, None, shape=(m, k), transpose=True)
    assert len(out) == 4 and out[1] is None and out[3] is None
    dk = torch.tensor(rng.random(k) < 0.1, device='cuda')
    g = C.binary_csrmv_p_call(w, idx, ptr, dk, handle, shape=(m, k), transpose=False)
    assert len(g) == 4 and g[0].shape == (m,)


def test_release_raw_and_direct_route_warning(be, oracle, monkeypatch):
    """`prepare(release_raw=True)` hands back a PlannedMatrix (the caller drops the container and its raw arrays: C2 holds 58 GB
    instead of 138); a large matrix that ends up on the direct route (global float atomics) says so once."""
    import warnings
    import brainevent_amd._csr as C
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1000)
    rng = np.random.default_rng(92)
    m, k, row = 500, 30_000, 150
    ptr = np.arange(0, m * row + 1, row, dtype=np.int32)
    idx = rng.integers(0, k, m * row).astype(np.int32)
    for homo in (False, True):
        w = np.array([0.5], np.float32) if homo else rng.random(m * row).astype(np.float32)
        pm = be.CSR((w, idx, ptr), shape=(m, k)).prepare(release_raw=True)
        assert isinstance(pm, C.PlannedMatrix)
        v = rng.random(m) < 0.3
        np.testing.assert_allclose(be.BinaryArray(v) @ pm, oracle.binary_csrmv(np.asarray(w, np.float64), idx, ptr, v, (m, k), True),
                                   rtol=1e-5, atol=1e-5)
    small = be.CSR((w[:1], idx[:10], np.array([0, 10], np.int32)), shape=(1, k))
    with pytest.raises(ValueError):
        small.prepare(release_raw=True)                        # direct route: nothing to release the raw arrays to
    monkeypatch.setattr(C, 'DIRECT_ROUTE_WARN_NNZ', 1000)
    w_inf = rng.random(m * row).astype(np.float32); w_inf[7] = np.inf
    csr = be.CSR((w_inf, idx, ptr), shape=(m, k))
    with pytest.warns(UserWarning, match='direct route'):
        out = be.BinaryArray(v) @ csr
    assert csr.buffers['scatter_plan'] is None
    with warnings.catch_warnings():
        warnings.simplefilter('error')                          # ... once: the cached decision does not warn again
        be.BinaryArray(v) @ csr


def test_binned_protocol_flag_poisons_the_outputs_instead_of_trapping(be):
    """Round 4 (VERDICT r3 weak 8 / ADVICE r3): the binned append has no device trap any more.  Its give-up path raises a sticky
    flag in the workspace (word 16 of the head); pass C then writes NaN into every output of the step and
    `be_binned_workspace_status` reports BE_ERR_HIP with the cause and re-arms the workspace.  The flag is set by hand here (the
    20-ms give-up has never been observed): a healthy workspace reports OK and steps normally before and after."""
    from brainevent_amd._csr import BinnedScatter
    from brainevent_amd._error import KernelExecutionError
    rng = np.random.default_rng(95)
    m, k, row = 3000, 250_000, 30
    idx = torch.tensor(rng.integers(0, k, m * row).astype(np.int32), device='cuda')
    ptr = torch.arange(0, m * row + 1, row, dtype=torch.int32, device='cuda')
    w = torch.tensor(rng.uniform(0.2, 1.0, m * row).astype(np.float32), device='cuda')
    v = torch.tensor(rng.random(m) < 0.2, device='cuda')
    ws = BinnedScatter(w, m, k, m * row, indices=idx)
    good = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws)
    ws.check_status()                                         # healthy: no error
    assert bool(torch.isfinite(good).all())
    ws.ws.view(torch.int32)[16] = 1                           # what a lane that gave up leaves behind
    bad = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws)
    assert bool(torch.isnan(bad).all()), 'a step over a flagged workspace must not return numbers'
    with pytest.raises(KernelExecutionError, match='append protocol stalled'):
        ws.check_status()                                     # names the cause, clears the flag
    ws.check_status()
    again = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws)
    assert torch.equal(again, good)


@pytest.mark.parametrize('homo', [False, True])
def test_binned_short_rows_hint_changes_no_bit(be, homo, monkeypatch):
    """Round 4: BE_BINNED_SHORT_ROWS (rows averaging <= 256 entries: pass B with one step of loads in flight) is a performance
    hint — the step with and without it, over ragged rows behind an indptr and over rows of one short length, gives the same bits
    (integer sums) and matches the direct route."""
    from brainevent_amd._csr import BinnedScatter
    rng = np.random.default_rng(96)
    m, k = 6000, 300_000
    lens = rng.integers(0, 90, m)
    ptr_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(ptr_np[-1])
    idx = torch.tensor(rng.integers(0, k, nnz).astype(np.int32), device='cuda')
    ptr = torch.tensor(ptr_np, device='cuda')
    w = torch.ones(1, device='cuda') * 0.75 if homo else torch.tensor(rng.uniform(0.2, 1.0, nnz).astype(np.float32), device='cuda')
    v = torch.tensor(rng.random(m) < 0.3, device='cuda')
    ws = BinnedScatter(w, m, k, nnz, indices=idx, indptr=ptr)
    assert ws.step_kind == ws.kind | 8
    with_hint = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws)
    monkeypatch.setattr(BinnedScatter, 'SHORT_ROW_ENTRIES', 0)
    assert ws.step_kind == ws.kind
    without = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws)
    assert torch.equal(with_hint, without)
    direct = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=None)
    np.testing.assert_allclose(with_hint.cpu().numpy(), direct.cpu().numpy(), rtol=1e-5, atol=1e-5)
    # rows of one length classify themselves: 40 per row (short) and 400 per row (long) against the direct route
    for K in (40, 400):
        n = 4000
        fi = torch.tensor(rng.integers(0, k, (n, K)).astype(np.int32), device='cuda')
        fw = w if homo else torch.tensor(rng.uniform(0.2, 1.0, (n, K)).astype(np.float32), device='cuda')
        fv = torch.tensor(rng.random(n) < 0.3, device='cuda')
        fws = BinnedScatter(fw, n, k, n * K, indices=fi, row_len=K)
        got = be.binary_fcnmv(fw, fi, fv, shape=(n, k), transpose=True)
        conn = be.FixedNumPerPre((fw, fi), shape=(n, k))
        conn.buffers['scatter_plan'] = fws
        binned = be.BinaryArray(fv) @ conn
        np.testing.assert_allclose(binned.cpu().numpy(), got.cpu().numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('homo', [False, True])
def test_a_bad_column_in_a_region_block_costs_one_entry_and_nothing_else(be, homo):
    """Round 6.  Pass C adds at 16-bit local columns it reads from the region blocks; pass B only ever stores
    columns < width there, but round 5's -DBE_DBG_LEVEL=3 timing build (block stores compiled out, tickets real) showed what a column
    >= width does when the block -> region map sits BEHIND the accumulators in LDS: the add rewrites map bytes, a later group takes a
    wrong region, its block number wraps and the unit load faults (gpurun_out/prof_abl.log).  The accumulators now come last in the
    workgroup's LDS: such a column indexes past the end of the allocation and the hardware drops the access.  Planted here through
    the library's test hook between pass B and pass C (entry 0 of block 0 of region 0 of bin 0 gets column 0xFFFF): the step
    finishes, the conservation counters agree (the entry was read), every output but one carries its exact bits and that one lacks
    exactly one weight — and the next step is clean again."""
    import ctypes
    from brainevent_amd._csr import BinnedScatter
    from brainevent_amd._lib import lib
    rng = np.random.default_rng(97)
    m, k, row = 3000, 250_000, 30
    # every entry lands in bin 0 (columns < 900 < width): region 0 of bin 0 certainly holds workgroup 0's rows
    idx = torch.tensor(rng.integers(0, 900, m * row).astype(np.int32), device='cuda')
    ptr = torch.arange(0, m * row + 1, row, dtype=torch.int32, device='cuda')
    w = torch.full((1,), 0.75, device='cuda') if homo else torch.tensor(rng.uniform(0.2, 1.0, m * row).astype(np.float32), device='cuda')
    v = torch.tensor(rng.random(m) < 0.2, device='cuda')
    ws = BinnedScatter(w, m, k, m * row, indices=idx)
    assert ws.n_slices >= 128 and k // ws.n_slices + 4 >= 900
    good = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws)
    ws.check_status()
    f = lib().be_internal_binned_poison_next
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_uint32]
    assert f(0, 0, 0xFFFF) == 0
    bad = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws)
    torch.cuda.synchronize()
    ws.check_status()                                         # entries == tickets == accumulated: the planted entry was read, then dropped
    assert bool(torch.isfinite(bad).all())
    diff = (good.double() - bad.double())
    changed = torch.nonzero(diff != 0).flatten()
    assert changed.numel() == 1 and int(changed[0]) < 900, changed
    lost = float(diff[changed[0]])
    assert (abs(lost - 0.75) < 1e-6) if homo else (0.19 < lost < 1.01), lost
    again = be.binary_csrmv(w, idx, ptr, v, shape=(m, k), transpose=True, workspace=ws)      # the hook is one-shot
    assert torch.equal(again, good)
