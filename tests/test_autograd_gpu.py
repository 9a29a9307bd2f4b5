"""torch.autograd through the event-driven products on the device: weight gradients bit-exact against the host model of
tests/test_autograd_cpu.py, spike and shared-weight gradients against an f64 dense reference, the forward pass unchanged,
routes, determinism, training and graph capture.
The sizes past one pass of every loop of the kernels are in tests/test_update_kernels_at_scale_gpu.py."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _csr as C
from test_autograd_cpu import active, model_dense_dw, model_rows_dw, model_rows_homo, random_csr

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
BATCHES = [None, 1, 3, 32, 33, 64, 100]          # None: mv


def dev():
    return torch.device('cuda')


def weights(rng, n, dtype, homo):
    w = torch.tensor(rng.standard_normal(1 if homo else n), dtype=torch.float64).to(dtype).to(dev())
    return w.requires_grad_()


def spikes_bm(rng, nb, n, p=0.3):
    return rng.random((1 if nb is None else nb, n)) < p


def grad_like(rng, shape, dtype):
    return torch.tensor(rng.standard_normal(shape), dtype=torch.float64).to(dtype).to(dev())


def as_bm(t: torch.Tensor, nb) -> np.ndarray:
    """g / spikes of the functional layout ([n] or [n, nb]) as batch-major float64 numpy."""
    a = t.detach().double().cpu().numpy() if t.dtype != torch.bool else t.cpu().numpy()
    return a.reshape(1, -1) if nb is None else a.T


def check_rows_dw(w, indices, rows, transpose, act, g_bm, homo):
    if homo:
        want = model_rows_homo(indices, rows, transpose, act, g_bm)
        tol = 1e-2 if w.dtype in (torch.float16, torch.bfloat16) else 1e-5
        assert float(w.grad.double().reshape(())) == pytest.approx(want, rel=tol, abs=tol * max(1.0, abs(want)))
    else:
        want = model_rows_dw(indices, rows, transpose, act, g_bm, w.dtype)
        assert torch.equal(w.grad.cpu(), want), (w.grad.cpu()[:8], want[:8])


# ------------------------------------------------------------------------------------------------ functional CSR matrix
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nb', BATCHES)
@pytest.mark.parametrize('transpose', [True, False])
@pytest.mark.parametrize('homo', [False, True])
def test_csr_functional_weight_grad(dtype, nb, transpose, homo):
    rng = np.random.default_rng([DTYPES.index(dtype), BATCHES.index(nb), int(transpose), int(homo)])
    m, k = 67, 93
    indices, indptr, rows = random_csr(rng, m, k, 0.2)
    w = weights(rng, indices.size, dtype, homo)
    n_spk = m if transpose else k
    s = spikes_bm(rng, nb, n_spk)
    idx, ptr = torch.tensor(indices, device=dev()), torch.tensor(indptr.astype(np.int32), device=dev())
    if nb is None:
        y = be.binary_csrmv(w, idx, ptr, torch.tensor(s[0], device=dev()), shape=(m, k), transpose=transpose)
    else:
        y = be.binary_csrmm(w, idx, ptr, torch.tensor(s.T.copy(), device=dev()), shape=(m, k), transpose=transpose)
    g = grad_like(rng, tuple(y.shape), dtype)
    y.backward(g)
    check_rows_dw(w, indices, rows, transpose, s, as_bm(g, nb), homo)


# ------------------------------------------------------------------------------------------------ spike encodings (containers)
def encodings(s: np.ndarray):
    t = torch.tensor(s, device=dev())
    yield 'bool', be.BinaryArray(t)
    yield 'uint8', be.BinaryArray(t.to(torch.uint8))
    yield 'float', be.BinaryArray(t.float())
    if s.ndim == 1:
        yield 'bitpacked', be.BitPackedBinary(t)
        yield 'compact', be.CompactBinary.from_array(t)


def containers(rng, m, k, dtype=torch.float32, homo=False):
    """(name, container, CSR-reading indices / rows of the stored arrays, stored shape, s @ M is the CSR-reading transpose)."""
    indices, indptr, rows = random_csr(rng, m, k, 0.15)
    w = weights(rng, indices.size, dtype, homo)
    yield 'CSR', be.CSR((w, torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())), shape=(m, k)), indices, rows, True
    yield 'CSC', be.CSC((w, torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())), shape=(k, m)), indices, rows, False
    nc = 5
    fidx = rng.integers(0, k, (m, nc)).astype(np.int32)
    fw = weights(rng, m * nc, dtype, homo)
    fw = fw if homo else fw.detach().reshape(m, nc).requires_grad_()
    frows = np.repeat(np.arange(m), nc)
    yield 'FixedNumPerPre', be.FixedNumPerPre((fw, torch.tensor(fidx, device=dev())), shape=(m, k)), fidx, frows, True
    yield 'FixedNumPerPost', be.FixedNumPerPost((fw, torch.tensor(fidx, device=dev())), shape=(k, m)), fidx, frows, False


@pytest.mark.parametrize('left', [True, False])
@pytest.mark.parametrize('batched', [False, True])
def test_container_weight_grad_all_encodings(left, batched):
    rng = np.random.default_rng(11 + left + 2 * batched)
    m, k = 70, 130
    for name, M, indices, rows, t_left in containers(rng, m, k):
        t = t_left if left else not t_left
        n_spk = M.shape[0] if left else M.shape[1]
        s = spikes_bm(rng, 3 if batched else None, n_spk)[:, :]
        s_in = s if batched else s[0]
        s_in = s_in if (left or not batched) else s.T.copy()
        for enc, ev in encodings(s_in):
            M.data.grad = None
            y = ev @ M if left else M @ ev
            g = grad_like(rng, tuple(y.shape), torch.float32)
            y.backward(g)
            g_np = g.double().cpu().numpy()
            g_bm = g_np.reshape(1, -1) if not batched else (g_np if left else g_np.T)
            want = model_rows_dw(indices, rows, t, s, g_bm, torch.float32).reshape(M.data.shape)
            assert torch.equal(M.data.grad.cpu(), want), (name, enc, left, batched)


@pytest.mark.parametrize('homo', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_container_dtypes(dtype, homo):
    rng = np.random.default_rng(5)
    m, k = 45, 77
    for name, M, indices, rows, t_left in containers(rng, m, k, dtype, homo):
        for left in (True, False):
            M.data.grad = None
            n_spk = M.shape[0] if left else M.shape[1]
            s = spikes_bm(rng, None, n_spk)
            ev = be.BinaryArray(torch.tensor(s[0], device=dev()))
            y = ev @ M if left else M @ ev
            g = grad_like(rng, tuple(y.shape), dtype)
            y.backward(g)
            t = t_left if left else not t_left
            if homo:
                want = model_rows_homo(indices, rows, t, s, g.double().cpu().numpy().reshape(1, -1))
                tol = 2e-2 if dtype in (torch.float16, torch.bfloat16) else 1e-5
                assert float(M.data.grad.double().reshape(-1)[0]) == pytest.approx(want, rel=tol, abs=tol), (name, left)
            else:
                want = model_rows_dw(indices, rows, t, s, g.double().cpu().numpy().reshape(1, -1), dtype).reshape(M.data.shape)
                assert torch.equal(M.data.grad.cpu(), want), (name, left)


# ------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nb', BATCHES)
@pytest.mark.parametrize('transpose', [True, False])
def test_dense_weight_grad(dtype, nb, transpose):
    rng = np.random.default_rng(17)
    R, Cn = 70, 150
    W = torch.tensor(rng.standard_normal((R, Cn))).to(dtype).to(dev()).requires_grad_()
    s = spikes_bm(rng, nb, R if transpose else Cn)
    if nb is None:
        y = be.binary_densemv(W, torch.tensor(s[0], device=dev()), transpose=transpose)
    else:
        y = be.binary_densemm(W, torch.tensor(s.T.copy(), device=dev()), transpose=transpose)
    g = grad_like(rng, tuple(y.shape), dtype)
    y.backward(g)
    want = model_dense_dw(transpose, s, as_bm(g, nb), dtype)
    assert torch.equal(W.grad.cpu(), want)


def test_dense_container_and_binary_array_tensor():
    rng = np.random.default_rng(19)
    W = torch.tensor(rng.standard_normal((40, 60)), dtype=torch.float32, device=dev(), requires_grad=True)
    D = be.Dense(W)
    s = spikes_bm(rng, 5, 40)
    for y in (be.BinaryArray(torch.tensor(s, device=dev())) @ D, be.BinaryArray(torch.tensor(s, device=dev())) @ W):
        W.grad = None
        g = grad_like(rng, tuple(y.shape), torch.float32)
        y.backward(g)
        assert torch.equal(W.grad.cpu(), model_dense_dw(True, s, g.double().cpu().numpy(), torch.float32))
    s2 = spikes_bm(rng, None, 60)
    W.grad = None
    y = D @ be.BinaryArray(torch.tensor(s2[0], device=dev()))
    g = grad_like(rng, tuple(y.shape), torch.float32)
    y.backward(g)
    assert torch.equal(W.grad.cpu(), model_dense_dw(False, s2, g.double().cpu().numpy().reshape(1, -1), torch.float32))


# ------------------------------------------------------------------------------------------------ spike gradients
def dense_of(name, M, indices, rows) -> torch.Tensor:
    """The container as a dense f64 matrix of its own shape (from the CSR reading of its arrays)."""
    w = M.data.detach().double().cpu().numpy()
    if name == 'Dense':
        return torch.from_numpy(w)
    S = np.zeros(M.shape if name in ('CSR', 'FixedNumPerPre') else M.shape[::-1])
    np.add.at(S, (rows, np.asarray(indices).reshape(-1)), np.broadcast_to(w.reshape(-1), rows.shape) if w.size == 1 else w.reshape(-1))
    return torch.from_numpy(S if name in ('CSR', 'FixedNumPerPre') else S.T)


@pytest.mark.parametrize('left', [True, False])
@pytest.mark.parametrize('nb', [None, 3])
@pytest.mark.parametrize('sdtype', [torch.float32, torch.float64])
def test_spike_grad_straight_through(left, nb, sdtype):
    rng = np.random.default_rng(23)
    m, k = 50, 80
    items = list(containers(rng, m, k))
    items.append(('Dense', be.Dense(torch.tensor(rng.standard_normal((m, k)), dtype=torch.float32, device=dev(),
                                                 requires_grad=True)), None, None, None))
    for name, M, indices, rows, _ in items:
        n_spk = M.shape[0] if left else M.shape[1]
        shape = (n_spk,) if nb is None else ((nb, n_spk) if left else (n_spk, nb))
        s = torch.tensor(rng.random(shape) < 0.3, dtype=sdtype, device=dev()).requires_grad_()
        y = be.BinaryArray(s) @ M if left else M @ be.BinaryArray(s)
        g = grad_like(rng, tuple(y.shape), torch.float32)
        y.backward(g)
        Md = dense_of(name, M, indices, rows)
        g64 = g.double().cpu()
        want = (g64 @ Md.T) if left else (Md.T @ g64)
        assert s.grad.dtype == sdtype and s.grad.shape == s.shape
        np.testing.assert_allclose(s.grad.double().cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-4, err_msg=name)


def test_functional_spike_grad_and_non_binary_values():
    """Float spikes of other values: the spike gradient is straight-through, the weight gradient uses the activity."""
    rng = np.random.default_rng(29)
    m, k = 30, 40
    indices, indptr, rows = random_csr(rng, m, k, 0.3)
    w = weights(rng, indices.size, torch.float32, False)
    sv = torch.tensor(rng.standard_normal(m), dtype=torch.float32, device=dev()).requires_grad_()
    idx, ptr = torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())
    y = be.binary_csrmv(w, idx, ptr, sv, shape=(m, k), transpose=True)
    g = grad_like(rng, (k,), torch.float32)
    y.backward(g)
    s_np = sv.detach().cpu().numpy().reshape(1, -1)
    assert torch.equal(w.grad.cpu(), model_rows_dw(indices, rows, True, active(s_np), g.double().cpu().numpy().reshape(1, -1),
                                                   torch.float32))
    dense = np.zeros((m, k))
    np.add.at(dense, (rows, indices), w.detach().double().cpu().numpy())
    np.testing.assert_allclose(sv.grad.double().cpu().numpy(), dense @ g.double().cpu().numpy(), rtol=1e-4, atol=1e-4)


def test_gradcheck_f64_weights():
    rng = np.random.default_rng(31)
    m, k = 8, 11
    indices, indptr, rows = random_csr(rng, m, k, 0.4)
    idx, ptr = torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())
    for transpose in (True, False):
        s = torch.tensor(rng.random((m if transpose else k, 3)) < 0.5, device=dev())
        w = weights(rng, indices.size, torch.float64, False)
        assert torch.autograd.gradcheck(lambda w_: be.binary_csrmm(w_, idx, ptr, s, shape=(m, k), transpose=transpose), (w,))
        W = torch.tensor(rng.standard_normal((m, k)), dtype=torch.float64, device=dev(), requires_grad=True)
        sd = torch.tensor(rng.random(m if transpose else k) < 0.5, device=dev())
        assert torch.autograd.gradcheck(lambda W_: be.binary_densemv(W_, sd, transpose=transpose), (W,))


# ------------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize('transpose', [True, False])
def test_no_active_spike_gives_zero_gradients(transpose):
    rng = np.random.default_rng(37)
    m, k = 130, 70
    indices, indptr, rows = random_csr(rng, m, k, 0.3)
    idx, ptr = torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())
    for homo in (False, True):
        w = weights(rng, indices.size, torch.float32, homo)
        for nb in (None, 33):
            n = m if transpose else k
            s = torch.zeros(n if nb is None else (n, nb), dtype=torch.bool, device=dev())
            f = be.binary_csrmv if nb is None else be.binary_csrmm
            y = f(w, idx, ptr, s, shape=(m, k), transpose=transpose)
            w.grad = None
            y.backward(torch.ones_like(y))
            assert torch.count_nonzero(w.grad).item() == 0 and not torch.isnan(w.grad).any()
    W = torch.ones((m, k), device=dev(), requires_grad=True)
    y = be.binary_densemm(W, torch.zeros((m if transpose else k, 5), dtype=torch.bool, device=dev()), transpose=transpose)
    y.backward(torch.ones_like(y))
    assert torch.count_nonzero(W.grad).item() == 0 and not torch.isnan(W.grad).any()


@pytest.mark.parametrize('transpose', [True, False])
def test_edge_structures(transpose):
    rng = np.random.default_rng(41)
    m, k = 97, 65            # not multiples of 64
    indices, indptr, rows = random_csr(rng, m, k, 0.1)
    keep = (rows < 10) | (rows >= 19)
    # rebuild consistently: drop the entries of rows 10..18, duplicate a column in row 0
    rows = rows[keep]
    indices = indices[keep]
    rows = np.concatenate([[0, 0], rows])
    indices = np.concatenate([[3, 3], indices]).astype(np.int32)
    order = np.argsort(rows, kind='stable')
    rows, indices = rows[order], indices[order]
    indptr = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=indptr[1:])
    for ptr_dtype in (torch.int32, torch.int64):
        w = weights(rng, indices.size, torch.float32, False)
        s = spikes_bm(rng, 3, m if transpose else k, 0.5)
        y = be.binary_csrmm(w, torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev(), dtype=ptr_dtype),
                            torch.tensor(s.T.copy(), device=dev()), shape=(m, k), transpose=transpose)
        g = grad_like(rng, tuple(y.shape), torch.float32)
        y.backward(g)
        assert torch.equal(w.grad.cpu(), model_rows_dw(indices, rows, transpose, s, g.double().cpu().numpy().T, torch.float32))
    # nse == 0
    for homo in (False, True):
        w = torch.ones(1 if homo else 0, device=dev(), requires_grad=True)
        y = be.binary_csrmv(w, torch.zeros(0, dtype=torch.int32, device=dev()), torch.zeros(m + 1, dtype=torch.int32, device=dev()),
                            torch.ones(m if transpose else k, dtype=torch.bool, device=dev()), shape=(m, k), transpose=transpose)
        y.sum().backward()
        assert w.grad.shape == w.shape and torch.count_nonzero(w.grad).item() == 0


# ------------------------------------------------------------------------------------------------ forward unchanged, routes
def test_forward_bit_identical_with_and_without_grad(monkeypatch):
    """The Function's forward pass is the existing path.  Routes that accumulate in a fixed order (gathers, the plan's integer
    sums, dense) must agree bit for bit; the direct scatter adds with float atomics, whose order is not fixed even between two
    runs without grad, so there the check is a tolerance."""
    rng = np.random.default_rng(43)
    for name, M, *_ in containers(rng, 60, 90):
        for left in (True, False):
            s = torch.tensor(spikes_bm(rng, None, M.shape[0] if left else M.shape[1])[0], device=dev())
            ev = be.BinaryArray(s)
            y1 = ev @ M if left else M @ ev
            with torch.no_grad():
                y0 = ev @ M if left else M @ ev
            assert y1.grad_fn is not None and y0.grad_fn is None
            scatter = left == (name in ('CSR', 'FixedNumPerPre'))
            if scatter:
                torch.testing.assert_close(y0, y1.detach(), rtol=1e-6, atol=1e-6)
            else:
                assert torch.equal(y0, y1.detach()), name
    m, k, nc = 600, 5000, 80
    ti = torch.tensor(rng.integers(0, k, m * nc).astype(np.int32), device=dev())
    tp = torch.tensor((np.arange(m + 1) * nc).astype(np.int32), device=dev())
    w = torch.tensor(rng.random(m * nc), dtype=torch.float32, device=dev())
    plan = C.ScatterPlan.build(w, ti, tp, shape=(m, k))
    s = torch.tensor(rng.random((m, 3)) < 0.1, device=dev())
    y0 = be.binary_csrmm(w, ti, tp, s, shape=(m, k), transpose=True, workspace=plan)
    y1 = be.binary_csrmm(w.clone().requires_grad_(), ti, tp, s, shape=(m, k), transpose=True, workspace=plan)
    assert y1.grad_fn is not None and torch.equal(y0, y1.detach())
    W = torch.tensor(rng.standard_normal((70, 90)), dtype=torch.float32, device=dev())
    sd = torch.tensor(rng.random((70, 5)) < 0.3, device=dev())
    y0 = be.binary_densemm(W, sd, transpose=True)
    y1 = be.binary_densemm(W.clone().requires_grad_(), sd, transpose=True)
    assert y1.grad_fn is not None and torch.equal(y0, y1.detach())


def test_gradient_independent_of_route(monkeypatch):
    rng = np.random.default_rng(47)
    m, k, nc = 600, 5000, 80
    idx = rng.integers(0, k, m * nc).astype(np.int32)
    ptr = (np.arange(m + 1) * nc).astype(np.int32)
    w0 = torch.tensor(rng.random(m * nc), dtype=torch.float32, device=dev())
    s = torch.tensor(rng.random(m) < 0.1, device=dev())
    g = grad_like(rng, (k,), torch.float32)
    ti, tp = torch.tensor(idx, device=dev()), torch.tensor(ptr, device=dev())
    grads = []
    for route in ('direct', 'plan', 'binned'):
        w = w0.clone().requires_grad_()
        ws = {'direct': None, 'plan': C.ScatterPlan.build(w0, ti, tp, shape=(m, k)),
              'binned': C.BinnedScatter(w0, m, k, m * nc, indices=ti, indptr=tp)}[route]
        y = be.binary_csrmv(w, ti, tp, s, shape=(m, k), transpose=True, workspace=ws)
        y.backward(g)
        grads.append(w.grad)
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1)
    w = w0.clone().requires_grad_()
    csr = be.CSR((w, ti, tp), shape=(m, k))
    (be.BinaryArray(s) @ csr).backward(g)
    grads.append(w.grad)
    for g2 in grads[1:]:
        assert torch.equal(grads[0], g2)
    # gather direction: streaming kernel vs mirror
    s2 = torch.tensor(rng.random(k) < 0.1, device=dev())
    g2 = grad_like(rng, (m,), torch.float32)
    out = []
    for mirror in (False, True):
        w = w0.clone().requires_grad_()
        csr = be.CSR((w, ti, tp), shape=(m, k))
        if mirror:
            csr.build_mirror()
        else:
            csr.buffers['mirror'] = None
        (csr @ be.BinaryArray(s2)).backward(g2)
        out.append(w.grad)
    assert torch.equal(out[0], out[1])


def test_deterministic_backward():
    rng = np.random.default_rng(53)
    m, k = 3000, 2000
    indices, indptr, rows = random_csr(rng, m, k, 0.02)
    idx, ptr = torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())
    s = torch.tensor(rng.random((m, 32)) < 0.2, device=dev())
    for homo in (False, True):
        w = weights(rng, indices.size, torch.float32, homo)
        g = grad_like(rng, (k, 32), torch.float32)
        res = []
        for _ in range(2):
            w.grad = None
            be.binary_csrmm(w, idx, ptr, s, shape=(m, k), transpose=True).backward(g)
            res.append(w.grad.clone())
        assert torch.equal(res[0], res[1])


def test_planned_matrix_refuses_gradients(monkeypatch):
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1)
    rng = np.random.default_rng(59)
    m, k, nc = 300, 4000, 60
    idx = torch.tensor(rng.integers(0, k, m * nc).astype(np.int32), device=dev())
    ptr = torch.tensor((np.arange(m + 1) * nc).astype(np.int32), device=dev())
    w = torch.rand(m * nc, device=dev())
    pm = be.CSR((w, idx, ptr), shape=(m, k)).prepare(release_raw=True)
    s = torch.rand(m, device=dev()).requires_grad_()
    with pytest.raises(be.UnsupportedOperationError):
        be.BinaryArray(s) @ pm
    with torch.no_grad():
        be.BinaryArray(s) @ pm


# ------------------------------------------------------------------------------------------------ training and capture
def test_sgd_follows_dense_model():
    """Three SGD steps through a CSR container track a dense torch model: the in-place updates reach the next forward pass
    (the cached plan refreshes on the version counter)."""
    rng = np.random.default_rng(61)
    m, k = 200, 150
    indices, indptr, rows = random_csr(rng, m, k, 0.3)
    w0 = rng.standard_normal(indices.size)
    w = torch.tensor(w0, dtype=torch.float64, device=dev(), requires_grad=True)
    csr = be.CSR((w, torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())), shape=(m, k))
    assert csr.data is w
    wd = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    ri, ci = torch.from_numpy(rows), torch.from_numpy(indices.astype(np.int64))
    opt, optd = torch.optim.SGD([w], lr=0.1), torch.optim.SGD([wd], lr=0.1)
    target = torch.tensor(rng.standard_normal((4, k)))
    for step in range(3):
        s = rng.random((4, m)) < 0.3
        y = be.BinaryArray(torch.tensor(s, device=dev())) @ csr
        dense = torch.zeros(m, k, dtype=torch.float64).index_put((ri, ci), wd)
        yd = torch.tensor(s, dtype=torch.float64) @ dense
        np.testing.assert_allclose(y.detach().cpu().numpy(), yd.detach().numpy(), rtol=1e-10, atol=1e-10)
        for o, out in ((opt, y.cpu()), (optd, yd)):
            o.zero_grad()
            ((out - target) ** 2).sum().backward()
            o.step()
    np.testing.assert_allclose(w.detach().cpu().numpy(), wd.detach().numpy(), rtol=1e-10, atol=1e-10)


def test_capture_forward_and_backward():
    """A training step (forward through a CSR gather and a Dense readout, then torch.autograd.grad) captured with
    capture_step replays to the eager gradients."""
    rng = np.random.default_rng(67)
    m, k = 400, 300
    indices, indptr, rows = random_csr(rng, m, k, 0.05)
    w = torch.tensor(rng.standard_normal(indices.size), dtype=torch.float32, device=dev(), requires_grad=True)
    csr = be.CSR((w, torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())), shape=(m, k))
    csr.buffers['mirror'] = None            # the streaming gather (no automatic mirror)
    W = torch.tensor(rng.standard_normal((m, 10)), dtype=torch.float32, device=dev(), requires_grad=True)
    D = be.Dense(W)
    s = torch.zeros((k, 8), device=dev())

    def step():
        h = csr @ be.BinaryArray(s)                       # [m, 8]
        out = be.BinaryArray(h.T) @ D                     # [8, 10]
        return torch.autograd.grad((out ** 2).sum(), (w, W))

    s.copy_(torch.tensor(rng.random((k, 8)) < 0.2, dtype=torch.float32))
    graphed = be.capture_step(step)
    for _ in range(2):
        s.copy_(torch.tensor(rng.random((k, 8)) < 0.2, dtype=torch.float32))
        got = [t.clone() for t in graphed()]
        want = step()
        for a, b in zip(got, want):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
            assert torch.count_nonzero(a).item() > 0
