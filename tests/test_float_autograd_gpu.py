"""torch.autograd through the float-operand products (csr @ x with a plain array; brainevent_amd/_autograd.py:
FloatRowsProduct) and the sampled dense-dense product under it (csrc/be_sddmm.hip, brainevent_amd/_sddmm.py).

Sizes come from CONSTS, the loop geometry of csrc/be_sddmm.hip (tests/test_float_autograd_cpu.py compares the table with the
source).  Which case crosses which bound:

  tile (entries per tile)            test_entry_count_around_a_tile, test_row_longer_than_a_tile, test_tile_of_empty_rows
  grid_cap (blocks)                  test_more_tiles_than_the_grid_cap (nb = 1: the grid-stride loop takes a second trip)
  vec_bytes, max_lanes (lanes/entry) test_nb_at_every_lane_boundary (V = vec_bytes / element size: 1 lane up to V elements, 2
                                     up to 2 V, 4, 8, max_lanes beyond 8 V; every threshold - 1, +0, + 1), test_error_bound
                                     (nb = 257: a lane takes more than one trip), test_unaligned_operand_view (element loads
                                     where 16-byte loads would be taken)
  threads                            groups in flight per block = threads / lanes: every case with more entries than that

Bit-for-bit cases use integer values in [-4, 4] and nb <= 64: every partial sum is then exact in f32, whatever the order, so the
one rounding to the weight dtype is all that is left.  The real-valued cases hold the kernel to the bound
|got - s| <= gamma * sum_b |P Q| + u_w |s|, gamma = nb u_acc / (1 - nb u_acc), which holds for any summation order."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _autograd as AG
from brainevent_amd import _sddmm as S
from test_float_autograd_cpu import model_sddmm

pytestmark = pytest.mark.gpu

#: the loop geometry of csrc/be_sddmm.hip
CONSTS = {'threads': 256, 'tile': 2048, 'grid_cap': 4096, 'vec_bytes': 16, 'max_lanes': 16}

DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
U_W = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def dev():
    return torch.device('cuda')


def vec_elems(dtype) -> int:
    return CONSTS['vec_bytes'] // torch.empty(0, dtype=dtype).element_size()


def lanes_for(nb: int, dtype) -> int:
    v = vec_elems(dtype)
    for lanes in (1, 2, 4, 8):
        if nb <= lanes * v:
            return lanes
    return CONSTS['max_lanes']


def nb_boundaries(dtype):
    """nb = 1 and every lanes-per-entry threshold (V, 2 V, 4 V, 8 V; V is the vector width too) - 1, + 0, + 1, up to 64."""
    v = vec_elems(dtype)
    return sorted({1} | {t + d for t in (v, 2 * v, 4 * v, 8 * v) for d in (-1, 0, 1) if 1 <= t + d <= 64})


# ------------------------------------------------------------------------------------------------ structures and operands
def structure(rng, row_lens, k):
    row_lens = np.asarray(row_lens, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(row_lens)])
    indices = rng.integers(0, k, int(indptr[-1])).astype(np.int32)
    rows = np.repeat(np.arange(len(row_lens)), row_lens)
    return indices, indptr, rows


def int_operands(rng, m, k, nb, dtype):
    P = torch.tensor(rng.integers(-4, 5, (m, nb)), dtype=dtype, device=dev())
    Q = torch.tensor(rng.integers(-4, 5, (k, nb)), dtype=dtype, device=dev())
    return P, Q


def real_operands(rng, m, k, nb, dtype, lo=0.5, hi=2.0):
    P = torch.tensor(rng.uniform(lo, hi, (m, nb)), dtype=dtype, device=dev())
    Q = torch.tensor(rng.uniform(lo, hi, (k, nb)), dtype=dtype, device=dev())
    return P, Q


def f64(t):
    return t.detach().double().cpu().numpy()


def run_ptr(indices, indptr, m, k, P, Q, ptr_dtype=torch.int32):
    return S.sddmm_rows(torch.tensor(indices, device=dev()), torch.tensor(indptr, dtype=ptr_dtype, device=dev()), -1, None, m, k, P, Q)


def check_exact(indices, indptr, rows, m, k, P, Q, **kw):
    got = run_ptr(indices, indptr, m, k, P, Q, **kw)
    want = model_sddmm(indices, rows, f64(P), f64(Q), P.dtype)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    return got


def dense_positions(M):
    """(row, column) in the matrix ``M`` stands for, of every stored entry in storage order."""
    r = M._stored_rows()
    idx = r.indices.reshape(-1).long().cpu()
    if r.indptr is None:
        rows = torch.arange(r.m).repeat_interleave(r.row_len)
    else:
        rows = torch.arange(r.m).repeat_interleave(torch.diff(r.indptr.long().cpu()))
    return (idx, rows) if M._stored_transposed else (rows, idx)


def make_container(kind, rng, shape, dtype=torch.float32, homo=False, integer=True):
    """A small matrix of ``shape`` in the given container, duplicates-free, with integer-valued (or real) weights that require
    grad.  The fixed-number containers hold 3 entries per stored row."""
    n0, n1 = shape
    stored_t = kind in ('csc', 'post')
    m, k = (n1, n0) if stored_t else (n0, n1)
    if kind in ('csr', 'csc'):
        lens = rng.integers(0, min(k, 6), m)
        lens[0] = 0
        lens[-1] = 0
    else:
        lens = np.full(m, 3)
    indices = np.concatenate([rng.permutation(k)[:n] for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nse = int(indptr[-1])
    vals = rng.integers(-3, 4, nse) if integer else rng.uniform(0.5, 2.0, nse)
    if kind in ('pre', 'post'):
        vals, idx = vals.reshape(m, 3), indices.reshape(m, 3)
    w = torch.tensor(2.0 if homo else vals, dtype=dtype, device=dev()).reshape(1 if homo else vals.shape).requires_grad_()
    if kind in ('csr', 'csc'):
        cls = be.CSR if kind == 'csr' else be.CSC
        return cls((w, torch.tensor(indices, device=dev()), torch.tensor(indptr, device=dev())), shape=shape)
    cls = be.FixedNumPerPre if kind == 'pre' else be.FixedNumPerPost
    return cls((w, torch.tensor(idx, device=dev())), shape=shape)


def dense_reference(M, x, left, g):
    """torch.autograd on the dense matrix: (gradient of the dense weights gathered at M's stored positions — summed for one
    shared weight —, gradient of x)."""
    pr, pc = dense_positions(M)
    w = M.data.detach().double().cpu().reshape(-1)
    Wd = torch.zeros(M.shape, dtype=torch.float64).index_put((pr, pc), w.expand(pr.numel()), accumulate=True).requires_grad_()
    xd = x.detach().double().cpu().requires_grad_()
    (xd @ Wd if left else Wd @ xd).backward(g.detach().double().cpu())
    dw = Wd.grad[pr, pc]
    return (dw.sum() if M.data.numel() == 1 else dw), xd.grad


KINDS = ['csr', 'csc', 'pre', 'post']


# ------------------------------------------------------------------------------------------------ 1. fails on the parent commit
@pytest.mark.parametrize('batched', [False, True])
@pytest.mark.parametrize('left', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_container_product_records_and_fills_the_weight_gradient(kind, left, batched):
    rng = np.random.default_rng(KINDS.index(kind) * 4 + left * 2 + batched)
    shape = (23, 31)
    M = make_container(kind, rng, shape)
    n_in = shape[0] if left else shape[1]
    n_out = shape[1] if left else shape[0]
    nb = 5
    xs = (n_in,) if not batched else ((nb, n_in) if left else (n_in, nb))
    gs = (n_out,) if not batched else ((nb, n_out) if left else (n_out, nb))
    x = torch.tensor(rng.integers(-4, 5, xs), dtype=torch.float32, device=dev(), requires_grad=True)
    g = torch.tensor(rng.integers(-4, 5, gs), dtype=torch.float32, device=dev())
    y = x @ M if left else M @ x
    assert y.grad_fn is not None and tuple(y.shape) == gs
    y.backward(g)
    assert M.data.grad is not None and M.data.grad.shape == M.data.shape and x.grad.shape == x.shape
    dw, dx = dense_reference(M, x, left, g)
    assert torch.equal(M.data.grad.double().cpu().reshape(-1), dw)
    assert torch.equal(x.grad.double().cpu(), dx)


@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('op', ['csrmv', 'csrmm', 'fcnmv', 'fcnmm'])
def test_functionals_record_and_fill_the_weight_gradient(op, transpose):
    rng = np.random.default_rng(len(op) + 7 * transpose)
    m, k, nb = 19, 27, 6
    M = make_container('csr' if op.startswith('csr') else 'pre', rng, (m, k))
    n_in = m if transpose else k
    x = torch.tensor(rng.integers(-4, 5, (n_in,) if op.endswith('mv') else (n_in, nb)), dtype=torch.float32, device=dev(),
                     requires_grad=True)
    if op.startswith('csr'):
        y = getattr(be, op)(M.data, M.indices, M.indptr, x, shape=(m, k), transpose=transpose)
    else:
        y = getattr(be, op)(M.data, M.indices, x, shape=(m, k), transpose=transpose)
    assert y.grad_fn is not None
    g = torch.tensor(rng.integers(-4, 5, tuple(y.shape)), dtype=torch.float32, device=dev())
    y.backward(g)
    pr, pc = dense_positions(M)
    Wd = torch.zeros((m, k), dtype=torch.float64).index_put((pr, pc), M.data.detach().double().cpu().reshape(-1)).requires_grad_()
    xd = x.detach().double().cpu().requires_grad_()
    ((Wd.T if transpose else Wd) @ xd).backward(g.double().cpu())
    assert torch.equal(M.data.grad.double().cpu().reshape(-1), Wd.grad[pr, pc])
    assert torch.equal(x.grad.double().cpu(), xd.grad)


def test_the_sampled_products_exist():
    assert callable(be.sddmm_coo_indices) and callable(be.sddmm_indices)
    rng = np.random.default_rng(0)
    assert callable(make_container('csr', rng, (5, 7)).sddmm)


# ------------------------------------------------------------------------------------------------ 2. untouched without grad
@pytest.mark.parametrize('left', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_no_node_and_the_same_bits_without_grad(kind, left):
    """The gather side runs on real values; the scatter side adds with float atomics, whose order is free, so it runs on
    integer values, where every order gives the same bits."""
    rng = np.random.default_rng(40 + KINDS.index(kind) + 4 * left)
    shape = (23, 31)
    scatter = (kind in ('csr', 'pre')) == left
    M = make_container(kind, rng, shape, integer=scatter)
    assert M._scatter_side(left) == scatter
    xv = rng.integers(-4, 5, (3, shape[0]) if left else (shape[1], 3)) if scatter else rng.standard_normal(
        (3, shape[0]) if left else (shape[1], 3))
    x = torch.tensor(xv, dtype=torch.float32, device=dev())
    with_grad = x @ M if left else M @ x
    assert with_grad.grad_fn is not None
    with torch.no_grad():
        without = x @ M if left else M @ x
    assert without.grad_fn is None and not without.requires_grad
    plain = M.with_data(M.data.detach())
    nothing = x @ plain if left else plain @ x
    assert nothing.grad_fn is None and not nothing.requires_grad
    assert torch.equal(with_grad.detach(), without) and torch.equal(without, nothing)


def test_numpy_operands_give_numpy_results_without_autograd():
    rng = np.random.default_rng(49)
    M = make_container('csr', rng, (23, 31))
    v = np.asarray(rng.standard_normal(31), np.float32)
    out = be.csrmv(M.data.detach().cpu().numpy(), M.indices.cpu().numpy(), M.indptr.cpu().numpy(), v, shape=(23, 31))
    assert isinstance(out, np.ndarray)
    y = M @ v                                   # weights that require grad, a numpy operand: taken by value, as before
    assert not (isinstance(y, torch.Tensor) and y.grad_fn is not None)


# ------------------------------------------------------------------------------------------------ 3. nb = 1 is exact
@pytest.mark.parametrize('dtype', DTYPES)
def test_nb_1_is_one_product_rounded_once(dtype):
    rng = np.random.default_rng(3)
    m, k = 300, 257
    indices, indptr, rows = structure(rng, rng.integers(0, 9, m), k)
    P = torch.tensor(rng.standard_normal((m, 1)), dtype=dtype, device=dev())
    Q = torch.tensor(rng.standard_normal((k, 1)), dtype=dtype, device=dev())
    check_exact(indices, indptr, rows, m, k, P, Q)


# ------------------------------------------------------------------------------------------------ 4. kernel boundaries
@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_entry_count_around_a_tile(delta):
    rng = np.random.default_rng(10 + delta)
    m, k, nb = 97, 211, 3
    nse = CONSTS['tile'] + delta
    lens = rng.multinomial(nse, np.ones(m) / m)
    indices, indptr, rows = structure(rng, lens, k)
    for dtype in (torch.float32, torch.bfloat16):
        P, Q = int_operands(rng, m, k, nb, dtype)
        check_exact(indices, indptr, rows, m, k, P, Q)


@pytest.mark.parametrize('dtype', DTYPES)
def test_row_longer_than_a_tile(dtype):
    rng = np.random.default_rng(21)
    k, nb = 301, vec_elems(dtype) + 1                   # (two lanes per entry)
    lens = [3, 0, CONSTS['tile'] + 5, 1, 0, 0, 2 * CONSTS['tile'] + 1, 7]
    indices, indptr, rows = structure(rng, lens, k)
    P, Q = int_operands(rng, len(lens), k, nb, dtype)
    check_exact(indices, indptr, rows, len(lens), k, P, Q)


@pytest.mark.parametrize('ptr_dtype', [torch.int32, torch.int64])
def test_tile_of_empty_rows(ptr_dtype):
    """More empty rows in a run than a tile holds entries, in the middle and at both ends; the walk steps over them."""
    rng = np.random.default_rng(22)
    t = CONSTS['tile']
    lens = np.concatenate([np.zeros(t + 3, int), rng.integers(1, 40, 150), np.zeros(t + 1, int), rng.integers(0, 3, 2500),
                           np.zeros(t, int)])
    m, k, nb = len(lens), 97, 2
    indices, indptr, rows = structure(rng, lens, k)
    P, Q = int_operands(rng, m, k, nb, torch.float32)
    check_exact(indices, indptr, rows, m, k, P, Q, ptr_dtype=ptr_dtype)


def test_empty_first_and_last_rows_and_empty_calls():
    rng = np.random.default_rng(23)
    lens = [0, 0, 5, 0, 9, 1, 0]
    indices, indptr, rows = structure(rng, lens, 13)
    P, Q = int_operands(rng, len(lens), 13, 4, torch.float16)
    check_exact(indices, indptr, rows, len(lens), 13, P, Q)
    # nse = 0, nb = 0, n_rows = 0: no launch
    none = S.sddmm_rows(torch.zeros(0, dtype=torch.int32, device=dev()), torch.zeros(8, dtype=torch.int32, device=dev()), -1, None,
                        7, 13, P, Q)
    assert none.shape == (0,)
    zero = run_ptr(indices, indptr, len(lens), 13, P[:, :0], Q[:, :0])
    assert zero.shape == (15,) and torch.count_nonzero(zero).item() == 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_nb_at_every_lane_boundary(dtype):
    rng = np.random.default_rng(24)
    m, k = 61, 89
    indices, indptr, rows = structure(rng, rng.integers(0, 12, m), k)
    for nb in nb_boundaries(dtype):
        P, Q = int_operands(rng, m, k, nb, dtype)
        check_exact(indices, indptr, rows, m, k, P, Q)


@pytest.mark.parametrize('dtype', DTYPES)
def test_unaligned_operand_view(dtype):
    """nb a multiple of the vector width, operands that start one element past a 16-byte boundary: element loads, same bits."""
    rng = np.random.default_rng(25)
    m, k, nb = 61, 89, 2 * vec_elems(dtype)
    indices, indptr, rows = structure(rng, rng.integers(0, 12, m), k)
    P, Q = int_operands(rng, m, k, nb, dtype)
    aligned = check_exact(indices, indptr, rows, m, k, P, Q)
    Pu = torch.empty(m * nb + 1, dtype=dtype, device=dev())[1:].view(m, nb).copy_(P)
    Qu = torch.empty(k * nb + 1, dtype=dtype, device=dev())[1:].view(k, nb).copy_(Q)
    assert Pu.data_ptr() % 16 != 0 and Qu.data_ptr() % 16 != 0 and Pu.is_contiguous()
    assert torch.equal(check_exact(indices, indptr, rows, m, k, Pu, Qu), aligned)
    # real values: the order of the sum does not depend on the kind of load either
    Pr, Qr = real_operands(rng, m, k, nb, dtype)
    Pu.copy_(Pr)
    Qu.copy_(Qr)
    assert torch.equal(run_ptr(indices, indptr, m, k, Pu, Qu), run_ptr(indices, indptr, m, k, Pr, Qr))


def test_more_tiles_than_the_grid_cap():
    rng = np.random.default_rng(26)
    n_conn = 1024
    m = (CONSTS['grid_cap'] + 2) * CONSTS['tile'] // n_conn + 1         # fixed rows: grid_cap + 2 tiles and a partial one
    k = 5000
    nse = m * n_conn
    assert nse > (CONSTS['grid_cap'] + 2) * CONSTS['tile']
    idx = torch.randint(0, k, (m, n_conn), dtype=torch.int32, device=dev())
    P, Q = int_operands(rng, m, k, 1, torch.float32)
    got = S.sddmm_rows(idx, None, n_conn, None, m, k, P, Q)
    want = (P[:, :1] * Q[idx.long().reshape(-1), 0].reshape(m, n_conn)).reshape(-1)
    assert torch.equal(got, want)
    ptr = torch.arange(m + 1, dtype=torch.int64, device=dev()) * n_conn
    assert torch.equal(S.sddmm_rows(idx.reshape(-1), ptr, -1, None, m, k, P, Q), want)


# ------------------------------------------------------------------------------------------------ 5. one matrix, three readings
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize('nb', [1, 5, 32, 33, 257])
def test_csr_fixed_and_coo_readings_agree_bit_for_bit(nb, dtype):
    rng = np.random.default_rng(nb)
    m, k, n_conn = 700, 311, 7                    # 4900 entries: more than two tiles
    idx = torch.tensor(rng.integers(0, k, (m, n_conn)), dtype=torch.int32, device=dev())
    P, Q = real_operands(rng, m, k, nb, dtype, -2.0, 2.0)
    fixed = S.sddmm_rows(idx, None, n_conn, None, m, k, P, Q)
    p32 = torch.arange(m + 1, dtype=torch.int32, device=dev()) * n_conn
    row_ids = torch.arange(m, dtype=torch.int32, device=dev()).repeat_interleave(n_conn)
    assert torch.equal(S.sddmm_rows(idx.reshape(-1), p32, -1, None, m, k, P, Q), fixed)
    assert torch.equal(S.sddmm_rows(idx.reshape(-1), p32.long(), -1, None, m, k, P, Q), fixed)
    assert torch.equal(S.sddmm_rows(idx.reshape(-1), None, -1, row_ids, m, k, P, Q), fixed)
    assert torch.equal(S.sddmm_rows(idx, None, n_conn, None, m, k, P, Q), fixed)                 # two runs
    # COO in another order: every entry keeps its bits
    perm = torch.tensor(rng.permutation(m * n_conn), device=dev())
    shuffled = S.sddmm_rows(idx.reshape(-1)[perm].contiguous(), None, -1, row_ids[perm].contiguous(), m, k, P, Q)
    assert torch.equal(shuffled, fixed[perm])
    # the public function reads the same entries: A = P, B = Q.T
    pub = be.sddmm_coo_indices(P, Q.T, row_ids, idx.reshape(-1))
    assert pub.dtype == dtype and torch.equal(pub, fixed)
    pairs = torch.stack([row_ids, idx.reshape(-1)], dim=1)
    assert torch.equal(be.sddmm_indices(P, Q.T, pairs), fixed)


# ------------------------------------------------------------------------------------------------ 6. real values: the bound
def check_bound(got, P64, Q64, rows, cols, nb, dtype):
    """|got - s| <= gamma sum_b |P Q| + u_w |s|, gamma = nb u_acc / (1 - nb u_acc): any summation order of nb products in
    the accumulation type, then one rounding to the weight dtype."""
    u_acc = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    gamma = nb * u_acc / (1 - nb * u_acc)
    prod = P64[rows] * Q64[cols]
    s = prod.sum(1)
    bound = gamma * np.abs(prod).sum(1) + U_W[dtype] * np.abs(s)
    err = np.abs(f64(got) - s)
    worst = float((err / bound).max()) if err.size else 0.0
    print(f"sddmm bound: dtype={dtype} nb={nb} max err / bound = {worst:.3f}")
    assert (err <= bound).all(), f"max err / bound = {worst}"


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nb', [2, 33, 257])
def test_error_bound(nb, dtype):
    rng = np.random.default_rng(nb + 1)
    m, k = 211, 173
    indices, indptr, rows = structure(rng, rng.integers(0, 30, m), k)
    P, Q = real_operands(rng, m, k, nb, dtype)
    got = run_ptr(indices, indptr, m, k, P, Q)
    check_bound(got, f64(P), f64(Q), rows, indices.astype(np.int64), nb, dtype)


# ------------------------------------------------------------------------------------------------ 7. operand and shared-weight gradients
@pytest.mark.parametrize('batched', [False, True])
@pytest.mark.parametrize('left', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_shared_weight_gradient_is_the_dense_one(kind, left, batched):
    rng = np.random.default_rng(70 + KINDS.index(kind) * 4 + left * 2 + batched)
    shape = (23, 31)
    M = make_container(kind, rng, shape, homo=True)
    n_in, n_out = (shape[0], shape[1]) if left else (shape[1], shape[0])
    nb = 4
    xs = (n_in,) if not batched else ((nb, n_in) if left else (n_in, nb))
    x = torch.tensor(rng.integers(-4, 5, xs), dtype=torch.float32, device=dev(), requires_grad=True)
    y = x @ M if left else M @ x
    g = torch.tensor(rng.integers(-4, 5, tuple(y.shape)), dtype=torch.float32, device=dev())
    y.backward(g)
    dw, dx = dense_reference(M, x, left, g)
    assert M.data.grad.shape == M.data.shape == (1,)
    assert M.data.grad.double().item() == dw.item()
    assert torch.equal(x.grad.double().cpu(), dx)


@pytest.mark.parametrize('kind', ['csr', 'post'])
def test_scatter_direction_operand_gradient_with_and_without_a_live_mirror(kind):
    """The operand gradient of the gather-side product is a scatter over the stored rows: float atomics without a mirror, a
    gather over the mirror once one is alive (never built by the backward pass).  Integer values: both are exact."""
    rng = np.random.default_rng(80)
    shape = (23, 31)
    M = make_container(kind, rng, shape)
    left = M._stored_transposed                # the gather side of this container
    assert not M._scatter_side(left)
    x = torch.tensor(rng.integers(-4, 5, (3, shape[0]) if left else (shape[1], 3)), dtype=torch.float32, device=dev(),
                     requires_grad=True)
    grads = []
    for with_mirror in (False, True):
        if with_mirror:
            M.build_mirror(keep_raw=True)
        assert (AG._live_mirror(M) is not None) == with_mirror
        x.grad = M.data.grad = None
        y = x @ M if left else M @ x
        g = torch.tensor(rng.integers(-4, 5, tuple(y.shape)), dtype=torch.float32, device=dev())
        y.backward(g)
        assert (AG._live_mirror(M) is not None) == with_mirror           # (the backward pass built none)
        dw, dx = dense_reference(M, x, left, g)
        assert torch.equal(x.grad.double().cpu(), dx)
        assert torch.equal(M.data.grad.double().cpu().reshape(-1), dw)
        grads.append(x.grad.clone())


# ------------------------------------------------------------------------------------------------ 8. the gradient's order
@pytest.mark.parametrize('kind', KINDS)
def test_weight_gradient_follows_the_containers_own_order_through_the_mirror_route(kind):
    rng = np.random.default_rng(90 + KINDS.index(kind))
    shape = (23, 31)
    M = make_container(kind, rng, shape).prepare(mirror=True)
    left = not M._stored_transposed            # the scatter side: the forward pass gathers over the mirror
    assert M._scatter_side(left) and AG._live_mirror(M) is not None
    x = torch.tensor(rng.integers(-4, 5, (4, shape[0]) if left else (shape[1], 4)), dtype=torch.float32, device=dev(),
                     requires_grad=True)
    y = x @ M if left else M @ x
    g = torch.tensor(rng.integers(-4, 5, tuple(y.shape)), dtype=torch.float32, device=dev())
    y.backward(g)
    dw, dx = dense_reference(M, x, left, g)
    assert M.data.grad.shape == M.data.shape
    assert torch.equal(M.data.grad.double().cpu().reshape(-1), dw)
    assert torch.equal(x.grad.double().cpu(), dx)
    Wd = torch.tensor(M.with_data(M.data.detach()).todense(), dtype=torch.float64)
    xd = x.detach().double().cpu()
    assert torch.equal(y.detach().double().cpu(), xd @ Wd if left else Wd @ xd)


# ------------------------------------------------------------------------------------------------ 9. M.sddmm
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('kind', KINDS)
def test_container_sddmm(kind, dtype):
    rng = np.random.default_rng(100 + KINDS.index(kind))
    shape, nb = (23, 31), 33
    M = make_container(kind, rng, shape, dtype=dtype)
    A_, B_ = real_operands(rng, shape[0], shape[1], nb, dtype)
    B_ = B_.T.contiguous()                                     # [nb, shape[1]]
    R = M.sddmm(A_, B_)
    assert type(R) is type(M) and R.shape == M.shape and R.data.shape == M.data.shape and R.data.dtype == dtype
    assert R.indices.data_ptr() == M.indices.data_ptr()                 # the structure is shared, not copied
    if kind in ('csr', 'csc'):
        assert R.indptr.data_ptr() == M.indptr.data_ptr()
    assert R.data.grad_fn is None
    pr, pc = dense_positions(M)
    check_bound(R.data.reshape(-1), f64(A_), f64(B_).T.copy(), pr.numpy(), pc.numpy(), nb, dtype)
    # numpy operands are taken too; the result stays a container
    Rn = M.sddmm(f64(A_).astype(np.float32), f64(B_).astype(np.float32))
    assert torch.equal(Rn.data, R.data)


def test_sddmm_refusals_and_numpy_results():
    rng = np.random.default_rng(110)
    M = make_container('csr', rng, (23, 31), homo=True)
    with pytest.raises(be.UnsupportedOperationError):
        M.sddmm(np.ones((23, 2), np.float32), np.ones((2, 31), np.float32))
    A_, B_ = np.ones((4, 3), np.float32), np.full((3, 5), 2.0, np.float32)
    out = be.sddmm_coo_indices(A_, B_, np.array([0, 3, 3]), np.array([4, 0, 2]))
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.tolist() == [6.0, 6.0, 6.0]
    with pytest.raises(ValueError):
        be.sddmm_coo_indices(A_, B_, np.array([0, 4]), np.array([0, 0]))          # row 4 of 4
    with pytest.raises(ValueError):
        be.sddmm_coo_indices(A_, B_, np.array([0, 1]), np.array([0, -1]))
    with pytest.raises(TypeError):
        be.sddmm_coo_indices(A_, B_, np.array([0.0, 1.0]), np.array([0, 1]))


# ------------------------------------------------------------------------------------------------ 10. graph capture
def test_capture_forward_and_backward():
    """A step holding the forward and backward pass of csr @ x (weights and operand) captured with capture_step replays to the
    eager gradients: nothing on the path synchronises the host."""
    rng = np.random.default_rng(120)
    m, k, nb = 400, 300, 8
    indices, indptr, rows = structure(rng, rng.integers(0, 20, m), k)
    w = torch.tensor(rng.standard_normal(indices.size), dtype=torch.float32, device=dev(), requires_grad=True)
    csr = be.CSR((w, torch.tensor(indices, device=dev()), torch.tensor(indptr, dtype=torch.int32, device=dev())), shape=(m, k))
    x = torch.zeros((k, nb), device=dev(), requires_grad=True)
    h = torch.zeros((nb, m), device=dev())

    def step():
        y = csr @ x                                   # gather
        z = h @ csr                                   # scatter side (float atomics; no mirror is built at this size)
        return torch.autograd.grad((y ** 2).sum() + (z ** 2).sum(), (w, x))

    with torch.no_grad():
        x.copy_(torch.tensor(rng.standard_normal((k, nb)), dtype=torch.float32))
        h.copy_(torch.tensor(rng.standard_normal((nb, m)), dtype=torch.float32))
    graphed = be.capture_step(step)
    for _ in range(2):
        with torch.no_grad():
            x.copy_(torch.tensor(rng.standard_normal((k, nb)), dtype=torch.float32))
            h.copy_(torch.tensor(rng.standard_normal((nb, m)), dtype=torch.float32))
        got = [t.clone() for t in graphed()]
        want = step()
        # dw is bit-reproducible; dx of the gather product is a float-atomic scatter of <= 20 terms of magnitude <= ~30 each,
        # whose order is free: two orders differ by at most n u sum|terms| ~ 20 * 2^-24 * 600 < 1e-3
        for a, b in zip(got, want):
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-3)
            assert torch.count_nonzero(a).item() > 0
