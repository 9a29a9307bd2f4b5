"""The JIT-connectivity products under torch.autograd on the device: be_jit_param_grad (csrc/be_jitc_grad.hip) through
``jit_param_sums``, and ``_autograd.JitProduct`` through the twelve functionals and the six containers.

The expectation for the two sums is ``S0 = sum(C * (P @ Q.T))`` and ``S1 = sum(T * (P @ Q.T))`` in float64, ``C`` the oracle's
structure of the draw (its scalar family with weight 1) and ``T`` the oracle's ``t`` on it (the family with parameters (0, 1),
formed in f32 as the device forms it).  Cases past one grid pass compare with the composition of the float twins on the device
instead (parameters (1, 0) and (0, 1), then ``sum(P * r)``), in f64: the oracle is a Python loop.

Tolerances (derived, not tuned).  ``E = sum_edges |P[r] . Q[j]|``, ``A = sum_edges sum_b |P[r, b]| |Q[j, b]|``:
  * S0 on integer operands in [-4, 4] is exact in f64 in any order: equality.  On other operands a product of two values of
    at most 24 significant bits is exact in f64 (f64 operands: one rounding) and the additions round: ``|err| <= (n + 1) 2^-53 A``
    for ``n`` addends, far below ``1e-12 A`` at the few thousand edges of these cases.
  * S1: the device's ``t`` against the oracle's is granted ``TOL_t`` per weight (tests/test_jitc_dt2t_gpu.py: TOL — 1e-6 uniform,
    1e-4 normal), so ``|err| <= TOL_t E + 1e-12 A`` (``A = E`` on integer operands of one sign pattern per edge; ``A >= E``
    always, and the 1e-12 term only covers the f64 additions).  Scalar: ``S1 == 0``.
  * a parameter gradient adds one rounding to the parameter's dtype: ``+ u |s|``, ``u = 2^-24`` for f32.
  * operand gradients: the tolerance tests/test_float_gpu.py holds the same float twin to (rtol 1e-5, atol 1e-5 max(1, |ref|max)).

Sizes follow the two constants of the walk (tests/test_jitc_autograd_cpu.py pins them to the source): JIT_PARAM_GRAD_THREADS /
stride generator rows per block, JIT_PARAM_GRAD_GRID_CAP blocks per launch."""
import functools

import numpy as np
import pytest
import torch

from brainevent_amd import _autograd as AG
from brainevent_amd import _jitc
from test_jitc_dt2t_gpu import TOL as TOL_T

pytestmark = pytest.mark.gpu

CAP = _jitc.JIT_PARAM_GRAD_GRID_CAP
THREADS = _jitc.JIT_PARAM_GRAD_THREADS
F32 = np.float32
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
PARAMS = {'s': (0.5,), 'u': (0.1, 0.9), 'n': (0.3, 1.7)}
MODE = {32: 'mv', 4: 'mm'}


@functools.lru_cache(maxsize=None)
def _gen(family, prob, seed, gshape, transpose, corder, mode):
    """The oracle's generator matrix (rows = walk owners) in float64: the structure (``'s'``: 0 / 1) or ``t`` on it."""
    from oracle import oracle_np
    w0, w1 = (F32(1.0), 0.0) if family == 's' else (F32(0.0), F32(1.0))
    G = oracle_np.jit_generator_matrix(family, w0, w1, prob, seed, shape=gshape, transpose=transpose, corder=corder,
                                       matrix_mode=mode, dtype=np.float32).astype(np.float64)
    G.setflags(write=False)
    return G


def _ct(family, prob, seed, gshape, transpose, corder, mode):
    C = _gen('s', prob, seed, gshape, transpose, corder, mode)
    return C, (np.zeros_like(C) if family == 's' else _gen(family, prob, seed, gshape, transpose, corder, mode))


def _want(C, T, P, Q):
    """(S0, S1, E, A) in float64 from the values the device receives."""
    PQ = P @ Q.T
    return float((C * PQ).sum()), float((T * PQ).sum()), float((C * np.abs(PQ)).sum()), float((C * (np.abs(P) @ np.abs(Q).T)).sum())


def _rounded(x, dtype):
    """``x`` as a device tensor of ``dtype`` and the float64 values it holds."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dtype).cuda()
    return t, t.double().cpu().numpy()


def _sums(family, Pt, Qt, *, prob, seed, shape1, stride):
    s = _jitc.jit_param_sums(family, Pt, Qt, clen=_jitc._initialize_conn_length(prob), seed=seed, shape1=shape1, stride=stride)
    assert isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.float64 and s.shape == (2,)
    return s.cpu().numpy()


def _ints(rng, shape):
    return rng.integers(-4, 5, shape).astype(np.float64)


def _check_sums(family, got, C, T, P, Q, exact_s0):
    s0, s1, E, A_ = _want(C, T, P, Q)
    print(f'S0 got {got[0]!r} want {s0!r}   S1 got {got[1]!r} want {s1!r}   E {E!r} A {A_!r}')
    if exact_s0:
        assert got[0] == s0
    else:
        assert abs(got[0] - s0) <= 1e-12 * A_
    if family == 's':
        assert got[1] == 0.0
    else:
        assert abs(got[1] - s1) <= TOL_T[family] * E + 1e-12 * A_


# ------------------------------------------------------------------------------------------------ 1. the kernel: chunk edges
@pytest.mark.parametrize('shape1', [3, 31, 33, 130])
@pytest.mark.parametrize('stride', [32, 4])
@pytest.mark.parametrize('corder', [True, False])
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_chunk_edges(family, corder, stride, shape1):
    """Walks narrower than the stride and a ragged last chunk: the walk runs over ``shape[1]`` in both orientations."""
    n_rows, prob, seed, nb = 11, 0.3, 5, 3
    gshape, transpose = (n_rows, shape1), not corder
    C, T = _ct(family, prob, seed, gshape, transpose, corder, MODE[stride])
    assert C.shape == (n_rows, shape1)
    rng = np.random.default_rng(shape1 + stride)
    P, Q = _ints(rng, (n_rows, nb)), _ints(rng, (shape1, nb))
    got = _sums(family, torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda(), prob=prob, seed=seed, shape1=shape1, stride=stride)
    _check_sums(family, got, C, T, P, Q, exact_s0=True)


@pytest.mark.parametrize('stride', [32, 4])
@pytest.mark.parametrize('family', ['u', 'n'])
def test_long_walk_side(family, stride):
    """``shape = (3000, 8)``, ``corder=False``: the walk runs over 3000 positions in chunks of 2 — 1500 chunks, every one of
    them narrower than the stride, under a single block of generator rows."""
    gshape, prob, seed, nb = (3000, 8), 0.3, 9, 2
    C, T = _ct(family, prob, seed, gshape, False, False, MODE[stride])
    assert C.shape == (8, 3000) and C.sum() > 5000
    rng = np.random.default_rng(stride)
    P, Q = _ints(rng, (8, nb)), _ints(rng, (3000, nb))
    got = _sums(family, torch.from_numpy(P).float().cuda(), torch.from_numpy(Q).float().cuda(), prob=prob, seed=seed, shape1=8,
                stride=stride)
    _check_sums(family, got, C, T, P, Q, exact_s0=True)


# ------------------------------------------------------------------------------------------------ 2. batch width x dtype
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.float16, torch.bfloat16])
@pytest.mark.parametrize('nb', [1, 2, 8, 9, 33])
@pytest.mark.parametrize('stride', [32, 4])
def test_batch_width_and_dtype(stride, nb, dtype):
    """Operands are rounded to the dtype first; the expectation is formed from the rounded values."""
    family, gshape, prob, seed = 'n', (23, 37), 0.25, 3
    C, T = _ct(family, prob, seed, gshape, False, True, MODE[stride])
    rng = np.random.default_rng(nb)
    Pt, P = _rounded(rng.standard_normal((23, nb)), dtype)
    Qt, Q = _rounded(rng.standard_normal((37, nb)), dtype)
    got = _sums(family, Pt, Qt, prob=prob, seed=seed, shape1=37, stride=stride)
    _check_sums(family, got, C, T, P, Q, exact_s0=False)


# ------------------------------------------------------------------------------------------------ 3. more rows than one grid pass
@pytest.mark.parametrize('stride', [32, 4])
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_more_rows_than_one_grid_pass(be, family, stride):
    """``cap x rows-per-block + 3`` generator rows: every block takes more than one task.  Against the composition of the float
    twins (gather orientation, f64: deterministic, no atomics) — independent of the new kernel; tolerance ``1e-12 sum |d|`` over
    the elements ``d`` of ``P * r``."""
    n_rows, walk, prob, seed = CAP * (THREADS // stride) + 3, 40, 0.1, 17
    nb = 1 if stride == 32 else 3
    g = torch.Generator().manual_seed(stride)
    P = torch.randn(n_rows, nb, generator=g, dtype=torch.float64).cuda()
    Q = torch.randn(walk, nb, generator=g, dtype=torch.float64).cuda()
    got = _sums(family, P, Q, prob=prob, seed=seed, shape1=walk, stride=stride)
    clen = _jitc._initialize_conn_length(prob)
    one, zero = torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)
    twin = getattr(be, f"jit{'n' if family == 's' else family}{'mv' if stride == 32 else 'mm'}_p_call")
    X = Q[:, 0] if stride == 32 else Q
    kw = dict(shape=(n_rows, walk), transpose=False, corder=True)
    # (1, 0): every edge weighs 1 in all three families; (0, 1): every edge weighs t (uniform: low 0, high 1)
    r0 = twin(one, zero if family != 'u' else one, clen, X, seed, **kw)[0].reshape(n_rows, nb)
    r1 = twin(zero, one, clen, X, seed, **kw)[0].reshape(n_rows, nb)
    d0, d1 = P * r0, P * r1
    want0, want1 = float(d0.sum()), float(d1.sum())
    print(f'S0 got {got[0]!r} want {want0!r}   S1 got {got[1]!r} want {want1!r}')
    assert float(r0.abs().sum()) > n_rows                                            # (the draw is not empty)
    assert abs(got[0] - want0) <= 1e-12 * float(d0.abs().sum())
    if family == 's':
        assert got[1] == 0.0
    else:
        assert abs(got[1] - want1) <= 1e-12 * float(d1.abs().sum())
    again = _sums(family, P, Q, prob=prob, seed=seed, shape1=walk, stride=stride)
    assert again.tobytes() == got.tobytes()                                          # reproducible: the same 16 bytes


# ------------------------------------------------------------------------------------------------ 4. rows that are skipped
@pytest.mark.parametrize('nb', [1, 3])
@pytest.mark.parametrize('stride', [32, 4])
def test_zero_rows_of_p_are_skipped(stride, nb):
    family, gshape, prob, seed = 'n', (19, 41), 0.3, 21
    C, T = _ct(family, prob, seed, gshape, False, True, MODE[stride])
    rng = np.random.default_rng(7)
    P, Q = _ints(rng, (19, nb)), _ints(rng, (41, nb))
    P[P == 0] = 1.0
    P[[0, 9, 18]] = 0.0                                                              # first, middle and last row
    got = _sums(family, torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda(), prob=prob, seed=seed, shape1=41, stride=stride)
    _check_sums(family, got, C, T, P, Q, exact_s0=True)
    zero = _sums(family, torch.zeros(19, nb).cuda(), torch.from_numpy(Q).float().cuda(), prob=prob, seed=seed, shape1=41, stride=stride)
    assert zero.tobytes() == np.zeros(2).tobytes()


# ------------------------------------------------------------------------------------------------ 5. degenerate inputs
@pytest.mark.parametrize('stride', [32, 4])
def test_degenerate_inputs(stride):
    dev = 'cuda'
    kw = dict(seed=3, shape1=7, stride=stride)
    ones = lambda *s: torch.ones(*s, device=dev)
    zeros2 = np.zeros(2).tobytes()
    assert _sums('n', ones(5, 2), ones(7, 2), prob=0.0, **kw).tobytes() == zeros2           # prob = 0: nothing is drawn
    assert _sums('n', ones(0, 2), ones(7, 2), prob=0.5, **kw).tobytes() == zeros2           # no generator rows
    assert _sums('u', ones(5, 2), ones(0, 2), prob=0.5, **kw).tobytes() == zeros2           # no walk
    assert _sums('s', ones(5, 0), ones(7, 0), prob=0.5, **kw).tobytes() == zeros2           # no batch
    rng = np.random.default_rng(1)
    for n_rows, prob in ((1, 0.5), (6, 1.0)):                                              # a single row; every position drawn
        C, T = _ct('n', prob, 3, (n_rows, 7), False, True, MODE[stride])
        if prob == 1.0:
            assert C.min() == 1.0
        P, Q = _ints(rng, (n_rows, 2)), _ints(rng, (7, 2))
        got = _sums('n', torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda(), prob=prob, **kw)
        _check_sums('n', got, C, T, P, Q, exact_s0=True)


# ------------------------------------------------------------------------------------------------ 6. the functionals
SHAPE, PROB, SEED = (13, 17), 0.2, 7


def _lens(gshape, transpose):
    return (gshape[0], gshape[1]) if transpose else (gshape[1], gshape[0])             # (in_len, out_len)


def _param(value, pshape, pdev):
    return torch.full(pshape, value, dtype=torch.float32, device=pdev, requires_grad=True)


def _dense_autograd(family, C, T, gen_is_out, X, g, left_2d=False):
    """torch.autograd in float64 over the dense matrix ``D (out_len, in_len)`` (``G`` when ``gen_is_out``, else ``G.T``):
    ``(d params, dX, E, A)`` for ``Y = D @ X`` (``X [in_len, nb]``; ``left_2d``: ``Y = X @ D.T`` with ``X [nb, in_len]``)."""
    ps = [torch.tensor(float(F32(p)), dtype=torch.float64, requires_grad=True) for p in PARAMS[family]]
    Ct, Tt = torch.tensor(C), torch.tensor(T)
    G = {'s': lambda: ps[0] * Ct, 'u': lambda: ps[0] * Ct + Tt * (ps[1] - ps[0]), 'n': lambda: ps[0] * Ct + ps[1] * Tt}[family]()
    D = G if gen_is_out else G.T
    Xt = torch.tensor(np.asarray(X, np.float64), requires_grad=True)
    gt = torch.tensor(np.asarray(g, np.float64))
    Y = Xt @ D.T if left_2d else D @ Xt
    Y.backward(gt)
    x_nm, g_nm = (Xt.detach().T, gt.T) if left_2d else (Xt.detach().reshape(Xt.shape[0], -1), gt.reshape(gt.shape[0], -1))
    P, Q = (g_nm, x_nm) if gen_is_out else (x_nm, g_nm)
    E = float((Ct * (P @ Q.T).abs()).sum())
    A_ = float((Ct * (P.abs() @ Q.abs().T)).sum())
    return [p.grad for p in ps], Xt.grad, Y.detach(), E, A_


def _check_param_grads(family, params, want, E, A_):
    for p, w in zip(params, want):
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device
        got, w = float(p.grad.double().reshape(-1)[0]), float(w)
        tol = TOL_T[family] * E + 1e-12 * A_ + U[p.dtype] * abs(w)
        print(f'd param got {got!r} want {w!r} tol {tol!r}')
        assert abs(got - w) <= tol


def _check_operand_grad(got, want):
    want = want.numpy()
    np.testing.assert_allclose(got.double().cpu().numpy(), want, rtol=1e-5, atol=1e-5 * max(1.0, float(np.abs(want).max())))


@pytest.mark.parametrize('variant', [((), 'cuda'), ((1,), 'cpu')], ids=['scalar-device', 'one-cpu'])
@pytest.mark.parametrize('corder', [True, False])
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('rank', [1, 2])
@pytest.mark.parametrize('event', [False, True], ids=['float', 'binary'])
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_functionals(be, family, event, rank, transpose, corder, variant):
    """All twelve: a node is recorded, every parameter's gradient and the operand's agree with dense autograd on the oracle matrix.
    The binary ones get float spikes in {0, 0.5, 1}: 0.5 counts as 1 in the parameter gradients, and the tensor receives M.T @ g."""
    pshape, pdev = variant
    f = getattr(be, f"{'binary_' if event else ''}jit{family}{'mv' if rank == 1 else 'mm'}")
    in_len, out_len = _lens(SHAPE, transpose)
    nb = 1 if rank == 1 else 5
    rng = np.random.default_rng(in_len + 3 * nb)
    xs = (in_len,) if rank == 1 else (in_len, nb)
    x_np = rng.choice([0.0, 0.5, 1.0], xs).astype(F32) if event else rng.standard_normal(xs).astype(F32)
    g_np = rng.standard_normal((out_len,) if rank == 1 else (out_len, nb)).astype(F32)
    params = [_param(p, pshape, pdev) for p in PARAMS[family]]
    x = torch.tensor(x_np, device='cuda', requires_grad=True)
    out = f(*params, PROB, x, SEED, shape=SHAPE, transpose=transpose, corder=corder)
    assert isinstance(out, torch.Tensor) and out.grad_fn is not None
    out.backward(torch.tensor(g_np, device='cuda'))
    C, T = _ct(family, PROB, SEED, SHAPE, transpose, corder, 'mv' if rank == 1 else 'mm')
    x_eff = (x_np > 0).astype(np.float64) if event else x_np
    dps, dX, Y, E, A_ = _dense_autograd(family, C, T, corder, x_eff, g_np)
    np.testing.assert_allclose(out.detach().double().cpu().numpy(), Y.numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(Y.abs().max())))
    _check_param_grads(family, params, dps, E, A_)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == x.dtype
    _check_operand_grad(x.grad, dX)


def test_only_what_requires_grad_gets_one(be):
    """A python parameter, a tensor that does not require grad and ``prob`` / ``seed`` stay out of the graph."""
    loc = torch.tensor(0.3, device='cuda', requires_grad=True)
    x = torch.randn(17, device='cuda')
    out = be.jitnmv(loc, 1.7, PROB, x, SEED, shape=SHAPE)
    out.sum().backward()
    assert loc.grad is not None and x.grad is None
    scale = torch.tensor(1.7, requires_grad=True)
    out = be.jitnmv(torch.tensor(0.3), scale, PROB, x, SEED, shape=SHAPE)
    out.sum().backward()
    C, T = _ct('n', PROB, SEED, SHAPE, False, True, 'mv')
    P, Q = np.ones((13, 1)), x.double().cpu().numpy().reshape(-1, 1)
    _, s1, E, A_ = _want(C, T, P, Q)
    assert abs(float(scale.grad) - s1) <= TOL_T['n'] * E + 1e-12 * A_ + U[torch.float32] * abs(s1)


# ------------------------------------------------------------------------------------------------ 7. event operands
@pytest.mark.parametrize('corder', [True, False])
@pytest.mark.parametrize('kind', ['bool', 'uint8', 'float', 'numpy-bool', 'bitpacked', 'compact'])
def test_event_operands(be, kind, corder):
    """bool / uint8 / float spikes and the packed containers against the scatter- and gather-side container product: the
    parameter gradients use the activity; only a float spike tensor in a BinaryArray receives a gradient."""
    family, n = 'n', SHAPE[0]
    rng = np.random.default_rng(5)
    act = rng.random(n) < 0.4
    spikes = {'bool': lambda: torch.tensor(act, device='cuda'),
              'uint8': lambda: torch.tensor(act.astype(np.uint8) * 3, device='cuda'),
              'float': lambda: torch.tensor(np.where(act, 0.5, -1.0).astype(F32), device='cuda', requires_grad=True),
              'numpy-bool': lambda: act,
              'bitpacked': lambda: torch.tensor(act, device='cuda'),
              'compact': lambda: torch.tensor(act, device='cuda')}[kind]()
    ev = {'bitpacked': lambda s: be.BitPackedBinary(s), 'compact': lambda s: be.CompactBinary.from_array(s)}.get(kind, be.BinaryArray)(spikes)
    params = [_param(p, (), 'cuda') for p in PARAMS[family]]
    M = be.JITCNormalR((*params, PROB, SEED), shape=SHAPE, corder=corder)
    out = ev @ M                                                                  # [17]
    assert isinstance(out, torch.Tensor) and out.grad_fn is not None
    g_np = rng.standard_normal(SHAPE[1]).astype(F32)
    out.backward(torch.tensor(g_np, device='cuda'))
    # events @ M (R container): shape, transpose=True, corder = not M.corder
    C, T = _ct(family, PROB, SEED, SHAPE, True, not corder, 'mv')
    dps, dX, Y, E, A_ = _dense_autograd(family, C, T, not corder, act.astype(np.float64), g_np)
    np.testing.assert_allclose(out.detach().double().cpu().numpy(), Y.numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(Y.abs().max())))
    _check_param_grads(family, params, dps, E, A_)
    if kind == 'float':
        _check_operand_grad(spikes.grad, dX)


def test_float_spikes_inside_packed_containers_get_no_gradient(be):
    s = torch.tensor(np.where(np.arange(13) % 3 == 0, 1.0, 0.0).astype(F32), device='cuda', requires_grad=True)
    loc = _param(0.3, (), 'cuda')
    M = be.JITCNormalR((loc, 1.7, PROB, SEED), shape=SHAPE)
    (be.BitPackedBinary(s) @ M).sum().backward()
    assert loc.grad is not None and s.grad is None


# ------------------------------------------------------------------------------------------------ 8. the containers
CLASSES = {('s', 'R'): 'JITCScalarR', ('s', 'C'): 'JITCScalarC', ('u', 'R'): 'JITCUniformR', ('u', 'C'): 'JITCUniformC',
           ('n', 'R'): 'JITCNormalR', ('n', 'C'): 'JITCNormalC'}


def _logical(family, kind, corder, mode):
    """(C, T) of the container's logical matrix ``SHAPE`` (the orientation of ``M @ v``: tests/test_jitc_dt2t_gpu.py)."""
    gshape, transpose = (SHAPE, False) if kind == 'R' else (SHAPE[::-1], True)
    C, T = _ct(family, PROB, SEED, gshape, transpose, corder, mode)
    return (C, T) if corder else (C.T, T.T)


def _container_case(be, family, kind, corder, left, rank, event, prepare=None, scale=None, prepared=None):
    params = [_param(p, (), 'cuda') for p in PARAMS[family]]
    M = getattr(be, CLASSES[family, kind])((*params, PROB, SEED), shape=SHAPE, corder=corder)
    if prepare:
        M.prepare(prepare)
        if prepared is not None:
            prepared(M)
    n_in, n_out = (SHAPE[0], SHAPE[1]) if left else (SHAPE[1], SHAPE[0])
    nb = 4
    rng = np.random.default_rng(11 + rank)
    xs = (n_in,) if rank == 1 else ((nb, n_in) if left else (n_in, nb))
    gs = (n_out,) if rank == 1 else ((nb, n_out) if left else (n_out, nb))
    x_np = rng.choice([0.0, 0.5, 1.0], xs).astype(F32) if event else rng.standard_normal(xs).astype(F32)
    g_np = rng.standard_normal(gs).astype(F32)
    x = torch.tensor(x_np, device='cuda', requires_grad=True)
    operand = be.BinaryArray(x) if event else x
    Ms = M if scale is None else scale * M
    out = (operand @ Ms) if left else (Ms @ operand)
    assert isinstance(out, torch.Tensor) and out.grad_fn is not None and tuple(out.shape) == gs
    out.backward(torch.tensor(g_np, device='cuda'))
    return M, params, x, x_np, g_np, out.detach()


def _container_expectation(family, kind, corder, left, rank, event, x_np, g_np):
    C, T = _logical(family, kind, corder, 'mv' if rank == 1 else 'mm')               # D = SHAPE
    x_eff = (x_np > 0).astype(np.float64) if event else x_np
    if left:                                                                         # x @ D  ==  D.T @ x
        return _dense_autograd(family, C.T, T.T, True, x_eff, g_np, left_2d=rank == 2)
    return _dense_autograd(family, C, T, True, x_eff, g_np)


@pytest.mark.parametrize('event', [False, True], ids=['array', 'events'])
@pytest.mark.parametrize('rank', [1, 2])
@pytest.mark.parametrize('left', [False, True], ids=['M@x', 'x@M'])
@pytest.mark.parametrize('corder', [True, False])
@pytest.mark.parametrize('kind', ['R', 'C'])
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_containers(be, family, kind, corder, left, rank, event):
    M, params, x, x_np, g_np, out = _container_case(be, family, kind, corder, left, rank, event)
    dps, dX, Y, E, A_ = _container_expectation(family, kind, corder, left, rank, event, x_np, g_np)
    np.testing.assert_allclose(out.double().cpu().numpy(), Y.numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(Y.abs().max())))
    _check_param_grads(family, params, dps, E, A_)
    _check_operand_grad(x.grad, dX)


@pytest.mark.parametrize('mode', ['mv', 'mm'])
@pytest.mark.parametrize('left', [False, True], ids=['M@s', 's@M'])
@pytest.mark.parametrize('family', ['s', 'n'])
def test_prepared_containers_keep_their_route_and_their_gradients(be, family, left, mode, monkeypatch):
    """After ``prepare()`` the forward is the stored matrix's product — the very tensor that product returned, once —, and the
    gradients are those of the walk.  A second call of the stored product gives the same bits for the scalar family (counts x
    weight: exact); the other families' stored sums are fixed-point sums of f32 weights, repeatable to 1e-6 (``prepare()``)."""
    rank = 1 if mode == 'mv' else 2
    calls = []

    def spy(M):
        S = M.buffers['materialized_' + mode]
        name = '__rmatmul__' if left else '__matmul__'
        orig = getattr(type(S), name)

        def product(self, other):
            r = orig(self, other)
            if self is S:
                calls.append(r)
            return r
        monkeypatch.setattr(type(S), name, product)

    M, params, x, x_np, g_np, out = _container_case(be, family, 'R', False, left, rank, True, prepare=mode, prepared=spy)
    monkeypatch.undo()
    assert len(calls) == 1 and torch.equal(out, calls[0].detach())
    S = M.buffers['materialized_' + mode]
    with torch.no_grad():
        stored = (be.BinaryArray(x.detach()) @ S) if left else (S @ be.BinaryArray(x.detach()))
    print(f'stored product, second call: max |diff| {float((out - stored).abs().max())!r} of max {float(stored.abs().max())!r}')
    if family == 's':
        assert torch.equal(out, stored)
    else:
        torch.testing.assert_close(out, stored, rtol=1e-6, atol=1e-6 * float(stored.abs().max()))
    M0, params0, x0, *_ = _container_case(be, family, 'R', False, left, rank, True)
    for p, p0 in zip(params, params0):
        assert torch.equal(p.grad, p0.grad)                                            # the same walk, the same bytes
    dps, dX, Y, E, A_ = _container_expectation(family, 'R', False, left, rank, True, x_np, g_np)
    _check_param_grads(family, params, dps, E, A_)
    _check_operand_grad(x.grad, dX)


def test_scaled_container_reaches_the_leaf(be):
    """``(0.5 * M) @ x``: the arithmetic keeps tensor parameters in the graph, so the leaf receives half the gradient."""
    M, params, x, x_np, g_np, _ = _container_case(be, 's', 'R', True, False, 1, False, scale=0.5)
    M1, params1, x1, *_ = _container_case(be, 's', 'R', True, False, 1, False)
    assert params[0].grad is not None
    # d/dw sum(g * (0.5 w) C x) = 0.5 S0, one f32 multiply after the rounding of S0
    assert float(params[0].grad) == float(F32(0.5) * params1[0].grad.cpu().numpy())
    dps, dX, Y, E, A_ = _container_expectation('s', 'R', True, False, 1, False, x_np, g_np)
    _check_operand_grad(x.grad, 0.5 * dX)


# ------------------------------------------------------------------------------------------------ 9. nothing requires grad
def test_no_grad_no_node_same_bits(be, monkeypatch):
    """Without a gradient to take — no tensor requires grad, ``torch.no_grad()``, numpy operands — the call is the operator
    call it was: no node, no parameter-gradient launch, the operator's own bits."""
    def boom(*a, **k):
        raise AssertionError('recorded a node where nothing requires grad')
    rng = np.random.default_rng(2)
    x_np = rng.standard_normal(17).astype(F32)
    s_np = rng.random(17) < 0.4
    x, s = torch.tensor(x_np, device='cuda'), torch.tensor(s_np, device='cuda')
    clen = _jitc._initialize_conn_length(PROB)
    kw = dict(shape=SHAPE, transpose=False, corder=True)
    base_f = _jitc.jitnmv_p(F32(0.3), F32(1.7), clen, x, SEED, out_dtype=torch.float32, **kw)
    base_b = _jitc.binary_jitnmv_p(F32(0.3), F32(1.7), clen, s, SEED, out_dtype=torch.float32, **kw)
    loc = torch.tensor(0.3, device='cuda', requires_grad=True)
    xg = x.clone().requires_grad_(True)
    with torch.no_grad():
        monkeypatch.setattr(AG.JitProduct, 'apply', boom)
        r = be.jitnmv(loc, 1.7, PROB, xg, SEED, **kw)
        assert r.grad_fn is None and torch.equal(r, base_f)
        r = be.JITCNormalR((loc, 1.7, PROB, SEED), shape=SHAPE, corder=True) @ be.BinaryArray(s)
        assert r.grad_fn is None and torch.equal(r, base_b)
    r = be.jitnmv(0.3, 1.7, PROB, x, SEED, **kw)
    assert r.grad_fn is None and torch.equal(r, base_f)
    r = be.binary_jitnmv(torch.tensor(0.3), 1.7, PROB, s, SEED, **kw)
    assert r.grad_fn is None and torch.equal(r, base_b)
    r = be.jitnmv(F32(0.3), F32(1.7), PROB, x_np, SEED, **kw)
    assert isinstance(r, np.ndarray) and np.array_equal(r, base_f.cpu().numpy())
    r = be.JITCNormalR((F32(0.3), F32(1.7), PROB, SEED), shape=SHAPE, corder=True) @ be.BinaryArray(s_np)
    assert isinstance(r, np.ndarray) and np.array_equal(r, base_b.cpu().numpy())
    monkeypatch.undo()
    out = be.jitnmv(loc, 1.7, PROB, xg, SEED, **kw)                                  # ... and with grad mode on, the same bits
    assert out.grad_fn is not None and torch.equal(out.detach(), base_f)
