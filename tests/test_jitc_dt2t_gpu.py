"""The JIT-connectivity per-synapse products on the device: jit{s,u,n}mv_dt2t, JITC*.dt2t / .dt2t_transposed and the
canonical (sorted) materialisation they are defined on (brainevent_amd/_jitc.py, k_jit_fill_sorted in csrc/be_jitc.hip).

The expectation is the oracle's generator matrix, oriented as tests/test_jitc_gpu.py::test_jitc_materialisation_matches_ops_
and_oracle orients it (D = G when corder, else G.T); the STRUCTURE is the scalar-family matrix of the same (prob, seed) — a
drawn uniform / normal weight may be 0 —, the entries are taken row-major with ascending columns.  Tolerances are that test's:
1e-6 (scalar, uniform), 1e-4 (normal).  y lies in [0.5, 1): |w y - w' y| <= |w - w'|, so a weight within the tolerance gives a
product within it (the product itself is one f32 multiply on both sides).

Sizes follow the two constants of the sorted fill (tests/test_jitc_dt2t_cpu.py pins them to the source): JIT_SORTED_WINDOW
columns per bitmap window, JIT_SORTED_GRID_CAP owner rows per launch."""
import functools

import numpy as np
import pytest
import torch

from brainevent_amd import _jitc

pytestmark = pytest.mark.gpu

W = _jitc.JIT_SORTED_WINDOW
CAP = _jitc.JIT_SORTED_GRID_CAP
F32 = np.float32
PARAMS = {'s': (F32(0.5),), 'u': (F32(0.1), F32(0.9)), 'n': (F32(0.2), F32(1.3))}
NAMES = {'s': 'JITCScalar', 'u': 'JITCUniform', 'n': 'JITCNormal'}
TOL = {'s': 1e-6, 'u': 1e-6, 'n': 1e-4}


@functools.lru_cache(maxsize=None)
def _dense(family, prob, seed, gshape, transpose, corder):
    """D (out_len, in_len) of the oracle for the mv draw; 's' is drawn with weight 1 (the structure)."""
    from oracle import oracle_np
    w0, w1 = (F32(1.0), 0.0) if family == 's' else PARAMS[family]
    G = oracle_np.jit_generator_matrix(family, w0, w1, prob, seed, shape=gshape, transpose=transpose, corder=corder,
                                       matrix_mode='mv', dtype=np.float32)
    D = G if corder else G.T
    D.setflags(write=False)
    return D


def _expected(family, prob, seed, gshape, transpose, corder, y, by_row):
    """(values, rows, cols) of the canonical CSR: structure from the scalar draw, weights from the family's."""
    rows, cols = np.nonzero(_dense('s', prob, seed, gshape, transpose, corder))          # row-major, ascending columns
    w = np.full(rows.size, PARAMS['s'][0], F32) if family == 's' else _dense(family, prob, seed, gshape, transpose, corder)[rows, cols]
    return (w * y[rows if by_row else cols]).astype(F32), rows, cols


def _orientation(cls_kind, shape):
    return (shape, False) if cls_kind == 'R' else (shape[::-1], True)


def _y(n, seed=0):
    return np.random.default_rng(seed).uniform(0.5, 1.0, n).astype(F32)


def _matrix(be, family, cls_kind, shape, prob, seed, corder, tensors=False):
    params = tuple(torch.tensor(float(p)) for p in PARAMS[family]) if tensors else PARAMS[family]
    return getattr(be, NAMES[family] + cls_kind)((*params, prob, seed), shape=shape, corder=corder)


def _close(got, want, family):
    assert got.shape == want.shape and got.dtype == F32
    np.testing.assert_allclose(got, want, rtol=TOL[family], atol=TOL[family])


# ------------------------------------------------------------------------------------------------ 1. base grid
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
@pytest.mark.parametrize('cls_kind', ['R', 'C'])
@pytest.mark.parametrize('corder', [False, True])
def test_container_methods_match_the_oracle(be, family, cls_kind, corder):
    shape, prob, seed = (37, 52), 0.2, 13
    gshape, transpose = _orientation(cls_kind, shape)
    M = _matrix(be, family, cls_kind, shape, prob, seed, corder)
    for by_row in (True, False):
        y = _y(shape[0] if by_row else shape[1])
        want, rows, _ = _expected(family, prob, seed, gshape, transpose, corder, y, by_row)
        assert rows.size > 100
        got = (M.dt2t if by_row else M.dt2t_transposed)(y, None)
        assert isinstance(got, np.ndarray)
        _close(got, want, family)
        _close((M.dt2t if by_row else M.dt2t_transposed)(y), want, family)      # (w may be left out; the cached offsets serve this one)
    assert ('materialized_mv_indptr' in M.buffers) == corder              # fused exactly when materialize() returns a CSR
    assert isinstance(M.materialize('mv'), be.CSR if corder else be.CSC)


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
@pytest.mark.parametrize('corder', [False, True])
@pytest.mark.parametrize('transpose', [False, True])
def test_functions_match_the_oracle(be, family, corder, transpose):
    shape, prob, seed = (37, 52), 0.2, 13
    y = _y(shape[1] if transpose else shape[0], 1)
    want, _, _ = _expected(family, prob, seed, shape, False, corder, y, not transpose)
    f = getattr(be, f'jit{family}mv_dt2t')
    got = f(*PARAMS[family], prob, y, seed, shape=shape, transpose=transpose, corder=corder)
    assert isinstance(got, np.ndarray)
    _close(got, want, family)
    got_t = f(*PARAMS[family], prob, torch.from_numpy(y).cuda(), seed, shape=shape, transpose=transpose, corder=corder)
    assert isinstance(got_t, torch.Tensor) and got_t.is_cuda
    np.testing.assert_array_equal(got_t.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ 2. fused == composed, bitwise
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
@pytest.mark.parametrize('cls_kind', ['R', 'C'])
def test_fused_route_equals_the_canonical_matrix_times_y_bitwise(be, family, cls_kind):
    """Each value is one f32 multiply of the same weight and the same y element on both sides."""
    shape, prob, seed = (37, 52), 0.2, 13
    M = _matrix(be, family, cls_kind, shape, prob, seed, True)
    S = M.materialize('mv', canonical=True)
    assert isinstance(S, be.CSR)
    ptr, idx = S.indptr.to(torch.int64), S.indices.to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(shape[0], device=ptr.device), ptr[1:] - ptr[:-1])
    data = S.data if S.data.numel() > 1 else S.data.expand(idx.numel())
    for by_row in (True, False):
        y = torch.from_numpy(_y(shape[0] if by_row else shape[1], 2)).cuda()
        want = data * y[rows if by_row else idx]
        got = (M.dt2t if by_row else M.dt2t_transposed)(y, None)
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 3. canonical materialisation
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
@pytest.mark.parametrize('corder', [False, True])
@pytest.mark.parametrize('mode', ['mv', 'mm'])
def test_canonical_materialisation_is_sorted_repeatable_and_the_same_matrix(be, family, corder, mode):
    shape = (37, 52)
    M = _matrix(be, family, 'R', shape, 0.2, 13, corder)
    A_, B_ = M.materialize(mode, canonical=True), M.materialize(mode, canonical=True)
    assert isinstance(A_, be.CSR if corder else be.CSC)
    idx, ptr = A_.indices.cpu().numpy().astype(np.int64), A_.indptr.cpu().numpy().astype(np.int64)
    assert ptr.size == (shape[0] if corder else shape[1]) + 1 and ptr[-1] == idx.size > 100
    owner = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    same = owner[1:] == owner[:-1]
    assert np.all(np.diff(idx)[same] > 0), "indices do not ascend strictly within an owner"
    np.testing.assert_array_equal(B_.indices.cpu().numpy(), A_.indices.cpu().numpy())
    np.testing.assert_array_equal(B_.data.cpu().numpy(), A_.data.cpu().numpy())
    np.testing.assert_array_equal(B_.indptr.cpu().numpy(), A_.indptr.cpu().numpy())
    np.testing.assert_array_equal(A_.todense(), M.materialize(mode).todense())
    view = M.mv if mode == 'mv' else M.mm
    np.testing.assert_array_equal(view.todense(canonical=True), A_.todense())
    np.testing.assert_array_equal(view.tocsr(canonical=True).todense(), A_.todense())
    np.testing.assert_array_equal(M.tocsc(mode, canonical=True).todense(), A_.todense())


def test_canonical_materialisation_over_the_long_side_takes_several_chunk_groups(be):
    """Column-owned walk over 300 rows with chunks a quarter of shape[1] = 20 wide: 60 chunks, 8 walker groups."""
    shape = (300, 20)
    M = be.JITCNormalR((*PARAMS['n'], 0.3, 5), shape=shape, corder=False)
    A_ = M.materialize('mv', canonical=True)
    assert isinstance(A_, be.CSC)
    idx, ptr = A_.indices.cpu().numpy().astype(np.int64), A_.indptr.cpu().numpy().astype(np.int64)
    owner = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    assert np.all(np.diff(idx)[owner[1:] == owner[:-1]] > 0)
    np.testing.assert_array_equal(A_.todense(), M.materialize('mv').todense())
    np.testing.assert_allclose(A_.todense(), _dense('n', 0.3, 5, shape, False, False), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ 4. window and chunk edges
WIDTHS = [4 * (2 * W + 777) + 3,      # every chunk spans three windows, the last chunk is ragged
          W + 1, 3, 31, 33]


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
@pytest.mark.parametrize('width', WIDTHS)
def test_window_and_chunk_edges(be, family, width):
    shape, prob, seed = (5, width), 0.01, 7
    M = _matrix(be, family, 'R', shape, prob, seed, True)
    for by_row in (True, False):
        y = _y(shape[0] if by_row else shape[1], 3)
        want, rows, cols = _expected(family, prob, seed, shape, False, True, y, by_row)
        got = (M.dt2t if by_row else M.dt2t_transposed)(y, None)
        _close(got, want, family)
    S = M.materialize('mv', canonical=True)
    np.testing.assert_array_equal(S.indices.cpu().numpy(), cols.astype(np.int32))
    np.testing.assert_array_equal(S.indptr.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=5))]))
    if width > W:
        chunk = (width + 3) // 4
        assert np.any(cols >= 3 * chunk) and rows.size > 1000       # the last, short chunk is populated


@pytest.mark.parametrize('width', [3, 31, 33])
def test_narrow_walks_with_many_entries(be, width):
    """The narrow widths again at a density where they hold entries (at prob 0.01 most of their rows are empty): a walk
    narrower than the lane stride, and shape[1] < 4 (chunks one column wide)."""
    shape, prob, seed = (5, width), 0.5, 7
    M = _matrix(be, 'n', 'R', shape, prob, seed, True)
    for by_row in (True, False):
        y = _y(shape[0] if by_row else shape[1], 3)
        want, rows, cols = _expected('n', prob, seed, shape, False, True, y, by_row)
        assert rows.size >= 3
        _close((M.dt2t if by_row else M.dt2t_transposed)(y, None), want, 'n')
    np.testing.assert_array_equal(M.materialize('mv', canonical=True).indices.cpu().numpy(), cols.astype(np.int32))


# ------------------------------------------------------------------------------------------------ 5. degenerate rows
@pytest.mark.parametrize('family', ['s', 'n'])
def test_mostly_empty_rows(be, family):
    shape, prob, seed = (300, 300), 1e-4, 2
    counts = np.count_nonzero(_dense('s', prob, seed, shape, False, True), axis=1)
    assert counts[0] == 0 and counts[-1] == 0 and counts.sum() >= 3 and np.count_nonzero(counts) < 30
    M = _matrix(be, family, 'R', shape, prob, seed, True)
    for by_row in (True, False):
        y = _y(300, 4)
        want, _, cols = _expected(family, prob, seed, shape, False, True, y, by_row)
        _close((M.dt2t if by_row else M.dt2t_transposed)(y, None), want, family)
    S = M.materialize('mv', canonical=True)
    np.testing.assert_array_equal(np.diff(S.indptr.cpu().numpy()), counts)
    np.testing.assert_array_equal(S.indices.cpu().numpy(), cols.astype(np.int32))


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
@pytest.mark.parametrize('shape, prob', [((1, 200), 0.1), ((9, 70), 1.0)])
def test_single_row_and_full_matrix(be, family, shape, prob):
    seed = 11
    f = getattr(be, f'jit{family}mv_dt2t')
    for corder in (True, False):
        for transpose in (False, True):
            y = _y(shape[1] if transpose else shape[0], 5)
            want, rows, _ = _expected(family, prob, seed, shape, False, corder, y, not transpose)
            if prob == 1.0:
                assert rows.size == shape[0] * shape[1]
            _close(f(*PARAMS[family], prob, y, seed, shape=shape, transpose=transpose, corder=corder), want, family)


@pytest.mark.parametrize('corder', [False, True])
def test_prob_zero_on_the_device(be, corder):
    y = torch.ones(7, device='cuda')
    r = be.jitnmv_dt2t(*PARAMS['n'], 0.0, y, 3, shape=(7, 9), corder=corder)
    assert isinstance(r, torch.Tensor) and r.is_cuda and r.shape == (0,) and r.dtype == torch.float32
    M = be.JITCUniformR((*PARAMS['u'], 0.0, 3), shape=(7, 9), corder=corder)
    assert M.dt2t(y).shape == (0,)
    out = torch.empty(0, device='cuda')
    assert M.dt2t(y, out=out) is out
    assert M.materialize('mv', canonical=True).nse == 0


# ------------------------------------------------------------------------------------------------ 6. more rows than one grid pass
def test_more_rows_than_one_grid_pass(be):
    """CAP + 1000 owner rows: the rows beyond the grid are taken in a second pass of the same workgroups.  The oracle's Python
    walk takes over 4 s at this size, so the expectation is built on the device from the UNSORTED fill (be_jitc_csr_fill, which
    the oracle checks elsewhere): its entries sorted by (row, column), its weights moved along, times y."""
    shape, prob, seed = (CAP + 1000, 40), 0.1, 17
    M = _matrix(be, 'n', 'R', shape, prob, seed, True, tensors=True)
    U = M.materialize('mv')
    ptr, idx = U.indptr.to(torch.int64), U.indices.to(torch.int64)
    counts = ptr[1:] - ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(shape[0], device=ptr.device), counts)
    order = torch.argsort(rows * shape[1] + idx)
    cols, w = idx[order], U.data[order]
    assert abs(idx.numel() - shape[0] * shape[1] * prob) < 6 * np.sqrt(shape[0] * shape[1] * prob)
    assert int(counts[CAP:].sum()) > 1000                                     # the second pass has entries to place
    for by_row in (True, False):
        y = torch.from_numpy(_y(shape[0] if by_row else shape[1], 6)).cuda()
        got = (M.dt2t if by_row else M.dt2t_transposed)(y, None)
        np.testing.assert_array_equal(got.cpu().numpy(), (w * y[rows if by_row else cols]).cpu().numpy())
    S = M.materialize('mv', canonical=True)
    np.testing.assert_array_equal(S.indices.cpu().numpy(), cols.to(torch.int32).cpu().numpy())
    np.testing.assert_array_equal(S.data.cpu().numpy(), w.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 7. out=, the cache
@pytest.mark.parametrize('corder', [False, True])
def test_out_is_written_in_place_and_aliasing_y_is_rejected(be, corder):
    shape, prob, seed = (37, 52), 0.2, 13
    M = _matrix(be, 'u', 'R', shape, prob, seed, corder)
    y = _y(shape[0], 8)
    want, rows, _ = _expected('u', prob, seed, shape, False, corder, y, True)
    out = torch.full((rows.size,), -1.0, device='cuda')
    assert M.dt2t(y, None, out=out) is out
    _close(out.cpu().numpy(), want, 'u')
    out2 = torch.full((rows.size,), -1.0, device='cuda')
    assert be.jitumv_dt2t(*PARAMS['u'], prob, y, seed, shape=shape, corder=corder, out=out2) is out2
    np.testing.assert_array_equal(out2.cpu().numpy(), out.cpu().numpy())
    with pytest.raises(ValueError, match='shape'):
        M.dt2t(y, out=torch.empty(rows.size + 1, device='cuda'))
    big = torch.ones(max(rows.size, shape[0]), device='cuda')
    with pytest.raises(ValueError, match='alias'):
        M.dt2t(big[:shape[0]], out=big[:rows.size])


def test_the_cached_offsets_skip_the_count_walk_and_do_not_follow_the_transpose(be, monkeypatch):
    shape, prob, seed = (37, 52), 0.2, 13
    M = _matrix(be, 'n', 'R', shape, prob, seed, True)
    seen = []
    real = _jitc.fn
    monkeypatch.setattr(_jitc, 'fn', lambda name: (seen.append(name), real(name))[1])
    y = _y(shape[0], 9)
    first = M.dt2t(y)
    assert seen.count('be_jitc_csr_count') == 1 and seen.count('be_jitc_fill_sorted') == 1 and 'be_jitc_csr_fill' not in seen
    key = [k for k in M.buffers if str(k).startswith('materialized_')]
    assert len(key) == 1 and M.buffers[key[0]].dtype == torch.int64 and M.buffers[key[0]].numel() == shape[0] + 1
    np.testing.assert_array_equal(M.dt2t(y), first)
    assert seen.count('be_jitc_csr_count') == 1 and seen.count('be_jitc_fill_sorted') == 2
    T = M.T
    assert not [k for k in T.buffers if str(k).startswith('materialized_')]
    # M.T is the transposed matrix: y by ITS column is y by M's row, and its row-major order is M's column-major one
    want, rows, cols = _expected('n', prob, seed, shape, False, True, y, True)
    order = np.lexsort((rows, cols))
    _close(T.dt2t_transposed(y), want[order], 'n')
    assert M.prepare('mv') is M and key[0] in M.buffers                       # (prepare() keeps its own key beside it)
    np.testing.assert_array_equal(M.dt2t(y), first)
