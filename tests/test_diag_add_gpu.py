"""diag_add on the device (brainevent_amd/_diag.py, csrc/be_arith.hip: be_diag_scan / be_diag_move / be_diag_fill) against the
numpy restatement of the rule in tests/test_diag_add_cpu.py, exactly: structure arrays as integers, values on integer-valued
weights (every sum exact in every dtype).

Sizes come from CONSTS, the geometry of csrc/be_arith.hip (tests/test_diag_add_cpu.py compares the table with the source): a
tile is `tile` consecutive entries; a lane of the scan kernel owns `scan_per` consecutive ones.  The int64 path beyond 2^31
entries is not run here; its dtype decision is a host function (tests/test_diag_add_cpu.py)."""
import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd._diag import DiagPlan

pytestmark = pytest.mark.gpu

CONSTS = {'threads': 256, 'tile': 2048, 'grid_cap': 4096, 'scan_per': 8}
T = CONSTS['tile']
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]

from test_diag_add_cpu import diag_rule, diag_values          # noqa: E402  (after CONSTS: that module reads it lazily)


def dev(x):
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to('cuda')


def host(t):
    t = t.detach().cpu()
    return (t.double() if t.dtype.is_floating_point else t).numpy()


def structure(rng, lens, n_cols, ptr_dtype=np.int32, sort=False):
    indptr = np.zeros(len(lens) + 1, dtype=ptr_dtype)
    np.cumsum(lens, out=indptr[1:])
    indices = rng.integers(0, n_cols, int(indptr[-1])).astype(np.int32)          # unsorted, with duplicates
    if sort:
        for r in range(len(lens)):
            indices[indptr[r]:indptr[r + 1]].sort()
    return indptr, indices


def check(indptr, indices, shape, dtype=torch.float32, shared=False, cls=be.CSR, positions=True):
    """M.diag_add(d) and csr_diag_position on one structure against the rule; returns (M, result)."""
    rng = np.random.default_rng(len(indices))
    n_diag = min(shape)
    w = np.array([3.0]) if shared else rng.integers(-8, 9, len(indices)).astype(np.float64)
    d = rng.integers(-8, 9, n_diag).astype(np.float64)
    want = diag_rule(indptr, indices, n_diag)
    M = cls((dev(w).to(dtype), dev(indices), dev(indptr)), shape=shape,
            indptr_dtype=torch.int64 if indptr.dtype == np.int64 else torch.int32)
    R = M.diag_add(dev(d).to(dtype))
    assert type(R) is cls and R.shape == M.shape and R.data.dtype == dtype and R.indices.dtype == torch.int32
    assert R.indptr.dtype == M.indptr.dtype
    np.testing.assert_array_equal(host(R.indptr), want[0])
    np.testing.assert_array_equal(host(R.indices), want[1])
    np.testing.assert_array_equal(host(R.data), diag_values(w, d, want))
    plan = M.buffers['diag_positions']
    assert isinstance(plan, DiagPlan) and plan.new_indices is R.indices and plan.new_indptr is R.indptr
    np.testing.assert_array_equal(host(plan.diag_dest), want[3])
    if positions:
        got = be.csr_diag_position(dev(indptr), dev(indices), shape=shape if cls is be.CSR else shape[::-1])
        for g, wnt in zip(got, want):
            assert g.dtype == (torch.int32 if wnt.dtype == np.int32 else M.indptr.dtype)
            np.testing.assert_array_equal(host(g), wnt)
        if not shared:
            nd = be.csr_diag_add(M.data, got, dev(d).to(dtype))
            assert nd.dtype == dtype
            np.testing.assert_array_equal(host(nd), host(R.data))
    return M, R


# ------------------------------------------------------------------------------------------------ the rule, small
def test_the_reference_docstring_example():
    indptr, indices = np.array([0, 1, 2, 4], np.int32), np.array([0, 2, 0, 2], np.int32)
    M = be.CSR((dev(np.ones(4, np.float32)), dev(indices), dev(indptr)), shape=(3, 3))
    R = M.diag_add(dev(np.array([0.1, 0.2, 0.3], np.float32)))
    assert R.indptr.tolist() == [0, 1, 3, 5] and R.indices.tolist() == [0, 1, 2, 0, 2]
    np.testing.assert_array_equal(host(R.data), np.array([1.1, .2, 1, 1, 1.3], np.float32).astype(np.float64))
    pos = be.csr_diag_position(indptr, indices, shape=(3, 3))
    assert all(isinstance(p, np.ndarray) for p in pos)                             # numpy in, numpy out
    assert pos[2].tolist() == [0, 2, 3, 4] and pos[3].tolist() == [0, 1, 4]
    nd = be.csr_diag_add(np.ones(4, np.float32), pos, np.array([0.1, 0.2, 0.3], np.float32))
    np.testing.assert_array_equal(nd, np.array([1.1, .2, 1, 1, 1.3], np.float32))


SMALL = {
    'all present': lambda rng: (np.arange(8, dtype=np.int32), np.arange(7, dtype=np.int32), (7, 7)),
    'all missing': lambda rng: (np.arange(8, dtype=np.int32), ((np.arange(7) + 3) % 7).astype(np.int32), (7, 7)),
    'nothing stored': lambda rng: (np.zeros(8, np.int32), np.zeros(0, np.int32), (7, 7)),
    'mixed, unsorted, duplicates, empty rows': lambda rng: structure(rng, rng.integers(0, 9, 23) * (rng.random(23) < 0.8), 9) + ((23, 9),),
    'mixed, sorted': lambda rng: structure(rng, rng.integers(0, 9, 23), 23, sort=True) + ((23, 23),),
    'more columns than rows': lambda rng: structure(rng, rng.integers(0, 6, 11), 40) + ((11, 40),),
    'more rows than columns': lambda rng: structure(rng, rng.integers(0, 6, 40), 11) + ((40, 11),),
    'duplicate diagonals': lambda rng: (np.array([0, 4, 7, 7], np.int32), np.array([0, 2, 0, 0, 1, 1, 0], np.int32), (3, 3)),
}


@pytest.mark.parametrize('ptr_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('case', sorted(SMALL))
def test_small_structures(case, ptr_dtype):
    indptr, indices, shape = SMALL[case](np.random.default_rng(sorted(SMALL).index(case)))
    check(indptr.astype(ptr_dtype), indices, shape)


def test_the_last_duplicate_receives_the_addend():
    indptr, indices, shape = SMALL['duplicate diagonals'](None)
    M = be.CSR((dev(np.arange(1, 8, dtype=np.float32)), dev(indices), dev(indptr)), shape=shape)
    R = M.diag_add(dev(np.array([10, 20, 30], np.float32)))
    assert R.indices.tolist() == [0, 2, 0, 0, 1, 1, 0, 2]
    assert R.data.tolist() == [1, 2, 3, 14, 5, 26, 7, 30]


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shared', [False, True])
def test_every_dtype_and_a_shared_weight(dtype, shared):
    rng = np.random.default_rng(5)
    indptr, indices = structure(rng, rng.integers(0, 9, 31), 31)
    M, R = check(indptr, indices, (31, 31), dtype=dtype, shared=shared, positions=False)
    assert R.data.numel() == R.indices.numel()                                     # a shared weight is expanded


# ------------------------------------------------------------------------------------------------ tile boundaries
def _lens_summing_to(rng, n_rows, total):
    cuts = np.sort(rng.integers(0, total + 1, n_rows - 1))
    return np.diff(np.concatenate([[0], cuts, [total]]))


def _long_row(rng):
    """a row of more than two tiles whose insertion point falls in the second tile: indices below the diagonal first"""
    indptr = np.array([0, 2, 2 + 2 * T + 9, 2 * T + 14], np.int32)
    indices = rng.integers(0, 3, 2 * T + 14).astype(np.int32)
    row = indices[2:2 + 2 * T + 9]
    row[:] = 0
    row[T + 77:] = rng.choice([0, 2], len(row) - T - 77)
    row[T + 77] = 2
    return indptr, indices, (3, 3)


TILES = {
    'tile-1': lambda rng: structure(rng, _lens_summing_to(rng, 41, T - 1), 41) + ((41, 41),),
    'tile': lambda rng: structure(rng, _lens_summing_to(rng, 41, T), 41) + ((41, 41),),
    'tile+1': lambda rng: structure(rng, _lens_summing_to(rng, 41, T + 1), 41) + ((41, 41),),
    'a long row, insertion in its second tile': _long_row,
    'runs of empty rows': lambda rng: structure(rng, np.array([0] * (T + 3) + [5, 7] + [0] * (T + 3) + [4] + [0] * (T + 3)),
                                                3 * T + 12) + ((3 * T + 12, 3 * T + 12),),
    'rows cut by the lanes of the scan': lambda rng: structure(rng, rng.integers(0, 3 * CONSTS['scan_per'], 300), 300) + ((300, 300),),
}


@pytest.mark.parametrize('ptr_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('case', sorted(TILES))
def test_tile_boundaries(case, ptr_dtype):
    indptr, indices, shape = TILES[case](np.random.default_rng(100 + sorted(TILES).index(case)))
    check(indptr.astype(ptr_dtype), indices, shape)


def test_past_the_grid_cap():
    """grid_cap + 2 tiles and a partial one: 4095 rows of one length over 4095 columns; the rule vectorised in torch (every
    row's indices ascend, so the insertion point is a count) — the loop of the rule itself is held to it at a small size."""
    n = 4095
    k = ((CONSTS['grid_cap'] + 2) * T) // n + 1
    assert n * k > (CONSTS['grid_cap'] + 2) * T and (n * k) % T != 0
    g = torch.Generator(device='cuda').manual_seed(3)
    cols = torch.sort(torch.randint(0, n, (n, k), device='cuda', generator=g), dim=1).values.to(torch.int32)
    for size in (64, n):
        c = (cols[:size, :k] % size).sort(dim=1).values.to(torch.int32).contiguous()
        w = torch.randint(-8, 9, (size * k,), device='cuda', generator=g).float()
        d = torch.randint(-8, 9, (size,), device='cuda', generator=g).float()
        indptr = (torch.arange(size + 1, device='cuda') * k).to(torch.int32)
        M = be.CSR((w, c.reshape(-1), indptr), shape=(size, size), check_structure=False)
        R = M.diag_add(d)
        i = torch.arange(size, device='cuda')[:, None]
        missing = ~(c == i).any(dim=1)
        before = (c < i).sum(dim=1)                                                   # where a missing diagonal goes
        last = k - 1 - torch.flip(c == i, dims=[1]).int().argmax(dim=1)               # the last stored copy
        shift = torch.cumsum(missing.long(), 0) - missing.long()
        e = torch.arange(size * k, device='cuda').reshape(size, k)
        o2n = e + shift[:, None] + (missing[:, None] & (torch.arange(k, device='cuda')[None] >= before[:, None])).long()
        dest = torch.where(missing, i[:, 0] * k + before, i[:, 0] * k + last) + shift
        new_nse = size * k + int(missing.sum())
        want_idx = torch.empty(new_nse, dtype=torch.int32, device='cuda')
        want_idx[o2n.reshape(-1)] = c.reshape(-1)
        want_idx[dest[missing]] = i[:, 0][missing].int()
        want = torch.zeros(new_nse, device='cuda')
        want[o2n.reshape(-1)] = w
        want[dest] += d
        assert torch.equal(R.indices, want_idx) and torch.equal(R.data, want)
        assert torch.equal(R.indptr.long(), indptr.long() + torch.cat([shift, shift[-1:] + missing[-1:].long()]))
        if size == 64:
            rule = diag_rule(host(indptr), host(c.reshape(-1)), size)
            np.testing.assert_array_equal(host(R.indices), rule[1])
            np.testing.assert_array_equal(host(R.data), diag_values(host(w), host(d), rule))


# ------------------------------------------------------------------------------------------------ containers
@pytest.mark.parametrize('cls', [be.CSR, be.CSC], ids=lambda c: c.__name__)
@pytest.mark.parametrize('shape', [(37, 53), (53, 37), (41, 41)])
def test_the_dense_truth(cls, shape):
    rng = np.random.default_rng(9)
    mat = (rng.integers(-8, 9, shape) * (rng.random(shape) < 0.2)).astype(np.float32)
    d = rng.integers(-8, 9, min(shape)).astype(np.float32)
    want = mat.copy()
    want[np.arange(len(d)), np.arange(len(d))] += d
    for src in (dev(mat), mat):
        M = cls.fromdense(src)
        R = M.diag_add(dev(d) if isinstance(src, torch.Tensor) else d)
        assert type(R) is cls and R._numpy_result == M._numpy_result
        np.testing.assert_array_equal(R.todense(), want)
        assert R.nse == M.nse + int((np.diagonal(mat) == 0).sum())
        np.testing.assert_array_equal(M.todense(), mat)
    # ... and the result multiplies like any other matrix
    R = cls.fromdense(dev(mat)).diag_add(dev(d))
    spk = be.BinaryArray(dev(rng.random(shape[0]) < 0.5))
    np.testing.assert_array_equal((spk @ R).cpu().numpy(), (spk @ cls.fromdense(dev(want))).cpu().numpy())


def test_two_runs_give_identical_bytes():
    rng = np.random.default_rng(10)
    indptr, indices = structure(rng, rng.integers(0, 40, 300), 300)
    w, d = dev(rng.random(len(indices)).astype(np.float32)), dev(rng.random(300).astype(np.float32))
    runs = []
    for _ in range(2):
        R = be.CSR((w, dev(indices), dev(indptr)), shape=(300, 300)).diag_add(d)
        runs.append((R.indptr.cpu().numpy().tobytes(), R.indices.cpu().numpy().tobytes(), R.data.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


def test_the_plan_is_cached_and_the_result_carries_its_own():
    rng = np.random.default_rng(11)
    indptr, indices = structure(rng, rng.integers(0, 9, 50), 50)
    M = be.CSR((dev(rng.integers(-8, 9, len(indices)).astype(np.float32)), dev(indices), dev(indptr)), shape=(50, 50))
    d = dev(rng.integers(-8, 9, 50).astype(np.float32))
    R1 = M.diag_add(d)
    plan = M.buffers['diag_positions']
    R2 = M.diag_add(d)
    assert M.buffers['diag_positions'] is plan and R2.indices is R1.indices and R2.indptr is R1.indptr
    assert torch.equal(R1.data, R2.data)
    own = R1.buffers['diag_positions']
    assert isinstance(own, DiagPlan) and own is plan.result_plan and own.new_indices is R1.indices
    S1 = R1.diag_add(d)                                          # no scan: the plan it came with, unchanged
    assert R1.buffers['diag_positions'] is own and S1.buffers['diag_positions'] is own
    assert S1.indices is R1.indices and S1.indptr is R1.indptr and S1.nse == R1.nse
    np.testing.assert_array_equal(S1.todense(), M.todense() + 2 * np.diag(host(d)).astype(np.float32))
    pos = own.positions()
    assert torch.equal(pos[2], torch.arange(R1.nse, device='cuda', dtype=pos[2].dtype)) and pos[3] is plan.diag_dest
    step = be.capture_step(lambda: M.diag_add(d))              # a call on the cached plan syncs nothing: it captures
    S2 = step()
    torch.cuda.synchronize()
    assert torch.equal(S2.data, R1.data)
