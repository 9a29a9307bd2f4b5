"""The host side of the FP8 gather direction: the numpy restatement (tests/csr_f8_gather_cases.py) against a loop over Python ints
and against the scatter restatement of the transposed structure, the constants the GPU cases are sized by against the source
text, ``Float8CSC`` and the ``.T`` views on the host with every refusal raised before any device call (the device is barred),
and the new entry points in the ABI table."""
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _abi
from brainevent_amd import _array as A
from brainevent_amd import _csr_f8 as F
import csr_f8_cases as K
import csr_f8_gather_cases as G

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'brainevent_amd' / 'csrc'
FMTS = sorted(K.E)


@pytest.fixture
def no_device(monkeypatch):
    def barred(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(A, 'device', barred)
    monkeypatch.setattr(A, 'to_device', barred)
    monkeypatch.setattr(A, 'workspace', barred)


@pytest.mark.parametrize('fmt', FMTS)
def test_the_restatement_against_a_loop_over_python_ints(fmt):
    m, k = 23, 17
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=5)
    active = np.random.default_rng(6).random((3, k)) < 0.5
    dec = torch.from_numpy(np.arange(256, dtype=np.uint8)).view(K.DTYPE[fmt]).to(torch.float64).numpy()
    for scale in (1.0, 0.25, 0.3):
        got = G.expected_gather(codes, indices, indptr, active, fmt, scale)
        assert got.shape == (3, m) and got.dtype == np.float32
        inv = np.ldexp(np.float64(np.float32(scale)), -K.E[fmt])
        for b in range(3):
            R = [sum(int(dec[codes[e]] * 2 ** K.E[fmt]) for e in range(indptr[i], indptr[i + 1]) if active[b, indices[e]])
                 for i in range(m)]
            assert R == [int(r) for r in G.row_sums(codes, indices, indptr, active[b], fmt)]
            want = np.array([np.float32(np.float64(r) * inv) for r in R], dtype=np.float32)
            assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_row_sums_are_the_column_sums_of_the_transposed_structure(fmt, seed):
    m, k = 40 + seed, 29 - seed
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=seed)
    tc, ti, tp = G.transposed(codes, indices, indptr, k)
    assert len(tp) == k + 1 and tp[-1] == len(indices) and sorted(zip(ti.tolist(), tc.tolist())) == sorted(
        zip(np.repeat(np.arange(m), np.diff(indptr)).tolist(), codes.tolist()))
    rng = np.random.default_rng(seed)
    for p in (0.0, 0.3, 1.0):
        s = rng.random(k) < p
        assert np.array_equal(G.row_sums(codes, indices, indptr, s, fmt), K.column_sums(tc, ti, tp, s, m, fmt))
        assert np.array_equal(G.expected_gather(codes, indices, indptr, s, fmt, 0.3).view(np.uint32),
                              K.expected(tc, ti, tp, s, m, fmt, 0.3).view(np.uint32))
    # fixed rows and rows of given lengths are what they say
    c, i, p = G.fixed_rows(5, 9, 3, fmt, 1)
    assert len(c) == len(i) == 15 and list(np.diff(p)) == [3] * 5
    c, i, p = G.rows_of_lengths([0, 2, 5], 9, fmt, 1)
    assert len(c) == len(i) == 7 and list(p) == [0, 0, 2, 7]


def test_the_constants_the_gpu_cases_are_sized_by_are_the_sources():
    src = (CSRC / 'be_csr_f8_gather.hip').read_text()
    tiers = {int(l): int(a) for l, a in re.findall(r'kF8GatherLpr(\d+)MaxRow = (\d+)', src)}
    assert tiers == G.LPR_MAX_ROW
    for l in G.LPR_MAX_ROW:
        assert re.search(rf'avg <= kF8GatherLpr{l}MaxRow\) return {l};|avg <= kF8GatherLpr{l}MaxRow \? {l} : 64;', src), l
    assert 'be_dispatch_int<2, 4, 8, 16, 32, 64>(f8_gather_lpr_of(nnz / m)' in src and G.LPRS == (2, 4, 8, 16, 32, 64)
    assert [G.lpr_of(a) for a in (0, 8, 9, 20, 21, 45, 46, 100, 101, 200, 201, 10000)] == [2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert all(G.lpr_of(G.avg_for(l)) == l for l in G.LPRS)
    assert re.search(r'constexpr int kF8GatherThreads = (\d+);', src).group(1) == str(G.THREADS)
    assert re.search(r'constexpr int kF8GatherGridCap = (\d+);', src).group(1) == str(G.GRID_CAP)
    assert 'grid_for(m, kF8GatherThreads / LPR, kF8GatherGridCap)' in src
    assert re.search(r'constexpr int64_t kF8GatherLdsBitmapBytes = (\d+) \* 1024;', src).group(1) == str(G.LDS_BITMAP_BYTES // 1024)
    assert 'const bool in_lds = n_words * 4 <= kF8GatherLdsBitmapBytes;' in src
    # four consecutive entries per lane and load, QUADS passes per trip of the walk
    assert 'constexpr int PASS = 4 * LPR;' in src and 'j += kF8GatherQuads * PASS' in src and G.pass_of(16) == 64
    assert re.search(r'constexpr int kF8GatherQuads = (\d+);', src).group(1) == str(G.QUADS)
    # the mirror fill: k_t_fill's lanes per row and grid, and its one-byte payload
    conv = (CSRC / 'be_convert.hip').read_text()
    tiers = re.findall(r'if \(avg_row <= (\d+)\) return launch_fill<(\d+), PT>', conv)
    assert {int(l): int(a) for a, l in tiers} == G.FILL_LPR_MAX_ROW and 'return launch_fill<64, PT>' in conv
    assert 'grid_for(m, 256 / LPR, 256 * 16)' in conv and (G.FILL_THREADS, G.FILL_GRID_CAP) == (256, 4096)
    assert 'if (WB == 1) w_out[slot] = w_in[j];' in conv and 'case 1: BE_T_FILL(1); break;' in conv


@pytest.mark.parametrize('fmt', FMTS)
def test_float8csc_on_the_host_and_the_transpose_views(fmt, no_device):
    fc = K.finite_codes(fmt)
    cols = [([3, 0, 3], fc[[1, 2, 3]]), ([], []), ([5], fc[[200]])]          # three stored columns over six row ids
    codes, indices, indptr = K.from_rows(cols, 6)
    W = be.Float8CSC((codes, indices, indptr), shape=(6, 3), scale=0.5, fmt=fmt)
    assert W.fmt == fmt and W.dtype == K.DTYPE[fmt] and W.shape == (6, 3) and W.nse == 4 and W.scale == 0.5 and W.ndim == 2
    assert 'Float8CSC' in repr(W) and fmt in repr(W) and 'shape=(6, 3)' in repr(W)
    dec = torch.from_numpy(codes.copy()).view(K.DTYPE[fmt]).float().numpy() * np.float32(0.5)
    dense = np.zeros((6, 3), np.float32)
    np.add.at(dense, (indices, [0, 0, 0, 2]), dec)
    assert isinstance(W.todense(), np.ndarray) and np.array_equal(W.todense(), dense)
    # .T: the other view over the very same arrays and state; .T.T: the original type and shape
    R = W.T
    assert type(R) is be.Float8CSR and R.shape == (3, 6) and np.array_equal(R.todense(), dense.T)
    assert R.codes is W.codes and R.indices is W.indices and R.indptr is W.indptr and R._rows is W._rows
    assert R.scale == W.scale and R.fmt == W.fmt and R.nse == W.nse
    assert type(R.T) is be.Float8CSC and R.T.shape == (6, 3) and R.T._rows is W._rows and type(W.transpose()) is be.Float8CSR
    S = be.Float8CSR((codes, indices, indptr), shape=(3, 6), scale=0.5, fmt=fmt)
    assert type(S.T) is be.Float8CSC and S.T.shape == (6, 3) and S.T.codes is S.codes and type(S.T.T) is be.Float8CSR
    assert S.T.T.shape == (3, 6) and np.array_equal(S.T.todense(), dense)
    Wt = be.Float8CSC((torch.from_numpy(codes.copy()).view(K.DTYPE[fmt]), torch.from_numpy(indices), torch.from_numpy(indptr).long()),
                      shape=(6, 3))
    assert Wt.scale == 1.0 and Wt.fmt == fmt and isinstance(Wt.todense(), torch.Tensor)
    assert W._plan is None and W._mirror is None and hasattr(W, 'build_mirror') and hasattr(W, 'tocsc') and not hasattr(W, 'tocsr')
    assert hasattr(be.CSC, 'quantize_fp8')


def test_float8csc_refusals(no_device):
    codes, indices, indptr = K.from_rows([([1, 2], [8, 9]), ([0], [16])], 6)
    mk = lambda **kw: be.Float8CSC((codes, indices, indptr), **{'shape': (6, 2), 'fmt': 'e4m3', **kw})
    W = mk()
    x = np.ones(2, dtype=np.float32)
    with pytest.raises(TypeError, match=r'Float8CSC multiplies event operands only.*tocsc\(\)'):
        W @ x
    with pytest.raises(TypeError, match=r'event operands only.*tocsc\(\)'):
        W.__rmatmul__(np.ones(6, dtype=np.float32))
    with pytest.raises(TypeError, match=r'event operands only.*tocsc\(\)'):
        torch.ones(3, 6) @ W
    for op in (lambda: W + 1, lambda: 1 + W, lambda: W - W, lambda: W * 2.0, lambda: 2.0 * W, lambda: W / 2, lambda: -W, lambda: abs(W),
               lambda: W ** 2, lambda: W[0], lambda: W.slice_rows([0]), lambda: W.solve(x), lambda: W.update_on_pre(x, x),
               lambda: W.update_on_post(x, x), lambda: W.update_on_binary_pre(x, x), lambda: W.update_on_binary_post(x, x),
               lambda: W.diag_add(x), lambda: W.with_data(x)):
        with pytest.raises(TypeError, match=r'Float8CSC is read-only.*tocsc\(\) gives the f32 CSC back'):
            op()
    # shapes and gradients are checked before the device is asked for, in both directions
    with pytest.raises(ValueError, match='not aligned'):
        W @ be.BinaryArray(np.ones(6, dtype=bool))                       # the scatter takes k = 2 events
    with pytest.raises(ValueError, match='not aligned'):
        be.BinaryArray(np.ones(2, dtype=bool)) @ W                       # the gather takes m = 6
    with pytest.raises(ValueError, match='not aligned'):
        be.BinaryArray(np.ones((3, 5), dtype=bool)) @ W
    with pytest.raises(ValueError, match='not aligned'):
        W @ be.BinaryArray(np.ones((3, 5), dtype=bool))
    with pytest.raises(TypeError, match='no gradients'):
        be.BinaryArray(torch.ones(6, requires_grad=True)) @ W
    with pytest.raises(TypeError, match='no gradients'):
        W @ be.BinaryArray(torch.ones(2, requires_grad=True))
    # construction: Float8CSR's checks, over the columns
    with pytest.raises(ValueError, match="fmt='e4m3' or fmt='e5m2'"):
        mk(fmt=None)
    with pytest.raises(ValueError, match='does not match'):
        be.Float8CSC((torch.zeros(3).to(torch.float8_e5m2), indices, indptr), shape=(6, 2), fmt='e4m3')
    with pytest.raises(TypeError, match=r'Float8CSC takes.*uint8 codes.*CSC\.quantize_fp8'):
        be.Float8CSC((np.zeros(3, dtype=np.float32), indices, indptr), shape=(6, 2), fmt='e4m3')
    with pytest.raises(ValueError, match='one-dimensional'):
        be.Float8CSC((np.zeros((3, 1), dtype=np.uint8), indices, indptr), shape=(6, 2), fmt='e4m3')
    with pytest.raises(ValueError, match='3 indices'):
        be.Float8CSC((np.zeros(2, dtype=np.uint8), indices, indptr), shape=(6, 2), fmt='e4m3')
    with pytest.raises(ValueError, match='finite'):
        mk(scale=float('inf'))
    with pytest.raises(TypeError, match='requires grad'):
        mk(scale=torch.ones((), requires_grad=True))
    with pytest.raises(ValueError, match='out of bounds'):
        mk(shape=(2, 2))                                                  # row id 2 in a matrix of 2 rows
    with pytest.raises(ValueError, match='indptr length'):
        mk(shape=(6, 3))
    with pytest.raises(TypeError, match='integer'):
        be.Float8CSC((codes, indices.astype(np.float32), indptr), shape=(6, 2), fmt='e4m3')
    bad = codes.copy()
    bad[1] = 0x7f
    with pytest.raises(ValueError, match='non-finite'):
        be.Float8CSC((bad, indices, indptr), shape=(6, 2), fmt='e4m3')


def test_float8csr_matmul_events_still_raises_and_names_the_transpose(no_device):
    codes, indices, indptr = K.from_rows([([1, 2], [8, 9]), ([0], [16])], 6)
    W = be.Float8CSR((codes, indices, indptr), shape=(2, 6), fmt='e4m3')
    with pytest.raises(NotImplementedError, match=r'gather direction, W8 @ events.*events @ W8\.T'):
        W @ be.BinaryArray(np.ones(6, dtype=bool))
    with pytest.raises(TypeError, match=r'event operands only.*tocsr\(\)'):
        W @ np.ones(6, dtype=np.float32)
    # the spelling that is built takes the k inputs of the gather
    with pytest.raises(ValueError, match='not aligned'):
        be.BinaryArray(np.ones(2, dtype=bool)) @ W.T


def test_csc_quantize_fp8_on_the_host(no_device):
    _, indices, indptr = K.random_matrix(7, 30, 'e4m3', seed=3)
    w = np.random.default_rng(1).standard_normal(len(indices)).astype(np.float32)
    src = types.SimpleNamespace(data=torch.from_numpy(w), indices=torch.from_numpy(indices), indptr=torch.from_numpy(indptr),
                                shape=(30, 7), nse=len(indices), _numpy_result=True)
    for fmt in FMTS:
        Q, R = F.csc_quantize_fp8(src, fmt), F.csr_quantize_fp8(types.SimpleNamespace(**{**vars(src), 'shape': (7, 30)}), fmt)
        assert type(Q) is be.Float8CSC and Q.shape == (30, 7) and Q.scale == R.scale and Q.fmt == fmt
        assert torch.equal(Q.codes.view(torch.uint8), R.codes.view(torch.uint8))
        assert Q.indices.data_ptr() == src.indices.data_ptr() and Q.indptr.data_ptr() == src.indptr.data_ptr()
        assert np.array_equal(Q.todense(), R.todense().T)


def test_the_new_entry_points_are_in_the_abi_table_and_the_header():
    header = (ROOT / 'include' / 'brainevent_amd.h').read_text()
    table = _abi._SIGNATURES
    names = ('be_binary_csrmv_nt_f8_workspace_bytes', 'be_binary_csrmm_nt_f8_workspace_bytes', 'be_binary_csrmv_nt_f8',
             'be_binary_csrmm_nt_f8', 'be_csr_to_csc_fill_block_u8')
    text = (ROOT / 'brainevent_amd' / '_abi.py').read_text()
    for n in names:
        assert re.search(rf'\b{n}\(', header), n
        assert re.search(rf"\b{n}='[il]:[a-zA-Z]+'", text), n
        assert n in table and n in _abi.PROTOTYPES
    # the gather takes the scatter's arguments; the one-byte fill the fill's minus weight_bytes
    sig = lambda n: re.search(rf"\b{n}='([il]:[a-zA-Z]+)'", text).group(1)
    assert sig('be_binary_csrmm_nt_f8') == sig('be_binary_csrmm_t_f8') and sig('be_binary_csrmv_nt_f8') == sig('be_binary_csrmv_t_f8')
    full = sig('be_csr_to_csc_fill_block')
    assert sig('be_csr_to_csc_fill_block_u8') == full[:-3] + full[-2:]
    assert 'Gather direction' in header and 'be_csr_to_csc_fill_block_u8:' in header
