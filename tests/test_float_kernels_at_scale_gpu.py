"""The float-operand twins (csrc/be_float.hip: csrmv / csrmm / fcnmv / fcnmm; csrc/be_jitc_float.hip: jit{s,u,n}{mv,mm}) past
their one-pass sizes and in all four dtypes: every grid-stride loop, column tile, LDS piece and tail branch of the two files
is crossed by a named case and compared with a float64 reference (oracle_np for CSR / FCN, oracle_c.jit_float for JIT, both
pinned by tests/test_oracle.py).

Exact data, exact comparison: where the caller supplies the weights (CSR, FCN, JIT scalar) they are integers in [-8, 8] and
the operand integers in [-4, 4] with about 20 % zeros.  Every partial sum is then an integer below 2**24 (asserted per case
from the reference), exact in f32 in any order — float atomics, LDS fixed point and lane shuffles are all deterministic — and
the result must EQUAL the reference rounded once to the output dtype.  The generated-weight families (uniform, normal) are
compared under an error bound derived from the kernels' arithmetic in `jit_bound`; each case asserts on the host that its bound
is at most a quarter of the smallest non-zero addend, so a lost or doubled addend cannot hide in it.  Every case first asserts,
from the CONSTS table (tests/test_float_kernels_thresholds_cpu.py compares it with the sources), that its sizes cross the
loop bound it is there for; the JIT scatter cases also assert which C entry point served them.

Which loop or branch is reached where:
  k_fcsrmv_nt / k_fcsrmv_t row loop, LPR 4 / 16 / 64, grid at its cap     test_csr_row_loops_past_the_grid_cap, test_fcn_row_loops_past_the_grid_cap
  k_fcsrmm_nt / k_fcsrmm_t row loop, every CPG, partial / three tiles      test_mm_rows_past_the_grid_cap_all_widths_all_dtypes
  f64 / f16 / bf16 operands (Vec4 loads, f32 image)                        test_mm_rows_past_the_grid_cap_all_widths_all_dtypes, test_tails_and_alignment
  k_img_round stride loop (k * n > 524 288), mv and mm                     test_half_precision_image_round_loop
  load_group tail branch, nnz % 4, row starts mod 4, short straddling rows test_tails_and_alignment
  one row of 200 000 entries under each lane variant                       test_one_long_row_among_empty_rows
  masked entries read operand row 0                                        test_masked_entries_do_not_leak_operand_row_0
  nothing outside an aligned view is read                                  test_views_into_larger_buffers
  +inf reaches exactly the outputs that reference it                       test_infinite_operand_value_reaches_exactly_its_outputs
  random structures around every bound                                     test_random_structures
  k_jit_f_gather row loop, stride 32                                       test_jit_gather_mv_row_loop
  k_jit_f_gather row loop stride 4, kTile passes, k_jit_f_gather_reduce    test_jit_gather_mm_row_loop_and_tiles
  k_jit_f_scatter task loop (f64, forced f32), k_jit_f_round loop          test_jit_atomic_scatter_task_loop, test_jit_atomic_scatter_half_precision_round_loop
  k_jit_f_scatter task index beyond 2**32                                  test_jit_atomic_scatter_above_2_32_tasks
  k_jit_f_scatter_lds, ONE_PIECE = false, mv and mm                        test_jit_lds_scatter_several_pieces
  hundreds of chunks / one chunk narrower than the lane stride             test_jit_chunk_geometry
  gridDim.y = n_chunks above the device's limit                            test_jit_refuses_more_chunks_than_grid_rows
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from brainevent_amd import _jitc as J
from brainevent_amd._error import KernelExecutionError
from brainevent_amd._lib import fn as lib_fn
from oracle import oracle_c

pytestmark = pytest.mark.gpu

# The loop bounds of the two kernel files as the cases below use them, with where they stand in the sources.
CONSTS = {
    'float.grid_cap': 256 * 16,        # grid_for(m, rows per block, 256 * 16): be_float.hip:210, :214, :225, :229
    'float.mm_rows_per_block': 4,      # csrmm: a wave per row, four waves: be_float.hip:214, :229 (mv: 256 / LPR rows, :210, :225)
    'float.avg_short': 24,             # nnz // m <= 24: 4 lanes per row: be_float.hip:211, :226
    'float.avg_medium': 160,           # nnz // m <= 160: 16 lanes per row, above: 64: be_float.hip:211, :226
    'float.round_grid_cap': 2048,      # k_img_round: grid_for(k * n, 256, 2048): be_float.hip:236
    'jit.kTile': 8,                    # columns of a matrix operand per pass: be_jitc_float.hip:170
    'jit.gather_grid_cap': 4096,       # gcap(out_len, 256 / stride, 4096): be_jitc_float.hip:181
    'jit.reduce_grid_cap': 2048,       # k_jit_f_gather_reduce: gcap(m * NC, 256, 2048): be_jitc_float.hip:185, :193
    'jit.scatter_grid_cap': 256 * 32,  # k_jit_f_scatter: gcap(tasks, 256, 256 * 32): be_jitc_float.hip:202
    'jit.round_grid_cap': 2048,        # k_jit_f_round: gcap(out_len * n, 256, 2048): be_jitc_float.hip:213
    'jit.kPieceU64': 16384,            # LDS accumulators of one scatter workgroup: be_jitc_shared.h:237
}
K = CONSTS
LANES = (4, 16, 64)                                                        # lanes per row of the mv kernels
MV_SPAN = {lpr: K['float.grid_cap'] * (256 // lpr) for lpr in LANES}       # rows one trip of the grid covers: 262 144 / 65 536 / 16 384
MM_SPAN = K['float.grid_cap'] * K['float.mm_rows_per_block']               # 16 384
IMG_ROUND_SPAN = 256 * K['float.round_grid_cap']                           # 524 288
JIT_GATHER_SPAN = {s: K['jit.gather_grid_cap'] * (256 // s) for s in (32, 4)}      # 32 768 (mv) / 262 144 (mm) output rows
JIT_REDUCE_SPAN = 256 * K['jit.reduce_grid_cap']                           # 524 288
JIT_SCATTER_SPAN = 256 * K['jit.scatter_grid_cap']                         # 2 097 152 (row, chunk, lane) tasks
JIT_ROUND_SPAN = 256 * K['jit.round_grid_cap']                             # 524 288

DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
HALF_ULP = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
MM_WIDTHS = [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130]               # every CPG, a partly filled last tile, three tiles


def lanes_for(avg: int) -> int:
    """be_float.hip:211, :226."""
    return 4 if avg <= K['float.avg_short'] else (16 if avg <= K['float.avg_medium'] else 64)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def small_ints(rng, shape, hi, zeros=0.0):
    """float64 integers in [-hi, hi]; `zeros`: that share set to zero on top."""
    a = rng.integers(-hi, hi + 1, shape).astype(np.float64)
    if zeros:
        a[rng.random(shape) < zeros] = 0
    return a


def rounded(ref64, dtype):
    """The float64 reference rounded ONCE to the output dtype (through f32 for the 16-bit types: the kernels round an exact f32
    sum; the f32 step is exact for integers below 2**24)."""
    t = torch.from_numpy(np.ascontiguousarray(ref64))
    return t.to(dtype) if dtype == torch.float64 else t.to(torch.float32).to(dtype)


def bits(t):
    """The elements' bytes, in row-major order whatever the tensor's strides (a transposed [n, 1] result has a last stride != 1)."""
    return t.detach().cpu().reshape(-1).clone().view(torch.uint8)


def assert_exact(got, ref64, dtype, tag, finite=True):
    ref64 = np.asarray(ref64, np.float64)
    if finite:
        assert np.isfinite(ref64).all(), tag
    mag = np.abs(ref64[np.isfinite(ref64)])
    assert mag.size == 0 or float(mag.max()) < 2.0 ** 24, f'{tag}: |sum| reaches {mag.max()}: not exact in f32'
    want = rounded(ref64, dtype)
    assert isinstance(got, torch.Tensor) and got.dtype == dtype and tuple(got.shape) == tuple(want.shape), (tag, got.dtype, got.shape)
    g = got.detach().cpu()
    if not torch.equal(g, want):
        bad = torch.nonzero(~((g == want) | (torch.isnan(g) & torch.isnan(want))).reshape(-1)).reshape(-1)
        i = int(bad[0])
        raise AssertionError(f'{tag}: {bad.numel()} of {g.numel()} outputs differ; first at flat index {i}: '
                             f'got {float(g.reshape(-1)[i])}, reference {float(want.reshape(-1)[i])}')


# =========================================================================================================== CSR / FCN
def csr_from_lens(rng, lens, k, first_col=0):
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(first_col, k, int(ptr[-1])).astype(np.int32)
    return idx, ptr


def weights_for(rng, nnz, homo):
    """Integers in [-8, 8]; the shared weight is a non-zero one."""
    return np.array([-5.0]) if homo else small_ints(rng, nnz, 8)


def float_product(be, oracle, w64, idx, ptr, shape, X64, transpose, dtype, tag, ptr_dtype=np.int32, fcn_conn=None, finite=True,
                  ref=None):
    """One product on the device against the float64 oracle, exactly.  `fcn_conn`: the FCN entry points (indices [m, n_conn]);
    `ref`: the oracle's result for these very arguments when the caller already has it (it does not depend on the dtype)."""
    m, k = shape
    vec = X64.ndim == 1
    w_t, x_t = dev(w64, dtype), dev(X64, dtype)
    if fcn_conn is None:
        f = be.csrmv if vec else be.csrmm
        got = f(w_t, dev(idx, torch.int32), torch.from_numpy(ptr.astype(ptr_dtype)).cuda(), x_t, shape=shape, transpose=transpose)
    else:
        f = be.fcnmv if vec else be.fcnmm
        w2 = w_t if w_t.numel() == 1 else w_t.reshape(m, fcn_conn)
        got = f(w2, dev(idx.reshape(m, fcn_conn), torch.int32), x_t, shape=shape, transpose=transpose)
    if ref is None:
        ref = float_reference(oracle, w64, idx, ptr, shape, X64, transpose)
    assert_exact(got, ref, dtype, tag, finite=finite)
    return got


def float_reference(oracle, w64, idx, ptr, shape, X64, transpose):
    ref = (oracle.csrmv if X64.ndim == 1 else oracle.csrmm)(w64, idx, ptr, X64, shape, transpose)
    assert ref.dtype == np.float64
    return ref


def row_loop_cases(be, oracle, lens_of, k, fcn):
    """m at the cap + 1 (exactly one row on the second trip) and a little above it, for each lane variant, both directions, both
    weight modes."""
    for lpr in LANES:
        rpb = 256 // lpr
        for m in (MV_SPAN[lpr] + 1, MV_SPAN[lpr] + 3 * rpb + 5):
            rng = np.random.default_rng(1000 * lpr + m % 997)
            lens = lens_of(rng, lpr, m)
            idx, ptr = csr_from_lens(rng, lens, k)
            nnz = int(ptr[-1])
            avg = int(lens[0]) if fcn else nnz // m
            assert lanes_for(avg) == lpr, (avg, lpr)
            assert m > MV_SPAN[lpr] and -(-m // rpb) > K['float.grid_cap'], 'the row loop must take a second trip'
            if m == MV_SPAN[lpr] + 1:
                assert -(-m // rpb) == K['float.grid_cap'] + 1 and m - MV_SPAN[lpr] == 1
            for transpose in (False, True):
                x = small_ints(rng, m if transpose else k, 4, zeros=0.2)
                x[-1] = 3.0                                  # the last operand element counts (the last row when it is the input side)
                for homo in (False, True):
                    w = weights_for(rng, nnz, homo)
                    float_product(be, oracle, w, idx, ptr, (m, k), x, transpose, torch.float32,
                                  f'lpr={lpr} m={m} transpose={transpose} homo={homo}', fcn_conn=int(lens[0]) if fcn else None)


def test_csr_row_loops_past_the_grid_cap(be, oracle):
    def lens_of(rng, lpr, m):
        lo, hi = {4: (0, 6), 16: (22, 34), 64: (150, 176)}[lpr]
        lens = rng.integers(lo, hi + 1, m)
        lens[-1] = max(lens[-1], 3)                          # the row of the second trip is not empty
        return lens
    row_loop_cases(be, oracle, lens_of, k=20011, fcn=False)


def test_fcn_row_loops_past_the_grid_cap(be, oracle):
    def lens_of(rng, lpr, m):
        n_conn = {4: 3, 16: 27, 64: 161}[lpr]
        assert n_conn % 4 != 0
        return np.full(m, n_conn)
    row_loop_cases(be, oracle, lens_of, k=20011, fcn=True)


@pytest.mark.parametrize('fcn', [False, True], ids=['csr', 'fcn'])
def test_mm_rows_past_the_grid_cap_all_widths_all_dtypes(be, oracle, fcn):
    """csrmm / fcnmm with m above 16 384 rows (4 rows per block, 4096 blocks) at every column-group width, in the four dtypes, both
    directions, both weight modes; with transpose=True the 16-bit outputs at n = 130 also cross the k_img_round loop."""
    m, k = MM_SPAN + 5, 4100
    assert -(-m // K['float.mm_rows_per_block']) > K['float.grid_cap']
    rng = np.random.default_rng(77)
    lens = np.full(m, 3) if fcn else rng.integers(0, 8, m)
    lens[-1] = 3
    idx, ptr = csr_from_lens(rng, lens, k)
    nnz = int(ptr[-1])
    assert k * max(MM_WIDTHS) > IMG_ROUND_SPAN
    for n in MM_WIDTHS:
        for transpose in (False, True):
            X = small_ints(rng, (m if transpose else k, n), 4, zeros=0.2)
            X[-1, -1] = 2.0
            for homo in (False, True):
                w = weights_for(rng, nnz, homo)
                ref = float_reference(oracle, w, idx, ptr, (m, k), X, transpose)
                for dtype in DTYPES:
                    float_product(be, oracle, w, idx, ptr, (m, k), X, transpose, dtype,
                                  f'n={n} transpose={transpose} homo={homo} {dtype}', fcn_conn=3 if fcn else None, ref=ref)


def test_half_precision_image_round_loop(be, oracle):
    """f16 / bf16, transpose=True: sums run in an f32 image that k_img_round converts; k * n > 524 288 puts its grid (2048 blocks
    of 256) on a second trip.  mv (n = 1) and mm (n = 3)."""
    rng = np.random.default_rng(78)
    for n, k in ((1, IMG_ROUND_SPAN + 13), (3, IMG_ROUND_SPAN // 3 + 7)):
        assert k * n > IMG_ROUND_SPAN
        m = 6000
        lens = rng.integers(0, 40, m)
        lens[-1] = 2
        idx, ptr = csr_from_lens(rng, lens, k)
        idx[-1] = k - 1                                       # the last element of the image is written
        X = small_ints(rng, m if n == 1 else (m, n), 4, zeros=0.2)
        if n == 1:
            X[-1] = 1.0
        else:
            X[-1, :] = 1.0
        for homo in (False, True):
            w = weights_for(rng, int(ptr[-1]), homo)
            w[-1] = 7.0 if not homo else w[-1]
            for dtype in (torch.float16, torch.bfloat16):
                got = float_product(be, oracle, w, idx, ptr, (m, k), X, True, dtype, f'n={n} homo={homo} {dtype}')
                assert float(got.reshape(-1)[-1]) != 0.0


def straddling_structure(nnz_mod, avg_class):
    """Rows of length 0, 1, 2, 3, 5 and 9 starting at every residue mod 4 (so lengths 2 and 3 straddle a group of four, 0 and 1
    sit on either side of one), one long row that sets the nnz // m hint of the lane variant, and a last row cut so that
    nnz % 4 == nnz_mod: the array's last group is then read entry by entry."""
    lens = []
    pos = 0
    for r in range(4):
        for length in (0, 1, 2, 3, 5, 9):
            pad = (r - pos) % 4
            if pad:
                lens.append(pad)
                pos += pad
            assert pos % 4 == r
            lens.append(length)
            pos += length
    n_rows = len(lens) + 2
    target = {4: 0, 16: K['float.avg_short'] + 2, 64: K['float.avg_medium'] + 2}[avg_class]
    lens.append(target * n_rows)
    pos += lens[-1]
    lens.append(6 + (nnz_mod - (pos + 6)) % 4)
    lens = np.array(lens)
    assert lens.sum() % 4 == nnz_mod and lanes_for(int(lens.sum()) // len(lens)) == avg_class
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    for length in (0, 1, 2, 3):
        assert {int(s) % 4 for s, l in zip(starts, lens) if l == length} == {0, 1, 2, 3}
    return lens


def test_tails_and_alignment(be, oracle):
    """nnz % 4 in {0, 1, 2, 3} under each lane variant, all four kernels, both weight modes, int32 and int64 indptr; the other
    three dtypes (their own four-weight loads) with int32 indptr."""
    k = 53
    for avg_class in LANES:
        for nnz_mod in range(4):
            lens = straddling_structure(nnz_mod, avg_class)
            m = len(lens)
            rng = np.random.default_rng(10 * avg_class + nnz_mod)
            idx, ptr = csr_from_lens(rng, lens, k)
            for transpose in (False, True):
                rows_in = m if transpose else k
                for X in (small_ints(rng, rows_in, 4, zeros=0.2), small_ints(rng, (rows_in, 3), 4, zeros=0.2)):
                    for homo in (False, True):
                        w = weights_for(rng, int(ptr[-1]), homo)
                        if not homo:
                            w[-1] = 6.0                      # the very last entry counts
                        ref = float_reference(oracle, w, idx, ptr, (m, k), X, transpose)
                        for dtype, ptr_dtype in ((torch.float32, np.int32), (torch.float32, np.int64), (torch.float64, np.int32),
                                                 (torch.float16, np.int32), (torch.bfloat16, np.int32)):
                            float_product(be, oracle, w, idx, ptr, (m, k), X, transpose, dtype,
                                          f'lanes={avg_class} nnz%4={nnz_mod} transpose={transpose} ndim={X.ndim} homo={homo} '
                                          f'{dtype} {ptr_dtype.__name__}', ptr_dtype=ptr_dtype, ref=ref)


def test_one_long_row_among_empty_rows(be, oracle):
    """One row of 200 000 entries; the number of (nearly all empty) rows around it picks nnz // m and with it the lane variant."""
    long_len = 200_000
    for lpr, m in ((4, 10_000), (16, 2_000), (64, 1_000)):
        rng = np.random.default_rng(lpr)
        lens = np.zeros(m, np.int64)
        lens[m // 3] = long_len
        lens[[1, m - 1]] = (2, 3)
        assert lanes_for(int(lens.sum()) // m) == lpr
        k = 30_011
        idx, ptr = csr_from_lens(rng, lens, k)
        for transpose in (False, True):
            for X in (small_ints(rng, m if transpose else k, 4, zeros=0.2), small_ints(rng, (m if transpose else k, 5), 4, zeros=0.2)):
                if transpose:
                    X[m // 3] = 3.0                           # the long row is not skipped as a zero of the operand
                for homo in (False, True):
                    w = weights_for(rng, int(ptr[-1]), homo)
                    float_product(be, oracle, w, idx, ptr, (m, k), X, transpose, torch.float32,
                                  f'lanes={lpr} transpose={transpose} ndim={X.ndim} homo={homo}')


def test_masked_entries_do_not_leak_operand_row_0(be, oracle):
    """A masked entry of an aligned group reads operand row 0 (load_group).  Row 0 of the operand is NaN, no entry refers to
    column 0 and row 0 is empty, so no product may contain it: all four kernels, both weight modes, finite and exact."""
    k = 61
    for avg_class in LANES:
        lens = straddling_structure(1, avg_class)
        lens = np.concatenate([[0], lens])                    # row 0 empty: with transpose=True the operand's row 0 feeds nothing
        m = len(lens)
        rng = np.random.default_rng(avg_class + 5)
        idx, ptr = csr_from_lens(rng, lens, k, first_col=1)
        assert (idx != 0).all() and ptr[1] == 0
        for transpose in (False, True):
            rows_in = m if transpose else k
            for X in (small_ints(rng, rows_in, 4, zeros=0.2), small_ints(rng, (rows_in, 3), 4, zeros=0.2)):
                clean = X.copy()
                clean[0] = 0.0
                X[0] = np.nan
                for homo in (False, True):
                    w = weights_for(rng, int(ptr[-1]), homo)
                    ref = (oracle.csrmv if X.ndim == 1 else oracle.csrmm)(w, idx, ptr, clean, (m, k), transpose)
                    f = be.csrmv if X.ndim == 1 else be.csrmm
                    got = f(dev(w, torch.float32), dev(idx, torch.int32), dev(ptr, torch.int32), dev(X, torch.float32), shape=(m, k),
                            transpose=transpose)
                    assert bool(torch.isfinite(got).all()), (avg_class, transpose, X.ndim, homo)
                    assert_exact(got, ref, torch.float32, f'lanes={avg_class} transpose={transpose} ndim={X.ndim} homo={homo}')


def test_views_into_larger_buffers(be, oracle):
    """Weights and indices handed over as 16-byte-aligned views into larger buffers whose surroundings hold NaN weights and valid
    indices: the kernels read aligned groups of four but never outside [0, nnz) — the outputs are those of the plain arrays."""
    k = 47
    for dtype in DTYPES:
        for nnz_mod in range(4):
            lens = straddling_structure(nnz_mod, 4)
            m = len(lens)
            rng = np.random.default_rng(nnz_mod + 40)
            idx, ptr = csr_from_lens(rng, lens, k)
            nnz = int(ptr[-1])
            w = small_ints(rng, nnz, 8)
            front = 16                                        # elements: 32 bytes of f16 at the least
            w_big = torch.full((front + nnz + 16,), float('nan'), dtype=dtype, device='cuda')
            w_big[front:front + nnz] = dev(w, dtype)
            i_big = torch.ones(front + nnz + 16, dtype=torch.int32, device='cuda')
            i_big[front:front + nnz] = dev(idx, torch.int32)
            w_view, i_view = w_big[front:front + nnz], i_big[front:front + nnz]
            assert w_view.data_ptr() % 16 == 0 and i_view.data_ptr() % 16 == 0 and w_view.data_ptr() != w_big.data_ptr()
            for transpose in (False, True):
                rows_in = m if transpose else k
                for X in (small_ints(rng, rows_in, 4, zeros=0.2), small_ints(rng, (rows_in, 3), 4, zeros=0.2)):
                    f = be.csrmv if X.ndim == 1 else be.csrmm
                    got = f(w_view, i_view, dev(ptr, torch.int32), dev(X, dtype), shape=(m, k), transpose=transpose)
                    ref = (oracle.csrmv if X.ndim == 1 else oracle.csrmm)(w, idx, ptr, X, (m, k), transpose)
                    assert_exact(got, ref, dtype, f'{dtype} nnz%4={nnz_mod} transpose={transpose} ndim={X.ndim}')


def test_infinite_operand_value_reaches_exactly_its_outputs(be, oracle):
    """+inf in the operand at a place referenced by known entries of positive weight: +inf in exactly those outputs, every other
    output finite and exact (the oracle carries the same inf)."""
    rng = np.random.default_rng(91)
    m, k = 900, 700
    lens = rng.integers(0, 30, m)
    lens[[10, 500]] = (7, 12)
    idx, ptr = csr_from_lens(rng, lens, k)
    nnz = int(ptr[-1])
    row_of = np.repeat(np.arange(m), lens)
    col_hot, row_hot = 123, 500
    idx[ptr[10] + 2] = col_hot
    for homo in (False, True):
        w = np.array([4.0]) if homo else small_ints(rng, nnz, 8)
        if not homo:
            w[(idx == col_hot) | (row_of == row_hot)] = 2.0   # positive where the infinite value arrives: inf, not -inf or nan
        for n in (1, 3):
            for transpose in (False, True):
                rows_in = m if transpose else k
                X = small_ints(rng, rows_in if n == 1 else (rows_in, n), 4, zeros=0.2)
                X[row_hot if transpose else col_hot] = np.inf
                hit = np.zeros(k if transpose else m, bool)
                hit[idx[row_of == row_hot] if transpose else row_of[idx == col_hot]] = True
                assert 0 < hit.sum() < hit.size
                got = float_product(be, oracle, w, idx, ptr, (m, k), X, transpose, torch.float32,
                                    f'homo={homo} n={n} transpose={transpose}', finite=False)
                g = got.cpu().numpy().reshape(hit.size, -1)
                assert (g[hit] == np.inf).all() and np.isfinite(g[~hit]).all()


STRESS_SEEDS = int(os.environ.get('BE_STRESS_SEEDS', '10'))


@pytest.mark.parametrize('seed', range(STRESS_SEEDS))
def test_random_structures(be, oracle, seed):
    """Random m, k, row-length law, n and dtype under the same exact-data policy; m on either side of the row loop's one-trip
    span, FCN row lengths on either side of the 24 / 160 lane thresholds.  BE_STRESS_SEEDS sets how many (default 10)."""
    rng = np.random.default_rng(5000 + seed)
    fcn = bool(rng.integers(0, 2))
    n = int(rng.choice([1, 1, 1, 2, 3, 5, 8, 9, 17, 33, 65]))
    dtype = DTYPES[int(rng.integers(0, 4))]
    transpose, homo = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    lpr = int(rng.choice(LANES))
    span = MV_SPAN[lpr] if n == 1 else MM_SPAN
    m = int(span + rng.choice([-1, 0, 1, 2, int(rng.integers(3, 700))])) if rng.random() < 0.7 else int(rng.integers(1, 3000))
    k = int(rng.integers(1, 40_000))
    if fcn:
        n_conn = int(rng.choice({4: [1, 3, 23, 24], 16: [25, 27, 159, 160], 64: [161, 163]}[lpr])) if n == 1 else int(rng.integers(1, 7))
        lens = np.full(m, n_conn)
    elif n > 1:
        lens = rng.integers(0, 9, m)
    else:
        law = int(rng.integers(0, 3))
        mean = {4: 3, 16: 30, 64: 170}[lpr]
        lens = (rng.integers(0, 2 * mean + 1, m) if law == 0 else rng.geometric(1.0 / (mean + 1), m) - 1 if law == 1
                else np.where(rng.random(m) < 0.05, rng.integers(0, 40 * mean + 1, m), 0))
    idx, ptr = csr_from_lens(rng, lens, k)
    nnz = int(ptr[-1])
    X = small_ints(rng, (m if transpose else k) if n == 1 else (m if transpose else k, n), 4, zeros=0.2)
    w = weights_for(rng, nnz, homo)
    float_product(be, oracle, w, idx, ptr, (m, k), X, transpose, dtype,
                  f'seed={seed} fcn={fcn} m={m} k={k} n={n} nnz={nnz} {dtype} transpose={transpose} homo={homo}',
                  fcn_conn=int(lens[0]) if fcn else None)


# =========================================================================================================== JIT connectivity
# Weight parameters: the scalar weight an integer (exact data); uniform and normal keep every weight away from zero
# (w_low >= 0.5; loc - 6.5 * scale >= 0.5, 6.5 being the library's own bound on |normal01|) so that, with operand magnitudes
# >= 1, the smallest non-zero addend |w x| is at least W_MIN.
JIT_PARAMS = {'s': (3.0,), 'u': (0.5, 1.5), 'n': (2.0, 0.125)}
W_MIN = {'u': 0.5, 'n': 2.0 - 6.5 * 0.125}
W_MAX = {'u': 1.5, 'n': 2.0 + 6.5 * 0.125}
assert min(W_MIN.values()) >= 0.5
NORMAL_WEIGHT_RTOL = 1e-5      # device logf against libm logf in the tails of the probit: what tests/test_oracle.py grants libm against numpy


def jit_chunks(shape, walk_len):
    chunk = max(1, (shape[1] + 3) // 4)
    return chunk, -(-walk_len // chunk)


def scatter_pieces(shape, out_len, stride):
    """scatter_geom (be_jitc_shared.h) restated: (largest Q of a residue class, pieces, piece_len)."""
    chunk, _ = jit_chunks(shape, out_len)
    q_max = -(-min(chunk, out_len) // stride)
    pieces = max(1, -(-q_max // K['jit.kPieceU64']))
    per_piece = -(-q_max // pieces)
    return q_max, pieces, max(256, (per_piece + 255) & ~255)


def jit_reference(family, X64, shape, transpose, corder, prob, seed, mm):
    p = JIT_PARAMS[family]
    w0, w1 = (p[0], 0.0) if family == 's' else p
    return oracle_c.jit_float(family, w0, w1, prob, X64, seed, shape=shape, transpose=transpose, corder=corder, stride=4 if mm else 32)


def jit_bound(family, route, dtype, ref, S, in_len, xmax):
    """Largest |device - reference| a correct kernel can show at each output, for the generated-weight families.
    S = sum |w x| over the output's addends (the same oracle run on |X|: all weights are positive).  A = number of addends of
    the output, bounded by S / W_MIN since every addend is at least W_MIN.
      gather:  products and sums in double: A additions, each off by at most 2^-53 of a partial sum <= S     -> A 2^-53 S
      atomic:  f32 (f64 for f64) atomic adds: one rounding for the product, A for the additions              -> (A + 1) u S, u = 2^-24 | 2^-53
      lds:     each product is rounded to f32 (2^-24 |w x|, in all 2^-24 S) and cut to a multiple of 2^-e_fix (A 2^-e_fix); the
               integer sums are exact; the reduce rounds the sum to f32 before the output dtype (2^-24 |ref|)
      normal:  every weight may differ from the oracle's by NORMAL_WEIGHT_RTOL of the largest weight            -> A rtol W_MAX xmax
    plus one rounding of the result to the output dtype (half an ulp: HALF_ULP |ref|)."""
    A = np.ceil(S / W_MIN[family])
    out_round = HALF_ULP[dtype] * np.abs(ref)
    if route == 'gather':
        b = A * 2.0 ** -53 * S
    elif route == 'atomic':
        b = (A + 1) * (2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24) * S
    else:
        wmax = J._jit_params(family, *JIT_PARAMS[family])[2]
        e_fix = J._fixed_scale_exp(wmax * xmax * 1.001, in_len)            # the exponent _jit_float_hip hands to the kernel
        b = A * 2.0 ** -e_fix + 2.0 ** -24 * S + 2.0 ** -24 * np.abs(ref)
    if family == 'n':
        b = b + A * NORMAL_WEIGHT_RTOL * W_MAX['n'] * xmax
    return b + out_round


def jit_expectation(family, route, dtype, X64, shape, transpose, corder, prob, seed, mm):
    """(reference, bound or None) with the host-side checks of the assertion policy; no device involved."""
    ref = jit_reference(family, X64, shape, transpose, corder, prob, seed, mm)
    assert np.count_nonzero(ref) > ref.size // 50, 'the case must compare sums, not zeros'
    if family == 's':
        return ref, None
    nz = np.abs(X64[X64 != 0])
    assert nz.min() >= 1.0
    S = jit_reference(family, np.abs(X64), shape, transpose, corder, prob, seed, mm)
    in_len = shape[0] if transpose else shape[1]
    bound = jit_bound(family, route, dtype, ref, S, in_len, float(nz.max()))
    smallest_addend = W_MIN[family] * float(nz.min())
    assert float(bound.max()) <= 0.25 * smallest_addend, (
        f'bound {bound.max()} could hide a lost addend of {smallest_addend} (largest S {S.max()})')
    return ref, bound


def jit_product(be, family, dtype, X64, shape, transpose, corder, prob, seed, mm):
    f = getattr(be, f"jit{family}{'mm' if mm else 'mv'}")
    wargs = tuple(torch.tensor(p, dtype=dtype) for p in JIT_PARAMS[family])
    return f(*wargs, prob, dev(X64, dtype), seed, shape=shape, transpose=transpose, corder=corder)


def jit_case(be, family, route, dtype, shape, transpose, corder, prob, seed, n, tag, log=None, repeat=False, X64=None):
    """n = 0: a vector operand (stride 32); n >= 1: a matrix of n columns (stride 4).  `route`: 'gather' | 'atomic' | 'lds'.
    `X64`: the operand, when the case needs a particular one (default: integers in [-4, 4], a fifth of them zero)."""
    assert corder == (route == 'gather')
    mm = n > 0
    in_len = shape[0] if transpose else shape[1]
    rng = np.random.default_rng(seed)
    if X64 is None:
        X64 = small_ints(rng, (in_len, n) if mm else in_len, 4, zeros=0.2)
    tag = f'{tag} jit{family}{"mm" if mm else "mv"} {dtype} n={n}'
    ref, bound = jit_expectation(family, route, dtype, X64, shape, transpose, corder, prob, seed, mm)
    if log is not None:
        del log[:]
    got = jit_product(be, family, dtype, X64, shape, transpose, corder, prob, seed, mm)
    if log is not None:
        served = [s for s in log if s in ('be_jitmm_float', 'be_jitmm_float_scatter')]
        assert served == [{'lds': 'be_jitmm_float_scatter'}.get(route, 'be_jitmm_float')], (tag, served)
    if bound is None:
        assert_exact(got, ref, dtype, tag)
    else:
        assert got.dtype == dtype and tuple(got.shape) == ref.shape, tag
        err = np.abs(got.detach().cpu().to(torch.float64).numpy() - ref)
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), (f'{tag}: {int((err > bound).sum())} of {err.size} outputs outside their bound; worst at flat index '
                                      f'{worst}: error {err.reshape(-1)[worst]}, bound {bound.reshape(-1)[worst]}')
    if repeat:      # fixed-point sums do not depend on the order of the atomics: a second call gives the same bits
        again = jit_product(be, family, dtype, X64, shape, transpose, corder, prob, seed, mm)
        assert torch.equal(bits(got), bits(again)), f'{tag}: not repeatable'
    return got


@pytest.fixture
def entry_log(monkeypatch):
    """Names of the C entry points `_jitc` looks up, in call order."""
    names = []
    real = J.fn

    def logged(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)
    monkeypatch.setattr(J, 'fn', logged)
    return names


@pytest.fixture
def atomics_only(monkeypatch):
    """No operand keeps this many bits at the fixed-point exponent: the f32 / f16 / bf16 scatter takes the float-atomic kernel."""
    monkeypatch.setattr(J, 'JIT_FLOAT_MIN_BITS', 500)


GATHER_MV = [((40_000, 3_000), False), ((3_000, JIT_GATHER_SPAN[32] + 9), True)]      # (shape, transpose): out_len 40 000 / 32 777


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_jit_gather_mv_row_loop(be, family):
    """k_jit_f_gather, stride 32: 8 rows per block, 4096 blocks — out_len above 32 768 puts the row loop on a second trip.  Both
    transpose values (the shape swapped accordingly); f64 / f16 / bf16 on the scalar family."""
    for shape, transpose in GATHER_MV:
        out_len = shape[1] if transpose else shape[0]
        assert out_len > JIT_GATHER_SPAN[32]
        for dtype in ([torch.float32] if family != 's' else DTYPES) + ([torch.float64] if family != 's' else []):
            jit_case(be, family, 'gather', dtype, shape, transpose, True, 0.01, 41, 0, f'shape={shape} transpose={transpose}')


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_jit_gather_mm_row_loop_and_tiles(be, family):
    """k_jit_f_gather, stride 4: 64 rows per block — out_len above 262 144; a one-column matrix (the NC = 1 kernels at stride 4),
    7 / 8 columns (one pass, partly filled / full), 9 and 17 (two and three passes, partly filled last tile: the c0 offset);
    k_jit_f_gather_reduce runs m * 8 > 524 288 elements: its own loop takes several trips."""
    shape, transpose = (JIT_GATHER_SPAN[4] + 70, 40), False
    out_len = shape[0]
    assert out_len > JIT_GATHER_SPAN[4] and out_len * K['jit.kTile'] > JIT_REDUCE_SPAN
    for n in (1, 7, 8, 9, 17):
        assert -(-n // K['jit.kTile']) == {1: 1, 7: 1, 8: 1, 9: 2, 17: 3}[n]
        for dtype in [torch.float32] + ([torch.float64, torch.float16, torch.bfloat16] if n == 9 and family == 's' else []) + \
                ([torch.float64] if n == 9 and family != 's' else []):
            jit_case(be, family, 'gather', dtype, shape, transpose, True, 0.1, 43, n, f'shape={shape}')


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_jit_atomic_scatter_task_loop(be, family, entry_log, monkeypatch):
    """k_jit_f_scatter: one thread per (row, chunk, lane) task, 8192 blocks of 256 — in_len * chunks * stride above 2 097 152.
    f64 always takes this kernel; f32 when the operand does not resolve at the fixed-point exponent (forced here)."""
    for shape, n in (((JIT_SCATTER_SPAN // (4 * 32) + 16, 600), 0), ((JIT_SCATTER_SPAN // (4 * 4) + 28, 64), 3), ((JIT_SCATTER_SPAN // (4 * 4) + 28, 64), 9)):
        in_len, out_len = shape
        chunk, n_chunks = jit_chunks(shape, out_len)
        stride = 4 if n else 32
        assert n_chunks == 4 and in_len * n_chunks * stride > JIT_SCATTER_SPAN
        assert in_len > (131_072 if n else 16_384)
        prob = 0.004 if n == 0 else 0.0008
        jit_case(be, family, 'atomic', torch.float64, shape, True, False, prob, 45, n, f'shape={shape}', log=entry_log)
        with monkeypatch.context() as mp:
            mp.setattr(J, 'JIT_FLOAT_MIN_BITS', 500)
            jit_case(be, family, 'atomic', torch.float32, shape, True, False, prob, 46, n, f'shape={shape} (forced)', log=entry_log)


@pytest.mark.parametrize('family', ['s', 'u'])
def test_jit_atomic_scatter_above_2_32_tasks(be, family, entry_log):
    """k_jit_f_scatter's task index is 64-bit: in_len * chunks * 32 above 2**32.  A long output walked in 33 600 chunks; only four
    operand rows are non-zero — the first, one in the middle and two whose tasks lie beyond 2**32 — so the other rows are skipped
    at the cost of one load each and the reference stays cheap."""
    shape = (33_600_000, 4_000)                               # transpose=False, corder=False: in_len = 4000, out_len = walk = 33.6 M
    in_len, out_len = shape[1], shape[0]
    chunk, n_chunks = jit_chunks(shape, out_len)
    per_row = n_chunks * 32
    assert in_len * per_row > 2 ** 32
    rows = [0, 1234, 3996, 3999]
    assert rows[2] * per_row >= 2 ** 32, 'two non-zero rows own tasks beyond 2**32'
    X64 = np.zeros(in_len)
    X64[rows] = (2.0, -3.0, 4.0, 1.0)
    got = jit_case(be, family, 'atomic', torch.float64, shape, False, False, 0.05, 48, 0, f'shape={shape}', log=entry_log, X64=X64)
    del got
    torch.cuda.empty_cache()


def test_jit_atomic_scatter_half_precision_round_loop(be, entry_log, atomics_only):
    """f16 / bf16 through the atomic kernel: sums in an f32 image, k_jit_f_round converts out_len * n > 524 288 elements (2048 blocks
    of 256: a second trip).  Exact data (scalar family)."""
    for shape, n in (((300, JIT_ROUND_SPAN + 12), 0), ((300, JIT_ROUND_SPAN // 8 + 5), 8)):
        assert shape[1] * max(n, 1) > JIT_ROUND_SPAN
        for dtype in (torch.float16, torch.bfloat16):
            got = jit_case(be, 's', 'atomic', dtype, shape, True, False, 0.01, 47, n, f'shape={shape}', log=entry_log)
            assert int(torch.count_nonzero(got.reshape(-1)[JIT_ROUND_SPAN:])) > 0, 'the second trip must hold non-zero outputs'


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_jit_lds_scatter_several_pieces(be, family, entry_log):
    """k_jit_f_scatter_lds with ONE_PIECE = false: a residue class has more than kPieceU64 = 16 384 positions, so it is cut into
    pieces of a multiple of 256 accumulators and the last piece is partly filled.  mv: shape[1] above 2 097 152 (chunk / 32),
    mm: above 262 144 (chunk / 4) with 1, 3 and 8 columns (different `parts`).  Each call must be served by
    be_jitmm_float_scatter and repeat bit for bit."""
    for shape, n in (((300, 32 * 4 * K['jit.kPieceU64'] + 2851), 0), ((200, 4 * 4 * K['jit.kPieceU64'] + 27), 1),
                     ((200, 4 * 4 * K['jit.kPieceU64'] + 27), 3), ((200, 4 * 4 * K['jit.kPieceU64'] + 27), 8)):
        stride = 4 if n else 32
        assert shape[1] > (262_144 if n else 2_097_152)
        q_max, pieces, piece_len = scatter_pieces(shape, shape[1], stride)
        assert pieces >= 2 and q_max % 256 != 0 and (q_max - 1) % 256 != 0, (q_max, pieces)
        assert 0 < q_max - (pieces - 1) * piece_len < piece_len, 'the last piece must be partly filled'
        dtypes = [torch.float32] + ([torch.float16, torch.bfloat16] if family == 's' and n in (0, 3) else [])
        for dtype in dtypes:
            jit_case(be, family, 'lds', dtype, shape, True, False, 0.005 if n == 0 else 0.02, 49, n, f'shape={shape}', log=entry_log,
                     repeat=True)


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_jit_chunk_geometry(be, family, entry_log, monkeypatch):
    """The chunk width is a quarter of shape[1] but the walk may run over shape[0]: (5000, 40) walked over its long side has 500
    chunks of 10 (gridDim.y = 500 in the gather, 500 * stride residue classes in the scatter); (20, 1000) walked over its short
    side has one chunk of width 20 < 32 lanes, where the lanes from 20 on have nothing to visit — and at stride 4 five positions
    per lane.  Gather, LDS scatter and atomic scatter, vector and matrix operands."""
    for shape, chunks, p_gather, p_scatter in (((5000, 40), 500, 0.02, 0.1), ((20, 1000), 1, 0.3, 0.05)):
        for n in (0, 3):
            # gather walks in_len: transpose=True makes that shape[0]
            chunk, n_chunks = jit_chunks(shape, shape[0])
            assert n_chunks == chunks
            if chunks == 1:
                assert shape[0] < chunk and (n or shape[0] < 32), 'one chunk narrower than the lane stride'
            jit_case(be, family, 'gather', torch.float32, shape, True, True, p_gather, 51, n, f'shape={shape}')
            # scatter walks out_len: transpose=False makes that shape[0]
            jit_case(be, family, 'lds', torch.float32, shape, False, False, p_scatter, 52, n, f'shape={shape}', log=entry_log, repeat=True)
            jit_case(be, family, 'atomic', torch.float64, shape, False, False, p_scatter, 53, n, f'shape={shape}', log=entry_log)
            with monkeypatch.context() as mp:
                mp.setattr(J, 'JIT_FLOAT_MIN_BITS', 500)
                jit_case(be, family, 'atomic', torch.float32, shape, False, False, p_scatter, 54, n, f'shape={shape} (forced)', log=entry_log)


def test_jit_refuses_more_chunks_than_grid_rows(be):
    """The gather kernels (and the scatter's reduce) launch with gridDim.y = n_chunks; a tall, thin shape walked over its long side
    asks for more than the device launches.  The C entry points refuse it, naming the chunk count, before anything is launched."""
    limit = int(lib_fn('be_device_max_grid_y', ctypes.c_int64, [])())
    assert 0 < limit < 2 ** 24, limit
    rows = limit + 1                                          # chunks of width 1: shape[1] = 4
    shape = (rows, 4)
    assert jit_chunks(shape, rows) == (1, rows)
    x = torch.ones(rows, dtype=torch.float32, device='cuda')
    X = torch.ones((rows, 2), dtype=torch.float32, device='cuda')
    spikes = torch.ones(rows, dtype=torch.bool, device='cuda')
    w = np.float32(1.0)
    for call in (lambda: be.jitsmv(w, 0.5, x, 3, shape=shape, transpose=True, corder=True),
                 lambda: be.jitumm(w, np.float32(2.0), 0.5, X, 3, shape=shape, transpose=True, corder=True),
                 lambda: be.binary_jitsmv(w, 0.5, spikes, 3, shape=shape, transpose=True, corder=True)):
        with pytest.raises(KernelExecutionError, match=rf'{rows} chunks'):
            call()
    # a chunk count below the limit is served
    ok_shape = (limit - 1, 4)
    got = be.jitsmv(w, 0.5, x[:limit - 1], 3, shape=ok_shape, transpose=True, corder=True)
    ref = oracle_c.jit_float('s', 1.0, 0.0, 0.5, np.ones(limit - 1), 3, shape=ok_shape, transpose=True, corder=True, stride=32)
    assert_exact(got, ref, torch.float32, 'limit - 1 chunks')
