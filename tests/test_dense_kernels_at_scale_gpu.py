"""The event-driven dense products (csrc/be_dense.hip: k_densemm_t, k_densemm_nt, k_densemm_mfma, k_densemm_nt_mfma16,
k_densemm_nt_mfma_f32, k_densemm_t_mfma_f32 and the mask, list, scan and reduce kernels around them) past their one-pass sizes:
every grid-stride loop, LDS chunk, row-part split, unroll tail and dispatch switch of the file is crossed by a named case.

Assertion policy (that of tests/test_float_kernels_at_scale_gpu.py, whose helpers are imported): the weights are integers from
+-{1 ... 8} without zeros (a lost or doubled row always shows; all of them exact in bf16), a product is w * 1 or w * 0 and every
accumulator is f32 or f64, so every partial sum is an exact integer in any order as long as the sum of |w| over an output's
active entries stays below 2**24.  Every case asserts that on the host (8 * the largest number of active entries of a batch row
bounds it from above), that the reference rounded to the output dtype is finite, and then that the result EQUALS the float64
reference rounded once (through f32 for the 16-bit types).  There is no tolerance in this file.  The reference is a float64
numpy matmul of the 0/1 activity with the weights; wherever the operands are small enough the same call also runs
oracle_np.binary_densemm on the spike values themselves and asserts that the two agree bit for bit.

Every case first asserts, from the CONSTS table (tests/test_dense_kernels_thresholds_cpu.py compares it with the source) and host
restatements of densemm_any's dispatch, parts_for, mfma_parts and n_tiles_of, which kernel its shape takes and that it crosses the
bound it is there for; `check_all_crossings` repeats those assertions without a device.

Which loop or branch is reached where:
  k_gl_scan second trip (more than 1024 tiles), per-group lists, k_gl_write<false, false>   test_gl_scan_second_trip_per_group_lists
  scan route of densemm_nt_vec (k_gl_scan + k_gl_write<true, false>), stream and gather,
    VEC 1 with the slow mask path and a ragged last tile                                     test_scan_route_nt_vec
  scan route of densemm_t_mfma, f16 / bf16 / f32                                             test_scan_route_t_mfma
  k_gl_write<true, true> at 1024 tiles (the last workgroup sums 1023) and one tile past it   test_self_scan_at_its_limit_and_past_it
  k_dense_masks<SpikeBool / SpikeFloat>, k_dense_masks_bits stride loops (k > 524 288)       test_mask_stride_loops
  k_densemm_nt row loop (m > 8192), NBT 1 / 8 / 32, gather (main loop + tail) and stream     test_nt_row_loop_second_trip
  k_densemm_nt stream loop: U = 4 pieces in flight against the piece-by-piece tail           test_nt_stream_unroll_split
  k_densemm_t at parts == 1 (one group / eight groups), k_dense_reduce stride loop           test_t_vec_one_part
  k_densemm_t at parts == 15, UNR = 8 main loop against its tail on constructed counts       test_t_vec_fifteen_parts_unroll_split
  k_densemm_t at parts == 32 with fewer active rows than parts                               test_t_vec_more_parts_than_active_rows
  RowLoad<float, 4>, <double, 2>, <__half, 8>, <__hip_bfloat16, 8> and <W, 1>                test_every_row_load_width
  k_densemm_mfma: kMfmaChunk staged steps, 16 parts, ragged last chunk; second batch pass    test_mfma_chunks_sixteen_parts
  k_densemm_mfma at parts == 1, k_mfma_reduce stride loop                                    test_mfma_chunks_one_part
  k_densemm_t_mfma_f32: kTfChunk staged steps at 16 parts and at 1 part                      test_tf32_chunks
  row parts with an empty K range; no spikes at all; none in the second batch pass           test_mfma_empty_ranges_and_silent_batches
  column tiles with a partly filled last tile, nb 9 ... 65                                   test_mfma_partly_filled_column_tiles
  k_densemm_nt_mfma16: kNtChunk mask chunks, clamped last rows, ragged last step             test_nt_mfma16_mask_chunks
  k_densemm_nt_mfma_f32: the same                                                            test_nt_mfma_f32_mask_chunks
  shortest contractions that take the W @ S.T MFMA kernels                                   test_nt_mfma_shortest_contractions
  bit-packed batches (BE_SPIKE_BITS) on each of the four routes, k % 32 != 0                 test_bit_packed_batches_on_every_route
  a spike operand that is not 8-byte aligned (slow branch of k_dense_masks_count)            test_spike_operand_off_alignment

Not here: k_densemm_nt_mfma (BE_NT_MFMA16 = 0) is not compiled in by default.  The k > 524 288 mask loop on the W @ S.T MFMA route
would need a 4 GB matrix (4096 rows at least); densemm_nt_mfma launches the same k_dense_masks instantiations on the same grid
(launch_dense_masks) as the S @ W vector route, where test_mask_stride_loops crosses it.
"""
import numpy as np
import pytest
import torch

from brainevent_amd import _array as A
from brainevent_amd import _dense as D
from oracle import oracle_np
from test_float_kernels_at_scale_gpu import DTYPES, assert_exact, rounded

pytestmark = pytest.mark.gpu

# The loop bounds and dispatch thresholds of be_dense.hip as the cases below use them.
CONSTS = {
    'kTile': 2048,                        # rows per workgroup of the list kernels (k_gl_count, k_gl_write, k_dense_masks_count*)
    'kGroup': 4,                          # batch rows per wave of k_densemm_t
    'kMaxChunk': 32,                      # batch rows per pass (one uint32 mask per row)
    'masks.grid_cap': 2048,               # k_dense_masks / k_dense_masks_bits: grid_cap_fwd(k, 256, 2048)
    'self_scan.max_tiles': 1024,          # nt <= 1024: k_gl_write<true, true> sums the tiles in front of it, no k_gl_scan
    'scan.block': 1024,                   # tiles per trip of k_gl_scan
    'nt.rows_per_block': 4,               # k_densemm_nt: grid_cap(m, 4, 256 * 8), a wave per weight row
    'nt.grid_cap': 256 * 8,
    'nt.U': 4,                            # 16-byte pieces in flight per lane in the stream loop of k_densemm_nt
    'dense_reduce.grid_cap': 2048,        # k_dense_reduce: grid_cap(nb * n, 256, 2048)
    'mfma_reduce.grid_cap': 2048,         # k_mfma_reduce: grid_cap(nc * n, 256, 2048)
    'kMfmaCols': 256,                     # columns per workgroup of k_densemm_mfma (k_densemm_t_mfma_f32: twice that)
    'kMfmaChunk': 64,                     # K-steps of 16 union rows staged in LDS at a time (k_densemm_mfma)
    'mfma.wg_target': 768,                # BE_MFMA_WG_TARGET: column tiles x row parts aimed at
    'mfma.parts_clamp': 16,
    'kNtChunk': 4096,                     # masks staged in LDS at a time (k_densemm_nt_mfma16, k_densemm_nt_mfma_f32)
    'kTfChunk': 128,                      # steps of 2 union rows staged in LDS at a time (k_densemm_t_mfma_f32)
    'parts_for.target_one_group': 2048,   # parts_for: workgroups to aim for / row parts at most, one batch group ...
    'parts_for.target': 1024,             # ... and several
    'parts_for.cap_one_group': 32,
    'parts_for.cap': 16,
    'UNR': 8,                             # row loads in flight per lane in k_densemm_t's main loop
    't_mfma.min_nb': 8,                   # densemm_any: S @ W takes the MFMA kernels from here on (f16, bf16, f32)
    'nt_mfma.min_nb': 8,                  # BE_NT_MFMA_MIN_NB (f16, bf16)
    'nt_mfma_f32.min_nb': 8,
    'nt_mfma.min_rows': 4096,
    'nt_mfma.min_cols_16bit': 32,
    'nt_mfma.min_cols_f32': 8,
}
K = CONSTS
F32, F64, F16, BF16 = DTYPES
assert (F32, F64, F16, BF16) == (torch.float32, torch.float64, torch.float16, torch.bfloat16)
MASKS_SPAN = 256 * K['masks.grid_cap']                      # 524 288 spikes per trip of the mask kernels
NT_ROW_SPAN = K['nt.rows_per_block'] * K['nt.grid_cap']     # 8 192 weight rows per trip of k_densemm_nt
REDUCE_SPAN = 256 * K['dense_reduce.grid_cap']              # 524 288 outputs per trip of k_dense_reduce
MFMA_REDUCE_SPAN = 256 * K['mfma_reduce.grid_cap']          # 524 288 outputs per trip of k_mfma_reduce
SELF_SCAN_ROWS = K['self_scan.max_tiles'] * K['kTile']      # 2 097 152: the longest contraction that scans itself
W_ABS_MAX = 8
ORACLE_LIMIT = 1 << 24                                      # weights x batch rows up to which oracle_np's per-column loop runs too


# =========================================================================================================== host restatements
def vec_of(dtype):
    """Vec16<W>::n: elements of a 16-byte load."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def route(shape, nb, transpose, dtype):
    """densemm_any restated: (host function, VEC).  The other half of vec_ok, a 16-byte aligned weight pointer, is asserted on
    the device tensor in `run`."""
    rows_w, cols_w = shape
    V = vec_of(dtype)
    vec_ok = cols_w % V == 0
    if transpose:
        if dtype in (F16, BF16, F32) and vec_ok and nb >= K['t_mfma.min_nb']:
            return 't_mfma', V
        return 't_vec', (V if vec_ok else 1)
    if dtype in (F16, BF16) and vec_ok and nb >= K['nt_mfma.min_nb'] and rows_w >= K['nt_mfma.min_rows'] and cols_w >= K['nt_mfma.min_cols_16bit']:
        return 'nt_mfma', V
    if dtype == F32 and vec_ok and nb >= K['nt_mfma_f32.min_nb'] and rows_w >= K['nt_mfma.min_rows'] and cols_w >= K['nt_mfma.min_cols_f32']:
        return 'nt_mfma', V
    return 'nt_vec', (V if vec_ok else 1)


def n_tiles_of(k):
    return -(-k // K['kTile'])


def groups_of(nb):
    """Batch groups of the first pass (densemm_t_vec sizes `parts` by it)."""
    return (min(nb, K['kMaxChunk']) + K['kGroup'] - 1) // K['kGroup']


def parts_for(n, vec, n_groups):
    tasks = -(-n // (64 * vec)) * n_groups
    wgs = (tasks + 3) // 4
    one = n_groups == 1
    target = K['parts_for.target_one_group'] if one else K['parts_for.target']
    cap = K['parts_for.cap_one_group'] if one else K['parts_for.cap']
    return max(1, min(cap, target // max(wgs, 1)))


def mfma_parts(n):
    tiles = -(-n // K['kMfmaCols'])
    return max(1, min(K['mfma.parts_clamp'], K['mfma.wg_target'] // max(tiles, 1)))


def t_mfma_geom(n, dtype, n_union):
    """densemm_t_mfma + the heads of k_densemm_mfma / k_densemm_t_mfma_f32: (parts, steps, steps per part, steps per LDS chunk)."""
    f32 = dtype == F32
    parts = mfma_parts(n // 2) if f32 else mfma_parts(n)
    steps = -(-n_union // (2 if f32 else 16))
    return parts, steps, -(-steps // parts), K['kTfChunk'] if f32 else K['kMfmaChunk']


def passes(nb):
    return [(b0, min(K['kMaxChunk'], nb - b0)) for b0 in range(0, nb, K['kMaxChunk'])]


# =========================================================================================================== data
def weights(seed, shape):
    """int8 from +-{1 ... 8}, no zeros (a stream of its own: `draw` may be given the same seed)."""
    v = np.random.default_rng([seed, 1]).integers(0, 16, shape, dtype=np.int8)
    return np.where(v < 8, v - 8, v - 7).astype(np.int8)


def draw(seed, nb, k, firing, last=False):
    """[nb, k] bool, batch-major as the kernels take it.  `last`: entry k - 1 of batch row 0 set (the last tile counts)."""
    S = np.random.default_rng([seed, 2]).random((nb, k)) < firing
    if last:
        S[0, -1] = True
    return S


def float_values(S):
    """Float spikes from {0.7, 0, -1.0}: active when > 0, and only there."""
    off = np.random.default_rng(S.size).random(S.shape) < 0.5
    return np.where(S, 0.7, np.where(off, 0.0, -1.0)).astype(np.float32)


def pack_rows(S):
    """[nb, k] bool (host) -> [nb, ceil(k / 32)] words on the device, bit i % 32 of word i // 32."""
    pad = (-S.shape[1]) % 32
    b = np.packbits(np.pad(S, ((0, 0), (0, pad))), axis=1, bitorder='little')
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int32)).cuda()


def reference(W8, S, transpose, values=None):
    """float64 [nb, out_len].  `values`: the float spikes the device gets, for the oracle."""
    nb = S.shape[0]
    assert W8.dtype == np.int8 and S.dtype == bool and (W8 != 0).all() and int(np.abs(W8).max()) <= W_ABS_MAX
    assert S.shape[1] == (W8.shape[0] if transpose else W8.shape[1])
    # sum of |w| over the active entries of any output <= 8 * active entries of its batch row: every partial sum is exact in f32
    assert W_ABS_MAX * int(S.sum(axis=1).max()) < 2 ** 24
    W64 = W8.astype(np.float64)
    ref = S.astype(np.float64) @ (W64 if transpose else W64.T)
    if W8.size * nb <= ORACLE_LIMIT:
        spikes = (S if values is None else values).T
        assert np.array_equal(oracle_np.binary_densemm(W64, spikes, transpose).T, ref), 'the matmul must equal the oracle'
    return ref


def operand(S, kind):
    """(device operand, spike dtype code, float values or None).  kind: 'bool' | 'float' | 'bits' | 'bool+1' (one byte off)."""
    if kind == 'bool':
        return torch.from_numpy(S).cuda(), A.BE_SPIKE_BOOL, None
    if kind == 'float':
        v = float_values(S)
        assert ((v > 0) == S).all()
        return torch.from_numpy(v).cuda(), A.BE_SPIKE_FLOAT, v
    if kind == 'bits':
        return pack_rows(S), A.BE_SPIKE_BITS, None
    assert kind == 'bool+1'
    buf = torch.zeros(S.size + 16, dtype=torch.bool, device='cuda')
    view = buf[1:1 + S.size].view(S.shape)
    view.copy_(torch.from_numpy(S))
    assert view.data_ptr() % 8 == 1 and view.is_contiguous()
    return view, A.BE_SPIKE_BOOL, None


def run(Wd, S, kind, transpose, ref, tag):
    """One product through the package's own host path (_dense._dense_batched -> the C entry points, prototypes from _lib.fn)."""
    op, sd, _ = operand(S, kind)
    assert Wd.data_ptr() % 16 == 0 and Wd.is_contiguous()
    got = D._dense_batched(Wd, op, sd, transpose)
    tag = f'{tag} shape={tuple(Wd.shape)} nb={S.shape[0]} {Wd.dtype} {kind} transpose={transpose}'
    assert bool(torch.isfinite(rounded(ref, Wd.dtype)).all()), tag
    assert bool(torch.isfinite(got).all()), f'{tag}: non-finite outputs'
    assert_exact(got, ref, Wd.dtype, tag)
    return got


def dense_case(W8, S, transpose, combos, tag, expect_route=None):
    """The product of one (weights, spikes) pair for every (dtype, kind) of `combos`, against one shared reference."""
    refs = {}
    for dtype, kind in combos:
        if expect_route is not None:
            assert route(W8.shape, S.shape[0], transpose, dtype)[0] == expect_route, (tag, dtype)
        fl = kind == 'float'
        if fl not in refs:
            refs[fl] = reference(W8, S, transpose, float_values(S) if fl else None)
        run(torch.from_numpy(W8).cuda().to(dtype), S, kind, transpose, refs[fl], tag)
    return refs[False] if False in refs else refs[True]


def union(S, b0=0, nc=None):
    return int(S[b0:(None if nc is None else b0 + nc)].any(axis=0).sum())


# =========================================================================================================== scans and lists
GL_SCAN_T_VEC = ((2_099_213, 4), 5, 0.02)


def cross_gl_scan_t_vec():
    shape, nb, _ = GL_SCAN_T_VEC
    assert route(shape, nb, True, F32) == ('t_vec', 4) and groups_of(nb) == 2
    assert n_tiles_of(shape[0]) > K['scan.block'], 'k_gl_scan must take a second trip'
    assert shape[0] % K['kTile'] != 0


def test_gl_scan_second_trip_per_group_lists(be):
    """build_lists (densemm_t_vec): 1026 tiles per group put k_gl_scan on a second trip whose offsets carry the 1024 tiles before
    it; two groups (nb 5), rows with spikes in the tiles past 1024 in both."""
    cross_gl_scan_t_vec()
    shape, nb, firing = GL_SCAN_T_VEC
    S = draw(81, nb, shape[0], firing, last=True)
    tail = K['scan.block'] * K['kTile']
    assert S[:4, tail:].any() and S[4:, tail:].any(), 'both groups must list rows past the first trip of the scan'
    dense_case(weights(81, shape), S, True, [(F32, 'bool')], 'gl_scan', 't_vec')


SCAN_NT_VEC = [((8, 2_099_208), 3, 0.2, False, 4), ((8, 2_099_208), 1, 0.001, True, 4), ((5, 2_099_213), 3, 0.2, False, 1)]


def cross_scan_nt_vec(i, n_union):
    shape, nb, _, gather, vec = SCAN_NT_VEC[i]
    k = shape[1]
    assert route(shape, nb, False, F32) == ('nt_vec', vec)
    assert n_tiles_of(k) > K['self_scan.max_tiles'], 'the scan route: k_gl_scan + k_gl_write<true, false>'
    assert (n_union * 16 < k) == gather, (n_union, k)
    if vec == 1:
        assert k % 8 != 0 and k % K['kTile'] != 0, 'the slow branch of k_dense_masks_count and a ragged last tile'


@pytest.mark.parametrize('i', range(len(SCAN_NT_VEC)))
def test_scan_route_nt_vec(be, i):
    """densemm_nt_vec past 1024 tiles: the union list comes from k_gl_scan + k_gl_write<true, false>; the stream route ignores it
    but reads its count, the gather route (n_union * 16 < k) walks it.  The 5 x 2 099 213 case has VEC 1, masks built row by row
    (k % 8 != 0) and a last tile of 13 columns."""
    shape, nb, firing, _, _ = SCAN_NT_VEC[i]
    S = draw(82 + i, nb, shape[1], firing, last=True)
    cross_scan_nt_vec(i, union(S))
    assert S[:, SELF_SCAN_ROWS:].any()
    dense_case(weights(82, shape), S, False, [(F32, 'bool')], 'scan nt_vec', 'nt_vec')


SCAN_T_MFMA = [((2_099_208, 8), F16), ((2_099_208, 8), BF16), ((2_099_208, 4), F32)]
SCAN_T_MFMA_NB, SCAN_T_MFMA_FIRING = 8, 0.01


def cross_scan_t_mfma():
    for shape, dtype in SCAN_T_MFMA:
        assert route(shape, SCAN_T_MFMA_NB, True, dtype)[0] == 't_mfma'
        assert n_tiles_of(shape[0]) > K['self_scan.max_tiles']


@pytest.mark.parametrize('i', range(len(SCAN_T_MFMA)))
def test_scan_route_t_mfma(be, i):
    """densemm_t_mfma past 1024 tiles: the union list the MFMA kernels walk comes from k_gl_scan + k_gl_write<true, false>."""
    cross_scan_t_mfma()
    shape, dtype = SCAN_T_MFMA[i]
    S = draw(85, SCAN_T_MFMA_NB, shape[0], SCAN_T_MFMA_FIRING, last=True)
    assert S[:, SELF_SCAN_ROWS:].any()
    dense_case(weights(85, shape), S, True, [(dtype, 'bool')], 'scan t_mfma', 't_mfma')


SELF_SCAN_K = [SELF_SCAN_ROWS, SELF_SCAN_ROWS + 8]      # 1024 tiles exactly / a 1025th tile of 8 rows


def cross_self_scan():
    assert [n_tiles_of(k) for k in SELF_SCAN_K] == [K['self_scan.max_tiles'], K['self_scan.max_tiles'] + 1]
    for k in SELF_SCAN_K:
        assert k % 8 == 0
        assert route((8, k), 3, False, F32) == ('nt_vec', 4) and route((k, 8), 8, True, F16)[0] == 't_mfma'


@pytest.mark.parametrize('k', SELF_SCAN_K)
def test_self_scan_at_its_limit_and_past_it(be, k):
    """The nt <= 1024 switch of densemm_nt_vec and densemm_t_mfma on both sides: 1024 tiles, where the last workgroup of
    k_gl_write<true, true> sums the 1023 tiles in front of it and writes the total, and 1025 tiles, the first size that scans."""
    cross_self_scan()
    S = draw(86, 8, k, 0.01, last=True)
    assert S[:, -K['kTile']:].any() and S[:3, -K['kTile']:].any()
    dense_case(weights(86, (k, 8)), S, True, [(F16, 'bool')], 'self-scan', 't_mfma')
    S3 = np.ascontiguousarray(S[:3])
    ref = dense_case(weights(87, (8, k)), S3, False, [(F32, 'bool')], 'self-scan', 'nt_vec')
    assert np.count_nonzero(ref) > 0
    # the gather route reads the list itself: one batch row, few enough spikes
    S1 = draw(88, 1, k, 0.001, last=True)
    assert union(S1) * 16 < k
    dense_case(weights(87, (8, k)), S1, False, [(F32, 'bool')], 'self-scan gather', 'nt_vec')


MASKS_SHAPE, MASKS_NB = (524_588, 8), 3


def cross_masks():
    assert MASKS_SHAPE[0] > MASKS_SPAN and -(-MASKS_SHAPE[0] // 256) > K['masks.grid_cap']
    for dtype in (F32, F64):
        assert route(MASKS_SHAPE, MASKS_NB, True, dtype)[0] == 't_vec', 'build_lists launches k_dense_masks / k_dense_masks_bits'
    assert MASKS_SHAPE[0] % 32 != 0


def test_mask_stride_loops(be):
    """k_dense_masks<SpikeBool>, k_dense_masks<SpikeFloat> and k_dense_masks_bits: 2048 workgroups of 256 cover 524 288 spikes per
    trip; 524 588 rows put each on a second trip (bit-packed: a last word of 12 bits).  f32 and f64 weights."""
    cross_masks()
    S = draw(89, MASKS_NB, MASKS_SHAPE[0], 0.2, last=True)
    assert S[:, MASKS_SPAN:].sum() > 100
    dense_case(weights(89, MASKS_SHAPE), S, True, [(F32, 'bool'), (F32, 'float'), (F32, 'bits'), (F64, 'bool'), (F64, 'float'), (F64, 'bits')],
               'mask loops', 't_vec')


# =========================================================================================================== W @ S.T, vector kernel
NT_ROWS_M = 8_229
NT_ROWS_K = {72: 4, 4096: 255}            # contraction length -> active columns that force the gather route
NT_ROWS_COMBOS = [(1, F32), (3, F32), (1, F16), (3, F16), (33, F64)]      # NBT 1 / 8 / 1 / 8 / 32 then a pass of one row


def cross_nt_rows():
    assert NT_ROWS_M > NT_ROW_SPAN and -(-NT_ROWS_M // K['nt.rows_per_block']) > K['nt.grid_cap'], 'a second trip of the row loop'
    for k, n_act in NT_ROWS_K.items():
        assert n_act * 16 < k <= (n_act + 1) * 16, 'the most active columns that still gather'
        for nb, dtype in NT_ROWS_COMBOS:
            assert route((NT_ROWS_M, k), nb, False, dtype) == ('nt_vec', vec_of(dtype))
    assert passes(33) == [(0, 32), (32, 1)]
    assert NT_ROWS_K[4096] >= 4 * 64 - 1, 'lanes 0 .. 62 take the four-in-flight gather loop, lane 63 its tail'


def gather_spikes(seed, nb, k, n_act):
    """Exactly n_act active columns, each in a random non-empty set of the batch rows (the last pass keeps at least one)."""
    rng = np.random.default_rng(seed)
    S = np.zeros((nb, k), bool)
    cols = rng.choice(k, n_act, replace=False)
    S[:, cols] = rng.random((nb, n_act)) < 0.5
    S[rng.integers(0, nb, n_act), cols] = True
    S[nb - 1, cols[0]] = True
    return S


@pytest.mark.parametrize('k', sorted(NT_ROWS_K))
def test_nt_row_loop_second_trip(be, k):
    """k_densemm_nt: 2048 workgroups of four waves, a wave per weight row — 8 229 rows put the row loop on a second trip of 37.
    One, three and 33 batch rows (NBT 1, 8, 32 and a second pass of one row at b0 = 32); the stream route at firing 0.3 and the
    gather route at the most active columns that still take it (255 of 4096: the four-in-flight loop and its tail; 4 of 72)."""
    cross_nt_rows()
    shape = (NT_ROWS_M, k)
    W8 = weights(90, shape)
    for nb, dtype in NT_ROWS_COMBOS:
        S = draw(90 + nb, nb, k, 0.3)
        G = gather_spikes(91 + nb, nb, k, NT_ROWS_K[k])
        for b0, nc in passes(nb):
            assert union(S, b0, nc) * 16 >= k and 0 < union(G, b0, nc) * 16 < k
        assert union(G) == NT_ROWS_K[k]
        for spk, name in ((S, 'stream'), (G, 'gather')):
            ref = dense_case(W8, spk, False, [(dtype, 'bool')], f'nt rows {name}', 'nt_vec')
            assert np.count_nonzero(ref[:, NT_ROW_SPAN:]) > 0, 'the second trip must hold non-zero outputs'


NT_SPLIT_M, NT_SPLIT_NB = 70, 3


def nt_split_ks(dtype):
    full = K['nt.U'] * 64 * vec_of(dtype)
    return [full - vec_of(dtype), full, full + vec_of(dtype)]


def cross_nt_split():
    for dtype in DTYPES:
        for k in nt_split_ks(dtype):
            assert route((NT_SPLIT_M, k), NT_SPLIT_NB, False, dtype) == ('nt_vec', vec_of(dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_nt_stream_unroll_split(be, dtype):
    """The stream loop of k_densemm_nt keeps U = 4 pieces of 16 bytes in flight per lane and finishes piece by piece: k one
    vector below 4 * 64 * VEC (lane 63 falls to the tail), at it (no tail at all) and one above (lane 0 comes back for one piece)."""
    cross_nt_split()
    for k in nt_split_ks(dtype):
        S = draw(92, NT_SPLIT_NB, k, 0.3, last=True)
        assert union(S) * 16 >= k
        dense_case(weights(92, (NT_SPLIT_M, k)), S, False, [(dtype, 'bool')], 'nt split', 'nt_vec')


# =========================================================================================================== S @ W, vector kernel
PARTS_ONE = [((70, 262_147), 1, 1), ((300, 16_391), 33, 8)]      # (shape, nb, batch groups)


def cross_parts_one():
    for shape, nb, groups in PARTS_ONE:
        assert route(shape, nb, True, F32) == ('t_vec', 1) and groups_of(nb) == groups
        assert parts_for(shape[1], 1, groups) == 1
    shape, nb, _ = PARTS_ONE[1]
    assert nb * shape[1] > REDUCE_SPAN and -(-nb * shape[1] // 256) > K['dense_reduce.grid_cap'], 'k_dense_reduce: a second trip'


@pytest.mark.parametrize('i', range(len(PARTS_ONE)))
def test_t_vec_one_part(be, i):
    """k_densemm_t with so many column strips that parts_for gives one row part: a wave walks its whole list alone (one batch
    group, 4097 strips; eight groups, 257 strips and a second pass of one batch row).  33 x 16 391 outputs also put
    k_dense_reduce on a second trip."""
    cross_parts_one()
    shape, nb, _ = PARTS_ONE[i]
    S = draw(93 + i, nb, shape[0], 0.5)
    ref = dense_case(weights(93, shape), S, True, [(F32, 'bool')], 'parts 1', 't_vec')
    if nb * shape[1] > REDUCE_SPAN:
        assert np.count_nonzero(ref.reshape(-1)[REDUCE_SPAN:]) > 0


PARTS_15_SHAPE, PARTS_15_NB, PARTS_15 = (600, 8_201), 8, 15
PARTS_15_COUNTS = [(0, 1), (PARTS_15 - 1, 8 * PARTS_15 - 1), (8 * PARTS_15, 8 * PARTS_15 + 1), (16 * PARTS_15 + 3, 0)]


def cross_parts_15():
    assert route(PARTS_15_SHAPE, PARTS_15_NB, True, F32) == ('t_vec', 1) and groups_of(PARTS_15_NB) == 2
    assert parts_for(PARTS_15_SHAPE[1], 1, 2) == PARTS_15 and K['UNR'] == 8
    # cnt = UNR * parts - 1: parts 0 .. 13 take the main loop once, part 14 only the tail; cnt = UNR * parts: every part once, no tail
    assert sorted(c for pair in PARTS_15_COUNTS for c in pair) == sorted(
        [0, 0, 1, PARTS_15 - 1, K['UNR'] * PARTS_15 - 1, K['UNR'] * PARTS_15, K['UNR'] * PARTS_15 + 1, 2 * K['UNR'] * PARTS_15 + 3])


def test_t_vec_fifteen_parts_unroll_split(be):
    """k_densemm_t at parts = 15: part p takes list entries p, p + 15, ... eight at a time (UNR) and then one by one.  The number
    of listed rows of each of the two batch groups is constructed: 0, 1, parts - 1, 8 parts - 1, 8 parts, 8 parts + 1, 16 parts + 3."""
    cross_parts_15()
    k = PARTS_15_SHAPE[0]
    W8 = weights(95, PARTS_15_SHAPE)
    rng = np.random.default_rng(95)
    for counts in PARTS_15_COUNTS:
        S = np.zeros((PARTS_15_NB, k), bool)
        for g, c in enumerate(counts):
            rows = rng.choice(k, c, replace=False)
            sub = rng.integers(1, 16, c)                          # a non-empty sub-mask per listed row
            for b in range(4):
                S[4 * g + b, rows] = (sub >> b) & 1 == 1
            assert int(S[4 * g:4 * g + 4].any(axis=0).sum()) == c
        dense_case(W8, S, True, [(F32, 'bool')], f'parts 15 counts={counts}', 't_vec')


PARTS_32_SHAPE, PARTS_32_ACTIVE = (20, 4_096), 5


def cross_parts_32():
    assert route(PARTS_32_SHAPE, 1, True, F32) == ('t_vec', 4)
    assert parts_for(PARTS_32_SHAPE[1], 4, 1) == K['parts_for.cap_one_group'] == 32 and PARTS_32_ACTIVE < 32


def test_t_vec_more_parts_than_active_rows(be):
    """k_densemm_t at the cap of 32 row parts with 5 listed rows: 27 parts find nothing and write zero partials."""
    cross_parts_32()
    S = np.zeros((1, PARTS_32_SHAPE[0]), bool)
    S[0, [0, 3, 7, 12, 19]] = True
    dense_case(weights(96, PARTS_32_SHAPE), S, True, [(F32, 'bool')], 'parts 32', 't_vec')


ROW_LOAD = {F32: {260: 4, 262: 1, 263: 1}, F64: {262: 2, 263: 1}, F16: {264: 8, 260: 1, 263: 1}, BF16: {264: 8, 260: 1, 263: 1}}
ROW_LOAD_K, ROW_LOAD_NB = 333, 3


def cross_row_load():
    for dtype, widths in ROW_LOAD.items():
        for n, vec in widths.items():
            assert route((ROW_LOAD_K, n), ROW_LOAD_NB, True, dtype) == ('t_vec', vec)
        assert vec_of(dtype) in widths.values() and 1 in widths.values()


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_row_load_width(be, dtype):
    """k_densemm_t through each RowLoad: 16 bytes per lane where the column count allows (f32 n % 4, f64 n % 2, f16 / bf16 n % 8)
    and one element per lane where it does not (an even and an odd count), five strips with a partly filled last one."""
    cross_row_load()
    S = draw(97, ROW_LOAD_NB, ROW_LOAD_K, 0.3)
    for n in ROW_LOAD[dtype]:
        dense_case(weights(97, (ROW_LOAD_K, n)), S, True, [(dtype, 'bool'), (dtype, 'float')], 'row load', 't_vec')


# =========================================================================================================== S @ W, MFMA kernels
MFMA_16 = ((40_000, 8), (8, 33), 0.3)


def cross_mfma_16(dtype, n_union):
    shape, nbs, _ = MFMA_16
    for nb in nbs:
        assert route(shape, nb, True, dtype)[0] == 't_mfma'
    parts, steps, per_part, chunk = t_mfma_geom(shape[1], dtype, n_union)
    assert parts == K['mfma.parts_clamp'] == 16 and n_union > 16_384
    assert per_part > 128 and per_part > chunk and per_part % chunk != 0, 'several staged chunks per part, the last one ragged'
    return per_part


@pytest.mark.parametrize('dtype', [F16, BF16])
def test_mfma_chunks_sixteen_parts(be, dtype):
    """k_densemm_mfma: about 37 700 union rows in 16 parts of 148 K-steps each — three staged chunks of 64, 64 and 20 per part,
    the ring running D zero steps past each chunk's end.  33 batch rows add a second pass of one row (47 steps per part)."""
    shape, nbs, firing = MFMA_16
    W8 = weights(98, shape)
    S_all = draw(98, max(nbs), shape[0], firing)
    for nb in nbs:
        S = np.ascontiguousarray(S_all[:nb])
        cross_mfma_16(dtype, union(S, 0, min(nb, 32)))
        dense_case(W8, S, True, [(dtype, 'bool')], 'mfma 16 parts', 't_mfma')


MFMA_1 = ((1_100, 98_312), 32, 0.5)


def cross_mfma_1(n_union):
    shape, nb, _ = MFMA_1
    assert route(shape, nb, True, F16)[0] == 't_mfma'
    parts, steps, per_part, chunk = t_mfma_geom(shape[1], F16, n_union)
    assert parts == 1 and n_union >= 1_040 and steps == per_part > chunk, 'a second staged chunk in a single part'
    assert nb * shape[1] > MFMA_REDUCE_SPAN, 'k_mfma_reduce: a second trip'


def test_mfma_chunks_one_part(be):
    """k_densemm_mfma at parts == 1 (385 column tiles): 1100 union rows are 69 K-steps, a chunk of 64 and one of 5 whose last
    step holds 12 rows.  32 x 98 312 outputs put k_mfma_reduce on its sixth trip."""
    shape, nb, firing = MFMA_1
    S = draw(99, nb, shape[0], firing)
    cross_mfma_1(union(S))
    ref = dense_case(weights(99, shape), S, True, [(F16, 'bool')], 'mfma 1 part', 't_mfma')
    assert np.count_nonzero(ref.reshape(-1)[MFMA_REDUCE_SPAN:]) > 0


TF_CHUNK = [((40_000, 8), 8, 0.3, 16), ((300, 196_612), 32, 0.5, 1)]      # (shape, nb, firing, parts)


def cross_tf_chunk(i, n_union):
    shape, nb, _, want_parts = TF_CHUNK[i]
    assert route(shape, nb, True, F32) == ('t_mfma', 4)
    parts, steps, per_part, chunk = t_mfma_geom(shape[1], F32, n_union)
    assert parts == want_parts and chunk == K['kTfChunk'] and per_part > chunk and per_part % chunk != 0, (parts, per_part)


@pytest.mark.parametrize('i', range(len(TF_CHUNK)))
def test_tf32_chunks(be, i):
    """k_densemm_t_mfma_f32: steps of two union rows, 128 staged at a time — 16 parts of about 1180 steps each, and one part of
    150 steps (193 workgroups of 512 columns, the last with 4)."""
    shape, nb, firing, _ = TF_CHUNK[i]
    S = draw(100 + i, nb, shape[0], firing)
    cross_tf_chunk(i, union(S))
    dense_case(weights(100, shape), S, True, [(F32, 'bool')], 'tf32 chunks', 't_mfma')


EMPTY = [((16, 8), F16), ((16, 8), BF16), ((16, 4), F32)]


def cross_empty():
    for shape, dtype in EMPTY:
        for nb in (8, 40):
            assert route(shape, nb, True, dtype)[0] == 't_mfma'
        parts, steps, per_part, _ = t_mfma_geom(shape[1], dtype, shape[0])
        assert parts == 16 and per_part * (parts - 1) >= steps, 'the last row part (at least) starts at or past the last step'
    assert passes(40) == [(0, 32), (32, 8)]


@pytest.mark.parametrize('i', range(len(EMPTY)))
def test_mfma_empty_ranges_and_silent_batches(be, i):
    """The S @ W MFMA kernels with 16 row parts and at most 16 union rows: most parts own an empty K range (t_begin past t_end)
    and write zeros.  Then no spike at all (n_union = 0: every output is an exact zero), and 40 batch rows whose last eight are
    silent (the second pass finds an empty union list)."""
    cross_empty()
    shape, dtype = EMPTY[i]
    W8 = weights(102, shape)
    dense_case(W8, draw(102, 8, shape[0], 0.5), True, [(dtype, 'bool'), (dtype, 'float')], 'empty ranges', 't_mfma')
    ref = dense_case(W8, np.zeros((8, shape[0]), bool), True, [(dtype, 'bool')], 'no spikes', 't_mfma')
    assert not ref.any()
    S = draw(103, 40, shape[0], 0.5)
    S[32:] = False
    ref = dense_case(W8, S, True, [(dtype, 'bool')], 'silent second pass', 't_mfma')
    assert ref[:32].any() and not ref[32:].any()


COL_TILES = [((640, 264), F16), ((640, 264), BF16), ((640, 516), F32)]
COL_TILES_NB = (9, 31, 32, 64, 65)


def cross_col_tiles():
    for shape, dtype in COL_TILES:
        cols = K['kMfmaCols'] * (2 if dtype == F32 else 1)
        assert cols < shape[1] < 2 * cols and shape[1] % vec_of(dtype) == 0, 'two column tiles, the second one vector wide'
        for nb in COL_TILES_NB:
            assert route(shape, nb, True, dtype)[0] == 't_mfma'


@pytest.mark.parametrize('i', range(len(COL_TILES)))
def test_mfma_partly_filled_column_tiles(be, i):
    """A second column tile that holds one 16-byte vector of columns (264 = 256 + 8 for f16 / bf16, 516 = 512 + 4 for f32), at
    9, 31, 32 batch rows (one pass, partly and fully used accumulator rows) and 64, 65 (two and three passes)."""
    cross_col_tiles()
    shape, dtype = COL_TILES[i]
    W8 = weights(104, shape)
    S_all = draw(104, max(COL_TILES_NB), shape[0], 0.3)
    for nb in COL_TILES_NB:
        dense_case(W8, np.ascontiguousarray(S_all[:nb]), True, [(dtype, 'bool')], 'column tiles', 't_mfma')


# =========================================================================================================== W @ S.T, MFMA kernels
NT_MFMA16 = [(4_097, 4_120), (4_097, 8_200)]
NT_MFMA16_NB = (8, 17, 33)
NT_MFMA_F32, NT_MFMA_F32_NB = (4_097, 4_100), (8, 33)


def cross_nt_mfma():
    for shape in NT_MFMA16:
        for dtype in (F16, BF16):
            for nb in NT_MFMA16_NB:
                assert route(shape, nb, False, dtype)[0] == 'nt_mfma'
        m, k = shape
        assert k > K['kNtChunk'] and k % K['kNtChunk'] != 0 and k % 32 != 0 and k % 8 == 0, 'a second mask chunk; a last step of 8 / 24 columns'
        assert m % 32 == 1, 'the last wave holds one real row: 31 clamped'
    assert -(-NT_MFMA16[1][1] // K['kNtChunk']) == 3
    m, k = NT_MFMA_F32
    for nb in NT_MFMA_F32_NB:
        assert route(NT_MFMA_F32, nb, False, F32)[0] == 'nt_mfma'
    assert k > K['kNtChunk'] and k % 8 == 4 and m % 32 == 1


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('shape', NT_MFMA16)
def test_nt_mfma16_mask_chunks(be, shape, dtype):
    """k_densemm_nt_mfma16: the masks of 4096 columns are staged in LDS at a time — 4120 and 8200 columns take a second and a
    third chunk, the last of 24 and 8 columns (a ragged last step: pieces past k are zeroed at use, their loads clamped into the
    row).  4097 rows: the last wave clamps 31 of its 32 rows.  8, 17 and 33 batch rows (both B fragments; a second pass of one)."""
    cross_nt_mfma()
    W8 = weights(105, shape)
    S_all = draw(105, max(NT_MFMA16_NB), shape[1], 0.3, last=True)
    assert S_all[:, K['kNtChunk']:].any(axis=1).all()
    for nb in NT_MFMA16_NB:
        dense_case(W8, np.ascontiguousarray(S_all[:nb]), False, [(dtype, 'bool')], 'nt mfma16 chunks', 'nt_mfma')


def test_nt_mfma_f32_mask_chunks(be):
    """k_densemm_nt_mfma_f32 on 4100 columns: a second mask chunk of 4 columns, half a step."""
    cross_nt_mfma()
    W8 = weights(106, NT_MFMA_F32)
    S_all = draw(106, max(NT_MFMA_F32_NB), NT_MFMA_F32[1], 0.3, last=True)
    for nb in NT_MFMA_F32_NB:
        dense_case(W8, np.ascontiguousarray(S_all[:nb]), False, [(F32, 'bool')], 'nt mfma f32 chunks', 'nt_mfma')


SHORTEST = [((4_097, 32), F16), ((4_097, 40), F16), ((4_097, 32), BF16), ((4_097, 40), BF16), ((4_097, 8), F32), ((4_097, 12), F32)]
SHORTEST_NB = (8, 32)


def cross_shortest():
    for shape, dtype in SHORTEST:
        low = K['nt_mfma.min_cols_f32'] if dtype == F32 else K['nt_mfma.min_cols_16bit']
        assert shape[1] in (low, low + vec_of(dtype))
        for nb in SHORTEST_NB:
            assert route(shape, nb, False, dtype)[0] == 'nt_mfma'
            assert route((shape[0], low - vec_of(dtype)), nb, False, dtype)[0] == 'nt_vec'


@pytest.mark.parametrize('i', range(len(SHORTEST)))
def test_nt_mfma_shortest_contractions(be, i):
    """The shortest contractions densemm_any gives to the W @ S.T MFMA kernels (32 for f16 / bf16, 8 for f32) and one vector
    more: every ring slot past the first step loads from a clamped address and is zeroed at use."""
    cross_shortest()
    shape, dtype = SHORTEST[i]
    W8 = weights(107, shape)
    S_all = draw(107, max(SHORTEST_NB), shape[1], 0.5, last=True)
    for nb in SHORTEST_NB:
        dense_case(W8, np.ascontiguousarray(S_all[:nb]), False, [(dtype, 'bool'), (dtype, 'float')], 'shortest', 'nt_mfma')


# =========================================================================================================== operands
BITS_ROUTES = [((333, 8), 3, True, F32, 't_vec'), ((333, 8), 9, True, F16, 't_mfma'), ((8, 333), 3, False, F32, 'nt_vec'),
               ((4_097, 40), 8, False, F16, 'nt_mfma')]


def cross_bits_routes():
    for shape, nb, transpose, dtype, want in BITS_ROUTES:
        assert route(shape, nb, transpose, dtype)[0] == want
        assert (shape[0] if transpose else shape[1]) % 32 != 0, 'a partly used last word per batch row'
    assert {r[4] for r in BITS_ROUTES} == {'t_vec', 't_mfma', 'nt_vec', 'nt_mfma'}


@pytest.mark.parametrize('i', range(len(BITS_ROUTES)))
def test_bit_packed_batches_on_every_route(be, i):
    """be_binary_densemm with BE_SPIKE_BITS (batch rows of ceil(k / 32) words) on each of the four host routes:
    k_dense_masks_bits (t_vec, nt_mfma) and k_dense_masks_count_bits (t_mfma, nt_vec), k % 32 != 0.  (k = 524 588:
    test_mask_stride_loops.)"""
    cross_bits_routes()
    shape, nb, transpose, dtype, want = BITS_ROUTES[i]
    k = shape[0] if transpose else shape[1]
    dense_case(weights(108, shape), draw(108, nb, k, 0.3, last=True), transpose, [(dtype, 'bits'), (dtype, 'bool')], 'bits', want)


OFF_ALIGNMENT = [((8, 4_104), 3, False, F32, 'nt_vec'), ((4_104, 8), 8, True, F16, 't_mfma')]


def cross_off_alignment():
    for shape, nb, transpose, dtype, want in OFF_ALIGNMENT:
        assert route(shape, nb, transpose, dtype)[0] == want, 'the routes that launch k_dense_masks_count'
        k = shape[0] if transpose else shape[1]
        assert k % 8 == 0 and n_tiles_of(k) == 3 and k % K['kTile'] == 8


@pytest.mark.parametrize('i', range(len(OFF_ALIGNMENT)))
def test_spike_operand_off_alignment(be, i):
    """A bool operand that starts one byte into a larger buffer, k % 8 == 0: k_dense_masks_count must not take its 8-byte loads
    and builds the masks spike by spike.  Same bits as the aligned run (and as the reference)."""
    cross_off_alignment()
    shape, nb, transpose, dtype, want = OFF_ALIGNMENT[i]
    k = shape[0] if transpose else shape[1]
    W8, S = weights(109, shape), draw(109, nb, k, 0.3, last=True)
    ref = reference(W8, S, transpose)
    Wd = torch.from_numpy(W8).cuda().to(dtype)
    aligned = run(Wd, S, 'bool', transpose, ref, 'aligned')
    shifted = run(Wd, S, 'bool+1', transpose, ref, 'one byte off')
    assert torch.equal(aligned, shifted)


# =========================================================================================================== without a device
def check_all_crossings():
    """Every crossing assertion above, without a device: the spikes the cases draw are drawn here too where a union count decides."""
    cross_gl_scan_t_vec()
    for i, (shape, nb, firing, _, _) in enumerate(SCAN_NT_VEC):
        cross_scan_nt_vec(i, union(draw(82 + i, nb, shape[1], firing, last=True)))
    cross_scan_t_mfma()
    cross_self_scan()
    cross_masks()
    cross_nt_rows()
    cross_nt_split()
    cross_parts_one()
    cross_parts_15()
    cross_parts_32()
    cross_row_load()
    S_all = draw(98, max(MFMA_16[1]), MFMA_16[0][0], MFMA_16[2])
    for dtype in (F16, BF16):
        for nb in MFMA_16[1]:
            assert cross_mfma_16(dtype, union(S_all, 0, min(nb, 32))) > 2 * K['kMfmaChunk']
    cross_mfma_1(union(draw(99, MFMA_1[1], MFMA_1[0][0], MFMA_1[2])))
    for i, (shape, nb, firing, _) in enumerate(TF_CHUNK):
        cross_tf_chunk(i, union(draw(100 + i, nb, shape[0], firing)))
    cross_empty()
    cross_col_tiles()
    cross_nt_mfma()
    cross_shortest()
    cross_bits_routes()
    cross_off_alignment()
