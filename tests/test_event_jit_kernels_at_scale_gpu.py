"""The event-driven JIT-connectivity products (csrc/be_jitc.hip, csrc/be_jitc_shared.h: binary_jit{s,u,n}{mv,mm}, the sharded entry
points and the materialisation) past their one-pass sizes: every grid-stride loop, LDS window, LDS piece, `parts` split and tail
branch of the two files is crossed by a named case and compared with a float64 reference, oracle_c.jit_float on the 0/1 image of the
spikes (tests/test_oracle.py pins it against the numpy oracle and, on a 0/1 vector, against oracle_c.jitmv).

Assertion policy (that of tests/test_float_kernels_at_scale_gpu.py, whose helpers are imported): the scalar family carries the
weight 3.0, every sum is an integer below 2**24 and the result must EQUAL the reference rounded once to the output dtype.  The
generated-weight families (uniform (0.5, 1.5), normal (2.0, 0.125) and their negatives) are compared under the bound `event_bound`
derives from the route's arithmetic; every bounded case asserts on the host, before the device is touched, that its largest bound is
at most a quarter of the smallest addend (a lost or doubled edge cannot hide) and every case that more than 2 % of the reference's
outputs are non-zero.  Every case first asserts from the CONSTS table (tests/test_event_jit_kernels_thresholds_cpu.py compares it
with the sources) that its sizes cross the bound it is there for; `check_all_crossings` repeats those assertions without a device.

Which loop or branch is reached where:
  k_jit_mv_gather row loop, second trip, m % 32 != 0, all operand kinds      test_mv_gather_row_loop_second_trip
  k_jit_gather_reduce loop (more than 524 288 rows)                            test_gather_reduce_second_trip
  k_jit_mv_gather<.., false> (bits from global) and the largest LDS chunk      test_mv_gather_bits_from_global_memory
  k_jit_mm_gather_lds with 2 / 3 windows (wstate / wq carry), u8 / u16 / u32   test_mm_gather_lds_windows
  k_jit_masks, k_jit_masks<SpikeFloat>, k_jit_masks_bits second trip           test_mm_gather_lds_windows[*-u8]
  b0 loop of be_binary_jitmm (33 / 40 columns), second pass at narrower masks  test_mm_gather_lds_windows[*-u32]
  k_jit_convert loop (out_len * n > 524 288), f32 scratch at b0 = 32           test_convert_loop_and_f32_scratch_beyond_32_columns
  k_jit_mm_gather (global masks), NCOL = 32 / 16 / 8                           test_mm_gather_global_masks
  k_jit_mv_scatter<MODE_SCALAR, false>, several pieces, last partly filled     test_mv_scatter_several_pieces[s]
  k_jit_mv_scatter<uniform / normal, false> against the oracle, negatives      test_mv_scatter_several_pieces[u / n]
  mm scatter (stride 4): several pieces, parts 8 / 2 / 1, reduce tail, b > 0   test_mm_scatter_several_pieces_and_parts
  scatter `a` loop second trip (active rows > parts * 1024), parts 2 / 16 / 5  test_scatter_active_row_loop_second_trip
  hundreds of chunks / one chunk narrower than the lane stride, negatives      test_chunk_geometry
  armed workspaces: equal byte size, other column count; firing 0.0 then 0.9   test_scatter_workspace_reuse
  be_binary_jitmv_rows with row0 past the first trip; be_binary_jitmv_sharded  test_gather_shard_beyond_one_trip, test_scatter_shards_several_pieces
  k_jit_csr_count / k_jit_csr_fill task loop (more than 2 097 152 tasks)       test_materialisation_beyond_one_grid
"""
import math

import numpy as np
import pytest
import torch

from brainevent_amd import _array as A
from brainevent_amd import _jitc as J
from brainevent_amd._dist import post_slice_bounds
from brainevent_amd._lib import check
from oracle import oracle_c
from test_float_kernels_at_scale_gpu import (DTYPES, HALF_ULP, JIT_PARAMS, NORMAL_WEIGHT_RTOL, W_MAX, W_MIN, assert_exact, bits, jit_chunks,
                                             scatter_pieces)

pytestmark = pytest.mark.gpu

# The loop bounds of be_jitc.hip / be_jitc_shared.h as the cases below use them.
CONSTS = {
    'mv_gather.rows_per_block': 32,       # gcap(m, 32, 512): 1024 threads = 32 half-waves, a row each (jit_mv_gather)
    'mv_gather.grid_cap': 512,
    'lds_limit': 150 * 1024,              # a chunk's packed spikes in LDS up to here (jit_mv_gather)
    'gather_reduce.grid_cap': 2048,       # k_jit_gather_reduce: gcap(m, 256, 2048)
    'masks.grid_cap': 2048,               # k_jit_masks / k_jit_masks<SpikeFloat> / k_jit_masks_bits: gcap(in_len, 256, 2048)
    'convert.grid_cap': 2048,             # k_jit_convert: gcap(out_len * n, 256, 2048)
    'mm.lds_window_bytes': 128 * 1024,    # masks of one window of k_jit_mm_gather_lds (jit_mm_run)
    'mm.max_windows': 256,                # more windows than this: k_jit_mm_gather (masks from global memory)
    'mm_global.grid_cap': 4096,           # k_jit_mm_gather: gcap(rows, 256, 4096)
    'materialise.grid_cap': 8192,         # k_jit_csr_count / k_jit_csr_fill: gcap(tasks, 256, 8192)
    'edge_weights.grid_cap': 8192,        # k_jit_edge_weights: gcap(n, 256, 8192)
    'kPieceU32': 32768,                   # LDS counters of one scalar-family scatter workgroup
    'kPieceU64': 16384,                   # LDS fixed-point sums of one uniform / normal scatter workgroup
    'wg_target': 256,                     # BE_JIT_WG_TARGET: scatter workgroups (classes x pieces x parts x columns) aimed at
    'parts_clamp': 16,                    # parts = clamp(wg_target / (classes * pieces * columns), 1, 16)
}
K = CONSTS
MV_GATHER_TRIP = K['mv_gather.rows_per_block'] * K['mv_gather.grid_cap']       # 16 384 output rows per trip of the row loop
REDUCE_SPAN = 256 * K['gather_reduce.grid_cap']                                # 524 288
MASKS_SPAN = 256 * K['masks.grid_cap']                                         # 524 288
CONVERT_SPAN = 256 * K['convert.grid_cap']                                     # 524 288
MATERIALISE_SPAN = 256 * K['materialise.grid_cap']                             # 2 097 152 (row, chunk, lane) tasks
EDGE_WEIGHTS_SPAN = 256 * K['edge_weights.grid_cap']                           # 2 097 152 listed edges
LDS_CHUNK_MAX = (K['lds_limit'] // 4 - 2) * 32                                 # 1 228 736: widest chunk whose bits are staged in LDS
SCATTER_BLOCK = 1024                                                           # threads of k_jit_mv_scatter: active rows per part and trip

# The float file's families and their negatives: |w| >= W_MIN in both, so the same guard applies.
PARAMS = dict(JIT_PARAMS)
PARAMS.update({'u-': (-1.5, -0.5), 'n-': (-2.0, 0.125)})
F32, F64, F16, BF16 = DTYPES
assert (F32, F64, F16, BF16) == (torch.float32, torch.float64, torch.float16, torch.bfloat16)


# =========================================================================================================== host side
def in_out(shape, transpose):
    return (shape[0], shape[1]) if transpose else (shape[1], shape[0])


def fixed_scale_exp(wmax, n_rows):
    """jit_scale_exp (be_jitc.hip, the mm path) and _jitc._fixed_scale_exp (the mv path) restated: |w| 2^e n_rows < 2^62."""
    e = math.frexp(wmax)[1] if wmax > 0 else 0
    lg = 1
    while (1 << lg) < n_rows + 1:
        lg += 1
    return max(-90, min(150, 62 - e - lg))


def scatter_geom(shape1, out_len, stride, scalar, n_cols=1):
    """scatter_geom (be_jitc_shared.h) restated: (classes, largest Q of a class, pieces, piece_len, parts)."""
    chunk, n_chunks = jit_chunks((0, shape1), out_len)
    classes = n_chunks * stride
    q_max = -(-min(chunk, out_len) // stride)
    pieces = max(1, -(-q_max // (K['kPieceU32'] if scalar else K['kPieceU64'])))
    per_piece = -(-q_max // pieces)
    piece_len = max(256, (per_piece + 255) & ~255)
    parts = max(1, min(K['wg_target'] // max(1, classes * pieces * n_cols), K['parts_clamp']))
    return classes, q_max, pieces, piece_len, parts


def mm_windows(shape1, walk_len, nc):
    """jit_mm_run restated: (bytes per mask, windows per chunk, columns per window)."""
    mask_sz = 1 if nc <= 8 else (2 if nc <= 16 else 4)
    chunk_cols = min(jit_chunks((0, shape1), walk_len)[0], walk_len)
    win_cap = K['mm.lds_window_bytes'] // mask_sz
    n_win = -(-chunk_cols // win_cap)
    return mask_sz, n_win, -(-chunk_cols // n_win)


def draw_spikes(seed, size, firing):
    return np.random.default_rng(seed).random(size) < firing


def reference(key, spk, shape, transpose, corder, prob, seed, stride):
    p = PARAMS[key]
    w0, w1 = (p[0], 0.0) if key == 's' else p
    ref = oracle_c.jit_float(key[0], w0, w1, prob, np.asarray(spk, np.float64), seed, shape=shape, transpose=transpose, corder=corder,
                             stride=stride)
    assert ref.dtype == np.float64
    return ref


def event_bound(key, route, dtype, ref, in_len):
    """Largest |device - reference| a correct kernel can show at each output, for the generated-weight families.  The operand is
    0/1 and all weights of a family have one sign, so S = sum |w| over the output's addends = |ref|, and the number of addends
    A <= S / W_MIN.  The oracle forms every weight in f32 and sums in double.
      mv_gather:  k_jit_mv_gather forms the weight in f32 (edge_weight<MODE, float>: the oracle's own), sums a lane's edges, the
                  32 lanes and (k_jit_gather_reduce) the chunk partials in double and stores once:            A 2^-53 S
      scatter:    (mv and mm) the f32 weight is cut to a multiple of 2^-e by fixed_from_f32 (it floors: the negative side too);
                  the 64-bit integer sums are exact; k_jit_scatter_reduce converts (long long) sum * 2^-e in double and passes it
                  through an f32 tile for every output type but f64.  e = _jitc._fixed_scale_exp(wmax, in_len) on the mv path,
                  jit_scale_exp (the same formula, restated in fixed_scale_exp) on the mm path:                A 2^-e + u |ref|,
                  u = 2^-24 | 2^-53 (f64)
      mm_gather:  f32 / f16 / bf16 outputs: f32 weight, sequential f32 adds in a register (acc_add_inplace):   A 2^-24 S
                  f64 outputs: the sums are double (A 2^-53 S) but the WEIGHT is formed in double as well
                  (edge_weight<MODE, double>: w0 + r * w1 without the two f32 roundings of the oracle's weight, each at most
                  2^-24 W_MAX):                                                                                + A 2^-23 W_MAX
      normal:     every weight may differ from the oracle's by NORMAL_WEIGHT_RTOL of the largest weight        + A rtol W_MAX
    plus one rounding of the result to the output dtype (HALF_ULP |ref|)."""
    fam = key[0]
    S = np.abs(ref)
    A_ = np.ceil(S / W_MIN[fam])
    if route == 'mv_gather':
        b = A_ * 2.0 ** -53 * S
    elif route == 'scatter':
        wmax = J._jit_params(fam, *PARAMS[key])[2]
        e = fixed_scale_exp(wmax, in_len)
        assert e == J._fixed_scale_exp(wmax, in_len)
        b = A_ * 2.0 ** -e + (2.0 ** -53 if dtype == F64 else 2.0 ** -24) * S
    elif route == 'mm_gather':
        b = A_ * 2.0 ** -53 * S + A_ * 2.0 ** -23 * W_MAX[fam] if dtype == F64 else A_ * 2.0 ** -24 * S
    else:
        raise ValueError(route)
    if fam == 'n':
        b = b + A_ * NORMAL_WEIGHT_RTOL * W_MAX['n']
    return b + HALF_ULP[dtype] * S


def expectation(key, route, dtype, ref, in_len):
    """The bound of a (reference, route, dtype) or None for the exact family, with the host-side checks of the policy."""
    assert np.count_nonzero(ref) > ref.size // 50, 'the case must compare sums, not zeros'
    if key == 's':
        assert float(np.abs(ref).max()) < 2.0 ** 24
        return None
    assert (ref <= 0).all() if key.endswith('-') else (ref >= 0).all()
    bound = event_bound(key, route, dtype, ref, in_len)
    assert float(bound.max()) <= 0.25 * W_MIN[key[0]], (
        f'bound {bound.max()} could hide a lost edge of weight {W_MIN[key[0]]} (largest |sum| {np.abs(ref).max()})')
    return bound


# =========================================================================================================== device side
def vector_operand(spk, kind):
    t = torch.from_numpy(spk).cuda()
    if kind == 'bool':
        return t
    if kind == 'float':
        return t.to(torch.float32)
    from brainevent_amd import bitpack
    return A.PackedSpikes(bitpack(t, 0).reshape(-1), spk.shape[0])          # the words themselves (BE_SPIKE_BITS): no pack launch


def matrix_operand(spk, kind):
    """[in_len, n] as the ops take it: the transposed view of a batch-major buffer (nothing is copied on the way in)."""
    s = torch.from_numpy(np.ascontiguousarray(spk.T)).cuda()
    return (s if kind == 'bool' else s.to(torch.float32)).T


def weight_args(key, dtype):
    return tuple(torch.tensor(p, dtype=dtype) for p in PARAMS[key])


def product(key, dtype, op, shape, transpose, corder, prob, seed, mm):
    call = getattr(J, f"binary_jit{key[0]}{'mm' if mm else 'mv'}_p_call")
    return call(*weight_args(key, dtype), J._initialize_conn_length(prob), op, seed, shape=shape, transpose=transpose, corder=corder)[0]


def product_mm_words(key, dtype, words, n, shape, transpose, corder, prob, seed):
    """be_binary_jitmm on a bit-packed batch (n rows of ceil(in_len / 32) words, BE_SPIKE_BITS): the C entry point itself, since
    the Python ops hand packed words over for vectors only."""
    in_len, out_len = in_out(shape, transpose)
    assert tuple(words.shape) == (n, (in_len + 31) // 32) and words.is_contiguous()
    out_bm = torch.empty((n, out_len), dtype=dtype, device='cuda')
    w0, w1, _ = J._jit_params(key[0], *(PARAMS[key] + (None,))[:2])
    gather = 1 if corder else 0
    ws = A.workspace(J.fn('be_binary_jitmm_workspace_bytes')(int(shape[1]), in_len, out_len, n, gather))
    check(J.fn('be_binary_jitmm')(J._FAMILY[key[0]], w0, w1, A.wcode(out_bm), J._initialize_conn_length(prob), seed & 0xFFFFFFFF,
                                   A.ptr(words), A.BE_SPIKE_BITS, A.ptr(out_bm), int(shape[1]), in_len, out_len, n, gather, A.ptr(ws),
                                   ws.numel(), A.stream_ptr()), 'be_binary_jitmm')
    return out_bm.T


def pack_rows(spk_bm):
    """[n, len] bool (host) -> [n, ceil(len / 32)] words on the device, bit i % 32 of word i // 32."""
    n, length = spk_bm.shape
    pad = (-length) % 32
    b = np.packbits(np.pad(spk_bm, ((0, 0), (0, pad))), axis=1, bitorder='little')
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int32)).cuda()


def compare(got, ref, bound, dtype, tag):
    if bound is None:
        return assert_exact(got, ref, dtype, tag)
    assert isinstance(got, torch.Tensor) and got.dtype == dtype and tuple(got.shape) == ref.shape, (tag, got.dtype, tuple(got.shape))
    err = np.abs(got.detach().cpu().to(torch.float64).numpy() - ref)
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (f'{tag}: {int((err > bound).sum())} of {err.size} outputs outside their bound; worst at flat index '
                                  f'{worst}: error {err.reshape(-1)[worst]}, bound {bound.reshape(-1)[worst]}')


def event_case(key, route, dtype, spk, ref, shape, transpose, corder, prob, seed, tag, kind='bool', repeat=False):
    """One product on the device against `ref` (the oracle on these spikes).  A 1-D `spk` runs the mv op (stride 32), a 2-D one the
    mm op (stride 4).  `kind`: 'bool' | 'float' | 'bits'."""
    assert corder == route.endswith('gather')
    mm = spk.ndim == 2
    in_len, out_len = in_out(shape, transpose)
    assert spk.shape[0] == in_len and ref.shape[0] == out_len
    tag = f'{tag} binary_jit{key}{"mm" if mm else "mv"} {dtype} {kind}' + (f' n={spk.shape[1]}' if mm else '')
    bound = expectation(key, route, dtype, ref, in_len)

    def run():
        if mm and kind == 'bits':
            return product_mm_words(key, dtype, pack_rows(np.ascontiguousarray(spk.T)), spk.shape[1], shape, transpose, corder, prob, seed)
        op = matrix_operand(spk, kind) if mm else vector_operand(spk, kind)
        return product(key, dtype, op, shape, transpose, corder, prob, seed, mm)
    got = run()
    compare(got, ref, bound, dtype, tag)
    if repeat:      # integer and fixed-point sums do not depend on the order of the LDS atomics: a second call gives the same bits
        assert torch.equal(bits(got), bits(run())), f'{tag}: not repeatable'
    return got


def keys_of(family, negative=False):
    return [family] + ([family + '-'] if negative and family != 's' else [])


# =========================================================================================================== mv gather
GATHER_ROWS = [((MV_GATHER_TRIP + 133, 3000), False), ((3000, MV_GATHER_TRIP + 133), True)]      # (shape, transpose): 16 517 outputs


def cross_mv_gather_rows(m):
    blocks = min(K['mv_gather.grid_cap'], -(-m // K['mv_gather.rows_per_block']))
    trip = blocks * K['mv_gather.rows_per_block']
    assert blocks == K['mv_gather.grid_cap'] and m > trip, 'the row loop must take a second trip'
    assert m % 32 != 0 and m % trip != 0, 'the padded trip (m_round) must end inside a half-wave block'
    return trip


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_mv_gather_row_loop_second_trip(be, family):
    """k_jit_mv_gather: 32 rows per block, 512 blocks — 16 517 outputs put the row loop on a second trip that ends 133 rows into its
    16 384 (m_round pads it: the 32-lane shuffle runs in every half-wave, the store only where row < m).  Both transpose values (four
    chunks of 750 / one chunk cut at the walk's end); bool, float and bit-packed vectors; every dtype on the scalar family."""
    for shape, transpose in GATHER_ROWS:
        in_len, m = in_out(shape, transpose)
        assert cross_mv_gather_rows(m) == MV_GATHER_TRIP
        spk = draw_spikes(61, in_len, 0.3)
        ref = reference(family, spk, shape, transpose, True, 0.02, 61, 32)
        cases = [('bool', F32), ('float', F32), ('bits', F32), ('bool', F64)] + ([('bits', F16), ('float', BF16)] if family == 's' else [])
        for kind, dtype in cases:
            got = event_case(family, 'mv_gather', dtype, spk, ref, shape, transpose, True, 0.02, 61, f'shape={shape}', kind=kind)
            assert int(torch.count_nonzero(got[MV_GATHER_TRIP:])) > 0, 'the second trip must hold non-zero outputs'


REDUCE_SHAPE = (REDUCE_SPAN + 12, 256)


@pytest.mark.parametrize('family', ['s', 'u'])
def test_gather_reduce_second_trip(be, family):
    """k_jit_gather_reduce: 2048 blocks of 256 — more than 524 288 output rows put its loop on a second trip (and the row loop of
    k_jit_mv_gather on its 33rd)."""
    shape = REDUCE_SHAPE
    assert shape[0] > REDUCE_SPAN and -(-shape[0] // 256) > K['gather_reduce.grid_cap']
    spk = draw_spikes(62, shape[1], 0.5)
    ref = reference(family, spk, shape, False, True, 0.1, 62, 32)
    got = event_case(family, 'mv_gather', F32, spk, ref, shape, False, True, 0.1, 62, f'shape={shape}')
    assert int(torch.count_nonzero(got[REDUCE_SPAN:])) > 0, 'the second trip must hold non-zero outputs'


BITS_GLOBAL_SHAPES = [((40, 4 * LDS_CHUNK_MAX + 420), False), ((40, 4 * LDS_CHUNK_MAX - 1), True)]      # (shape, bits staged in LDS)


def cross_bits_in_lds(shape, in_lds):
    chunk, n_chunks = jit_chunks(shape, shape[1])
    lds = (-(-min(chunk, shape[1]) // 32) + 2) * 4
    assert n_chunks == 4 and (lds <= K['lds_limit']) == in_lds, (chunk, lds)
    if in_lds:
        assert chunk == LDS_CHUNK_MAX and lds == K['lds_limit'], 'the largest chunk that is still staged in LDS'
    else:
        assert chunk > LDS_CHUNK_MAX


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_mv_gather_bits_from_global_memory(be, family):
    """k_jit_mv_gather<MODE, false>: a chunk of more than 1 228 736 columns does not fit the 150 KB of LDS and its bits are read from
    global memory; one column count below, the LDS branch at its very largest."""
    for shape, in_lds in BITS_GLOBAL_SHAPES:
        cross_bits_in_lds(shape, in_lds)
        spk = draw_spikes(63, shape[1], 0.3)
        ref = reference(family, spk, shape, False, True, 0.0005, 63, 32)
        event_case(family, 'mv_gather', F32, spk, ref, shape, False, True, 0.0005, 63, f'shape={shape}')


# =========================================================================================================== mm gather
# mask width -> (shape, prob, column counts, windows per chunk)
MM_LDS = {'u8': ((1100, 1_048_709), 0.002, (1, 7, 8), 3), 'u16': ((1100, 500_003), 0.004, (9, 16), 2),
          'u32': ((2100, 280_003), 0.004, (17, 32, 33, 40), 3)}


def cross_mm_windows(width):
    shape, _, cols, windows = MM_LDS[width]
    chunk, n_chunks = jit_chunks(shape, shape[1])
    for n in cols:
        first = min(n, 32)
        mask_sz, n_win, win_cols = mm_windows(shape[1], shape[1], first)
        assert mask_sz == {'u8': 1, 'u16': 2, 'u32': 4}[width] and n_win == windows and n_win <= K['mm.max_windows'], (n, mask_sz, n_win)
        assert 0 < chunk - (n_win - 1) * win_cols < win_cols, 'the last window must be partly filled'
        if n > 32:       # the second pass of the b0 loop: narrower masks, one window
            assert mm_windows(shape[1], shape[1], n - 32)[:2] == (1, 1)
    assert n_chunks == 4 and shape[1] - 3 * chunk < chunk, 'the last chunk is cut at the walk end'
    assert shape[0] % 1024 != 0 and -(-shape[0] // 1024) == (3 if width == 'u32' else 2)
    if width == 'u8':
        assert shape[1] > MASKS_SPAN, 'k_jit_masks*: a second trip of 2048 blocks of 256'


@pytest.mark.parametrize('width', ['u8', 'u16', 'u32'])
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_mm_gather_lds_windows(be, family, width):
    """k_jit_mm_gather_lds with a chunk swept in 3 (u8, u32) and 2 (u16) windows whose last is partly filled: the four walks of a row
    carry wstate / wq from window to window.  m = 1100 / 2100: two / three workgroups of 1024, the last partly idle.  33 and 40
    columns take a second pass of the b0 loop, with narrower masks in one window, into the outputs from column 32 on.  The u8 shape
    also puts the three mask kernels on a second trip.  One float and one bit-packed operand per mask width."""
    cross_mm_windows(width)
    shape, prob, cols, _ = MM_LDS[width]
    seed = 64
    spk_all = draw_spikes(seed, (shape[1], max(cols)), 0.2)
    ref_all = reference(family, spk_all, shape, False, True, prob, seed, 4)       # a column's sums do not depend on the other columns
    for n in cols:
        spk, ref = np.ascontiguousarray(spk_all[:, :n]), np.ascontiguousarray(ref_all[:, :n])
        dtypes = [F32] + ([F64, F16, BF16] if family == 's' and n in (8, 16, 33) else []) + ([F64] if family != 's' and n in (9, 33) else [])
        for dtype in dtypes:
            event_case(family, 'mm_gather', dtype, spk, ref, shape, False, True, prob, seed, f'shape={shape}')
        if n == cols[-1]:
            for kind in ('float', 'bits'):
                event_case(family, 'mm_gather', F32, spk, ref, shape, False, True, prob, seed, f'shape={shape}', kind=kind)


CONVERT_SHAPE, CONVERT_COLS = (CONVERT_SPAN // 40 + 70, 3000), 40


def test_convert_loop_and_f32_scratch_beyond_32_columns(be):
    """f16 / bf16 mm gather: the kernels write an f32 scratch that k_jit_convert rounds — out_len * n above 524 288 puts its loop on a
    second trip, and 40 columns put the second pass of the b0 loop at column 32 of that scratch."""
    shape, n = CONVERT_SHAPE, CONVERT_COLS
    assert shape[0] * n > CONVERT_SPAN and n > 32
    spk = draw_spikes(65, (shape[1], n), 0.3)
    ref = reference('s', spk, shape, False, True, 0.02, 65, 4)
    for dtype in (F16, BF16):
        got = event_case('s', 'mm_gather', dtype, spk, ref, shape, False, True, 0.02, 65, f'shape={shape}')
        assert int(torch.count_nonzero(got[:, 32:])) > 0 and int(torch.count_nonzero(got.T.reshape(-1)[CONVERT_SPAN:])) > 0


# NCOL of k_jit_mm_gather -> (batch columns, shape, columns that carry spikes)
MM_GLOBAL = {32: (17, (48, 4 * 8_388_608 + 500), (0, 8, 16)), 16: (9, (48, 4 * 16_777_216 + 500), (0, 8)),
             8: (8, (48, 4 * 33_554_432 + 500), (0, 7))}


def cross_mm_global(ncol):
    n, shape, carrying = MM_GLOBAL[ncol]
    mask_sz, n_win, _ = mm_windows(shape[1], shape[1], n)
    assert mask_sz == ncol // 8 and n_win > K['mm.max_windows'], (mask_sz, n_win)
    assert max(carrying) < n and shape[0] < 256 * K['mm_global.grid_cap']


@pytest.mark.parametrize('ncol', [32, 16, 8])
@pytest.mark.parametrize('family', ['s', 'u'])
def test_mm_gather_global_masks(be, family, ncol):
    """k_jit_mm_gather (masks read from global memory): a chunk that would need more than 256 LDS windows — 33.5 M / 67 M / 134 M
    input columns for 17 / 9 / 8 batch columns, the three NCOL variants.  48 generator rows; two or three columns carry about 500
    spikes' worth of addends per output, the others are all zero and must give exact zeros.  The operand is bit-packed (8 to 134 MB on
    the device) and the reference is taken one column at a time, so the host never holds in_len * n doubles."""
    cross_mm_global(ncol)
    n, shape, carrying = MM_GLOBAL[ncol]
    prob, seed = 0.0005, 66
    in_len = shape[1]
    firing = 500.0 / (in_len * prob)
    words = torch.zeros((n, (in_len + 31) // 32), dtype=torch.int32, device='cuda')
    refs = {}
    for c in carrying:
        rng = np.random.default_rng(seed + c)
        spk = np.zeros(in_len, bool)
        spk[rng.integers(0, in_len, int(firing * in_len))] = True
        spk[-1] = True                                            # the last mask of the last chunk counts
        words[c] = pack_rows(spk[None, :])[0]
        refs[c] = reference(family, spk, shape, False, True, prob, seed, 4)
        del spk
        expectation(family, 'mm_gather', F32, refs[c], in_len)
    got = product_mm_words(family, F32, words, n, shape, False, True, prob, seed)
    assert got.dtype == F32 and tuple(got.shape) == (shape[0], n)
    for c in range(n):
        if c in refs:
            compare(got[:, c], refs[c], expectation(family, 'mm_gather', F32, refs[c], in_len), F32, f'shape={shape} n={n} column {c}')
        else:
            assert int(torch.count_nonzero(got[:, c])) == 0, f'column {c} has no spikes'
    del words, got
    torch.cuda.empty_cache()


# =========================================================================================================== scatter
MV_PIECES = {'s': (300, 4 * 32 * K['kPieceU32'] + 2851), 'u': (300, 4 * 32 * K['kPieceU64'] + 2851), 'n': (300, 4 * 32 * K['kPieceU64'] + 2851)}


def cross_pieces(shape, stride, scalar, n_cols=1):
    classes, q_max, pieces, piece_len, parts = scatter_geom(shape[1], shape[1], stride, scalar, n_cols)
    assert pieces >= 2, (q_max, pieces)
    assert 0 < q_max - (pieces - 1) * piece_len < piece_len, 'the last piece must be partly filled'
    if not scalar:
        assert scatter_pieces(shape, shape[1], stride) == (q_max, pieces, piece_len)
    return classes, pieces, parts


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_mv_scatter_several_pieces(be, family):
    """k_jit_mv_scatter<MODE, ONE_PIECE = false>, stride 32: a residue class has more positions than one workgroup's LDS holds
    (32 768 counters, 16 384 fixed-point sums), so it is cut into pieces of a multiple of 256 and a walk adds only where
    qb <= q < qe, at slot q - qb; the last piece is partly filled.  Scalar: the four dtypes; uniform / normal: f32 and f64 and one
    negatively weighted case (the fixed-point split floors).  Every call repeats bit for bit."""
    shape = MV_PIECES[family]
    cross_pieces(shape, 32, family == 's')
    spk = draw_spikes(67, shape[0], 0.5)
    for key in keys_of(family, negative=True):
        ref = reference(key, spk, shape, True, False, 0.005, 67, 32)
        for dtype in (DTYPES if key == 's' else [F32, F64] if key == family else [F32]):
            event_case(key, 'scatter', dtype, spk, ref, shape, True, False, 0.005, 67, f'shape={shape}', repeat=True)


MM_PIECES = {'s': (200, 4 * 4 * K['kPieceU32'] + 27), 'u': (200, 4 * 4 * K['kPieceU64'] + 27), 'n': (200, 4 * 4 * K['kPieceU64'] + 27)}
MM_PIECES_PARTS = {1: 8, 3: 2, 8: 1, 33: 1, 40: 1}       # columns -> parts: 256 // (16 classes * 2 pieces * columns), at least 1


def cross_mm_pieces(family):
    shape = MM_PIECES[family]
    for n, parts in MM_PIECES_PARTS.items():
        classes, pieces, got_parts = cross_pieces(shape, 4, family == 's', n)
        assert (classes, pieces, got_parts) == (16, 2, parts), (n, classes, pieces, got_parts)
    chunk, _ = jit_chunks(shape, shape[1])
    assert chunk % 4 != 0, 'k_jit_scatter_reduce: the width of a chunk is no multiple of the stride'


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_mm_scatter_several_pieces_and_parts(be, family):
    """jit_scatter_batched at stride 4 (the mm scatter): two pieces per class, the last partly filled; 1 / 3 / 8 / 33 / 40 columns
    split the active rows of a class into 8 / 2 / 1 / 1 / 1 parts (parts = 16 and 5: test_scatter_active_row_loop_second_trip) and
    put gridDim.y / gridDim.z of the walk and the reduce above 32; a chunk width that is no multiple of 4 takes the tail test of
    k_jit_scatter_reduce.  f16 / bf16 at 3 columns, f64 at 8, one float operand, one negatively weighted case."""
    cross_mm_pieces(family)
    shape, prob, seed = MM_PIECES[family], 0.02, 68
    spk_all = draw_spikes(seed, (shape[0], 40), 0.5)
    ref_all = {key: reference(key, spk_all, shape, True, False, prob, seed, 4) for key in keys_of(family, negative=True)}
    for n in MM_PIECES_PARTS:
        spk, ref = np.ascontiguousarray(spk_all[:, :n]), np.ascontiguousarray(ref_all[family][:, :n])
        dtypes = [F32] + ([F16, BF16] if family == 's' and n == 3 else []) + ([F64] if n == 8 else [])
        for dtype in dtypes:
            event_case(family, 'scatter', dtype, spk, ref, shape, True, False, prob, seed, f'shape={shape}', repeat=(n == 3 and dtype == F32))
        if n == 3:
            event_case(family, 'scatter', F32, spk, ref, shape, True, False, prob, seed, f'shape={shape}', kind='float')
            if family != 's':
                event_case(family + '-', 'scatter', F32, spk, np.ascontiguousarray(ref_all[family + '-'][:, :n]), shape, True, False, prob,
                           seed, f'shape={shape}')


A_LOOP = [((40_000, 3000), 0, 2), ((40_000, 64), 1, 16), ((40_000, 64), 3, 5)]       # (shape, columns (0: a vector), parts)


def cross_a_loop(shape, n, parts, active):
    for scalar in (True, False):
        _, _, pieces, _, got_parts = scatter_geom(shape[1], shape[1], 4 if n else 32, scalar, max(n, 1))
        assert pieces == 1 and got_parts == parts, (scalar, pieces, got_parts)
    assert active > parts * SCATTER_BLOCK, 'more active rows than parts * 1024: a second trip of the `a` loop'


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_scatter_active_row_loop_second_trip(be, family):
    """k_jit_mv_scatter's loop over the active rows: `parts` workgroups of 1024 threads share a class, so more than parts * 1024
    active rows put it on a second trip — 36 000 active rows at parts = 2 (stride 32), 16 (stride 4, one column) and 5 (three
    columns)."""
    prob, seed = 0.001, 69
    for shape, n, parts in A_LOOP:
        spk = draw_spikes(seed, (shape[0], n) if n else shape[0], 0.9)
        cross_a_loop(shape, n, parts, int(spk.sum(axis=0).min()))
        ref = reference(family, spk, shape, True, False, prob, seed, 4 if n else 32)
        event_case(family, 'scatter', F32, spk, ref, shape, True, False, prob, seed, f'shape={shape}', repeat=True)


GEOMETRY = [((5000, 40), 500, 0.02, 0.1), ((20, 1000), 1, 0.3, 0.05)]      # (shape, chunks over shape[0], prob gather, prob scatter)


@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_chunk_geometry(be, family):
    """The chunk width is a quarter of shape[1] but the walk may run over shape[0]: (5000, 40) walked over its long side has 500
    chunks of 10 (gridDim.y = 500 in the gather, 500 * stride residue classes in the scatter); (20, 1000) walked over its short side
    has one chunk of width 20 < 32 lanes.  Gather and scatter, a vector and 3 columns, and the negatively weighted families."""
    for shape, chunks, p_gather, p_scatter in GEOMETRY:
        assert jit_chunks(shape, shape[0])[1] == chunks
        if chunks == 1:
            assert shape[0] < jit_chunks(shape, shape[0])[0] and shape[0] < 32, 'one chunk narrower than the lane stride'
        for n in (0, 3):
            for key in keys_of(family, negative=True):
                # the gather walks in_len: transpose=True makes that shape[0]; the scatter walks out_len: transpose=False
                for route, transpose, prob, seed in (('mm_gather' if n else 'mv_gather', True, p_gather, 70), ('scatter', False, p_scatter, 71)):
                    in_len, _ = in_out(shape, transpose)
                    spk = draw_spikes(seed + n, (in_len, n) if n else in_len, 0.5)
                    ref = reference(key, spk, shape, transpose, route != 'scatter', prob, seed, 4 if n else 32)
                    event_case(key, route, F32, spk, ref, shape, transpose, route != 'scatter', prob, seed, f'shape={shape}',
                               repeat=route == 'scatter')


def test_scatter_workspace_reuse(be):
    """Armed scatter workspaces: a one-column and a two-column mm scatter whose workspaces have the same byte size (the counters and
    lists of the two columns lie elsewhere in it), one after the other and again; then, on one armed mv workspace, a call at
    firing 0.0 followed by one at 0.9 (a stale counter would lengthen the second list).  Every call against the oracle."""
    prob, seed = 0.05, 72
    f_ws = J.fn('be_binary_jitmm_workspace_bytes')
    shapes = {1: (128, 900), 2: (64, 900)}
    assert f_ws(900, 128, 900, 1, 0) == f_ws(900, 64, 900, 2, 0)
    for n in (1, 2, 1, 2):
        shape = shapes[n]
        spk = draw_spikes(seed + n, (shape[0], n), 0.5)
        ref = reference('s', spk, shape, True, False, prob, seed, 4)
        event_case('s', 'scatter', F32, spk, ref, shape, True, False, prob, seed, f'shape={shape}')
    shape = (3000, 2600)
    for firing in (0.5, 0.0, 0.9, 0.0, 0.01):
        spk = draw_spikes(seed + int(firing * 1000), shape[0], firing)
        ref = reference('s', spk, shape, True, False, 0.01, seed, 32)
        if firing == 0.0:
            assert not spk.any() and not ref.any()
            assert_exact(product('s', F32, vector_operand(spk, 'bool'), shape, True, False, 0.01, seed, False), ref, F32, 'no spikes')
        else:
            event_case('s', 'scatter', F32, spk, ref, shape, True, False, 0.01, seed, f'shape={shape} firing={firing}')


# =========================================================================================================== sharded entry points
CLASSES = {'s': 'JITCScalarR', 'u': 'JITCUniformR', 'n': 'JITCNormalR'}
SHARD_GATHER_SHAPE = (2 * (MV_GATHER_TRIP + 133), 3000)


def host(x):
    return np.asarray(torch.as_tensor(x).cpu())


@pytest.mark.parametrize('family', ['s', 'u'])
def test_gather_shard_beyond_one_trip(be, family):
    """be_binary_jitmv_rows: rank 1 of 2 of a 33 034-row gather owns the rows from 16 517 on — row0 lies past the first trip of the
    unsharded row loop and the shard's own 16 517 rows take a second trip; the RNG is keyed by row0 + local row."""
    shape, prob, seed = SHARD_GATHER_SHAPE, 0.02, 73
    lo, hi = post_slice_bounds(shape[0], 2, 1)
    assert lo > MV_GATHER_TRIP and cross_mv_gather_rows(hi - lo) == MV_GATHER_TRIP
    M = getattr(be, CLASSES[family])((*weight_args(family, F32), prob, seed), shape=shape, corder=True)
    spk = draw_spikes(seed, shape[1], 0.3)
    ref = reference(family, spk, shape, False, True, prob, seed, 32)[lo:hi]
    bound = expectation(family, 'mv_gather', F32, ref, shape[1])
    sh = M.gather_shard(2, 1, 'right')
    assert (sh.lo, sh.hi) == (lo, hi)
    compare(torch.as_tensor(sh @ be.BinaryArray(torch.from_numpy(spk).cuda())), ref, bound, F32, f'rows [{lo}, {hi})')


@pytest.mark.parametrize('family', ['s', 'u'])
def test_scatter_shards_several_pieces(be, family):
    """be_binary_jitmv_sharded on the several-piece shapes: each of three ranks walks a third of the (chunk, lane) classes, every
    class in two or more pieces; its output equals the oracle on the columns it owns and is zero elsewhere."""
    shape, prob, seed = MV_PIECES[family], 0.005, 67
    cross_pieces(shape, 32, family == 's')
    M = getattr(be, CLASSES[family])((*weight_args(family, F32), prob, seed), shape=shape, corder=True)
    spk = draw_spikes(seed, shape[0], 0.5)
    ref = reference(family, spk, shape, True, False, prob, seed, 32)
    bound = expectation(family, 'scatter', F32, ref, shape[0])
    ev = be.BinaryArray(torch.from_numpy(spk).cuda())
    seen = np.zeros(shape[1], np.int32)
    for rank in range(3):
        sh = M.scatter_shard(3, rank)
        own = np.zeros(shape[1], bool)
        own[sh.owned_columns] = True
        seen += own
        assert np.count_nonzero(ref[own]) > own.sum() // 50
        compare(torch.as_tensor(ev @ sh), np.where(own, ref, 0.0), None if bound is None else np.where(own, bound, 0.0), F32, f'rank {rank}')
    assert (seen == 1).all()


# =========================================================================================================== materialisation
MATERIALISE = {'mv': ((MV_GATHER_TRIP + 133, 3000), 0.02, 32), 'mm': ((131_200, 64), 0.1, 4)}


def cross_materialise(mode):
    shape, _, stride = MATERIALISE[mode]
    tasks = shape[0] * jit_chunks(shape, shape[1])[1] * stride
    assert tasks > MATERIALISE_SPAN, 'k_jit_csr_count / k_jit_csr_fill: one thread per (row, chunk, lane), 8192 blocks of 256'


@pytest.mark.parametrize('mode', ['mv', 'mm'])
@pytest.mark.parametrize('family', ['s', 'u', 'n'])
def test_materialisation_beyond_one_grid(be, family, mode):
    """k_jit_csr_count / k_jit_csr_fill with more (row, chunk, lane) tasks than one trip of their grid, for the mv matrix (stride 32)
    and the mm matrix (stride 4): the counts equal the oracle's edge counts; indptr is their cumulative sum; every row's columns are
    in range and distinct; the stored weights are the device hashes at the stored (row, column) pairs, bit for bit; the edge set
    is pinned by the stored matrix's products with three random 0/1 vectors per side (exact for the scalar family, otherwise
    within an f32 sum of A addends in any order, (A + 1) 2^-24 S, plus the normal family's weight tolerance)."""
    cross_materialise(mode)
    shape, prob, stride = MATERIALISE[mode]
    seed = 74
    M = getattr(be, CLASSES[family])((*weight_args(family, F32), prob, seed), shape=shape, corder=True)
    counts_ref = oracle_c.jit_float('s', 1.0, 0.0, prob, np.ones(shape[1]), seed, shape=shape, transpose=False, corder=True, stride=stride)
    counts = M.owner_counts(mode)
    assert counts.dtype == torch.int32 and np.array_equal(host(counts), counts_ref)
    S = M.materialize(mode)
    assert isinstance(S, be.CSR) and S.shape == shape
    indptr, cols = S.indptr.long(), S.indices.long()
    nnz = int(counts_ref.sum())
    assert np.array_equal(host(indptr), np.concatenate([[0], np.cumsum(counts_ref)]).astype(np.int64)) and cols.numel() == nnz
    rows = torch.repeat_interleave(torch.arange(shape[0], device='cuda'), counts.long())
    assert int(cols.min()) >= 0 and int(cols.max()) < shape[1]
    assert torch.unique(rows * shape[1] + cols).numel() == nnz, 'a row holds a column twice'
    if family != 's':
        rep = EDGE_WEIGHTS_SPAN // nnz + 1                        # listed often enough for k_jit_edge_weights' own second trip
        assert rep * nnz > EDGE_WEIGHTS_SPAN
        w = J.jit_edge_weights(family, *PARAMS[family], seed, rows.to(torch.int32).repeat(rep), cols.to(torch.int32).repeat(rep))
        assert torch.equal(bits(S.data.repeat(rep)), bits(w)), 'stored weights differ from the device hashes at the stored pairs'
    for side in range(2):
        for k in range(3):
            transpose = side == 1
            in_len, _ = in_out(shape, transpose)
            spk = draw_spikes(seed + 10 * side + k, in_len, 0.3 if mode == 'mv' else (0.5 if not transpose else 0.001))
            ref = reference(family, spk, shape, transpose, not transpose, prob, seed, stride)
            assert np.count_nonzero(ref) > ref.size // 50
            ev = be.BinaryArray(torch.from_numpy(spk).cuda())
            got = torch.as_tensor(ev @ S if transpose else S @ ev)
            if family == 's':
                assert_exact(got, ref, F32, f'side {side} vector {k}')
            else:
                Ssum = np.abs(ref)
                A_ = np.ceil(Ssum / W_MIN[family])
                bound = (A_ + 1) * 2.0 ** -24 * Ssum + (A_ * NORMAL_WEIGHT_RTOL * W_MAX['n'] if family == 'n' else 0.0) + HALF_ULP[F32] * Ssum
                assert float(bound.max()) <= 0.25 * W_MIN[family]
                compare(got, ref, bound, F32, f'side {side} vector {k}')


# =========================================================================================================== without a device
def check_all_crossings():
    """Every crossing assertion above that needs neither the oracle nor a device (the CPU thresholds file runs it)."""
    for shape, transpose in GATHER_ROWS:
        cross_mv_gather_rows(in_out(shape, transpose)[1])
    assert REDUCE_SHAPE[0] > REDUCE_SPAN
    for shape, in_lds in BITS_GLOBAL_SHAPES:
        cross_bits_in_lds(shape, in_lds)
    for width in MM_LDS:
        cross_mm_windows(width)
    assert CONVERT_SHAPE[0] * CONVERT_COLS > CONVERT_SPAN
    for ncol in MM_GLOBAL:
        cross_mm_global(ncol)
    for family, shape in MV_PIECES.items():
        cross_pieces(shape, 32, family == 's')
        cross_mm_pieces(family)
    for shape, n, parts in A_LOOP:
        cross_a_loop(shape, n, parts, int(0.85 * shape[0]))
    lo, hi = post_slice_bounds(SHARD_GATHER_SHAPE[0], 2, 1)
    assert lo > MV_GATHER_TRIP and cross_mv_gather_rows(hi - lo)
    for mode in MATERIALISE:
        cross_materialise(mode)
