"""The spike encoders and the plan-less CSR products at the head of csrc/be_csr.hip (k_compact_spikes, k_compact_bits,
k_pack_spikes_vec, k_pack_spikes, k_unpack_spikes, k_csrmv_t_direct, k_csrmv_t_direct_indexed, k_csrmv_nt_indexed,
k_convert_from_f32, and k_batch_masks / k_coarsen_bits of the gather front end) past their one-pass sizes: every size dispatch,
capped grid, alignment branch and template instantiation of these kernels is crossed by a named case.

Assertion policy: every comparison in this module is an equality; there is no tolerance anywhere.  The references are plain numpy
on the host: `np.flatnonzero` for the id lists (the list is unordered — workgroups reserve their ranges with an atomic — so it is
sorted before it is compared), `np.packbits(..., bitorder='little').view(np.uint32)` after padding to a multiple of 32 for the
packed words, `np.add.at` in f64 for the products (tests/test_spike_front_kernels_thresholds_cpu.py holds each of them to a
brute-force loop at small sizes).  The products are exact in two ways.  (a) Weights that are signed multiples of 0.5 with the sum
of |w| over every output element — all stored entries counted, fired or not — within EXACT_MAX of the dtype: every partial sum of
every order of the float atomics (scatter) or of the wave's reduction (gather) is then exactly representable, and the one rounding
at the f16 / bf16 store is exact too.  (b) f32 weights with random mantissas on a structure in which at most one entry reaches an
output element: the output must be the weight's own bits (compared as int32) — what (a) cannot see, a weight taken from a
neighbouring slot that happens to hold the same value, shows here.

Every case is sized from the CONSTS table (the thresholds module compares it with the source) and asserts on the host that it
crosses the bound it is there for before it launches anything.

Which loop or branch is reached where:
  launch_compact: <SP,16,256> | <SP,16,1024> at 65 536 | 65 537, <SP,16,1024> | <SP,64,1024> at 2 097 152 | 2 097 153;
    tiles of 4096 / 16 384 / 65 536 elements: one, exactly one, one element more, several and a partial last one;
    SP = SpikeBool and SpikeFloat; densities 0, 1 %, 50 %, all ones; count re-zeroed by a second call      test_compact_ladder
  k_compact_spikes 16-byte path (aligned, per byte != 0) | scalar path (one byte off; the last group
    of an aligned vector with n % 16 != 0; every float)                                                    test_compact_ladder
  compact_any BE_SPIKE_BITS: k_compact_bits<1> | <4> at 2 097 152 | 2 097 153; workgroups of 256 / 1024 words; the mask of the
    bits past n; the w < n_words guard of <4> (words of all ones behind the vector)                        test_compact_ladder
  blockIdx.y of both compaction kernels: rows 1, 2 of a bool batch unaligned, active_stride, per-row counts
                                                                                                           test_compact_batched
  launch_pack vector | ballot choice: bool aligned; bool one byte off; float; batch with n % 16 == 0 | != 0
                                                           test_pack_vector_path, test_pack_ballot_path, test_pack_batched
  k_pack_spikes_vec: n < 32 (scalar tail only), whole words, partial last word, second trip of the capped grid
                                                                                                           test_pack_vector_path
  k_pack_spikes<SpikeFloat / SpikeBool>: n_round, the lane-32 guard at n % 64 = 0, 1, 31, 32, 33, 63, second trip
                                                                                                           test_pack_ballot_path
  k_unpack_spikes second trip, nothing written past n, unpack(pack(x)) == (x != 0)                         test_unpack_past_one_trip
  k_csrmv_t_direct<W, HOMO, ACC> for f32 / f64 / f16 / bf16, shared and per-entry weights; row loop second trip at
    8192 waves (nb 1) and at 2048 waves in each of 8 batch rows; int32 / int64 indptr / fixed row_len      test_direct_scatter
  k_convert_from_f32<f16 / bf16> second trip (k * nb > 524 288)                                            test_direct_scatter_convert_past_one_trip
  be_resolve_active BE_SPIKE_IDS (a list made by be_compact_spikes) against the bool encoding              test_direct_scatter_from_an_id_list
  k_csrmv_t_direct: a weight from its own slot (bitwise)                                                   test_direct_scatter_wrong_neighbour
  k_csrmv_t_direct_indexed<W, ACC, int32_t / int64_t>, row loop second trip, exact and bitwise             test_indexed_scatter
  k_csrmv_nt_indexed<W, int32_t / int64_t>: row loop second trip at 16 384 rows (nb 1), 4096 rows (nb 8); bool / float / bits
    inputs; exact and bitwise; one shared weight forwards to the plain product                             test_indexed_gather,
                                                                                          test_indexed_gather_one_fired_entry_per_row
  gather_g_shift 4 | 5 at 19 660 800 | 19 660 801 columns: both branches of k_coarsen_bits                 test_gather_coarse_group_edge
  k_batch_masks<SpikeBool / SpikeFloat> second trip; nc = 4, 9 (a partial second group of eight), 32       test_gather_fused_batch_masks

Not here: n near 2^32 for the uint32 ids and counts (16 GiB of list; the ids are computed in int64 and truncated once, at the
store).  A second trip of k_coarsen_bits (its grid covers 262 144 coarse words, the LDS bitmap holds 38 400) and g_shift >= 6
(k above 39 321 600 columns: the same loop as g_shift 5 with two words per group).  The 16-byte path of k_compact_spikes on a
batch whose rows are aligned is the path of the aligned single vector (blockIdx.y only moves the pointers).  Subnormal float
spikes: whether they compare as zero on this target is not for this module to decide.  BE_SPIKE_IDS with n_batch > 1 is refused
by the library (test_event_encodings_gpu.py).  The planned and binned scatter routes and the gather kernels behind the front end
have their own exact modules (test_gather_kernels_exact_gpu.py, test_plan_contracts_gpu.py).
"""
import functools

import numpy as np
import pytest
import torch

from test_gather_kernels_exact_gpu import EXACT_MAX, TORCH_DT, W_UNITS

pytestmark = pytest.mark.gpu

# The loop bounds and dispatch thresholds of be_csr.hip as the cases below use them.
CONSTS = {
    'block': 256,                           # threads per workgroup of every kernel here but the 1024-thread compactions
    'compact.small.tile': 256 * 16,         # launch_compact: elements per workgroup of k_compact_spikes<SP, 16, 256>
    'compact.small.max_n': 64 << 10,        # ... used up to this n
    'compact.mid.tile': 1024 * 16,          # k_compact_spikes<SP, 16, 1024>
    'compact.mid.max_n': 2 << 20,
    'compact.large.tile': 1024 * 64,        # k_compact_spikes<SP, 64, 1024>
    'bits.max_n_1': 2 << 20,                # compact_any: k_compact_bits<1> up to this n, <4> beyond
    'bits.words_1': 256,                    # words per workgroup of k_compact_bits<1>
    'bits.words_4': 1024,                   # ... of k_compact_bits<4>
    'pack.vec.grid_cap': 4096,              # k_pack_spikes_vec: grid_for((n + 31) / 32, 256, 4096), one word per thread and trip
    'pack.ballot.grid_cap': 2048,           # k_pack_spikes<SP>: grid_for(n, 256, 2048)
    'unpack.grid_cap': 4096,                # k_unpack_spikes: grid_for(n, 256, 4096)
    'convert.grid_cap': 2048,               # k_convert_from_f32: grid_for(k * nb, 256, 2048)
    'masks.grid_cap': 2048,                 # k_batch_masks: grid_for(k, 256, 2048)
    'masks.group': 8,                       # batch rows per group of loads in k_batch_masks
    'scatter.grid': 2048,                   # csrmv_t_direct: workgroups (4 waves each) for nb < 8
    'scatter.grid_batch': 512,              # ... for nb >= 8
    'indexed.grid_cap': 4096,               # csrmv_nt_indexed: grid_for(m, 4, 4096) for nb < 8
    'indexed.grid_cap_batch': 1024,         # ... for nb >= 8
    'batch_edge': 8,                        # nb >= 8 takes the smaller grids
    'lds_bitmap_bytes': 150 * 1024,         # kLdsBitmapBytes: the (coarse) bitmap a gather workgroup holds in LDS
    'coarsen.word_shift': 5,                # k_coarsen_bits: groups of whole words from this g_shift on
    'fused.min_batch': 4,                   # kFusedMinBatch (be_csr_shared.h)
    'fused.min_work': 768,                  # kFusedMinWork
}
K = CONSTS
BLOCK = K['block']
WAVES = BLOCK // 64                                                    # waves per workgroup of the direct kernels
PACK_VEC_SPAN = K['pack.vec.grid_cap'] * BLOCK * 32                    # 33 554 432 spikes per trip of k_pack_spikes_vec
PACK_BALLOT_SPAN = K['pack.ballot.grid_cap'] * BLOCK                   # 524 288 elements per trip of k_pack_spikes<SP>
UNPACK_SPAN = K['unpack.grid_cap'] * BLOCK                             # 1 048 576
CONVERT_SPAN = K['convert.grid_cap'] * BLOCK                           # 524 288
MASKS_SPAN = K['masks.grid_cap'] * BLOCK                               # 524 288
LDS_COLUMNS = K['lds_bitmap_bytes'] * 8                                # 1 228 800 bits of bitmap in LDS
G4_MAX_K = LDS_COLUMNS << (K['coarsen.word_shift'] - 1)                # 19 660 800: the last width with 16-column groups

BE_SPIKE_BOOL, BE_SPIKE_FLOAT, BE_SPIKE_BITS, BE_SPIKE_IDS = 0, 1, 2, 3
GARBAGE = 0x5a5a5a5a
ROW_LENS = (0, 1, 63, 64, 65, 129)
DTYPES = ('f32', 'f64', 'f16', 'bf16')
DENSITIES = (0.0, 0.01, 0.5, 1.0)
BOOL_ON = np.array([1, 2, 0x80, 0xff], dtype=np.uint8)                 # a spike is any nonzero byte
FLOAT_ON = np.array([1.0, 0.5, 2.0 ** -126, np.inf, 3e38], dtype=np.float32)       # active is v > 0 (no subnormals)
FLOAT_OFF = np.array([-1.0, 0.0, -0.0, np.nan, -np.inf], dtype=np.float32)

_T, _M, _L = K['compact.small.tile'], K['compact.mid.tile'], K['compact.large.tile']
COMPACT_SIZES = (1, 15, 16, 17, _T - 1, _T, _T + 1, K['compact.small.max_n'] - 1, K['compact.small.max_n'],
                 K['compact.small.max_n'] + 1, 5 * _M - 1, 5 * _M, 5 * _M + 1, K['compact.mid.max_n'], K['compact.mid.max_n'] + 1,
                 K['compact.mid.max_n'] + _L + 17)
_B1, _B4 = 32 * K['bits.words_1'], 32 * K['bits.words_4']
BITS_SIZES = (1, 31, 32, 33, _B1 - 1, _B1, _B1 + 1, 65_535, 65_536, 65_537, 5 * _B4 - 1, 5 * _B4, 5 * _B4 + 1, K['bits.max_n_1'],
              K['bits.max_n_1'] + 1, K['bits.max_n_1'] + 65_536 + 17)
PACK_VEC_SIZES = (1, 31, 32, 33, 64, PACK_VEC_SPAN + 32 * BLOCK + 5)
PACK_BALLOT_BASE = PACK_BALLOT_SPAN + 192
PACK_BALLOT_REMS = (0, 1, 31, 32, 33, 63)
UNPACK_N = UNPACK_SPAN + 33
SCATTER_ACTIVE = {1: K['scatter.grid'] * WAVES + 5, 8: K['scatter.grid_batch'] * WAVES + 3}       # active rows per batch row
SCATTER_M = {1: 10_240, 8: 2_600}
SCATTER_K = {1: 8_209, 8: 2_053}
GATHER_M = {1: K['indexed.grid_cap'] * WAVES + 5, 8: K['indexed.grid_cap_batch'] * WAVES + 5}
GATHER_K = 4_099
CONVERT_K = 65_545                                                     # with nb = 8: 524 360 outputs
FUSED_K = MASKS_SPAN + 5
FUSED_NB = (4, 9, 32)


# ============================================================================================ the host's choices, restated
def compact_kernel(n):
    """launch_compact restated: (elements per thread, threads) of the k_compact_spikes instance that takes n elements."""
    if n <= K['compact.small.max_n']:
        return 16, K['compact.small.tile'] // 16
    if n <= K['compact.mid.max_n']:
        return 16, K['compact.mid.tile'] // 16
    return 64, K['compact.large.tile'] // 64


def compact_tiles(n):
    per_thread, threads = compact_kernel(n)
    return -(-n // (per_thread * threads))


def bits_kernel(n):
    """compact_any restated: words per thread of the k_compact_bits instance."""
    return 1 if n <= K['bits.max_n_1'] else K['bits.words_4'] // BLOCK


def bits_tiles(n):
    return -(-((n + 31) // 32) // (BLOCK * bits_kernel(n)))


def pack_is_vector(address, itemsize, n, nb):
    """launch_pack restated: one-byte spikes at a 16-byte boundary, and every row of a batch at one too."""
    return itemsize == 1 and address % 16 == 0 and (nb == 1 or n % 16 == 0)


def scatter_waves(nb):
    return (K['scatter.grid_batch'] if nb >= K['batch_edge'] else K['scatter.grid']) * WAVES


def gather_rows_per_pass(nb):
    return (K['indexed.grid_cap_batch'] if nb >= K['batch_edge'] else K['indexed.grid_cap']) * WAVES


def g_shift_of(k):
    """gather_g_shift restated: the smallest group size 2^g whose coarse bitmap fits the LDS."""
    g = 0
    while (((k + (1 << g) - 1) >> g) + 31) // 32 * 4 > K['lds_bitmap_bytes']:
        g += 1
    return g


def takes_fused_route(avg_row, nb, dt, float_or_bool=True):
    """csrmv_nt's condition for the kernel fused over the batch, restated (avg_row = nnz // m, the wrapper's hint)."""
    return nb >= K['fused.min_batch'] and avg_row * nb >= K['fused.min_work'] and avg_row >= 16 and dt != 'f64' and float_or_bool


def check_all_crossings():
    """The arithmetic behind the table in the module docstring (also run without a device by the thresholds module)."""
    small, mid, large = (16, 256), (16, 1024), (64, 1024)
    assert [compact_kernel(n) for n in COMPACT_SIZES] == [small] * 9 + [mid] * 5 + [large] * 2
    assert [compact_tiles(n) for n in COMPACT_SIZES] == [1, 1, 1, 1, 1, 1, 2, 16, 16, 5, 5, 5, 6, 128, 33, 34]
    assert sum(n % 16 != 0 and n > 16 for n in COMPACT_SIZES) >= 6            # an aligned vector's last group is scalar
    assert COMPACT_SIZES[-1] % _L == 17                                       # the last tile of <SP,64,1024> holds 17 elements
    assert [bits_kernel(n) for n in BITS_SIZES] == [1] * 14 + [4, 4]
    assert [bits_tiles(n) for n in BITS_SIZES] == [1, 1, 1, 1, 1, 1, 2, 8, 8, 9, 20, 20, 21, 256, 65, 67]
    assert ((BITS_SIZES[-1] + 31) // 32) % K['bits.words_4'] == 1 and BITS_SIZES[-1] % 32 == 17
    assert ((BITS_SIZES[-2] + 31) // 32) % 4 == 1                             # <4>: three of a thread's words lie behind n_words
    # pack: vector path sizes; the big one takes a second trip of 256 full words and one partial word
    words = (PACK_VEC_SIZES[-1] + 31) // 32
    assert words == K['pack.vec.grid_cap'] * BLOCK + BLOCK + 1 and PACK_VEC_SIZES[-1] % 32 == 5
    assert all(pack_is_vector(0, 1, n, 1) for n in PACK_VEC_SIZES)
    assert not pack_is_vector(1, 1, 64, 1) and not pack_is_vector(0, 4, 64, 1)
    assert pack_is_vector(0, 1, 4112, 3) and not pack_is_vector(0, 1, 4099, 3) and 4112 % 32 == 16
    for r in PACK_BALLOT_REMS:
        assert (PACK_BALLOT_BASE + r) % 64 == r and PACK_BALLOT_BASE + r > PACK_BALLOT_SPAN
    assert UNPACK_N > UNPACK_SPAN and UNPACK_N % 32 == 1
    # direct products
    assert scatter_waves(1) == 8192 and scatter_waves(7) == 8192 and scatter_waves(8) == 2048
    assert gather_rows_per_pass(1) == 16_384 and gather_rows_per_pass(7) == 16_384 and gather_rows_per_pass(8) == 4096
    for nb in (1, 8):
        assert SCATTER_M[nb] >= SCATTER_ACTIVE[nb] > scatter_waves(nb) and GATHER_M[nb] > gather_rows_per_pass(nb)
    assert CONVERT_K * 8 > CONVERT_SPAN >= CONVERT_K * 7
    # gather front end
    assert G4_MAX_K == 19_660_800 and LDS_COLUMNS == 1_228_800
    assert [g_shift_of(k) for k in (LDS_COLUMNS, LDS_COLUMNS + 1, G4_MAX_K, G4_MAX_K + 1)] == [0, 1, 4, 5]
    assert g_shift_of(G4_MAX_K) < K['coarsen.word_shift'] <= g_shift_of(G4_MAX_K + 1)
    assert FUSED_K > MASKS_SPAN
    assert [nb % K['masks.group'] for nb in FUSED_NB] == [4, 1, 0] and [-(-nb // K['masks.group']) for nb in FUSED_NB] == [1, 2, 4]
    assert takes_fused_route(192, 4, 'f32') and not takes_fused_route(191, 4, 'f32') and not takes_fused_route(300, 3, 'f32')
    assert not takes_fused_route(300, 4, 'f64') and not takes_fused_route(15, 64, 'f32')


# ================================================================================================================ references
def ref_ids(fired):
    return np.flatnonzero(fired).astype(np.uint32)


def ref_words(fired):
    """Bit i % 32 of word i // 32, the bits past the end 0."""
    fired = np.asarray(fired, dtype=bool)
    padded = np.zeros(-(-fired.size // 32) * 32, dtype=bool)
    padded[:fired.size] = fired
    return np.packbits(padded, bitorder='little').view(np.uint32)


def ref_scatter(w_of_slot, idx, row_of, k, fired_rows):
    """out[b, idx[j]] += w[j] for the slots j of the rows that fired in batch row b; f64."""
    out = np.zeros((fired_rows.shape[0], k))
    for b, fired in enumerate(fired_rows):
        sel = fired[row_of]
        np.add.at(out[b], idx[sel], w_of_slot[sel])
    return out


def ref_gather(w_of_slot, idx, row_of, m, fired_cols):
    """out[b, r] = sum of w[j] over the slots j of row r whose column fired in batch row b; f64."""
    out = np.zeros((fired_cols.shape[0], m))
    for b, fired in enumerate(fired_cols):
        sel = fired[idx]
        np.add.at(out[b], row_of[sel], w_of_slot[sel])
    return out


def assert_exact_in(dt, w_of_slot, into, size, ref):
    """Condition (a) of the module docstring: |w| summed per output element over ALL slots stays within the dtype's exact range
    (so does every partial sum of any order), the weights are multiples of 0.5, and the result is representable."""
    total = np.zeros(size)
    np.add.at(total, into, np.abs(w_of_slot))
    assert total.max() <= EXACT_MAX[dt], (dt, total.max())
    assert np.all(w_of_slot * 2 == np.round(w_of_slot * 2))
    np.testing.assert_array_equal(torch.from_numpy(ref).to(TORCH_DT[dt]).double().numpy(), ref)


# =================================================================================================================== helpers
def lib():
    from brainevent_amd import _array as A
    from brainevent_amd._lib import call, fn
    return A, call, fn


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()       # (the shared host arrays are read-only)


def words_i32(words):
    return dev(np.ascontiguousarray(words).view(np.int32))


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def fired_of(rng, n, density):
    if density in (0.0, 1.0):
        return np.full(n, bool(density))
    return rng.random(n) < density


def bool_bytes(rng, fired):
    return np.where(fired, BOOL_ON[rng.integers(0, len(BOOL_ON), fired.shape, dtype=np.uint8)], 0).astype(np.uint8)


def float_values(rng, fired):
    on = FLOAT_ON[rng.integers(0, len(FLOAT_ON), fired.shape)]
    off = FLOAT_OFF[rng.integers(0, len(FLOAT_OFF), fired.shape)]
    v = np.where(fired, on, off).astype(np.float32)
    with np.errstate(invalid='ignore'):
        np.testing.assert_array_equal(v > 0, fired)
    return v


def at_offset(host_bytes, offset, fill=0xff):
    """A device copy of `host_bytes` that starts `offset` bytes past a 16-byte boundary, inside a buffer of `fill` bytes (an
    over-read would see spikes); returns (view, buffer)."""
    n = host_bytes.size
    buf = torch.full((n + 48,), fill, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n]
    view.copy_(torch.from_numpy(host_bytes))
    assert view.data_ptr() % 16 == offset % 16
    return view, buf


def bits_operand(fired, extra_words=8):
    """BE_SPIKE_BITS words of one vector with every bit past n set in the last word and `extra_words` words of all ones behind."""
    n = fired.size
    words = ref_words(fired).copy()
    if n % 32:
        words[-1] |= np.uint32(0xffffffff) << np.uint32(n % 32)
    return np.concatenate([words, np.full(extra_words, 0xffffffff, dtype=np.uint32)])


def run_compact(spikes, sd, n, want):
    """be_compact_spikes twice into the same buffers: the sorted list, the exact count, the entries behind the list untouched."""
    A, call, _ = lib()
    active = torch.full((n + 64,), -1, dtype=torch.int32, device='cuda')
    count = torch.full((2,), GARBAGE, dtype=torch.int32, device='cuda')
    for trip in range(2):
        call('be_compact_spikes', A.ptr(spikes), sd, n, A.ptr(active), A.ptr(count), A.stream_ptr())
        c, canary = (int(x) for x in count.cpu())
        assert c == want.size and canary == GARBAGE, f'trip {trip}: count {c}, reference {want.size}'
        got = host_u32(active)
        np.testing.assert_array_equal(np.sort(got[:c]), want, err_msg=f'trip {trip}')
        assert (got[c:] == 0xffffffff).all(), f'trip {trip}: written behind the list'


# ================================================================================================================= compaction
@pytest.mark.parametrize('i', range(len(COMPACT_SIZES)))
@pytest.mark.parametrize('enc', ['bool', 'float', 'bits'])
def test_compact_ladder(be, enc, i):
    n = (BITS_SIZES if enc == 'bits' else COMPACT_SIZES)[i]
    if i == 0:
        check_all_crossings()
    if enc == 'bits':
        assert bits_kernel(n) == (1 if i < 14 else 4)
    else:
        assert compact_kernel(n) == ((16, 256), (16, 1024), (64, 1024))[(i >= 9) + (i >= 14)]
    for density in DENSITIES:
        rng = np.random.default_rng([i, int(density * 100)])
        fired = fired_of(rng, n, density)
        want = ref_ids(fired)
        if density == 1.0:
            np.testing.assert_array_equal(want, np.arange(n, dtype=np.uint32))          # a permutation of arange(n)
        if enc == 'bool':
            v = bool_bytes(rng, fired)
            for offset in (0, 1):                      # 0: the 16-byte path (and a scalar last group); 1: the scalar path
                view, _buf = at_offset(v, offset)
                run_compact(view, BE_SPIKE_BOOL, n, want)
        elif enc == 'float':
            run_compact(dev(float_values(rng, fired)), BE_SPIKE_FLOAT, n, want)
        else:
            words = bits_operand(fired)
            assert words.size == (n + 31) // 32 + 8 and (n % 32 == 0 or words[(n - 1) // 32] >> np.uint32(n % 32) != 0)
            run_compact(words_i32(words), BE_SPIKE_BITS, n, want)


@pytest.mark.parametrize('enc', ['bool', 'float', 'bits'])
def test_compact_batched(be, enc):
    """blockIdx.y: three rows of 4099 spikes (rows 1 and 2 of the bool batch start 3 and 6 bytes past a 16-byte boundary), lists
    61 entries further apart than they need to be, one count per row, the padding between the lists untouched."""
    A, call, _ = lib()
    nb, n = 3, 4099
    stride = n + 61
    assert n % 16 == 3 and compact_tiles(n) == 2 and bits_tiles(n) == 1
    rng = np.random.default_rng(31)
    fired = np.stack([fired_of(rng, n, d) for d in (0.5, 0.01, 1.0)])
    if enc == 'bool':
        spikes, sd = dev(bool_bytes(rng, fired)), BE_SPIKE_BOOL
        assert spikes.data_ptr() % 16 == 0
    elif enc == 'float':
        spikes, sd = dev(float_values(rng, fired)), BE_SPIKE_FLOAT
    else:
        spikes, sd = words_i32(np.stack([bits_operand(f, 0) for f in fired])), BE_SPIKE_BITS
        assert spikes.shape == (nb, (n + 31) // 32)
    active = torch.full((nb * stride + 64,), -1, dtype=torch.int32, device='cuda')
    counts = torch.full((nb + 1,), GARBAGE, dtype=torch.int32, device='cuda')
    for trip in range(2):
        call('be_compact_spikes_batched', A.ptr(spikes), sd, n, nb, A.ptr(active), stride, A.ptr(counts), A.stream_ptr())
        c = counts.cpu().numpy()
        got = host_u32(active)
        assert c[nb] == GARBAGE
        for b in range(nb):
            want = ref_ids(fired[b])
            assert c[b] == want.size, f'row {b}'
            row = got[b * stride:(b + 1) * stride]
            np.testing.assert_array_equal(np.sort(row[:c[b]]), want, err_msg=f'row {b}')
            assert (row[c[b]:] == 0xffffffff).all(), f'row {b}: written behind the list'
        assert (got[nb * stride:] == 0xffffffff).all()


# ================================================================================================================ pack / unpack
def run_pack(spikes, sd, n, fired, nb=1):
    """be_pack_spikes (nb = 1) / be_pack_spikes_batched into a buffer of garbage words: row b is words [b * n_words, (b + 1) *
    n_words) — the ABI packs the rows densely, so the word behind a row is the next row's first — the bits past n are 0 (the
    reference's padding), and the canary words behind the last row are untouched."""
    A, call, _ = lib()
    n_words = (n + 31) // 32
    bits = torch.full((nb * n_words + 8,), GARBAGE, dtype=torch.int32, device='cuda')
    if nb == 1:
        call('be_pack_spikes', A.ptr(spikes), sd, n, A.ptr(bits), A.stream_ptr())
    else:
        call('be_pack_spikes_batched', A.ptr(spikes), sd, n, nb, A.ptr(bits), A.stream_ptr())
    got = host_u32(bits)
    for b, f in enumerate(np.atleast_2d(fired)):
        np.testing.assert_array_equal(got[b * n_words:(b + 1) * n_words], ref_words(f), err_msg=f'row {b}')
    assert (got[nb * n_words:] == GARBAGE).all(), 'written behind the last word'
    return bits


@pytest.mark.parametrize('n', PACK_VEC_SIZES)
def test_pack_vector_path(be, n):
    rng = np.random.default_rng(n % 1000)
    fired = fired_of(rng, n, 0.5)
    fired[-1] = True
    view, _buf = at_offset(bool_bytes(rng, fired), 0)
    assert pack_is_vector(view.data_ptr(), 1, n, 1)
    if n > 64:
        assert (n + 31) // 32 > K['pack.vec.grid_cap'] * BLOCK and n % 32 != 0         # second trip, partial last word
    run_pack(view, BE_SPIKE_BOOL, n, fired)


@pytest.mark.parametrize('rem', PACK_BALLOT_REMS)
@pytest.mark.parametrize('enc', ['float', 'bool+1'])
def test_pack_ballot_path(be, enc, rem):
    """n % 64 = rem just past one trip of the capped grid: lane 32 of the last wave stores the high word only when that word
    exists (rem > 32), and never behind the buffer."""
    n = PACK_BALLOT_BASE + rem
    assert n % 64 == rem and n > PACK_BALLOT_SPAN
    rng = np.random.default_rng(rem)
    fired = fired_of(rng, n, 0.5)
    fired[[-1, PACK_BALLOT_SPAN, PACK_BALLOT_SPAN - 1]] = True
    if enc == 'float':
        spikes, sd = dev(float_values(rng, fired)), BE_SPIKE_FLOAT
        assert not pack_is_vector(spikes.data_ptr(), 4, n, 1)
    else:
        (spikes, _buf), sd = at_offset(bool_bytes(rng, fired), 1), BE_SPIKE_BOOL
        assert not pack_is_vector(spikes.data_ptr(), 1, n, 1)
    run_pack(spikes, sd, n, fired)


@pytest.mark.parametrize('n', [4112, 4099])
@pytest.mark.parametrize('enc', ['bool', 'float'])
def test_pack_batched(be, enc, n):
    """Three rows: with n % 16 == 0 every bool row is aligned (vector path, n % 32 == 16: a scalar last word); n = 4099 is the
    ballot path, rows 1 and 2 unaligned."""
    nb = 3
    rng = np.random.default_rng(n)
    fired = np.stack([fired_of(rng, n, d) for d in (0.5, 0.01, 1.0)])
    if enc == 'bool':
        spikes, sd = dev(bool_bytes(rng, fired)), BE_SPIKE_BOOL
        assert pack_is_vector(spikes.data_ptr(), 1, n, nb) == (n == 4112)
    else:
        spikes, sd = dev(float_values(rng, fired)), BE_SPIKE_FLOAT
    run_pack(spikes, sd, n, fired, nb)


def test_unpack_past_one_trip(be):
    """k_unpack_spikes at 1 048 576 + 33 bits: bytes 0 / 1 only, nothing behind n, and unpack(pack(x)) is x != 0."""
    A, call, _ = lib()
    n = UNPACK_N
    assert n > UNPACK_SPAN
    rng = np.random.default_rng(8)
    fired = fired_of(rng, n, 0.5)
    fired[[UNPACK_SPAN - 1, UNPACK_SPAN, n - 1]] = True, True, True
    x = bool_bytes(rng, fired)
    view, _buf = at_offset(x, 0)
    bits = run_pack(view, BE_SPIKE_BOOL, n, fired)
    # (the words behind n in `bits` are garbage, the bits past n in the last word 0: neither may reach the output)
    out = torch.full((n + 64,), 0x77, dtype=torch.uint8, device='cuda')
    call('be_unpack_spikes', A.ptr(bits), n, A.ptr(out), A.stream_ptr())
    got = out.cpu().numpy()
    assert set(np.unique(got[:n]).tolist()) <= {0, 1}
    np.testing.assert_array_equal(got[:n], (x != 0).astype(np.uint8))
    assert (got[n:] == 0x77).all()
    # the same words with every bit past n set: still nothing of them in the output
    words = bits_operand(fired)
    out.fill_(0x77)
    call('be_unpack_spikes', A.ptr(words_i32(words)), n, A.ptr(out), A.stream_ptr())
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:n], fired.astype(np.uint8))
    assert (got[n:] == 0x77).all()


# ============================================================================================================ direct products
@functools.lru_cache(maxsize=None)
def row_lengths(m, seed):
    lens = np.random.default_rng(seed).permutation(np.resize(np.asarray(ROW_LENS, dtype=np.int64), m))
    lens.flags.writeable = False
    return lens


@functools.lru_cache(maxsize=None)
def ragged(m, k, seed, one_per_column=False):
    """Rows of ROW_LENS entries, shuffled.  Columns: a random permutation of the slots folded onto k columns, so every column
    holds at most ceil(nnz / k) entries (the exactness bound needs a ceiling, not a Poisson tail); `one_per_column`: at most one.
    Returns host arrays (lens, int64 indptr, int32 indices, row of each slot, a random permutation of the slots), read-only."""
    rng = np.random.default_rng([seed, k])
    lens = row_lengths(m, seed)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(ptr[-1])
    if one_per_column:
        assert nnz <= k
        idx = rng.permutation(k)[:nnz].astype(np.int32)
        assert np.bincount(idx, minlength=k).max() == 1
    else:
        idx = (rng.permutation(nnz) % k).astype(np.int32)
    row_of = np.repeat(np.arange(m), lens)
    perm = rng.permutation(nnz)
    for a in (ptr, idx, row_of, perm):
        a.flags.writeable = False
    return lens, ptr, idx, row_of, perm


@functools.lru_cache(maxsize=None)
def fixed_rows(m, k, row_len, seed):
    rng = np.random.default_rng(seed)
    idx = (rng.permutation(m * row_len) % k).astype(np.int32)
    row_of = np.repeat(np.arange(m), row_len)
    for a in (idx, row_of):
        a.flags.writeable = False
    return idx, row_of


@functools.lru_cache(maxsize=None)
def active_rows(m, seed, nb, n_active):
    """[nb, m] bool, a different vector per batch row: n_active rows each, only two of them empty — the list is unordered, so
    whichever rows the second trip of the row loop gets, most of them hold entries."""
    lens = row_lengths(m, seed)
    rng = np.random.default_rng([m, nb, n_active])
    full, empty = np.flatnonzero(lens > 0), np.flatnonzero(lens == 0)
    out = np.zeros((nb, m), dtype=bool)
    for b in range(nb):
        n_empty = min(2, empty.size)
        out[b, rng.choice(full, n_active - n_empty, replace=False)] = True
        out[b, rng.choice(empty, n_empty, replace=False)] = True
    assert (out.sum(1) == n_active).all() and (nb == 1 or len({r.tobytes() for r in out}) == nb)
    out.flags.writeable = False
    return out


def exact_weights(rng, n, dt, homo):
    """Signed multiples of 0.5 (host, f64): one shared weight or one per slot."""
    if homo:
        return np.asarray([-0.5])
    return rng.integers(1, W_UNITS[dt] + 1, n) * 0.5 * rng.choice([-1.0, 1.0], n)


def mantissa_weights(rng, n):
    """f32 bit patterns with a random sign and mantissa and an exponent in [2^-4, 2^4): neighbours differ in nearly every bit."""
    bits = (rng.integers(0, 2, n, dtype=np.int64) << 31) | (rng.integers(123, 131, n, dtype=np.int64) << 23) | rng.integers(0, 1 << 23, n, dtype=np.int64)
    return bits.astype(np.uint32).view(np.int32)


def direct(name, w, idx, ptr, row_len, perm, spikes, sd, out_len, m, k, nb):
    """The C entry point `name` (argument order as in _csr._csrmm_direct) into an output preset to NaN; returns it."""
    A, call, fn = lib()
    transpose = 'csrmm_t' in name
    if transpose:
        ws = A.workspace(fn('be_binary_csrmm_t_workspace_bytes')(m, k, nb, A.wcode(w)))
    else:
        ws = A.workspace(fn('be_binary_csrmm_nt_workspace_bytes')(m, k, nb))
    out = torch.full((nb, out_len), float('nan'), dtype=w.dtype, device='cuda')
    is64 = int(ptr is not None and ptr.dtype == torch.int64)
    head = (A.ptr(w), int(w.numel() == 1), A.wcode(w), A.ptr(idx), A.ptr(ptr), is64, row_len)
    tail = (A.ptr(spikes), sd, A.ptr(out), m, k, nb, A.ptr(ws), ws.numel(), A.stream_ptr())
    if name.endswith('_indexed'):
        call(name, *head, A.ptr(perm), int(perm is not None and perm.dtype == torch.int64), *tail)
    else:
        assert perm is None
        call(name, *head, *tail)
    return out


def as_f64(t):
    return t.double().cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize('nb', [1, 8])
@pytest.mark.parametrize('homo', [False, True])
@pytest.mark.parametrize('dt', DTYPES)
def test_direct_scatter(be, dt, homo, nb):
    """k_csrmv_t_direct: more active rows than the grid has waves, in every batch row; int32 / int64 indptr and a fixed row_len."""
    m, k, n_active = SCATTER_M[nb], SCATTER_K[nb], SCATTER_ACTIVE[nb]
    assert n_active > scatter_waves(nb)
    lens, ptr, idx, row_of, _ = ragged(m, k, 40 + nb)
    assert set(lens.tolist()) == set(ROW_LENS)
    fired = active_rows(m, 40 + nb, nb, n_active)
    assert (fired.sum(1) > scatter_waves(nb)).all() and (fired[:, lens > 0].sum(1) >= n_active - 2).all()        # per batch row
    rng = np.random.default_rng([50, nb, DTYPES.index(dt), homo])
    spikes = dev(bool_bytes(rng, fired))
    d_idx = dev(idx)
    for rows in ('int32', 'int64', 'fixed'):
        if rows == 'fixed':
            row_len = 65
            f_idx, f_row_of = fixed_rows(m, k, row_len, 60 + nb)
            w = exact_weights(rng, f_idx.size, dt, homo)
            wj = np.broadcast_to(w, f_idx.shape) if homo else w
            ref = ref_scatter(wj, f_idx, f_row_of, k, fired)
            assert_exact_in(dt, wj, f_idx, k, ref)
            got = direct('be_binary_csrmm_t', dev(w).to(TORCH_DT[dt]), dev(f_idx), None, row_len, None, spikes, BE_SPIKE_BOOL, k, m, k, nb)
        else:
            w = exact_weights(rng, idx.size, dt, homo)
            wj = np.broadcast_to(w, idx.shape) if homo else w
            ref = ref_scatter(wj, idx, row_of, k, fired)
            assert_exact_in(dt, wj, idx, k, ref)
            d_ptr = dev(ptr.astype(np.int32 if rows == 'int32' else np.int64))
            got = direct('be_binary_csrmm_t', dev(w).to(TORCH_DT[dt]), d_idx, d_ptr, -1, None, spikes, BE_SPIKE_BOOL, k, m, k, nb)
        assert got.dtype == TORCH_DT[dt] and np.count_nonzero(ref) > 0
        np.testing.assert_array_equal(as_f64(got), ref, err_msg=rows)


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_direct_scatter_convert_past_one_trip(be, dt):
    """f16 / bf16 outputs are accumulated in f32 and converted by k_convert_from_f32 over the flat [nb, k] result: 524 360
    elements, the last 72 of batch row 7 converted in the second trip."""
    nb, m, k = 8, SCATTER_M[8], CONVERT_K
    assert k * nb > CONVERT_SPAN >= k * (nb - 1)
    lens, ptr, idx, row_of, _ = ragged(m, k, 70)
    fired = active_rows(m, 70, nb, SCATTER_ACTIVE[nb]).copy()
    fired[nb - 1] = True                                     # (every row of the last batch row: its last columns are reached)
    rng = np.random.default_rng(71)
    w = exact_weights(rng, idx.size, dt, False)
    ref = ref_scatter(w, idx, row_of, k, fired)
    assert_exact_in(dt, w, idx, k, ref)
    assert np.count_nonzero(ref.reshape(-1)[CONVERT_SPAN:]) > 0
    got = direct('be_binary_csrmm_t', dev(w).to(TORCH_DT[dt]), dev(idx), dev(ptr), -1, None, dev(bool_bytes(rng, fired)), BE_SPIKE_BOOL,
                 k, m, k, nb)
    np.testing.assert_array_equal(as_f64(got), ref)


@pytest.mark.parametrize('homo', [False, True])
def test_direct_scatter_from_an_id_list(be, homo):
    """BE_SPIKE_IDS: the list that be_compact_spikes made, handed over as it lies on the device (count included), gives the bits
    of the bool encoding and the reference."""
    A, call, _ = lib()
    nb, m, k = 1, SCATTER_M[1], SCATTER_K[1]
    lens, ptr, idx, row_of, _ = ragged(m, k, 41)
    fired = active_rows(m, 41, nb, SCATTER_ACTIVE[nb])
    assert fired.sum() > scatter_waves(nb)
    rng = np.random.default_rng(80 + homo)
    w = exact_weights(rng, idx.size, 'f32', homo)
    wj = np.broadcast_to(w, idx.shape) if homo else w
    ref = ref_scatter(wj, idx, row_of, k, fired)
    assert_exact_in('f32', wj, idx, k, ref)
    spikes = dev(bool_bytes(rng, fired))
    ids = torch.full((m + 64,), -1, dtype=torch.int32, device='cuda')
    count = torch.full((1,), GARBAGE, dtype=torch.int32, device='cuda')
    call('be_compact_spikes', A.ptr(spikes), BE_SPIKE_BOOL, m, A.ptr(ids), A.ptr(count), A.stream_ptr())
    assert int(count.item()) == SCATTER_ACTIVE[nb]
    operand = A.ActiveIds(ids, count, m)
    d_w, d_idx, d_ptr = dev(w).float(), dev(idx), dev(ptr)
    got = direct('be_binary_csrmm_t', d_w, d_idx, d_ptr, -1, None, operand, BE_SPIKE_IDS, k, m, k, nb)
    plain = direct('be_binary_csrmm_t', d_w, d_idx, d_ptr, -1, None, spikes, BE_SPIKE_BOOL, k, m, k, nb)
    np.testing.assert_array_equal(as_f64(got), ref)
    assert same_bits(got, plain)
    np.testing.assert_array_equal(np.sort(host_u32(ids)[:SCATTER_ACTIVE[nb]]), ref_ids(fired[0]))       # the call left the list alone


@functools.lru_cache(maxsize=None)
def one_per_column_case(nb):
    m = SCATTER_M[nb]
    nnz = int(row_lengths(m, 90 + nb).sum())
    k = nnz + 37
    return (m, k) + ragged(m, k, 90 + nb, one_per_column=True)


def expect_own_bits(w_bits_of_slot, idx, row_of, k, fired_rows):
    """One stored entry per column at most: the output is that entry's weight, bit for bit, where its row fired, else +0.0."""
    out = np.zeros((fired_rows.shape[0], k), dtype=np.int32)
    for b, fired in enumerate(fired_rows):
        sel = fired[row_of]
        out[b, idx[sel]] = w_bits_of_slot[sel]
    return out


@pytest.mark.parametrize('nb', [1, 8])
def test_direct_scatter_wrong_neighbour(be, nb):
    m, k, lens, ptr, idx, row_of, _ = one_per_column_case(nb)
    fired = active_rows(m, 90 + nb, nb, SCATTER_ACTIVE[nb])
    assert (fired.sum(1) > scatter_waves(nb)).all()
    rng = np.random.default_rng(91 + nb)
    w = mantissa_weights(rng, idx.size)
    assert np.all(w[1:] != w[:-1])
    got = direct('be_binary_csrmm_t', dev(w).view(torch.float32), dev(idx), dev(ptr), -1, None, dev(bool_bytes(rng, fired)), BE_SPIKE_BOOL,
                 k, m, k, nb)
    np.testing.assert_array_equal(got.view(torch.int32).cpu().numpy(), expect_own_bits(w, idx, row_of, k, fired))


@pytest.mark.parametrize('perm_dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('dt', DTYPES)
def test_indexed_scatter(be, dt, perm_dtype):
    """k_csrmv_t_direct_indexed: slot j adds weights[perm[j]].  Past 8192 active rows on the ragged structure with exact weights;
    bitwise (f32 only) on the one-entry-per-column structure; one shared weight ignores perm."""
    nb, m, k = 1, SCATTER_M[1], SCATTER_K[1]
    lens, ptr, idx, row_of, perm = ragged(m, k, 41)
    fired = active_rows(m, 41, nb, SCATTER_ACTIVE[nb])
    assert fired.sum() > scatter_waves(nb) and not np.array_equal(perm, np.arange(perm.size))
    rng = np.random.default_rng([100, DTYPES.index(dt)])
    w = exact_weights(rng, idx.size, dt, False)
    ref = ref_scatter(w[perm], idx, row_of, k, fired)
    assert_exact_in(dt, w[perm], idx, k, ref)
    assert not np.array_equal(ref, ref_scatter(w, idx, row_of, k, fired))
    spikes = dev(bool_bytes(rng, fired))
    d_perm = dev(perm).to(perm_dtype)
    d_idx, d_ptr = dev(idx), dev(ptr.astype(np.int32))
    got = direct('be_binary_csrmm_t_indexed', dev(w).to(TORCH_DT[dt]), d_idx, d_ptr, -1, d_perm, spikes, BE_SPIKE_BOOL, k, m, k, nb)
    np.testing.assert_array_equal(as_f64(got), ref)
    # one shared weight: the entry point forwards to the plain product
    w1 = dev(np.asarray([1.5])).to(TORCH_DT[dt])
    got = direct('be_binary_csrmm_t_indexed', w1, d_idx, d_ptr, -1, d_perm, spikes, BE_SPIKE_BOOL, k, m, k, nb)
    plain = direct('be_binary_csrmm_t', w1, d_idx, d_ptr, -1, None, spikes, BE_SPIKE_BOOL, k, m, k, nb)
    ref1 = ref_scatter(np.full(idx.size, 1.5), idx, row_of, k, fired)
    assert_exact_in(dt, np.full(idx.size, 1.5), idx, k, ref1)
    assert same_bits(got, plain)
    np.testing.assert_array_equal(as_f64(got), ref1)
    if dt != 'f32':
        return
    m, k, lens, ptr, idx, row_of, perm = one_per_column_case(nb)
    fired = active_rows(m, 90 + nb, nb, SCATTER_ACTIVE[nb])
    w = mantissa_weights(rng, idx.size)
    got = direct('be_binary_csrmm_t_indexed', dev(w).view(torch.float32), dev(idx), dev(ptr), -1, dev(perm).to(perm_dtype),
                 dev(bool_bytes(rng, fired)), BE_SPIKE_BOOL, k, m, k, nb)
    np.testing.assert_array_equal(got.view(torch.int32).cpu().numpy(), expect_own_bits(w[perm], idx, row_of, k, fired))


def gather_operand(rng, fired, enc):
    """[nb, k] fired columns as the operand of the gather entry points: bool bytes, floats or packed words (bits past k set)."""
    if enc == 'bool':
        return dev(bool_bytes(rng, fired)), BE_SPIKE_BOOL
    if enc == 'float':
        return dev(float_values(rng, fired)), BE_SPIKE_FLOAT
    return words_i32(np.stack([bits_operand(f, 0) for f in fired])), BE_SPIKE_BITS


@pytest.mark.parametrize('nb', [1, 8])
@pytest.mark.parametrize('enc', ['bool', 'float', 'bits'])
def test_indexed_gather(be, enc, nb):
    """k_csrmv_nt_indexed: more rows than the grid has waves; every dtype, int32 and int64 perm, int32 / int64 indptr and a fixed
    row_len; one shared weight with a perm is the plain product."""
    m, k = GATHER_M[nb], GATHER_K
    assert m > gather_rows_per_pass(nb)
    lens, ptr, idx, row_of, perm = ragged(m, k, 110 + nb)
    assert set(lens.tolist()) == set(ROW_LENS) and (lens[gather_rows_per_pass(nb):] > 0).any()
    rng = np.random.default_rng([111, nb, ('bool', 'float', 'bits').index(enc)])
    fired = rng.random((nb, k)) < 0.25
    fired[:, k - 3:] = True
    spikes, sd = gather_operand(rng, fired, enc)
    d_idx, d_ptr = dev(idx), dev(ptr.astype(np.int32))
    configs = [(dt, perm_dtype, ('int32', 'int64')[(i + j) % 2]) for i, dt in enumerate(DTYPES) for j, perm_dtype in enumerate((torch.int32, torch.int64))]
    for dt, perm_dtype, rows in configs + [('f32', torch.int64, 'fixed'), ('bf16', torch.int32, 'fixed')]:
        if rows == 'fixed':
            row_len = 65
            c_idx, c_row_of = fixed_rows(m, k, row_len, 120 + nb)
            c_perm, c_ptr, c_d_idx = np.random.default_rng(121).permutation(c_idx.size), None, dev(c_idx)
        else:
            row_len, c_idx, c_row_of, c_perm, c_d_idx = -1, idx, row_of, perm, d_idx
            c_ptr = d_ptr if rows == 'int32' else dev(ptr)
        w = exact_weights(rng, c_idx.size, dt, False)
        ref = ref_gather(w[c_perm], c_idx, c_row_of, m, fired)
        assert_exact_in(dt, w[c_perm], c_row_of, m, ref)
        assert np.count_nonzero(ref[:, gather_rows_per_pass(nb):]) > 0 and not np.array_equal(ref, ref_gather(w, c_idx, c_row_of, m, fired))
        got = direct('be_binary_csrmm_nt_indexed', dev(w).to(TORCH_DT[dt]), c_d_idx, c_ptr, row_len, dev(c_perm).to(perm_dtype), spikes, sd,
                     m, m, k, nb)
        assert got.dtype == TORCH_DT[dt]
        np.testing.assert_array_equal(as_f64(got), ref, err_msg=f'{dt} {rows}')
    w1 = dev(np.asarray([-0.5], dtype=np.float32))
    got = direct('be_binary_csrmm_nt_indexed', w1, d_idx, d_ptr, -1, dev(perm), spikes, sd, m, m, k, nb)
    plain = direct('be_binary_csrmm_nt', w1, d_idx, d_ptr, -1, None, spikes, sd, m, m, k, nb)
    assert same_bits(got, plain)
    np.testing.assert_array_equal(as_f64(got), ref_gather(np.full(idx.size, -0.5), idx, row_of, m, fired))


@pytest.mark.parametrize('perm_dtype', [torch.int32, torch.int64])
def test_indexed_gather_one_fired_entry_per_row(be, perm_dtype):
    """Bitwise: every row with entries has exactly one whose column fired, f32 weights with random mantissas reached through a
    random permutation — out[r] is that weight's bits (the other lanes add +0.0), 0 for an empty row."""
    nb, m, k = 1, GATHER_M[1], GATHER_K
    lens, ptr, _, row_of, perm = ragged(m, k, 111)
    rng = np.random.default_rng(130)
    fired = np.zeros((nb, k), dtype=bool)
    fired[0, rng.choice(k, k // 4, replace=False)] = True
    on, off = np.flatnonzero(fired[0]), np.flatnonzero(~fired[0])
    idx = off[rng.integers(0, off.size, row_of.size)].astype(np.int32)
    rows = np.flatnonzero(lens > 0)
    chosen = ptr[rows] + rng.integers(0, lens[rows])                    # one slot of every row with entries
    idx[chosen] = on[rng.integers(0, on.size, rows.size)]
    assert (np.bincount(row_of[fired[0][idx]], minlength=m) == (lens > 0)).all()
    w = mantissa_weights(rng, idx.size)
    want = np.zeros((nb, m), dtype=np.int32)
    want[0, rows] = w[perm][chosen]
    got = direct('be_binary_csrmm_nt_indexed', dev(w).view(torch.float32), dev(idx), dev(ptr), -1, dev(perm).to(perm_dtype),
                 dev(bool_bytes(rng, fired)), BE_SPIKE_BOOL, m, m, k, nb)
    np.testing.assert_array_equal(got.view(torch.int32).cpu().numpy(), want)


# ========================================================================================================= gather front end
@pytest.mark.parametrize('k', [G4_MAX_K, G4_MAX_K + 1])
@pytest.mark.parametrize('homo', [False, True])
def test_gather_coarse_group_edge(be, oracle, k, homo):
    """The public gather at the last width whose coarse groups are 16 columns (k_coarsen_bits reads part of a word) and the first
    with groups of a whole word: 200 ragged rows, the last 64 columns populated and fired, 2 % of the others — a group of 32
    columns fires in about half of the cases, so the coarse filter both passes and drops entries."""
    from test_gather_kernels_exact_gpu import exact_ref, exact_weights as positive_weights, gpu_mv, spikes as spike_vector, structure, tier_lens
    assert g_shift_of(k) == (4 if k == G4_MAX_K else 5)
    lens = tier_lens(8)
    idx, ptr = structure(lens, k, 140, last_columns=64)
    assert (idx >= k - 64).sum() >= 64 and len(lens) == 200
    w = positive_weights(140, idx.size, 'f32', homo)
    v = spike_vector(140, k, 0.02, last_columns=64)
    ref = exact_ref(oracle, w, idx, ptr, v, (len(lens), k), 'f32')
    assert np.count_nonzero(ref) > 100
    np.testing.assert_array_equal(gpu_mv(be, w, idx, ptr, v, (len(lens), k), 'f32'), ref)


@pytest.mark.parametrize('nb', FUSED_NB)
@pytest.mark.parametrize('enc', ['bool', 'float'])
def test_gather_fused_batch_masks(be, oracle, enc, nb):
    """The public batched gather on the route fused over the batch: k_batch_masks builds one word per input column from nb spike
    rows, eight at a time; 524 293 columns are a second trip of its capped grid, and the last 64 columns (all in that trip or
    next to it) are populated and fire differently in every batch row."""
    from test_gather_kernels_exact_gpu import exact_ref, exact_weights as positive_weights, structure
    k, m = FUSED_K, 100
    rng = np.random.default_rng(150 + nb)
    lens = rng.integers(200, 400, m)
    avg = int(lens.sum()) // m
    assert takes_fused_route(avg, nb, 'f32') and k > MASKS_SPAN
    idx, ptr = structure(lens, k, 150, last_columns=64)
    assert (idx >= MASKS_SPAN).sum() >= 5
    w = positive_weights(150, idx.size, 'f32', False)
    B = rng.random((k, nb)) < 0.1
    B[k - 64:] = rng.random((64, nb)) < 0.5
    assert len({B[k - 64:, c].tobytes() for c in range(nb)}) == nb
    operand = torch.from_numpy(B).cuda() if enc == 'bool' else torch.from_numpy(float_values(rng, B)).cuda()
    got = be.binary_csrmm(torch.from_numpy(w.astype(np.float32)).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(ptr).cuda(), operand,
                          shape=(m, k), transpose=False)
    got = got.double().cpu().numpy()
    assert got.shape == (m, nb)
    for c in range(nb):
        np.testing.assert_array_equal(got[:, c], exact_ref(oracle, w, idx, ptr, B[:, c], (m, k), 'f32'), err_msg=f'column {c}')
