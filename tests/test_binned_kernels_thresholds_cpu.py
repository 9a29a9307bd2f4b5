"""What tests/test_binned_kernels_exact_gpu.py sizes its cases by (the CONSTS table of tests/binned_cases.py and the geometry restated
from it) is what csrc/be_csr_binned.hip says.  No GPU needed: the source is read as text, and be_binned_bins and
be_binary_csrmm_t_binned_workspace_bytes are host functions.  When this fails after a retune (the LDS budget, a block size, kMaxBins,
the capacity formula, a batch floor), move the table with the source and re-size the GPU cases the failure message lists."""
import re
from pathlib import Path

import numpy as np
import pytest

import binned_cases as B
from binned_cases import CONSTS, KINDS

SOURCE = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc' / 'be_csr_binned.hip'
TEXT = SOURCE.read_text()

BLOCKS = 'test_block_sizes, test_no_geometry, test_overflow and every case that asserts its block size'
GEO = 'test_geometry_branches, test_unmapped_directory, test_parts'
BATCH = 'test_batch, test_batch_union_encodings, test_unmapped_directory'


def _prod(*g):
    v = 1
    for x in g:
        v *= int(x)
    return v


def _at(i):
    return lambda *g: int(g[i])


# table key -> (regular expression, its groups -> the value, how often the source holds it, the GPU cases sized by it)
PATTERNS = {
    'lds.bytes': (r'(160) \* (1024) - (?:512|kAccStaticBytes)', _prod, 5, f'{BLOCKS}; {GEO}'),
    'stream.margin': (r'budget = 160 \* 1024 - (\d+) - \(int64_t\)kStreamFixedWords \* 4;', _prod, 1, BLOCKS),
    'stream.waves': (r'constexpr int kStreamWaves = (\d+);', _prod, 1, BLOCKS),
    'stream.threads': (r'#define BE_STREAM_THREADS (\d+)', _prod, 1, BLOCKS),
    'fixed.table_words': (r'constexpr int kStreamWl = kStreamWaves \* \((\d+) \* (\d+) \+ (\d+) \+ (\d+)\);',
                          lambda a, b, c, d: int(a) * int(b) + int(c) + int(d), 1, BLOCKS),
    'fixed.list_words': (r'constexpr int kStreamFixedWords = kStreamWl \+ kStreamWaves \* (\d+) \+ (\d+) \+ (\d+) \+ (\d+);', _at(0), 1, BLOCKS),
    'fixed.ticket_words': (r'constexpr int kStreamFixedWords = kStreamWl \+ kStreamWaves \* (\d+) \+ (\d+) \+ (\d+) \+ (\d+);', _at(1), 1, BLOCKS),
    'fixed.dummy_words': (r'constexpr int kStreamFixedWords = kStreamWl \+ kStreamWaves \* (\d+) \+ (\d+) \+ (\d+) \+ (\d+);', _at(2), 1, BLOCKS),
    'fixed.align_words': (r'constexpr int kStreamFixedWords = kStreamWl \+ kStreamWaves \* (\d+) \+ (\d+) \+ (\d+) \+ (\d+);', _at(3), 1, BLOCKS),
    'ring': (r'#define BE_RING (\d+) ', _prod, 1, BLOCKS),
    'per_bin.entry_bytes_counted': (r'per_bin = kRing \* \(int64_t\)cap \* \(kind_counted\(homo\) \? (\d+) : (\d+)\) \+ (\d+) \+ (\d+) \* kRing;',
                                    _at(0), 1, BLOCKS),
    'per_bin.entry_bytes_weighted': (r'per_bin = kRing \* \(int64_t\)cap \* \(kind_counted\(homo\) \? (\d+) : (\d+)\) \+ (\d+) \+ (\d+) \* kRing;',
                                     _at(1), 1, BLOCKS),
    'per_bin.words_bytes': (r'per_bin = kRing \* \(int64_t\)cap \* \(kind_counted\(homo\) \? (\d+) : (\d+)\) \+ (\d+) \+ (\d+) \* kRing;',
                            _at(2), 1, BLOCKS),
    'per_bin.ring_bytes': (r'per_bin = kRing \* \(int64_t\)cap \* \(kind_counted\(homo\) \? (\d+) : (\d+)\) \+ (\d+) \+ (\d+) \* kRing;',
                           _at(3), 1, BLOCKS),
    'cap.largest': (r'for \(int cap = forced > 0 \? forced : (\d+); cap >= (\d+); cap >>= 1\)', _at(0), 1, BLOCKS),
    'cap.smallest': (r'for \(int cap = forced > 0 \? forced : (\d+); cap >= (\d+); cap >>= 1\)', _at(1), 1, BLOCKS),
    'max_bins': (r'constexpr int kMaxBins = (\d+);', _prod, 1, f'test_no_geometry, test_block_sizes (counted, 8 entries); {BATCH}'),
    'stream.grid': (r'constexpr int kStreamGrid = (\d+);', _prod, 1, 'every case sized with room (need_capacity); test_overflow'),
    'acc.static_bytes': (r'constexpr int64_t kAccStaticBytes = 4 \* \(kStreamGrid \+ kStreamGrid \+ 1 \+ 16\) \+ (\d+);',
                         lambda g: 4 * (2 * CONSTS['stream.grid'] + 1 + 16) + int(g), 1, 'test_unmapped_directory (the k of its cases)'),
    'acc.local_column_max': (r'1ll << slice_shift\), (\d+)\) & ~3ll;', _prod, 2, GEO),
    'geo.small_k': (r'\} else if \(k <= (\d+) \* (\d+)\) \{', _prod, 1, 'test_geometry_branches (k = 65537)'),
    'geo.small_width': (r'g\.width = std::min<int64_t>\((\d+), max_w\);', _prod, 1, 'every case at slice_shift 4 (bins of 16 columns)'),
    'geo.pow2_shift': (r'\n    int sh = (\d+);', _prod, 1, 'test_geometry_branches (k = 65537, shift 8, weighted)'),
    'cap_blocks.num': (r'per_region = bin_capacity / kStreamGrid \* (\d+) / (\d+) \+ (\d+);', _at(0), 1, 'test_overflow; need_capacity'),
    'cap_blocks.den': (r'per_region = bin_capacity / kStreamGrid \* (\d+) / (\d+) \+ (\d+);', _at(1), 1, 'test_overflow; need_capacity'),
    'cap_blocks.add': (r'per_region = bin_capacity / kStreamGrid \* (\d+) / (\d+) \+ (\d+);', _at(2), 1, 'test_overflow; need_capacity'),
    'cap_blocks.extra': (r'return \(per_region \+ cap - 1\) / cap \+ (\d+);', _prod, 1, 'test_overflow; need_capacity'),
    'batch.pass': (r'int gb = \(int\)std::min<int64_t>\(n_batch, (\d+)\);', _prod, 1, BATCH),
    'batch.floor_counted': (r'stream_cap\(\(int\)\(nbb \* gb\), homo\) < \(kind_counted\(homo\) \? (\d+) : (\d+)\)', _at(0), 1, 'test_batch (batch-cut)'),
    'batch.floor_weighted': (r'stream_cap\(\(int\)\(nbb \* gb\), homo\) < \(kind_counted\(homo\) \? (\d+) : (\d+)\)', _at(1), 1, 'test_batch (batch-cut)'),
    'batch.capacity_add': (r'\(bg\.g\.n_bins > 0 \? bg\.g\.n_bins : 1\)\) \+ (\d+);', _prod, 1, BATCH),
    'short_row': (r'constexpr int64_t kShortRow = (\d+);', _prod, 1, 'test_fixed_length_rows (256, 257), test_short_rows_hint'),
    'task.rows_floor': (r'constexpr int kTaskRowsFloor = (\d+), kTaskGroupsCap = (\d+);', _at(0), 1, 'test_task_size'),
    'task.groups_cap': (r'constexpr int kTaskRowsFloor = (\d+), kTaskGroupsCap = (\d+);', _at(1), 1, 'test_task_size'),
    'stream.u': (r'#define BE_STREAM_U (\d+) ', _prod, 1, 'test_block_sizes (512 entries per round), test_short_rows_hint'),
    'bin.u': (r'#define BE_BIN_U (\d+) ', _prod, 1, 'test_parts, test_unmapped_directory'),
    'parts.total': (r'int parts = (\d+) / \(n_vbins > 0 \? n_vbins : 1\);', _prod, 1, 'test_parts'),
    'parts.max': (r'parts = parts < 1 \? 1 : \(parts > (\d+) \? (\d+) : parts\);', lambda a, b: int(a) if a == b else -1, 1, 'test_parts'),
    'audit.off': (r'constexpr int64_t kBinAuditOff = (\d+);', _prod, 1, 'every case (the workspace size)'),
    'audit.grid_c': (r'constexpr int kBinAuditGridC = (\d+);', _prod, 1, 'every case (the workspace size)'),
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, value, count, cases = PATTERNS[key]
    found = re.findall(pattern, TEXT)
    assert len(found) == count, f"{key}: be_csr_binned.hip holds /{pattern}/ {len(found)} times — the GPU cases sized by it need a look: {cases}"
    values = {value(*([g] if isinstance(g, str) else g)) for g in found}
    assert values == {CONSTS[key]}, f"{key}: be_csr_binned.hip says {sorted(values)}, tests/binned_cases.py assumes {CONSTS[key]}: re-size {cases}"


def test_what_follows_from_the_table():
    """The class boundaries, the k = 65537 branches, the batch passes, the parts and the map sizes the cases are named for."""
    B.check_derived()
    assert B.stream_budget() == CONSTS['lds.bytes'] - CONSTS['stream.margin'] - 4 * B.stream_fixed_words()
    # five classes for each kind, each twice the block size of the next, none past kMaxBins
    for kind in KINDS:
        bounds = B.class_bounds(kind)
        assert [b[0] for b in bounds.values()][1:] == [b[1] + 1 for b in bounds.values()][:-1]
        assert all(lo <= hi <= CONSTS['max_bins'] for lo, hi in bounds.values())
    # the map of pass C in the unmapped cases: 16 bytes next to 64-bit sums, none next to 32-bit ones
    assert [B.geometry_batch(B.unmapped_k(kind), 16, kind, 2)[3] for kind in KINDS] == [16, 0, 0]
    assert [B.unmapped_k(kind) for kind in KINDS] == [(CONSTS['lds.bytes'] - CONSTS['acc.static_bytes']) // b & ~3 for b in (8, 4, 4)]


def test_launch_shapes_around_the_constants():
    """What the GPU cases take for granted besides the numbers: five block-size arms in each of the three dispatches of pass B
    (per weight type, counted and weighted) and of pass C (counted, 64-bit, 32-bit), the launch shapes, the counters' layout."""
    arms = sorted(B.CAPS)
    assert sorted(int(x) for x in re.findall(r'BE_BIN_STREAM\(WT, true, (\d+)\)', TEXT)) == arms
    assert sorted(int(x) for x in re.findall(r'BE_BIN_STREAM\(WT, false, (\d+)\)', TEXT)) == arms
    assert sorted(int(x) for x in re.findall(r' BE_BIN_ACC\(true, (\d+)\)', TEXT)) == arms
    assert sorted(int(x) for x in re.findall(r' BE_BIN_ACC\(false, (\d+)\)', TEXT)) == arms
    assert sorted(int(x) for x in re.findall(r' BE_BIN_ACC32\((\d+)\);', TEXT)) == arms
    assert len(re.findall(r'BE_BIN_STREAM_W\((?:__half|__hip_bfloat16|float)\)', TEXT)) == 3
    assert len(re.findall(r'hipLaunchKernelGGL\(kern, dim3\(kStreamGrid\), dim3\(BE_STREAM_THREADS\), dyn, st,', TEXT)) == 1
    assert len(re.findall(r'hipLaunchKernelGGL\(kern, dim3\(acc_grid\), dim3\(1024\), lds, st,', TEXT)) == 2
    assert CONSTS['stream.threads'] == 64 * CONSTS['stream.waves']
    assert len(re.findall(r'constexpr int kRing = BE_RING,', TEXT)) == 1
    assert len(re.findall(r'k > 256 \* std::min<int64_t>\(max_w, 16384\)', TEXT)) == 1 and 1 << CONSTS['geo.pow2_shift'] == 16384
    assert len(re.findall(r'constexpr int64_t kBinAuditBytes = \(3 \* 256 \+ kBinAuditGridC\) \* 8;', TEXT)) == 1
    assert len(re.findall(r'const bool short_rows = indptr == nullptr \? \(row_len > 0 && row_len <= kShortRow\) : \(homo & 8\) != 0;', TEXT)) == 1
    assert len(re.findall(r'const uint32_t sign_mask = \(homo & 4\) \? 0x7fffffffu : 0xffffffffu;', TEXT)) == 1
    assert len(re.findall(r'const bool huge = __ballot\(len >= \(1ull << 26\)\) != 0;', TEXT)) == 1        # (not reached at test size)
    csr_py = (SOURCE.parent.parent / '_csr.py').read_text()
    assert len(re.findall(rf"SHORT_ROW_ENTRIES = {CONSTS['short_row']} ", csr_py)) == 1


# ------------------------------------------------------------------------------------------------- the library's host functions
SWEEP_K = sorted({1, 7, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 20148, 20149, 40300, 40301, 65535, 65536, 65537, 100_000, 1 << 20,
                  4_194_304, 4_194_305, 5_000_000, 10_000_000, 33_554_432, 100_000_000, (1 << 31) - 1}
                 | {16 * (n + d) for kind in KINDS for lo, hi in B.class_bounds(kind).values() for n in (lo, hi) for d in (0, 1)})


@pytest.fixture(scope='module')
def lib():
    from brainevent_amd import _lib
    return _lib


def test_bins_match_the_library(lib):
    bins = lib.fn('be_binned_bins')
    for shift in range(4, 17):
        for kind in KINDS:
            for k in SWEEP_K:
                assert bins(k, shift, kind) == B.bins(k, shift, kind), (k, shift, kind)
    assert bins(100, 3, 0) == bins(100, 17, 0) == bins(0, 8, 0) == bins(100, 8, 3) == 0


def test_workspace_bytes_match_the_library(lib):
    """For every (m, k, n_batch, shift, bin_capacity) the GPU module uses, and a sweep: pins the restated cap, gb and cap_blocks."""
    nbytes = lib.fn('be_binary_csrmm_t_binned_workspace_bytes')
    keys = {B.build(name).ws_key() for name in B.CASES}
    keys |= {(1000, k, nb, shift, bc) for k in (125, 1120, 20148, 40300, 65537, 3_000_000) for nb in (1, 2, 9, 33, 70) for shift in (4, 9, 16)
             for bc in (8, 1000, 1 << 20)}
    keys |= {(64, k, 1, shift, 8) for k, shift, _ in B.unserved_shapes()}
    for key in sorted(keys):
        assert nbytes(*key) == B.workspace_bytes(*key), key


# ------------------------------------------------------------------------------------------------------ the generator's claim
@pytest.mark.parametrize('name', list(B.CASES))
def test_case_is_exact(name):
    """64 sum |w| < 2^24 over every column, and the f64 reference equals the sums taken in integers of 1/64 — so it is THE value,
    whatever the order of the additions — and survives the cast to f32."""
    c = B.build(name)
    c.check_exact()
    if c.cap:
        assert c.geometry()[2] == c.cap
    ref = c.reference()
    units = np.round(c.entry_weights() * 64).astype(np.int64)
    assert np.array_equal(units / 64.0, c.entry_weights())
    rows = c.rows_of_entries
    for b in range(c.n_batch):
        sel = c.spikes[b][rows] & (c.indices < c.k)
        exact = np.zeros(c.k, np.int64)
        np.add.at(exact, c.indices[sel], units[sel])
        assert np.array_equal(exact / 64.0, ref[b]) and np.abs(exact).max(initial=0) < 2 ** 24
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    n, bad, past = c.counts()
    assert n > 0 and (bad > 0) == ('column-past-k' in name or 'slack' in name) and past <= bad
    assert c.spikes.flags.writeable is False and c.indices.flags.writeable is False
