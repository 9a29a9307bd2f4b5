"""Synaptic delays without a device: the numpy restatement of tests/delay_cases.py against a brute-force dense evaluation, the
eager validation of ``SpikeRing`` / ``DelayedCSR`` (refused before any device call), the public names, and the tile constants
of csrc/be_delay.hip that the GPU cases of tests/test_delay_gpu.py are sized by.  When the thresholds test fails after a retune,
move ``delay_cases.TILES`` with the source: the GPU cases follow it by themselves (they are written in terms of the table)."""
import re
from pathlib import Path

import numpy as np
import pytest

from brainevent_amd import _delay
import delay_cases as DC

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_pre,n_post,depth,max_row,parallel', [(9, 14, 3, 6, False), (40, 25, 7, 20, True), (1, 5, 1, 4, False)])
def test_restatement_matches_the_dense_evaluation(n_pre, n_post, depth, max_row, parallel):
    data, indices, indptr, delays = DC.exact_case(3, n_pre, n_post, depth, max_row, parallel=parallel)
    if parallel:         # parallel synapses are really there: some (row, col) pair is stored more than once
        rows = np.repeat(np.arange(n_pre), np.diff(indptr))
        assert len(set(zip(rows.tolist(), indices.tolist()))) < indices.size
    rng = np.random.default_rng(5)
    ring = DC.ring_np(n_pre, depth)
    for _ in range(2 * depth + 1):
        ring.push(rng.random(n_pre) < 0.4)
        got = DC.delayed_currents_np(data, indices, indptr, delays, ring, n_post)
        ref = DC.dense_delayed_np(data, indices, indptr, delays, ring, n_post, depth)
        assert np.array_equal(got, ref)          # multiples of 1/64: exact in f64 in any order


def test_split_restatement_is_the_stable_sort():
    lens, indptr = DC.row_lengths_case(1)
    m, depth = len(lens), 7
    delays = DC.delay_pattern('reversed', 2, indptr, depth)
    indptr_s, perm, row_mask = DC.split_by_delay_np(indptr, delays, m, depth)
    assert indptr_s.shape == (depth * m + 1,) and indptr_s[-1] == indptr[-1]
    rows = np.repeat(np.arange(m), np.diff(indptr))
    for d in range(depth):
        for i in range(m):
            seg = perm[indptr_s[d * m + i]:indptr_s[d * m + i + 1]]
            assert np.array_equal(seg, np.nonzero((rows == i) & (delays == d))[0])        # in the original order
            assert bool(DC.unpack_words_np(row_mask[d], m)[i]) == (seg.size > 0)
    assert np.array_equal(np.sort(perm), np.arange(indptr[-1]))


def test_ring_restatement():
    ring = DC.ring_np(5, 3)
    assert ring.ids().size == 0 and not ring.age(2).any()
    a, b = np.array([1, 0, 0, 1, 0], bool), np.array([0., -1., 2., 0., 0.5])
    ring.push(a)
    ring.push(b)                                    # floats: active when > 0
    assert np.array_equal(ring.age(0), [False, False, True, False, True]) and np.array_equal(ring.age(1), a)
    assert np.array_equal(ring.ids(), [2, 4, 5, 8])
    mask = DC.pack_rows_np(np.array([[1, 1, 0, 1, 1], [0, 1, 1, 1, 1], [1, 1, 1, 1, 1]], bool))
    assert np.array_equal(ring.ids(row_mask=mask), [4, 8])
    assert np.array_equal(DC.unpack_words_np(DC.pack_rows_np(np.arange(70) % 3 == 0)[0], 70)[:70], np.arange(70) % 3 == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the package: names and eager validation
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_names(be):
    assert be.SpikeRing.__module__ == be.DelayedCSR.__module__ == 'brainevent_amd._delay'
    assert callable(be.CSR.with_delays) and callable(be.FixedNumPerPre.with_delays)
    for name in ('push', 'events', 'ids', 'reset'):
        assert callable(getattr(be.SpikeRing, name))
    for name in ('prepare', 'with_data', 'set_data_'):
        assert callable(getattr(be.DelayedCSR, name))


def _parts(nnz_delays=None, delays_dtype=np.int64):
    data = np.ones(5, np.float32)
    indices = np.array([0, 2, 1, 1, 3], np.int32)
    indptr = np.array([0, 2, 2, 5], np.int32)
    delays = np.zeros(5 if nnz_delays is None else nnz_delays, dtype=delays_dtype)
    return data, indices, indptr, delays


def test_eager_validation_needs_no_device(be):
    """Every refusal below comes before the first device call: this test runs where there is no GPU."""
    with pytest.raises(ValueError, match='4 delays for 5 stored entries'):
        be.DelayedCSR(_parts(nnz_delays=4), shape=(3, 4), depth=2)
    for depth in (0, 257):
        with pytest.raises(ValueError, match=r'depth must lie in \[1, 256\]'):
            be.DelayedCSR(_parts(), shape=(3, 4), depth=depth)
    with pytest.raises(TypeError, match='integer'):
        be.DelayedCSR(_parts(delays_dtype=np.float32), shape=(3, 4), depth=2)
    import torch
    with pytest.raises(TypeError, match='integer'):
        be.DelayedCSR(_parts()[:3] + (torch.zeros(5),), shape=(3, 4), depth=2)
    with pytest.raises(ValueError, match='below 2\\^31'):
        be.SpikeRing(1 << 27, 16)
    with pytest.raises(ValueError, match='below 2\\^31'):
        be.DelayedCSR(_parts(), shape=(1 << 23, 4), depth=256)
    with pytest.raises(ValueError, match='indptr must have'):
        be.DelayedCSR(_parts(), shape=(4, 4), depth=2)
    with pytest.raises(ValueError, match='one element or one per stored entry'):
        be.DelayedCSR((np.ones(3, np.float32),) + _parts()[1:], shape=(3, 4), depth=2)
    with pytest.raises(ValueError, match=r'\[n_pre, row_len\]'):
        be.DelayedCSR((np.ones(5, np.float32), np.zeros(5, np.int32), None, np.zeros(5, int)), shape=(3, 4), depth=2)
    with pytest.raises(ValueError):
        be.SpikeRing(0, 4)
    with pytest.raises(ValueError):
        be.SpikeRing(10, 0)


def test_mismatched_ring_is_refused(be):
    check_ring_matches = _delay.check_ring_matches
    check_ring_matches(70, 7, (70, 300), 7)
    check_ring_matches(70, 9, (70, 300), 7)                  # a deeper ring is fine
    with pytest.raises(ValueError, match='71 neurons.*70 rows'):
        check_ring_matches(71, 7, (70, 300), 7)
    with pytest.raises(ValueError, match='remembers 6 steps.*depth 7'):
        check_ring_matches(70, 6, (70, 300), 7)


# ---------------------------------------------------------------------------------------------------------------------------
# the tile constants of be_delay.hip
# ---------------------------------------------------------------------------------------------------------------------------
PATTERNS = {
    'kMaxDepth': r'constexpr\s+int\s+kMaxDepth\s*=\s*(\d+)',
    'kSplitThreads': r'constexpr\s+int\s+kSplitThreads\s*=\s*(\d+)',
    'kSplitGridCap': r'constexpr\s+int\s+kSplitGridCap\s*=\s*(\d+)',
    'kMaskGridCap': r'constexpr\s+int\s+kMaskGridCap\s*=\s*(\d+)',
    'kRingThreads': r'constexpr\s+int\s+kRingThreads\s*=\s*(\d+)',
    'kRingPer': r'constexpr\s+int\s+kRingThreads\s*=\s*\d+\s*,\s*kRingPer\s*=\s*(\d+)',
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(DC.TILES)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_tile_constant_matches_the_source(key):
    text = (CSRC / 'be_delay.hip').read_text()
    found = re.findall(PATTERNS[key], text)
    assert found, f"{key}: be_delay.hip no longer holds /{PATTERNS[key]}/ — the GPU cases sized by it need a look"
    assert {int(v) for v in found} == {DC.TILES[key]}, f"{key}: be_delay.hip says {found}, tests/delay_cases.py assumes {DC.TILES[key]}"


def test_tiles_are_derived_as_the_cases_assume(be):
    text = (CSRC / 'be_delay.hip').read_text()
    assert re.search(r'kSplitTile\s*=\s*kSplitThreads\s*;', text)                      # 4 waves x 64 entries per step
    assert re.search(r'kRingTileBits\s*=\s*kRingThreads\s*\*\s*kRingPer\s*;', text)
    assert re.search(r'kRingTileBits\s*==\s*kRingThreads\s*\*\s*32', text)             # push tile == compaction tile
    assert re.search(r'dim3\(kSplitThreads\)', text) and re.search(r'dim3\(kRingThreads\)', text)
    assert _delay.MAX_DELAY_DEPTH == DC.TILES['kMaxDepth']
    assert DC.SPLIT_TILE == 256 and DC.RING_TILE_BITS == 8192 and DC.SPLIT_ROWS_PER_PASS == 16384
