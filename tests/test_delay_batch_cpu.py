"""Batched spike rings without a device: the numpy restatement of tests/delay_batch_cases.py against a brute-force
per-bit loop over the device layout, every refusal of the batched ring (raised before any device call), and the grid constants
of csrc/be_delay.hip that the GPU cases of tests/test_delay_batch_gpu.py are sized by."""
import re
from pathlib import Path

import numpy as np
import pytest

from brainevent_amd import _delay
import delay_cases as DC
import delay_batch_cases as BC

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True], ids=['all', 'masked'])
@pytest.mark.parametrize('depth', [1, 3, 40])
@pytest.mark.parametrize('n', [1, 31, 32, 33])
def test_restatement_matches_the_per_bit_loop(n, depth, masked):
    batch = 3
    rng = np.random.default_rng(100 * depth + n)
    ring = BC.batch_ring_np(n, depth, batch)
    mask = BC.random_mask(rng, depth, n) if masked else None
    for t in range(2 * depth + 2):                       # from a silent ring, through the first wrap of head, to a full one
        if t % (depth + 1) == 0:                         # checked at a few heads (every step at depth 1)
            for ages in {1, max(1, depth - 1), depth}:
                want = BC.unrolled_words_brute(ring.bits(), ring.head, n, depth, batch, ages, mask)
                got = ring.stacked_words(ages, mask)
                assert got.dtype == np.uint32 and got.shape == (batch, (ages * n + 31) // 32)
                assert np.array_equal(got, want), (t, ages)
        ring.push(rng.random((batch, n)) < 0.4)
    assert ring.head == (2 * depth + 2) % depth


def test_restatement_of_the_layout():
    ring = BC.batch_ring_np(5, 3, 2)
    assert not ring.bits().any() and ring.head == 0 and not ring.stacked_words().any()
    a = np.array([[1, 0, 0, 1, 0], [0, 0, 0, 0, 1]], bool)
    b = np.array([[0., -1., 2., 0., 0.5], [1., 0., 0., 0., 0.]])         # floats: active when > 0
    ring.push(a)
    ring.push(b)
    assert ring.head == 2
    assert np.array_equal(ring.bits()[:, :, 0], [[0b01001, 0b10000], [0b10100, 0b00001], [0, 0]])
    # ages side by side, 5 bits each: row 0 = 10100 | 01001 << 5, row 1 = 00001 | 10000 << 5
    assert np.array_equal(ring.stacked_words()[:, 0], [0b10100 | (0b01001 << 5), 0b00001 | (0b10000 << 5)])
    words = DC.pack_rows_np(np.ones((2, 32), bool))                     # packed input with bits past n set: dropped
    ring.push_packed(words)
    assert np.array_equal(ring.age(0), np.ones((2, 5), bool)) and ring.head == 0
    ring.push(a)                                                        # the fourth push overwrites the first
    assert np.array_equal(ring.bits()[0, :, 0], [0b01001, 0b10000])


# ---------------------------------------------------------------------------------------------------------------------------
# the package: every refusal comes before the first device call
# ---------------------------------------------------------------------------------------------------------------------------
class _NoDevice:
    """A ``SpikeRing`` built without its device arrays: what the validation reads, and nothing a device call could use."""

    def __new__(cls, be, n, depth, batch):
        ring = object.__new__(be.SpikeRing)
        ring.n, ring.depth, ring.batch, ring._words = n, depth, batch, (n + 31) // 32
        ring._numpy = True
        return ring


def test_constructor_refusals(be):
    for bad in (0, -1, BC.MAX_BATCH + 1):
        with pytest.raises(ValueError, match=r'batch must lie in \[1, 65535\]'):
            be.SpikeRing(10, 4, batch=bad)
    with pytest.raises(ValueError, match='below 2\\^31'):
        be.SpikeRing(1 << 27, 16, batch=2)
    assert _delay.MAX_RING_BATCH == BC.MAX_BATCH


def test_push_refusals_need_no_device(be):
    ring = _NoDevice(be, 10, 4, 3)
    assert ring.shape == (3, 10) and ring.ndim == 2 and repr(ring) == 'SpikeRing(n=10, depth=4, batch=3)'
    for bad in (np.zeros(10, bool), np.zeros((2, 10), bool), np.zeros((3, 11), bool), np.zeros((3, 10, 1), bool)):
        with pytest.raises(ValueError, match=r'takes spikes of shape \(3, 10\)'):
            ring.push(bad)
        with pytest.raises(ValueError, match=r'takes spikes of shape \(3, 10\)'):
            ring.push(be.BinaryArray(bad))
    for bad in (np.zeros(1, np.int32), np.zeros((2, 1), np.int32), np.zeros((3, 2), np.int32)):
        with pytest.raises(ValueError, match=r'have shape \(3, 1\)'):
            ring.push_packed(bad)
    with pytest.raises(TypeError, match='32-bit words'):
        ring.push_packed(np.zeros((3, 1), np.int64))
    with pytest.raises(NotImplementedError, match='one vector'):
        ring.ids()
    with pytest.raises(ValueError, match=r'ages must lie in \[1, 4\]'):
        ring.stacked_bits(ages=5)
    with pytest.raises(ValueError, match='row_mask'):
        ring.stacked_bits(row_mask=np.zeros((4, 1), np.int32))
    with pytest.raises(ValueError, match=r'age must lie in'):
        ring.events(4)
    # a ring without a batch keeps its rule: a 2-D push is not built
    one = _NoDevice(be, 10, 4, None)
    assert one.shape == (10,) and one.ndim == 1 and repr(one) == 'SpikeRing(n=10, depth=4)'
    with pytest.raises(NotImplementedError, match=r'batch=B'):
        one.push(np.zeros((3, 10), bool))
    with pytest.raises(NotImplementedError, match='batched ring'):
        one.push_packed(np.zeros(1, np.int32))
    with pytest.raises(NotImplementedError, match='batched ring'):
        one.stacked_bits()


def test_product_refusals_need_no_device(be):
    D = object.__new__(be.DelayedCSR)                    # (the checks below read the shape and the depth only)
    D.shape, D.depth = (10, 20), 4
    with pytest.raises(NotImplementedError, match='one sample'):
        D.update_on_pre(_NoDevice(be, 10, 4, 3), np.zeros(20, np.float32))
    with pytest.raises(ValueError, match='11 neurons'):
        _NoDevice(be, 11, 4, 3) @ D
    with pytest.raises(ValueError, match='remembers 3 steps'):
        _NoDevice(be, 10, 3, 3) @ D
    with pytest.raises(NotImplementedError):
        D @ _NoDevice(be, 10, 4, 3)
    with pytest.raises(NotImplementedError):
        be.BinaryArray(np.zeros((3, 10), bool)) @ D      # a 2-D array of spikes carries no history
    with pytest.raises(NotImplementedError, match='DelayedCSR'):
        _NoDevice(be, 10, 4, 3) @ object()               # anything but a DelayedCSR, a plain CSR included
    with pytest.raises(NotImplementedError):
        object() @ _NoDevice(be, 10, 4, 3)
    with pytest.raises(NotImplementedError, match='batched rings are not built'):
        be.ValueRing.push(object.__new__(be.ValueRing), np.zeros((3, 10), np.float32))     # ValueRing stays 1-D


# ---------------------------------------------------------------------------------------------------------------------------
# the constants of be_delay.hip
# ---------------------------------------------------------------------------------------------------------------------------
PATTERNS = {
    'kRingMaxBatch': r'constexpr\s+int\s+kRingMaxBatch\s*=\s*(\d+)',
    'kUnrollThreads': r'constexpr\s+int\s+kUnrollThreads\s*=\s*(\d+)',
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(BC.TILES)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    text = (CSRC / 'be_delay.hip').read_text()
    found = re.findall(PATTERNS[key], text)
    assert found, f"{key}: be_delay.hip no longer holds /{PATTERNS[key]}/ — the GPU cases sized by it need a look"
    assert {int(v) for v in found} == {BC.TILES[key]}, f"{key}: be_delay.hip says {found}, the cases assume {BC.TILES[key]}"


def test_grids_are_what_the_cases_assume():
    text = (CSRC / 'be_delay.hip').read_text()
    # the push: (bit tiles, batch rows), the last of all tickets advances head
    assert re.search(r'const dim3 grid\(\(unsigned\)tiles,\s*\(unsigned\)n_batch\),\s*block\(kRingThreads\)', text)
    assert re.search(r't == gridDim\.x \* gridDim\.y - 1', text)
    assert re.search(r'tiles = \(n \+ kRingTileBits - 1\) / kRingTileBits', text)
    # the unroll: (word tiles of kUnrollThreads words, batch rows), one word per thread
    assert re.search(r'dim3\(\(unsigned\)\(\(out_words \+ kUnrollThreads - 1\) / kUnrollThreads\),\s*\(unsigned\)n_batch\)', text)
    assert re.search(r'w = \(int64_t\)blockIdx\.x \* kUnrollThreads \+ threadIdx\.x', text)
    # neither entry point lets the batch pass the grid's second dimension, and neither memsets
    assert len(re.findall(r'n_batch >= 1 && n_batch <= kRingMaxBatch', text)) == 2
    assert 'hipMemset' not in text
    unroll = text[text.index('extern "C" int be_spike_ring_unroll'):]
    unroll = unroll[:unroll.index('\n}\n')]
    assert 'be_fill_async' not in unroll and 'atomic' not in text[text.index('void __launch_bounds__(kUnrollThreads)'):
                                                                      text.index('// value-history ring')]
    assert BC.UNROLL_TILE_BITS == DC.RING_TILE_BITS == 8192
