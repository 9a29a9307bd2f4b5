"""``tests/plan_layout_cases.py`` — the scatter plan's layouts restated on the host — against itself (decode(encode(x)) is the
CSR's multiset), against blocks typed out by hand from the layout comments of ``csrc/be_csr_plan.hip``, and its ``THRESHOLDS`` table
against the source text.  No GPU needed.  When a constant test fails after a retune, move the table with the source and re-size the
GPU cases that ``plan_layout_cases``'s docstring lists for that bound."""
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import plan_layout_cases as L

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'


def f32(*values) -> bytes:
    return struct.pack(f'<{len(values)}f', *values)


def u16(*values) -> bytes:
    return struct.pack(f'<{len(values)}H', *values)


def shift_for(W: int) -> int:
    return min(15, max(4, int(np.ceil(np.log2(W)))))


def payload_for(layout, rng, n):
    if layout in ('u16w', 'd8'):
        w = (rng.integers(-512, 513, n) / 256.0).astype(np.float32)     # zeros among them
        if n > 2:
            w[1] = -0.0
        return w
    if layout == 'q8':
        return rng.integers(0, 256, n).astype(np.uint8)
    return None


# ------------------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize('W', [3, 255, 256, 257, 19999, 20000])
@pytest.mark.parametrize('layout', L.LAYOUTS)
def test_decode_of_encode_is_the_csr(layout, W):
    rng = np.random.default_rng(1000 + W)
    k = 3 * W + max(1, W // 3)                       # four slices, the last one partial
    rows = L.edge_rows(rng, k, W)
    if W >= 400 and layout in L.SORTED:
        rows += L.escape_rows(layout, W + 5)
    idx, ptr = L.csr_of(rows)
    m = len(rows)
    pay = payload_for(layout, rng, idx.size)
    shift = shift_for(W)
    enc = L.encode(layout, pay, idx, ptr, m, k, shift, W)
    assert enc.seg.shape == (m, 4, 2) and enc.seg.dtype == np.uint32
    # lay the blocks out as the table says, poison everywhere else: decode must read defined bytes only
    blob = np.full(enc.units * 128 + 128, 0xA5, np.uint8)
    starts = enc.seg[..., 0].reshape(-1).astype(np.int64)
    at = np.repeat(starts * 128 - enc.byte_off, enc.nbytes) + np.arange(enc.data.size)
    assert np.unique(at).size == at.size                   # blocks do not overlap
    blob[at] = enc.data
    np.testing.assert_array_equal(L.defined_bytes(layout, enc.seg, blob), enc.data)
    assert L.blocks_mismatch(enc, blob) is None
    got = L.triples(*L.decode(layout, enc.seg, blob, k, shift, W))
    np.testing.assert_array_equal(got, L.csr_triples(layout, pay, idx, ptr, m))
    # the table: starts are the running sum of ceil(bytes / 128); an empty block has no groups and base 0
    units = (enc.nbytes + 127) // 128
    np.testing.assert_array_equal(starts, np.concatenate([[0], np.cumsum(units)[:-1]]))
    assert enc.units == units.sum()
    assert (enc.seg[..., 1].reshape(-1)[enc.count == 0] == 0).all()
    # and a flipped bit anywhere in the defined bytes is seen
    if enc.data.size:
        blob[at[enc.data.size // 2]] ^= 1
        assert L.blocks_mismatch(enc, blob) is not None


def test_fixed_length_rows_and_int64_row_pointers_encode_alike():
    rng = np.random.default_rng(5)
    m, k, n = 9, 700, 6
    idx = rng.integers(0, k, m * n).astype(np.int32)
    w = payload_for('d8', rng, m * n)
    a = L.encode('d8', w, idx, n, m, k, 9, 300)
    b = L.encode('d8', w, idx, (np.arange(m + 1) * n).astype(np.int64), m, k, 9, 300)
    np.testing.assert_array_equal(a.seg, b.seg)
    np.testing.assert_array_equal(a.data, b.data)


def test_weights_widen_exactly():
    import torch
    h = np.array([1.5, -0.0, 6.1e-5, 65504.0], np.float16)
    np.testing.assert_array_equal(L.weight_bits(h), np.array([0x3fc00000, 0x80000000, 0x387fc000, 0x477fe000], np.uint32))
    b = torch.tensor([1.5, -2.0, 3.0e38], dtype=torch.bfloat16)
    np.testing.assert_array_equal(L.weight_bits(b), b.float().numpy().view(np.uint32))
    np.testing.assert_array_equal(L.weight_bits(torch.tensor([1.5], dtype=torch.bfloat16)), [0x3fc00000])


# ------------------------------------------------------------------------------------------------------------ known answers
def test_known_blocks_u16_weighted():
    """[ f32 weight x 4 n4 ][ uint16 local column x 4 n4 ], pads (column 2^shift, weight 0); seg = { start, n4 }."""
    idx = np.array([17, 3, 3, 0, 1, 2, 4, 5], np.int32)
    ptr = np.array([0, 3, 3, 8], np.int32)
    w = np.array([1.0, 2.0, -0.0, 1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    e = L.encode('u16w', w, idx, ptr, 3, 32, 4, 0)
    np.testing.assert_array_equal(e.seg, [[[0, 1], [1, 1]], [[2, 0], [2, 0]], [[2, 2], [3, 0]]])
    assert e.units == 3
    assert e.block(0, 0) == f32(2.0, -0.0, 0, 0) + u16(3, 3, 16, 16)          # one column twice: by weight bits (0x40.. < 0x80..)
    assert e.block(0, 1) == f32(1.0, 0, 0, 0) + u16(1, 16, 16, 16)
    assert e.block(1, 0) == b'' and e.block(1, 1) == b''
    assert e.block(2, 0) == f32(1, 2, 3, 4, 5, 0, 0, 0) + u16(0, 1, 2, 4, 5, 16, 16, 16)       # five entries: two groups, 48 bytes
    # six groups are 144 bytes: two units
    e = L.encode('u16w', np.ones(21, np.float32), np.zeros(21, np.int32), 21, 1, 8, 4, 0)
    np.testing.assert_array_equal(e.seg, [[[0, 6]]])
    assert e.units == 2 and e.block(0, 0) == f32(*([1.0] * 21 + [0.0] * 3)) + u16(*([0] * 21 + [16] * 3))


def test_known_blocks_u16_counted():
    """[ uint16 local column x 8 n8 ], pads = column 2^shift; seg = { start, n8 }."""
    idx = np.array([9, 1, 1, 15, 0, 2, 3, 4, 5, 20], np.int32)
    e = L.encode('u16c', None, idx, np.array([0, 10, 10], np.int32), 2, 40, 4, 0)
    np.testing.assert_array_equal(e.seg, [[[0, 2], [1, 1], [2, 0]], [[2, 0], [2, 0], [2, 0]]])
    assert e.block(0, 0) == u16(0, 1, 1, 2, 3, 4, 5, 9, 15, 16, 16, 16, 16, 16, 16, 16)
    assert e.block(0, 1) == u16(4, 16, 16, 16, 16, 16, 16, 16)
    # a width that is no power of two: slices of 10 columns, pads still 2^shift
    e = L.encode('u16c', None, idx, np.array([0, 10], np.int32), 1, 40, 4, 10)
    np.testing.assert_array_equal(e.seg, [[[0, 1], [1, 1], [2, 1], [3, 0]]])
    assert e.block(0, 0) == u16(0, 1, 1, 2, 3, 4, 5, 9)                        # eight entries: one full group, no pad
    assert e.block(0, 1) == u16(5, 16, 16, 16, 16, 16, 16, 16) and e.block(0, 2) == u16(0, 16, 16, 16, 16, 16, 16, 16)
    # nine groups are 144 bytes
    e = L.encode('u16c', None, np.arange(65, dtype=np.int32) % 16, 65, 1, 16, 4, 0)
    assert e.units == 2 and e.seg[0, 0, 1] == 9


def test_known_blocks_d8():
    """[ f32 weight x 4 ng ][ uint8 delta x 4 ng ]; sorted by (column, position); first delta 0; a gap g > 0 is (g - 1) // 255
    escapes (0, 255) and a remainder in [1, 255]; tail pads (0, 0); seg = { start, ng | first local column << 16 }."""
    idx = np.array([516, 5, 600, 260, 5], np.int32)
    w = np.array([4.0, 1.0, 5.0, 3.0, 2.0], np.float32)
    e = L.encode('d8', w, idx, np.array([0, 0, 5], np.int32), 2, 1200, 9, 600)
    np.testing.assert_array_equal(e.seg, [[[0, 0], [0, 0]], [[0, 2 | 5 << 16], [1, 1]]])
    # 5 (pos 1), 5 (pos 4), 260: gap 255 = remainder 255, 516: gap 256 = one escape and remainder 1, three pads
    assert e.block(1, 0) == f32(1.0, 2.0, 3.0, 0, 4.0, 0, 0, 0) + bytes([0, 0, 255, 255, 1, 0, 0, 0])
    assert e.block(1, 1) == f32(5.0, 0, 0, 0) + bytes([0, 0, 0, 0])
    assert e.units == 2
    # gaps of 510 (one escape, remainder 255) and 511 (two escapes, remainder 1) from local column 599 - 1021: the base is kept
    idx = np.array([10 + 510 + 511, 10, 10 + 510], np.int32)
    e = L.encode('d8', np.array([3.0, 1.0, 2.0], np.float32), idx, 3, 1, 1200, 11, 1200)
    np.testing.assert_array_equal(e.seg, [[[0, 2 | 10 << 16]]])
    assert e.block(0, 0) == f32(1.0, 0, 2.0, 0, 0, 3.0, 0, 0) + bytes([0, 255, 255, 255, 255, 1, 0, 0])
    # 25 items are seven groups: 140 bytes, two units
    e = L.encode('d8', np.ones(24, np.float32), L.escape_rows('d8', 0)[0], 24, 1, 600, 10, 600)
    np.testing.assert_array_equal(e.seg, [[[0, 7]]])
    assert e.units == 2
    assert e.block(0, 0) == f32(*([1.0] * 23 + [0.0, 1.0, 0, 0, 0])) + bytes([0] + [1] * 22 + [255, 1, 0, 0, 0])


def test_known_blocks_h8():
    """[ uint8 code x 8 ng ]: a gap g is g // 255 bytes of 255, then g % 255; tail pads 255; seg as d8."""
    rows = [[7, 1027, 516, 261, 7], [7, 1027, 516, 261, 7, 1028], [], [1999]]
    idx, ptr = L.csr_of(rows)
    e = L.encode('h8', None, idx, ptr, 4, 2000, 11, 2000)
    np.testing.assert_array_equal(e.seg, [[[0, 1 | 7 << 16]], [[1, 2 | 7 << 16]], [[2, 0]], [[2, 1 | 1999 << 16]]])
    # 7, 7, 261 (254), 516 (255 = escape, 0), 1027 (511 = two escapes, 1): eight codes, no pad
    assert e.block(0, 0) == bytes([0, 0, 254, 255, 0, 255, 255, 1])
    assert e.block(1, 0) == bytes([0, 0, 254, 255, 0, 255, 255, 1, 1] + [255] * 7)
    assert e.block(3, 0) == bytes([0] + [255] * 7)
    # a second slice starts again at delta 0 with its own base; 129 items are 17 groups, 136 bytes: two units
    e = L.encode('h8', None, np.array([599, 600, 0], np.int32), 3, 1, 1200, 10, 600)
    np.testing.assert_array_equal(e.seg, [[[0, 1], [1, 1]]])
    assert e.block(0, 0) == bytes([0, 255, 255, 89] + [255] * 4) and e.block(0, 1) == bytes([0] + [255] * 7)
    e = L.encode('h8', None, L.escape_rows('h8', 1)[0], 128, 1, 600, 10, 600)
    np.testing.assert_array_equal(e.seg, [[[0, 17 | 1 << 16]]])
    assert e.units == 2 and e.block(0, 0) == bytes([0] + [1] * 126 + [255, 1] + [255] * 7)


def test_known_blocks_q8():
    """[ uint8 code x 4 ng ][ uint8 delta x 4 ng ] with d8's delta, escape and pad rules; the code 0x00 is a weight like any."""
    idx = np.array([516, 5, 600, 260, 5], np.int32)
    codes = np.array([0x7e, 0x38, 0x01, 0xb8, 0x00], np.uint8)
    e = L.encode('q8', codes, idx, np.array([0, 5], np.int32), 1, 1200, 9, 600)
    np.testing.assert_array_equal(e.seg, [[[0, 2 | 5 << 16], [1, 1]]])
    assert e.block(0, 0) == bytes([0x38, 0x00, 0xb8, 0, 0x7e, 0, 0, 0]) + bytes([0, 0, 255, 255, 1, 0, 0, 0])
    assert e.block(0, 1) == bytes([0x01, 0, 0, 0]) + bytes([0, 0, 0, 0])
    # a real entry of code 0x00 at a remainder of 255 is stored like an escape and is still counted as an item
    e = L.encode('q8', np.array([0x40, 0x00, 0x41], np.uint8), np.array([0, 255, 256], np.int32), 3, 1, 600, 10, 600)
    assert e.block(0, 0) == bytes([0x40, 0x00, 0x41, 0]) + bytes([0, 255, 1, 0])
    # 65 items are 17 groups: 136 bytes, two units
    e = L.encode('q8', np.full(64, 0x38, np.uint8), L.escape_rows('q8', 2)[0], 64, 1, 600, 10, 600)
    np.testing.assert_array_equal(e.seg, [[[0, 17 | 2 << 16]]])
    assert e.units == 2
    assert e.block(0, 0) == bytes([0x38] * 63 + [0, 0x38, 0, 0, 0]) + bytes([0] + [1] * 62 + [255, 1, 0, 0, 0])


def test_expected_order_and_sort_branch():
    idx, ptr = L.csr_of([[5, 3, 3, 9, 0], [], [2, 1]])
    np.testing.assert_array_equal(L.expected_order(idx, ptr), [4, 1, 2, 0, 3, 1, 0])
    assert L.expected_order(idx, ptr).dtype == np.uint16
    rng = np.random.default_rng(3)
    assert L.sort_branch(0, 90000, []).branch == 'short-ascending'
    assert L.sort_branch(2, 90000, [4, 3]).branch == 'short-bitonic'
    assert L.sort_branch(256, 90000, rng.integers(0, 90000, 256)).branch == 'short-bitonic'
    assert L.sort_branch(257, 90000, np.sort(rng.integers(0, 90000, 257))).branch == 'ascending'
    b = L.sort_branch(257, 90000, rng.integers(0, 90000, 257))                  # six buckets of 15000 columns
    assert b.branch == 'counting' and b.forms <= {'rank32', 'rank4'} and 'rank64' not in b.forms
    assert L.sort_branch(300, 2_000_000, rng.integers(0, 2_000_000, 300)).forms == {'rank64'}   # seven buckets of 285715 >= 2^18
    for big, want in ((64, {'rank32'}), (65, {'rank32', 'rank4'}), (256, {'rank32', 'rank4'})):
        b = L.sort_branch(600, 90000, L.row_with_bucket(rng, 600, big, 90000))
        assert (b.branch, b.largest, set(b.forms)) == ('counting', big, want)
    b = L.sort_branch(600, 90000, L.row_with_bucket(rng, 600, 257, 90000))
    assert (b.branch, b.largest) == ('fallback', 257)
    assert L.sort_branch(3000, 90000, np.full(3000, 777)).branch == 'ascending'


# ------------------------------------------------------------------------------------------------------------ constants
NUM = r'(\d+)'
PATTERNS = {          # table key -> regular expressions with one group = the value; every match of every pattern must agree
    'scan.chunk': [r'constexpr\s+int\s+kScanChunk\s*=\s*' + NUM],
    'scan.pass': [r'base\s*<\s*n_blocks\s*;\s*base\s*\+=\s*' + NUM, r'__launch_bounds__\(' + NUM + r'\)\s*k_scan_sums',
                  r'k_scan_sums\s*,\s*dim3\(1\)\s*,\s*dim3\(' + NUM + r'\)'],
    'grid.u16_cap': [r'k_plan_count\s*,\s*dim3\(grid_for\(m_rows\s*,\s*1\s*,\s*(\d+\s*\*\s*\d+)\)\)\s*,\s*dim3\(256\)',
                     r'const\s+int\s+grid\s*=\s*grid_for\(m\s*,\s*1\s*,\s*(\d+\s*\*\s*\d+)\)'],
    'grid.sorted_cap': [r'dim3\(grid_for\(m(?:_rows)?\s*,\s*1\s*,\s*(\d+\s*\*\s*\d+)\)\)\s*,\s*dim3\(1024\)',
                        r'const\s+int\s+g8\s*=\s*grid_for\(m\s*,\s*1\s*,\s*(\d+\s*\*\s*\d+)\)'],
    'kMaxSlices': [r'constexpr\s+int\s+kMaxSlices\s*=\s*' + NUM],
    'kD8MaxRow': [r'constexpr\s+int\s+kD8MaxRow\s*=\s*' + NUM],
    'kD8MaxSlices': [r'constexpr\s+int\s+kD8MaxSlices\s*=\s*' + NUM],
    'sort.bucket_target': [r'\(len\s*\+\s*\d+\)\s*/\s*' + NUM + r'\)'],
    'sort.max_buckets': [r'\(len\s*\+\s*\d+\)\s*/\s*\d+\)\s*:\s*' + NUM + r'u\s*;'],
    'sort.short_row': [r'len\s*>\s*' + NUM + r'\s*&&\s*blockDim\.x\s*==\s*1024'],
    'sort.bucket_one_per_lane': [r'if\s*\(B\s*<=\s*' + NUM + r'u\)'],
    'sort.bucket_limit': [r'too_big\s*=\s*mine\s*>\s*' + NUM + r'u'],
    'sort.key32_bits': [r'if\s*\(bw\s*<\s*\(1u\s*<<\s*' + NUM + r'\)\)'],
    'kD8MaxWidth': [r'constexpr\s+int\s+kD8MaxWidth\s*=\s*' + NUM],
    'kH8MaxWidth': [r'constexpr\s+int\s+kH8MaxWidth\s*=\s*' + NUM],
}
N_MATCHES = {'grid.u16_cap': 3, 'grid.sorted_cap': 6, 'sort.bucket_target': 2}      # launches / uses that must all be found


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(L.THRESHOLDS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_threshold_matches_the_source(key):
    text = (CSRC / 'be_csr_plan.hip').read_text()
    found = []
    for pattern in PATTERNS[key]:
        hits = re.findall(pattern, text)
        assert hits, f"{key}: be_csr_plan.hip no longer holds /{pattern}/ — the GPU cases sized by it need a look"
        found += hits
    assert len(found) >= N_MATCHES.get(key, 1), f'{key}: only {len(found)} places found'
    values = {int(np.prod([int(f) for f in v.split('*')])) for v in found}
    assert values == {L.THRESHOLDS[key]}, (
        f"{key}: be_csr_plan.hip says {found}, tests/plan_layout_cases.py assumes {L.THRESHOLDS[key]}: move the table and re-size "
        f"the cases of tests/test_plan_build_exact_gpu.py that its docstring lists for this bound")


def test_group_sizes_and_bytes_match_the_source():
    """24 / 16 bytes per u16 group, 20 per d8 group, 8 per h8 group; the sort key keeps 16 bits of position."""
    text = (CSRC / 'be_csr_plan.hip').read_text()
    assert re.search(r'plan_group\(bool homo\)\s*\{\s*return homo \? 8u : 4u;', text)
    assert re.search(r'n_groups \* \(homo \? 16u : 24u\);\s*return \(bytes \+ 127u\) >> 7;', text)
    assert re.search(r'd8_block_units\(uint32_t ng\)\s*\{\s*return \(ng \* 20u \+ 127u\) >> 7;', text)
    assert re.search(r'h8_block_units\(uint32_t ng\)\s*\{\s*return \(ng \* 8u \+ 127u\) >> 7;', text)
    assert re.search(r'H8 \|\| Q8 \? h8_block_units\(ng\) : d8_block_units\(ng\)', text)
