"""The loop bounds that tests/test_convert_kernels_at_scale_gpu.py sizes its cases by (its CONSTS table) are the ones in
csrc/be_convert.hip.  No GPU needed: the source is read as text.  When this fails after a retune (a grid cap, kScanTile, the strip
of the totals' scan, a lane threshold), move the table with the source and re-size the GPU cases that module's docstring lists
for the bound."""
import re
from pathlib import Path

import pytest

from test_convert_kernels_at_scale_gpu import CONSTS, check_all_crossings

SOURCE = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc' / 'be_convert.hip'

# table key -> (regular expression whose groups multiply to the value; every match must agree, GPU cases sized by the bound)
PATTERNS = {
    'count.ids_per_thread': (r'k_t_count, dim3\(grid_for\(\(nnz \+ 3\) / (\d+), 256,',
                             'test_count_past_one_trip, test_out_of_range_ids_are_counted_not_dropped'),
    'count.grid_cap': (r'k_t_count, dim3\(grid_for\(\(nnz \+ 3\) / 4, 256, (\d+) \* (\d+)\)\)',
                       'test_count_past_one_trip, test_out_of_range_ids_are_counted_not_dropped'),
    'scan.tile': (r'constexpr int kScanTile = (\d+) \* (\d+);',
                  'test_scan_across_tiles, test_scan_past_one_strip_of_totals, test_scan_of_wide_counts_and_the_int32_output'),
    'scan.strip': (r'for \(int64_t b = 0; b < n_tiles; b \+= (\d+)\)', 'test_scan_past_one_strip_of_totals'),
    'cursor.grid_cap': (r'k_t_cursor_init, dim3\(grid_for\(nb, 256, (\d+)\)\)', 'test_scan_past_one_strip_of_totals'),
    'fill.grid_cap': (r'const int grid = grid_for\(m, 256 / LPR, (\d+) \* (\d+)\);',
                      'test_fill_past_one_trip, test_column_blocks_at_scale'),
    'fill.avg_lpr1': (r'if \(avg_row <= (\d+)\) return launch_fill<1, PT>\(', 'test_fill_lane_choice_edges, test_fill_past_one_trip'),
    'fill.avg_lpr4': (r'if \(avg_row <= (\d+)\) return launch_fill<4, PT>\(', 'test_fill_lane_choice_edges, test_fill_past_one_trip'),
    'fill.avg_lpr16': (r'if \(avg_row <= (\d+)\) return launch_fill<16, PT>\(', 'test_fill_lane_choice_edges, test_fill_past_one_trip'),
    'gather.grid_cap': (r'const int grid = grid_for\(n, 256, (\d+) \* (\d+)\);', 'test_gather_by_perm_past_one_trip'),
    'block': (r'__global__ void __launch_bounds__\((\d+)\) k_(?:t_count|t_cursor_init|t_fill|gather_by_perm)\(', 'every case'),
}
MATCHES = {'block': 4}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


def test_the_crossings_follow_from_the_table():
    check_all_crossings()


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, cases = PATTERNS[key]
    found = re.findall(pattern, SOURCE.read_text())
    assert len(found) == MATCHES.get(key, 1), (f"{key}: be_convert.hip holds /{pattern}/ {len(found)} times — the GPU cases sized by "
                                               f"it need a look: {cases}")
    values = set()
    for groups in found:
        v = 1
        for g in ([groups] if isinstance(groups, str) else groups):
            v *= int(g)
        values.add(v)
    assert values == {CONSTS[key]}, (f"{key}: be_convert.hip says {sorted(values)}, tests/test_convert_kernels_at_scale_gpu.py assumes "
                                     f"{CONSTS[key]}: re-size {cases}")


def test_launch_shapes_around_the_constants():
    """What the GPU cases take for granted besides the numbers: the workgroup sizes of the launches, the 1024-thread scan kernels
    (8 columns a thread, 16 waves whose sums the tile carry adds), one workgroup for the totals, the last lane choice, and that
    CscBuilder always asks for the 64-bit offsets (the int32 instantiation is reached by the direct call only)."""
    text = SOURCE.read_text()
    assert len(re.findall(r'dim3\(256\), 0, st', text)) == 4                   # count, cursor init, fill, gather
    assert len(re.findall(r'__launch_bounds__\(1024\) k_scan64_(?:totals|of_totals|apply)\(', text)) == 3
    assert len(re.findall(r'k_scan64_of_totals, dim3\(1\), dim3\(1024\)', text)) == 1
    assert len(re.findall(r'\(int64_t\)threadIdx\.x \* 8;', text)) == 2 and CONSTS['scan.tile'] == 1024 * 8
    assert len(re.findall(r'constexpr int kGroups = 256 / LPR;', text)) == 1
    assert len(re.findall(r'\n  return launch_fill<64, PT>\(', text)) == 1
    assert len(re.findall(r'const int64_t avg = nnz / m;', text)) == 1
    convert_py = (SOURCE.parent.parent / '_convert.py').read_text()
    assert len(re.findall(r"call\('be_csr_to_csc_indptr', A\.ptr\(self\.counts\), self\.k, A\.ptr\(self\.csc_indptr\), 1,", convert_py)) == 1
