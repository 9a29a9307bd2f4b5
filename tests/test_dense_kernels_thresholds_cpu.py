"""The loop bounds and dispatch thresholds that tests/test_dense_kernels_at_scale_gpu.py sizes its cases by (its CONSTS table) are
the ones in csrc/be_dense.hip, and the host formulas it restates (densemm_any's dispatch, parts_for, mfma_parts, the gather and
self-scan switches) are the ones written there.  No GPU needed: the source is read as text.  When this fails after a retune (a grid
cap, kMfmaChunk, kNtChunk, kTfChunk, BE_MFMA_WG_TARGET, the parts_for targets, an MFMA threshold), move the table with the source
and re-size the GPU cases named in the message."""
import re
from pathlib import Path

import pytest

from test_dense_kernels_at_scale_gpu import CONSTS, check_all_crossings

SOURCE = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc' / 'be_dense.hip'
PARTS_FOR_LINE = r'const int64_t target = n_groups == 1 \? %s : %s, cap = n_groups == 1 \? %s : %s;'
D, G = r'\d+', r'(\d+)'

# table key -> (regular expression whose groups multiply to the value; every match must agree, matches expected, GPU cases sized by it)
PATTERNS = {
    'kTile': (r'constexpr int kTile = (\d+);', 1, 'every case that counts tiles: test_gl_scan_*, test_scan_route_*, test_self_scan_*'),
    'kGroup': (r'constexpr int kGroup = (\d+);', 1, 'test_t_vec_one_part, test_t_vec_fifteen_parts_unroll_split'),
    'kMaxChunk': (r'constexpr int kMaxChunk = (\d+);', 1, 'every case with more than 32 batch rows'),
    'masks.grid_cap': (r'const dim3 grid\(grid_cap_fwd\(k, 256, (\d+)\)\);', 1, 'test_mask_stride_loops'),
    'self_scan.max_tiles': (r'if \(nt <= (\d+)\) \{', 2, 'test_self_scan_at_its_limit_and_past_it, test_scan_route_nt_vec, test_scan_route_t_mfma'),
    'scan.block': (r'for \(int64_t base = 0; base < n_tiles; base \+= (\d+)\) \{', 1, 'test_gl_scan_second_trip_per_group_lists'),
    'nt.rows_per_block': (r'dim3\(grid_cap\(m, (\d+), \d+ \* \d+\)\), dim3\(256\)', 1, 'test_nt_row_loop_second_trip'),
    'nt.grid_cap': (r'dim3\(grid_cap\(m, \d+, (\d+) \* (\d+)\)\), dim3\(256\)', 1, 'test_nt_row_loop_second_trip'),
    'nt.U': (r'constexpr int U = (\d+);', 1, 'test_nt_stream_unroll_split'),
    'dense_reduce.grid_cap': (r'k_dense_reduce<W>, dim3\(grid_cap\(nb \* n, 256, (\d+)\)\), dim3\(256\)', 1, 'test_t_vec_one_part'),
    'mfma_reduce.grid_cap': (r'k_mfma_reduce<W>, dim3\(grid_cap\(\(int64_t\)nc \* n, 256, (\d+)\)\), dim3\(256\)', 1, 'test_mfma_chunks_one_part'),
    'kMfmaCols': (r'#define BE_MFMA_COLS (\d+)\b', 1, 'test_mfma_partly_filled_column_tiles and every mfma_parts'),
    'kMfmaChunk': (r'constexpr int kMfmaChunk = (\d+);', 1, 'test_mfma_chunks_sixteen_parts, test_mfma_chunks_one_part'),
    'mfma.wg_target': (r'#define BE_MFMA_WG_TARGET (\d+)\b', 1, 'test_mfma_chunks_*, test_tf32_chunks, test_mfma_empty_ranges_and_silent_batches'),
    'mfma.parts_clamp': (r'return \(int\)\(p < 1 \? 1 : \(p > (\d+) \? \d+ : p\)\);', 1, 'test_mfma_chunks_sixteen_parts, test_tf32_chunks'),
    'kNtChunk': (r'constexpr int kNtChunk = (\d+);', 1, 'test_nt_mfma16_mask_chunks, test_nt_mfma_f32_mask_chunks'),
    'kTfChunk': (r'constexpr int kTfChunk = (\d+);', 1, 'test_tf32_chunks'),
    'parts_for.target_one_group': (PARTS_FOR_LINE % (G, D, D, D), 1, 'test_t_vec_one_part, test_t_vec_more_parts_than_active_rows'),
    'parts_for.target': (PARTS_FOR_LINE % (D, G, D, D), 1, 'test_t_vec_one_part, test_t_vec_fifteen_parts_unroll_split'),
    'parts_for.cap_one_group': (PARTS_FOR_LINE % (D, D, G, D), 1, 'test_t_vec_more_parts_than_active_rows'),
    'parts_for.cap': (PARTS_FOR_LINE % (D, D, D, G), 1, 'test_t_vec_fifteen_parts_unroll_split'),
    'UNR': (r'constexpr int UNR = (\d+);', 1, 'test_t_vec_fifteen_parts_unroll_split'),
    't_mfma.min_nb': (r'if \(vec_ok && nb >= (\d+)\) return densemm_t_mfma<W>', 1, 'every case that names t_mfma or t_vec'),
    'nt_mfma.min_nb': (r'#define BE_NT_MFMA_MIN_NB (\d+)\b', 1, 'every case that names nt_mfma or nt_vec'),
    'nt_mfma_f32.min_nb': (r'if \(vec_ok && nb >= (\d+) && rows_w >= \d+ && cols_w >= \d+\)', 1, 'test_nt_mfma_f32_mask_chunks, test_nt_row_loop_second_trip'),
    'nt_mfma.min_rows': (r'rows_w >= (\d+) && cols_w >= \d+\)', 2, 'test_nt_mfma*, test_nt_row_loop_second_trip'),
    'nt_mfma.min_cols_16bit': (r'nb >= BE_NT_MFMA_MIN_NB && rows_w >= \d+ && cols_w >= (\d+)\)', 1, 'test_nt_mfma_shortest_contractions'),
    'nt_mfma.min_cols_f32': (r'nb >= \d+ && rows_w >= \d+ && cols_w >= (\d+)\)', 1, 'test_nt_mfma_shortest_contractions'),
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, matches, cases = PATTERNS[key]
    found = re.findall(pattern, SOURCE.read_text())
    assert len(found) == matches, f"{key}: be_dense.hip holds /{pattern}/ {len(found)} times, not {matches} — look at {cases}"
    values = set()
    for groups in found:
        v = 1
        for g in ([groups] if isinstance(groups, str) else groups):
            v *= int(g)
        values.add(v)
    assert values == {CONSTS[key]}, (f"{key}: be_dense.hip says {sorted(values)}, tests/test_dense_kernels_at_scale_gpu.py assumes "
                                     f"{CONSTS[key]}: re-size {cases}")


# the dispatch conditions and formulas the GPU file restates on the host (route, parts_for, mfma_parts, t_mfma_geom, n_tiles_of, passes)
DISPATCH_TEXT = [
    # parts_for
    ('const int64_t tasks = ((n + 64 * vec - 1) / (64 * vec)) * n_groups;', 1),
    ('const int64_t wgs = (tasks + 3) / 4;', 1),
    ('int64_t p = target / (wgs > 0 ? wgs : 1);', 1),
    ('if (p < 1) p = 1;', 1),
    ('if (p > cap) p = cap;', 1),
    ('parts_used = parts_for(n, VEC, (int)((std::min<int64_t>(nb, kMaxChunk) + kGroup - 1) / kGroup));', 1),
    # mfma_parts and the K split of the S @ W MFMA kernels
    ('const int64_t tiles = (n + kMfmaCols - 1) / kMfmaCols;', 1),
    ('int64_t p = BE_MFMA_WG_TARGET / (tiles > 0 ? tiles : 1);', 1),
    ('const int parts = std::is_same<W, float>::value ? mfma_parts(n / 2) : mfma_parts(n);', 1),
    ('const uint32_t steps_total = (n_union + 15u) >> 4;', 1),
    ('const uint32_t steps_total = (n_union + 1u) >> 1;', 1),
    ('const uint32_t per_part = (steps_total + gridDim.y - 1) / gridDim.y;', 2),
    # densemm_any
    ('const bool vec_ok = (cols_w % V == 0) && ((reinterpret_cast<uintptr_t>(weights) & 15) == 0);', 1),
    ('if (vec_ok && nb >= 8) return densemm_t_mfma<W>(w, spikes_bm, sd, o, rows_w, cols_w, nb, ws, st);', 1),
    ('if (vec_ok && nb >= BE_NT_MFMA_MIN_NB && rows_w >= 4096 && cols_w >= 32)', 1),
    ('if (vec_ok && nb >= 8 && rows_w >= 4096 && cols_w >= 8)', 1),
    ('if (vec_ok) return densemm_t_vec<W, V>(w, spikes_bm, sd, o, rows_w, cols_w, nb, ws, st);', 1),
    ('return densemm_t_vec<W, 1>(w, spikes_bm, sd, o, rows_w, cols_w, nb, ws, st);', 1),
    ('if (vec_ok) return densemm_nt_vec<W, V>(w, spikes_bm, sd, o, rows_w, cols_w, nb, ws, st);', 1),
    ('return densemm_nt_vec<W, 1>(w, spikes_bm, sd, o, rows_w, cols_w, nb, ws, st);', 1),
    ('#define BE_NT_MFMA16 1', 1),
    # the switches inside the routes
    ('const bool gather = (int64_t)n_union * 16 < k;', 1),
    ('if (nt <= 1024) {', 2),
    ('inline int64_t n_tiles_of(int64_t k) { return (k + kTile - 1) / kTile; }', 1),
    ('for (int64_t b0 = 0; b0 < nb; b0 += kMaxChunk) {', 4),
    ('if (nc == 1) rc = densemm_nt_launch<W, VEC, 1>', 1),
    ('else if (nc <= 8) rc = densemm_nt_launch<W, VEC, 8>', 1),
    ('else rc = densemm_nt_launch<W, VEC, 32>', 1),
    ('for (; a + (uint32_t)(UNR - 1) * parts < cnt; a += (uint32_t)UNR * parts) {', 1),
    ('for (; a + 3u * 64u < n_union; a += 4u * 64u) {', 1),
    ('for (; j + (int64_t)(U - 1) * 64 * VEC < k; j += (int64_t)U * 64 * VEC) {', 1),
    ('if (base + 8 <= k && (k & 7) == 0 && (reinterpret_cast<uintptr_t>(spikes) & 7) == 0) {', 1),
]


def test_dispatch_conditions_are_the_ones_restated():
    text = SOURCE.read_text()
    for line, times in DISPATCH_TEXT:
        assert text.count(line) == times, (f"be_dense.hip holds {line!r} {text.count(line)} times, not {times}: "
                                           f"tests/test_dense_kernels_at_scale_gpu.py restates it on the host — move both together")


def test_every_gpu_case_crosses_its_bound():
    """The crossing assertions of the GPU cases (tiles against the scan limits, rows per trip against m, parts, steps per part against
    the staged chunks, the route every shape takes), here without a device."""
    check_all_crossings()
