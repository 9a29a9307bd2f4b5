"""The loop bounds and dispatch thresholds that the FP8 GPU cases are sized by (tests/dense_f8_cases.py, CONSTS) are the ones in
csrc/be_dense_f8.hip, and the host formulas restated there (f8_any's dispatch, f8_parts_for, f8_mfma_parts, the K split) are the
ones written in the source.  No GPU needed: the source is read as text.  When this fails after a retune, move the table with the
source and re-size the GPU cases named in the message."""
import re
from pathlib import Path

import pytest

from dense_f8_cases import CONSTS, check_all_crossings, route

SOURCE = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc' / 'be_dense_f8.hip'
PARTS_FOR_LINE = r'const int64_t target = n_groups == 1 \? %s : %s, cap = n_groups == 1 \? %s : %s;'
D, G = r'\d+', r'(\d+)'

# table key -> (regular expression with one group, matches expected, GPU cases sized by it)
PATTERNS = {
    'k8Group': (r'constexpr int k8Group = (\d+);', 1, 'test_vector_route_s_at_w'),
    'k8MaxChunk': (r'constexpr int k8MaxChunk = (\d+);', 1, 'every case with more than 32 batch rows'),
    'k8Tile': (r'constexpr int k8Tile = (\d+);', 1, 'the list kernels: every S @ W8 case'),
    'k8Vec': (r'constexpr int k8Vec = (\d+);', 1, 'every case that names a scalar-load variant'),
    'masks.grid_cap': (r'const dim3 grid\(f8_grid_cap\(k, 256, (\d+)\)\);', 1, 'the mask kernels'),
    'reduce.grid_cap': (r'k8_reduce, dim3\(f8_grid_cap\([^,]+, 256, (\d+)\)\), dim3\(256\)', 2, 'test_mfma_parts_and_chunks[one_part]'),
    't.UNR': (r'constexpr int UNR = (\d+);', 1, 'test_vector_route_s_at_w[more_rows_than_parts]'),
    'nt.U': (r'constexpr int U = (\d+);', 1, 'test_vector_route_w_at_s[unroll_and_tail], [odd_k_long]'),
    'nt.rows_per_block': (r'const dim3 grid\(f8_grid_cap\(m, (\d+), \d+\)\);', 1, 'test_vector_route_w_at_s[second_trip]'),
    'nt.grid_cap': (r'const dim3 grid\(f8_grid_cap\(m, \d+, (\d+)\)\);', 1, 'test_vector_route_w_at_s[second_trip]'),
    'self_scan.max_tiles': (r'if \(nt <= (\d+)\) \{', 1, 'test_list_building_past_the_self_scan_limit'),
    'scan.block': (r'for \(int64_t base = 0; base < n_tiles; base \+= (\d+)\) \{', 1, 'test_list_building_past_the_self_scan_limit'),
    'k8MfmaCols': (r'#define BE_F8_MFMA_COLS (\d+)\b', 1, 'test_mfma_parts_and_chunks'),
    'k8MfmaChunk': (r'constexpr int k8MfmaChunk = (\d+);', 1, 'test_mfma_parts_and_chunks[two_chunks_16_parts]'),
    'mfma.D': (r'#define BE_F8_MFMA_D (\d+)\b', 1, 'test_mfma_parts_and_chunks[two_chunks_16_parts]'),
    'mfma.wg_target': (r'#define BE_F8_MFMA_WG_TARGET (\d+)\b', 1, 'test_mfma_parts_and_chunks'),
    'mfma.parts_clamp': (r'return \(int\)\(p < 1 \? 1 : \(p > (\d+) \? \d+ : p\)\);', 1, 'test_mfma_parts_and_chunks'),
    't_mfma.min_nb': (r'if \(vec_ok && nb >= (\d+)\) return f8_t_mfma<FMT>', 1, 'every case that names t_mfma or t_vec'),
    'parts_for.target_one_group': (PARTS_FOR_LINE % (G, D, D, D), 1, 'test_vector_route_s_at_w'),
    'parts_for.target': (PARTS_FOR_LINE % (D, G, D, D), 1, 'test_vector_route_s_at_w'),
    'parts_for.cap_one_group': (PARTS_FOR_LINE % (D, D, G, D), 1, 'test_vector_route_s_at_w'),
    'parts_for.cap': (PARTS_FOR_LINE % (D, D, D, G), 1, 'test_vector_route_s_at_w'),
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, matches, cases = PATTERNS[key]
    found = re.findall(pattern, SOURCE.read_text())
    assert len(found) == matches, f"{key}: be_dense_f8.hip holds /{pattern}/ {len(found)} times, not {matches} — look at {cases}"
    assert {int(v) for v in found} == {CONSTS[key]}, (f"{key}: be_dense_f8.hip says {sorted(set(found))}, tests/dense_f8_cases.py "
                                                      f"assumes {CONSTS[key]}: re-size {cases}")


# the dispatch conditions and formulas tests/dense_f8_cases.py restates on the host (route, parts_for, mfma_parts, mfma_geom, passes)
DISPATCH_TEXT = [
    # f8_any: which shape takes which kernel
    ('const bool vec_ok = (cols_w % k8Vec == 0) && ((reinterpret_cast<uintptr_t>(weights) & 15) == 0);', 1),
    ('if (vec_ok && nb >= 8) return f8_t_mfma<FMT>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);', 1),
    ('if (vec_ok) return f8_t_vec<FMT, 16>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);', 1),
    ('return f8_t_vec<FMT, 1>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);', 1),
    ('if (vec_ok) return f8_nt_vec<FMT, 16>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);', 1),
    ('return f8_nt_vec<FMT, 1>(w, scale, spikes_bm, sd, out_bm, rows_w, cols_w, nb, ws, st);', 1),
    # f8_parts_for
    ('const int64_t tasks = ((n + 64 * vec - 1) / (64 * vec)) * n_groups;', 1),
    ('const int64_t wgs = (tasks + 3) / 4;', 1),
    ('int64_t p = target / (wgs > 0 ? wgs : 1);', 1),
    ('if (p < 1) p = 1;', 1),
    ('if (p > cap) p = cap;', 1),
    ('const int parts = f8_parts_for(n, VEC, (int)((std::min<int64_t>(nb, k8MaxChunk) + k8Group - 1) / k8Group));', 1),
    # f8_mfma_parts and the K split of k8_densemm_mfma
    ('const int64_t tiles = (n + k8MfmaCols - 1) / k8MfmaCols;', 1),
    ('int64_t p = BE_F8_MFMA_WG_TARGET / (tiles > 0 ? tiles : 1);', 1),
    ('const uint32_t steps_total = (n_union + 15u) >> 4;', 1),
    ('const uint32_t per_part = (steps_total + gridDim.y - 1) / gridDim.y;', 1),
    ('for (uint32_t c0 = t_begin; c0 < t_end; c0 += k8MfmaChunk) {', 1),
    ('for (uint32_t t0 = c0; t0 < c_end; t0 += D) {', 1),
    # f8_lists: one list takes the fused masks + counts, and no scan launch up to the limit
    ('if (nl == 1) {', 1),
    ('if (nt <= 1024) {', 1),
    ('const int slot = WHOLE ? k8MaxGroups : 0, nl = WHOLE ? 1 : n_groups;', 1),
    ('if (base + 8 <= k && (k & 7) == 0 && (reinterpret_cast<uintptr_t>(spikes) & 7) == 0) {', 1),
    # passes over the batch and the loops inside the vector kernels
    ('for (int64_t b0 = 0; b0 < nb; b0 += k8MaxChunk) {', 3),
    ('for (; a + (uint32_t)(UNR - 1) * parts < cnt; a += (uint32_t)UNR * parts) {', 1),
    ('for (; j + (int64_t)(U - 1) * 64 * VEC < k; j += (int64_t)U * 64 * VEC) {', 1),
    ('for (int64_t r = wave; r < m; r += n_waves) {', 1),
    ('if (nc == 1) hipLaunchKernelGGL((k8_densemm_nt<FMT, VEC, 1>)', 1),
    ('else if (nc <= 8) hipLaunchKernelGGL((k8_densemm_nt<FMT, VEC, 8>)', 1),
    ('else hipLaunchKernelGGL((k8_densemm_nt<FMT, VEC, 32>)', 1),
    # the epilogue: the scale is applied to the finished f32 sum, once
    ('out[i] = s * scale;', 1),
    ('out_bm[(int64_t)(b0 + b) * m + r] = s * scale;', 1),
    ('const float sc = (float)scale;', 1),
]


def test_dispatch_conditions_are_the_ones_restated():
    text = SOURCE.read_text()
    for line, times in DISPATCH_TEXT:
        assert text.count(line) == times, (f"be_dense_f8.hip holds {line!r} {text.count(line)} times, not {times}: "
                                           f"tests/dense_f8_cases.py restates it on the host — move both together")


def test_dispatch_restated():
    """Which shape takes which kernel."""
    assert route((64, 32), 8, True) == 't_mfma' and route((64, 32), 7, True) == 't_vec16'
    assert route((64, 33), 8, True) == 't_vec1' and route((64, 32), 8, True, aligned=False) == 't_vec1'
    assert route((64, 32), 1, False) == route((64, 32), 65, False) == 'nt_vec16'
    assert route((64, 31), 9, False) == 'nt_vec1' and route((64, 32), 9, False, aligned=False) == 'nt_vec1'


def test_fp8_stays_out_of_the_typed_dispatch():
    """FP8 has its own entry point: the typed-variant grammar, be_dispatch_wdtype and _W_CODE keep refusing it."""
    import torch
    from brainevent_amd import _array as A
    assert torch.float8_e4m3fn not in A._W_CODE and torch.float8_e5m2 not in A._W_CODE
    common = (SOURCE.parent / 'be_common.h').read_text()
    assert 'F8' not in common and 'fp8' not in common.lower()


def test_every_gpu_case_crosses_its_bound():
    check_all_crossings()
