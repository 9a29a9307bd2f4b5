"""The loop bounds that tests/test_event_jit_kernels_at_scale_gpu.py sizes its cases by (its CONSTS table) are the ones in
csrc/be_jitc.hip and csrc/be_jitc_shared.h, and the dispatch conditions it restates are the ones written there.  No GPU needed: the
sources are read as text.  When this fails after a retune (a grid cap, the LDS limit, the window size, kPieceU32 / kPieceU64,
BE_JIT_WG_TARGET), move the table with the source and re-size the GPU cases named in the message."""
import re
from pathlib import Path

import pytest

from test_event_jit_kernels_at_scale_gpu import CONSTS, check_all_crossings

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'

# table key -> (file, regular expression whose groups multiply to the value; every match must agree, matches expected, GPU cases sized by it)
PATTERNS = {
    'mv_gather.rows_per_block': ('be_jitc.hip', r'const dim3 grid\(gcap\(m, (\d+), \d+\), p\.n_chunks\);', 1,
                                 'test_mv_gather_row_loop_second_trip, test_gather_shard_beyond_one_trip'),
    'mv_gather.grid_cap': ('be_jitc.hip', r'const dim3 grid\(gcap\(m, \d+, (\d+)\), p\.n_chunks\);', 1,
                           'test_mv_gather_row_loop_second_trip, test_gather_shard_beyond_one_trip'),
    'lds_limit': ('be_jitc.hip', r'if \(lds <= (\d+) \* (\d+)\) \{', 1, 'test_mv_gather_bits_from_global_memory'),
    'gather_reduce.grid_cap': ('be_jitc.hip', r'k_jit_gather_reduce<MODE, W>\), dim3\(gcap\(m, 256, (\d+)\)\), dim3\(256\)', 1,
                               'test_gather_reduce_second_trip'),
    'masks.grid_cap': ('be_jitc.hip', r'k_jit_masks\w*(?:<Spike\w+>)?, dim3\(gcap\(in_len, 256, (\d+)\)\), dim3\(256\)', 3,
                       'test_mm_gather_lds_windows[*-u8]'),
    'convert.grid_cap': ('be_jitc.hip', r'k_jit_convert<float, \w+>\), dim3\(gcap\(n, 256, (\d+)\)\), dim3\(256\)', 2,
                         'test_convert_loop_and_f32_scratch_beyond_32_columns'),
    'mm.lds_window_bytes': ('be_jitc.hip', r'const int64_t win_cap = (\d+) \* (\d+) / mask_sz;', 1,
                            'test_mm_gather_lds_windows, test_mm_gather_global_masks'),
    'mm.max_windows': ('be_jitc.hip', r'if \(n_win <= (\d+) && p\.stride == 4', 1, 'test_mm_gather_lds_windows, test_mm_gather_global_masks'),
    'mm_global.grid_cap': ('be_jitc.hip', r'k_jit_mm_gather<MODE, A, \d+>\), dim3\(gcap\(rows, 256, (\d+)\)\), dim3\(256\)', 3,
                           'test_mm_gather_global_masks'),
    'materialise.grid_cap': ('be_jitc.hip', r'gcap\(n_rows \* p\.n_chunks \* stride, 256, (\d+)\)', 2, 'test_materialisation_beyond_one_grid'),
    'edge_weights.grid_cap': ('be_jitc.hip', r'const dim3 grid\(gcap\(n, 256, (\d+)\)\), block\(256\);', 1,
                              'test_materialisation_beyond_one_grid'),
    'kPieceU32': ('be_jitc_shared.h', r'kPieceU32 = (\d+)', 1,
                  'test_mv_scatter_several_pieces[s], test_mm_scatter_several_pieces_and_parts[s], test_scatter_shards_several_pieces[s]'),
    'kPieceU64': ('be_jitc_shared.h', r'kPieceU64 = (\d+)', 1,
                  'test_mv_scatter_several_pieces[u / n], test_mm_scatter_several_pieces_and_parts[u / n], test_scatter_shards_several_pieces[u]'),
    'wg_target': ('be_jitc_shared.h', r'#define BE_JIT_WG_TARGET (\d+)\b', 1,
                  'test_mm_scatter_several_pieces_and_parts, test_scatter_active_row_loop_second_trip'),
    'parts_clamp': ('be_jitc_shared.h', r'g\.parts = std::max\(1, std::min\(parts, (\d+)\)\);', 1,
                    'test_mm_scatter_several_pieces_and_parts, test_scatter_active_row_loop_second_trip'),
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    name, pattern, matches, cases = PATTERNS[key]
    found = re.findall(pattern, (CSRC / name).read_text())
    assert len(found) == matches, f"{key}: {name} holds /{pattern}/ {len(found)} times, not {matches} — look at {cases}"
    values = set()
    for groups in found:
        v = 1
        for g in ([groups] if isinstance(groups, str) else groups):
            v *= int(g)
        values.add(v)
    assert values == {CONSTS[key]}, (f"{key}: {name} says {sorted(values)}, tests/test_event_jit_kernels_at_scale_gpu.py assumes "
                                     f"{CONSTS[key]}: re-size {cases}")


# the dispatch conditions and formulas the GPU file restates on the host (mm_windows, scatter_geom, cross_bits_in_lds, the `a` loop)
DISPATCH_TEXT = {
    'be_jitc.hip': [
        ('const size_t lds = (size_t)(((std::min<int64_t>(p.chunk_size, p.walk_len) + 31) / 32) + 2) * 4;', 1),
        ('if (lds <= 150 * 1024) {', 1),
        ('hipLaunchKernelGGL((k_jit_mv_gather<MODE, false>), grid, dim3(1024), 0, st, p, bits, m, partial);', 1),
        ('const int64_t mask_sz = nc <= 8 ? 1 : (nc <= 16 ? 2 : 4);', 1),
        ('const int64_t n_win = (chunk_cols + win_cap - 1) / win_cap;', 1),
        ('const int64_t win_cols = (chunk_cols + n_win - 1) / n_win;', 1),
        ('if (n_win <= 256 && p.stride == 4 && rows > 0) {', 1),
        ('if (nc <= 8) hipLaunchKernelGGL((k_jit_mm_gather<MODE, A, 8>)', 1),
        ('else if (nc <= 16) hipLaunchKernelGGL((k_jit_mm_gather<MODE, A, 16>)', 1),
        ('else hipLaunchKernelGGL((k_jit_mm_gather<MODE, A, 32>)', 1),
        ('for (int64_t b0 = 0; b0 < n_batch; b0 += 32) {', 1),
        ('if (g.pieces == 1) {', 1),
        ('hipLaunchKernelGGL(kern, sgrid, dim3(1024), lds, st, p, active, count, g.pieces, g.parts, g.piece_len, fx_scale, partial,', 2),
        ('a < n_active; a += (uint64_t)parts * blockDim.x)', 1),
        ('return std::max(-90, std::min(150, 62 - e - lg));', 1),
    ],
    'be_jitc_shared.h': [
        ('const int64_t Qmax = (std::min<int64_t>(p.chunk_size, p.walk_len) + p.stride - 1) / p.stride;', 1),
        ('g.pieces = (int)std::max<int64_t>(1, (Qmax + cap - 1) / cap);', 1),
        ('g.piece_len = (uint32_t)std::max<int64_t>(256, (per_piece + 255) & ~255ll);', 1),
        ('int parts = (int)(BE_JIT_WG_TARGET / std::max<int64_t>(1, (int64_t)g.n_classes * g.pieces * n_batch));', 1),
        ('if ((q0 + qi + e) * S + l < width)', 1),
    ],
}


@pytest.mark.parametrize('name', sorted(DISPATCH_TEXT))
def test_dispatch_conditions_are_the_ones_restated(name):
    text = (CSRC / name).read_text()
    for line, times in DISPATCH_TEXT[name]:
        assert text.count(line) == times, (f"{name} holds {line!r} {text.count(line)} times, not {times}: "
                                           f"tests/test_event_jit_kernels_at_scale_gpu.py restates it on the host — move both together")


def test_every_gpu_case_crosses_its_bound():
    """The crossing assertions of the GPU cases (rows per trip against m, pieces, windows, parts, tasks against grid), here without a device."""
    check_all_crossings()


# ---- the walk and the weight-dtype dispatch are each stated once
WALK_SPELLINGS = ('lr_initial_q(', 'lr_next_nz(', 'q + 1u + lr_bounded(')      # start, step, step: the generator of every JITC kernel
# BE_REQUIRE checks of a weight dtype ahead of the dispatch (entry points that need the element size, or whose message carries their name)
DTYPE_CHECKS = {'be_dense.hip': 1, 'be_jitc_grad.hip': 1, 'be_slice.hip': 2}
# the one other place that sets the message itself: BE_FP_PASS, a launcher macro with its own arguments (be_fixed_point.hip)
DTYPE_SETTERS = {'be_common.h': 1, 'be_fixed_point.hip': 1}


def test_the_walk_and_the_dtype_dispatch_are_stated_once():
    """Every JITC kernel draws its matrix through JitWalk (be_jitc_shared.h): a second spelling of the start or the step anywhere
    under csrc/ is a second generator that only a full GPU parity run would tell apart.  Likewise the weight-dtype switch: its
    default case lives in be_dispatch_wdtype (be_common.h)."""
    texts = {p.name: p.read_text() for p in sorted(CSRC.iterdir()) if p.suffix in ('.hip', '.h')}
    for spelling in WALK_SPELLINGS:
        holders = sorted(name for name, text in texts.items() if spelling in text)
        assert holders == ['be_jitc_shared.h'], f"{spelling!r} is spelled in {holders}: the walk belongs to be_jitc_shared.h alone"
    message = '"unknown weight dtype"'
    setters = {name: text.count('be_set_error(' + message + ')') for name, text in texts.items()}
    assert {n: c for n, c in setters.items() if c} == DTYPE_SETTERS, "a hand-written weight-dtype switch: use be_dispatch_wdtype"
    checks = {name: len(re.findall(r'BE_REQUIRE\([^;]*' + re.escape(message) + r'\);', text)) for name, text in texts.items()}
    assert {n: c for n, c in checks.items() if c} == DTYPE_CHECKS
    for name, text in texts.items():      # nothing else mentions the message
        assert text.count('unknown weight dtype') == setters[name] + checks[name], name
