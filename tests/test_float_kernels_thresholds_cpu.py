"""The loop bounds that tests/test_float_kernels_at_scale_gpu.py sizes its cases by (its CONSTS table) are the ones in
csrc/be_float.hip, csrc/be_jitc_float.hip and csrc/be_jitc_shared.h.  No GPU needed: the sources are read as text.  When this
fails after a retune (a grid cap, kTile, kPieceU64, a lane threshold), move the table with the source and re-size the GPU cases
that module's docstring lists for the bound."""
import re
from pathlib import Path

import pytest

from test_float_kernels_at_scale_gpu import CONSTS

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'

# table key -> (file, regular expression whose groups multiply to the value; every match in the file must agree)
PATTERNS = {
    'float.grid_cap': ('be_float.hip', r'grid_for\(m,\s*(?:256 / LPR_|4),\s*(\d+) \* (\d+)\)'),
    'float.mm_rows_per_block': ('be_float.hip', r'k_fcsrmm_n?t<W, HOMO, CPG_>\), dim3\(grid_for\(m,\s*(\d+),'),
    'float.avg_short': ('be_float.hip', r'if \(avg_row <= (\d+)\) BE_F_N?T\(4\)'),
    'float.avg_medium': ('be_float.hip', r'else if \(avg_row <= (\d+)\) BE_F_N?T\(16\); else BE_F_N?T\(64\)'),
    'float.round_grid_cap': ('be_float.hip', r'k_img_round<W>\), dim3\(grid_for\(k \* n, 256, (\d+)\)'),
    'jit.kTile': ('be_jitc_float.hip', r'constexpr int kTile = (\d+);'),
    'jit.gather_grid_cap': ('be_jitc_float.hip', r'gcap\(out_len, \(int\)tpb, (\d+)\)'),
    'jit.reduce_grid_cap': ('be_jitc_float.hip', r'k_jit_f_gather_reduce<MODE, W, \w+>\), dim3\(gcap\(out_len(?: \* kTile)?, 256, (\d+)\)'),
    'jit.scatter_grid_cap': ('be_jitc_float.hip', r'gcap\(tasks, 256, (\d+) \* (\d+)\)'),
    'jit.round_grid_cap': ('be_jitc_float.hip', r'k_jit_f_round<W>\), dim3\(gcap\(out_len \* n, 256, (\d+)\)'),
    'jit.kPieceU64': ('be_jitc_shared.h', r'kPieceU64 = (\d+)'),
}
MATCHES = {'float.grid_cap': 4, 'float.mm_rows_per_block': 2, 'float.avg_short': 2, 'float.avg_medium': 2, 'jit.reduce_grid_cap': 2}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    name, pattern = PATTERNS[key]
    found = re.findall(pattern, (CSRC / name).read_text())
    assert len(found) == MATCHES.get(key, 1), f"{key}: {name} holds /{pattern}/ {len(found)} times — the GPU cases sized by it need a look"
    values = set()
    for groups in found:
        v = 1
        for g in ([groups] if isinstance(groups, str) else groups):
            v *= int(g)
        values.add(v)
    assert values == {CONSTS[key]}, (f"{key}: {name} says {sorted(values)}, tests/test_float_kernels_at_scale_gpu.py assumes "
                                     f"{CONSTS[key]}: re-size the cases its docstring lists for this bound")


def test_one_mv_block_serves_256_over_lanes_rows():
    """The mv kernels take 256 / LPR rows per block of 256 threads (the GPU cases compute the one-trip span from that)."""
    text = (CSRC / 'be_float.hip').read_text()
    assert len(re.findall(r'dim3\(grid_for\(m, 256 / LPR_, 256 \* 16\)\), dim3\(256\)', text)) == 2
    assert len(re.findall(r'256 / LPR\)', text)) >= 3
