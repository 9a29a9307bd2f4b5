"""The loop bounds that tests/test_update_kernels_at_scale_gpu.py sizes its cases by (its THRESHOLDS table) are the ones in
csrc/be_plasticity.hip, csrc/be_grad.hip and csrc/be_csr_shared.h.  No GPU needed: the sources are read as text.  When this
fails after a retune (kTile, a grid cap, cols_per_y, kMaxBatch), move the table with the source and re-size the GPU cases the
table's user names for that bound (the list in that module's docstring)."""
import re
from pathlib import Path

import pytest

from test_update_kernels_at_scale_gpu import THRESHOLDS

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'
FILES = {'plast': 'be_plasticity.hip', 'grad': 'be_grad.hip', 'shared': 'be_csr_shared.h'}

# table key -> (file, regular expression with one group = the value; every match in the file must agree)
PATTERNS = {
    'plast.kScanThreads': ('plast', r'constexpr\s+int\s+kScanThreads\s*=\s*(\d+)'),
    'plast.kScanPer': ('plast', r'constexpr\s+int\s+kScanThreads\s*=\s*\d+\s*,\s*kScanPer\s*=\s*(\d+)'),
    'plast.kRowThreads': ('plast', r'constexpr\s+int\s+kRowThreads\s*=\s*(\d+)'),
    'plast.kRowPer': ('plast', r'constexpr\s+int\s+kRowThreads\s*=\s*\d+\s*,\s*kRowPer\s*=\s*(\d+)'),
    'plast.rows_grid_cap': ('plast', r'grid_for\(\s*nnz_hint\s*,\s*kTile\s*,\s*(\d+)\s*\)'),
    'plast.nonzero_grid_cap': ('plast', r'k_plast_nonzero\s*,\s*dim3\(\s*grid_for\(\s*n\s*,\s*256\s*,\s*(\d+)\s*\)'),
    'plast.cols_per_y': ('plast', r'const\s+int64_t\s+cols_per_y\s*=\s*(\d+)\s*;'),
    'plast.dense_pre_grid': ('plast', r'grid_for\(\s*n_active_max\s*,\s*1\s*,\s*\(int\)\(\s*(\d+)\s*/\s*gy'),
    'plast.dense_post_grid_cap': ('plast', r'grid_for\(\s*n_rows\s*,\s*1\s*,\s*(\d+)\s*\)'),
    'grad.kRowThreads': ('grad', r'constexpr\s+int\s+kRowThreads\s*=\s*(\d+)'),
    'grad.kRowPer': ('grad', r'constexpr\s+int\s+kRowThreads\s*=\s*\d+\s*,\s*kRowPer\s*=\s*(\d+)'),
    'grad.rows_grid_cap': ('grad', r'int\s+rows_grid\(int64_t\s+nse\)\s*\{\s*return\s+grid_for\(\s*nse\s*,\s*kTile\s*,\s*(\d+)\s*\)'),
    'grad.cols_per_y': ('grad', r'const\s+int64_t\s+cols_per_y\s*=\s*(\d+)\s*;'),
    'grad.dense_grid': ('grad', r'grid_for\(\s*n_rows\s*,\s*1\s*,\s*\(int\)\(\s*(\d+)\s*/\s*gy'),
    'grad.pack_grid_cap': ('grad', r'grid_for\(\s*n\s*\*\s*nw\s*,\s*256\s*,\s*(\d+)\s*\)'),
    'grad.pack_ids_grid_cap': ('grad', r'k_grad_pack_ids\s*,\s*dim3\(\s*grid_for\(\s*n\s*,\s*256\s*,\s*(\d+)\s*\)'),
    'grad.finish_threads': ('grad', r'for\s*\(int\s+i\s*=\s*threadIdx\.x;\s*i\s*<\s*n;\s*i\s*\+=\s*(\d+)\)'),
    'kMaxBatch': ('shared', r'constexpr\s+int\s+kMaxBatch\s*=\s*(\d+)'),
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(THRESHOLDS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_threshold_matches_the_source(key):
    which, pattern = PATTERNS[key]
    text = (CSRC / FILES[which]).read_text()
    found = re.findall(pattern, text)
    assert found, f"{key}: {FILES[which]} no longer holds /{pattern}/ — the GPU cases sized by it need a look"
    assert {int(v) for v in found} == {THRESHOLDS[key]}, (
        f"{key}: {FILES[which]} says {found}, tests/test_update_kernels_at_scale_gpu.py assumes {THRESHOLDS[key]}: "
        "re-size the cases its docstring lists for this bound")


def test_tile_is_threads_times_per_thread():
    """Both files derive kTile as kRowThreads * kRowPer (the GPU cases compute the tile the same way), and the dense splits
    launch 256 threads."""
    for which in ('plast', 'grad'):
        text = (CSRC / FILES[which]).read_text()
        assert re.search(r'kTile\s*=\s*kRowThreads\s*\*\s*kRowPer\s*;', text), which
    assert re.search(r'k_grad_finish<W>\s*,\s*dim3\(1\)\s*,\s*dim3\((\d+)\)', (CSRC / FILES['grad']).read_text()).group(1) == \
        str(THRESHOLDS['grad.finish_threads'])
