"""The loop bounds and dispatch thresholds that tests/test_spike_front_kernels_at_scale_gpu.py sizes its cases by (its CONSTS
table) are the ones in csrc/be_csr.hip (the two constants of the fused gather route: csrc/be_csr_shared.h), and its numpy
references agree with brute-force loops.  No GPU needed: the source is read as text.  When this fails after a retune (a tile of the
compaction, a grid cap, a batch edge, the LDS bitmap), move the table with the source and re-size the GPU cases that the message
names."""
import re
from pathlib import Path

import numpy as np
import pytest

import test_spike_front_kernels_at_scale_gpu as G
from test_spike_front_kernels_at_scale_gpu import CONSTS, check_all_crossings

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'
SOURCE = CSRC / 'be_csr.hip'
SHARED = CSRC / 'be_csr_shared.h'

_COMPACT = r'tiles = \(n \+ (\d+) \* (\d+) - 1\) / \(\1 \* \2\);\n\s+hipLaunchKernelGGL\(\(k_compact_spikes<SP, %s>\), dim3\(\(unsigned\)tiles, \(unsigned\)nb\), dim3\(%s\)'
_FRONT = 'test_compact_ladder, test_compact_batched'
_SCATTER = ('test_direct_scatter, test_direct_scatter_convert_past_one_trip, test_direct_scatter_from_an_id_list, '
            'test_direct_scatter_wrong_neighbour, test_indexed_scatter')
_GATHER = 'test_indexed_gather, test_indexed_gather_one_fired_entry_per_row'

# table key -> (regular expression whose groups multiply to the value — for the keys in SHIFTED the first shifted left by the
# second —, GPU cases sized by the bound); every match must agree
PATTERNS = {
    'block': (r'__global__ void __launch_bounds__\((\d+)\) k_(?:compact_bits|unpack_spikes|pack_spikes_vec|pack_spikes|csrmv_t_direct|'
              r'csrmv_t_direct_indexed|csrmv_nt_indexed|convert_from_f32|coarsen_bits|batch_masks)\(', 'every case'),
    'compact.small.tile': (_COMPACT % ('16, 256', '256'), _FRONT),
    'compact.small.max_n': (r'if \(n <= \((\d+)ll << (\d+)\)\) \{ +// small vectors', _FRONT),
    'compact.mid.tile': (_COMPACT % ('16, 1024', '1024'), _FRONT),
    'compact.mid.max_n': (r'\} else if \(n <= \((\d+)ll << (\d+)\)\) \{ +// 16384 elements per workgroup', _FRONT),
    'compact.large.tile': (_COMPACT % ('64, 1024', '1024'), _FRONT),
    'bits.max_n_1': (r'if \(n <= \((\d+)ll << (\d+)\)\) \{\n\s+hipLaunchKernelGGL\(\(k_compact_bits<1>\)', _FRONT),
    'bits.words_1': (r'k_compact_bits<1>\), dim3\(\(unsigned\)\(\(n_words \+ 255\) / (\d+)\), \(unsigned\)nb\), dim3\(256\)', _FRONT),
    'bits.words_4': (r'k_compact_bits<4>\), dim3\(\(unsigned\)\(\(n_words \+ 1023\) / (\d+)\), \(unsigned\)nb\), dim3\(256\)', _FRONT),
    'pack.vec.grid_cap': (r'k_pack_spikes_vec, dim3\(grid_for\(\(n \+ 31\) / 32, 256, (\d+)\), \(unsigned\)nb\)', 'test_pack_vector_path'),
    'pack.ballot.grid_cap': (r'k_pack_spikes<SP>, dim3\(grid_for\(n, 256, (\d+)\), \(unsigned\)nb\)', 'test_pack_ballot_path'),
    'unpack.grid_cap': (r'k_unpack_spikes, dim3\(grid_for\(n, 256, (\d+)\)\)', 'test_unpack_past_one_trip'),
    'convert.grid_cap': (r'k_convert_from_f32<W>, dim3\(grid_for\(k \* nb, 256, (\d+)\)\)', 'test_direct_scatter_convert_past_one_trip'),
    'masks.grid_cap': (r'k_batch_masks<Spike(?:Float|Bool)>, dim3\(grid_for\(k, 256, (\d+)\)\)', 'test_gather_fused_batch_masks'),
    'masks.group': (r'for \(int b0 = 0; b0 < nc; b0 \+= (\d+)\)', 'test_gather_fused_batch_masks'),
    'scatter.grid': (r'const int gx = nb >= \d+ \? \d+ : (\d+);', _SCATTER),
    'scatter.grid_batch': (r'const int gx = nb >= \d+ \? (\d+) : \d+;', _SCATTER),
    'indexed.grid_cap': (r'const int grid = grid_for\(m, 4, nb >= \d+ \? \d+ : (\d+)\);', _GATHER),
    'indexed.grid_cap_batch': (r'const int grid = grid_for\(m, 4, nb >= \d+ \? (\d+) : \d+\);', _GATHER),
    'batch_edge': (r'(?:const int gx = nb >= (\d+) \? \d+ : \d+;|const int grid = grid_for\(m, 4, nb >= (\d+) \? \d+ : \d+\);)',
                   _SCATTER + ', ' + _GATHER),
    'lds_bitmap_bytes': (r'constexpr int64_t kLdsBitmapBytes = (\d+) \* (\d+);', 'test_gather_coarse_group_edge'),
    'coarsen.word_shift': (r'\n      if \(g_shift < (\d+)\) \{\n', 'test_gather_coarse_group_edge'),
    'fused.min_batch': (r'constexpr int kFusedMinBatch = (\d+);', 'test_gather_fused_batch_masks'),
    'fused.min_work': (r'constexpr int64_t kFusedMinWork = (\d+);', 'test_gather_fused_batch_masks'),
}
MATCHES = {'block': 10, 'masks.grid_cap': 2, 'batch_edge': 2}
SHIFTED = {'compact.small.max_n', 'compact.mid.max_n', 'bits.max_n_1'}
IN_SHARED_HEADER = {'fused.min_batch', 'fused.min_work'}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


def test_the_crossings_follow_from_the_table():
    check_all_crossings()


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, cases = PATTERNS[key]
    source = SHARED if key in IN_SHARED_HEADER else SOURCE
    found = re.findall(pattern, source.read_text())
    assert len(found) == MATCHES.get(key, 1), (f"{key}: {source.name} holds /{pattern}/ {len(found)} times — the GPU cases sized by it "
                                               f"need a look: {cases}")
    values = set()
    for groups in found:
        groups = [int(g) for g in ([groups] if isinstance(groups, str) else groups) if g != '']
        if key in SHIFTED:
            values.add(groups[0] << groups[1])
        else:
            v = 1
            for g in groups:
                v *= g
            values.add(v)
    assert values == {CONSTS[key]}, (f"{key}: {source.name} says {sorted(values)}, tests/test_spike_front_kernels_at_scale_gpu.py "
                                     f"assumes {CONSTS[key]}: re-size {cases}")


def test_launch_shapes_around_the_constants():
    """What the GPU cases take for granted besides the numbers: the 256-thread launches, a tile of the compaction being threads x
    elements per thread, n_round rounding to whole waves in k_pack_spikes and its lane-32 guard, the vector path's condition in
    launch_pack, nb >= 8 as the batch edge of both direct grids, four waves per workgroup of the direct kernels, the fused
    route's condition in csrmv_nt, the coarse groups' geometry, and active_stride = 0 for the single-vector compaction."""
    text = SOURCE.read_text()
    for kernel in ('k_pack_spikes_vec', 'k_pack_spikes<SP>', 'k_unpack_spikes', 'k_convert_from_f32<W>', r'\(k_csrmv_t_direct<W, HOMO, ACC>\)',
                   r'\(k_csrmv_t_direct_indexed<W, ACC, int64_t>\)', r'\(k_csrmv_t_direct_indexed<W, ACC, int32_t>\)',
                   r'\(k_csrmv_nt_indexed<W, int64_t>\)', r'\(k_csrmv_nt_indexed<W, int32_t>\)', r'k_batch_masks<SpikeFloat>',
                   r'k_batch_masks<SpikeBool>', 'k_coarsen_bits'):
        assert len(re.findall(r'hipLaunchKernelGGL\(' + kernel + r', dim3\([^;]*?\), dim3\(256\), 0,', text)) == 1, kernel
    assert len(re.findall(r'const int64_t tile = \(int64_t\)blockIdx\.x \* \(kThreads \* kCompactPerThread\);', text)) == 1
    assert len(re.findall(r'const int64_t first_word = \(\(int64_t\)blockIdx\.x \* 256 \+ threadIdx\.x\) \* kWords;', text)) == 1
    assert len(re.findall(r'const int64_t n_round = \(n \+ 63\) & ~\(int64_t\)63;', text)) == 1
    assert len(re.findall(r'if \(lane == 32 && \(i < n\)\) bits\[word\] = \(uint32_t\)\(mask >> 32\);', text)) == 1
    assert len(re.findall(r'if \(sizeof\(typename SP::type\) == 1 && \(reinterpret_cast<uintptr_t>\(spikes\) & 15\) == 0 && '
                          r'\(nb == 1 \|\| \(n & 15\) == 0\)\) \{', text)) == 1
    assert len(re.findall(r'sizeof\(typename SP::type\) == 1 && f \+ 16 <= n && \(reinterpret_cast<uintptr_t>\(spikes\) & 15\) == 0', text)) == 1
    assert len(re.findall(r'const int gx = nb >= 8 \? ', text)) == 1 and len(re.findall(r'grid_for\(m, 4, nb >= 8 \? ', text)) == 1
    assert len(re.findall(r'const uint32_t n_waves = \(gridDim\.x \* blockDim\.x\) >> 6;', text)) == 2
    assert len(re.findall(r'const int64_t n_waves = \(\(int64_t\)gridDim\.x \* blockDim\.x\) >> 6;\n  for \(int64_t r = wave; r < m; r \+= n_waves\) \{\n'
                          r'    const int64_t b = rp\.at\(r\), e = rp\.at\(r \+ 1\);\n    ACC acc = ACC\(0\);\n    for \(int64_t j = b \+ lane; j < e; j \+= 64\) \{\n'
                          r'      const uint32_t c = \(uint32_t\)indices\[j\];', text)) == 1
    assert len(re.findall(r'if \(nb >= kFusedMinBatch && m > 0 && \(nnz_hint / m\) \* nb >= kFusedMinWork && nnz_hint / m >= 16 && '
                          r'!std::is_same<W, double>::value &&\n\s+\(sd == BE_SPIKE_BOOL \|\| sd == BE_SPIKE_FLOAT\)\) \{', text)) == 1
    assert len(re.findall(r'while \(\(\(\(k \+ \(\(int64_t\)1 << g\) - 1\) >> g\) \+ 31\) / 32 \* 4 > kLdsBitmapBytes\) \+\+g;', text)) == 1
    assert len(re.findall(r'return compact_any\(spikes, spike_dtype, n, 1, active_ids, 0, count,', text)) == 1
    assert len(re.findall(r'pack_any\(spikes(?:_bm)?, spike_dtype, n, (?:1|n_batch), bits, \(n \+ 31\) / 32,', text)) == 2
    csr_py = (CSRC.parent / '_csr.py').read_text()          # the wrapper's hint for the gather: the average row length of a CSR
    assert len(re.findall(r'hint = row_len if transpose or indptr is None or perm is not None else int\(indices\.numel\(\) // max\(m, 1\)\)',
                          csr_py)) == 1


# ------------------------------------------------------------------------------- the numpy references against brute force
def _matrix(rng, m, k):
    lens = rng.permutation(np.resize(np.asarray(G.ROW_LENS), m))
    idx = rng.integers(0, k, int(lens.sum()))
    return lens, idx, np.repeat(np.arange(m), lens)


@pytest.mark.parametrize('n', [1, 2, 31, 32, 33, 63, 64, 65, 100])
def test_id_and_word_references_against_loops(n):
    rng = np.random.default_rng(n)
    for density in G.DENSITIES:
        fired = G.fired_of(rng, n, density)
        ids = [i for i in range(n) if fired[i]]
        assert G.ref_ids(fired).tolist() == ids and G.ref_ids(fired).dtype == np.uint32
        words = [0] * ((n + 31) // 32)
        for i in ids:
            words[i // 32] |= 1 << (i % 32)
        assert G.ref_words(fired).tolist() == words and G.ref_words(fired).dtype == np.uint32
        # the operands the GPU cases build from `fired`: nonzero bytes / v > 0 exactly where it fired, every bit past n set
        assert [int(b != 0) for b in G.bool_bytes(rng, fired)] == [int(f) for f in fired]
        assert [bool(v > 0) for v in G.float_values(rng, fired)] == [bool(f) for f in fired]
        op = G.bits_operand(fired, 2)
        assert op.size == len(words) + 2 and op[-1] == op[-2] == 0xffffffff
        for i in range(32 * len(words)):
            assert (int(op[i // 32]) >> (i % 32)) & 1 == (fired[i] if i < n else 1)


def test_product_references_against_loops():
    rng = np.random.default_rng(1)
    m, k, nb = 37, 23, 3
    lens, idx, row_of = _matrix(rng, m, k)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    w = G.exact_weights(rng, idx.size, 'f32', False)
    assert (w != 0).all() and (w < 0).any() and (w > 0).any() and np.all(w * 2 == np.round(w * 2))
    perm = rng.permutation(idx.size)
    rows_fired, cols_fired = rng.random((nb, m)) < 0.5, rng.random((nb, k)) < 0.5
    for wj in (w, w[perm]):
        scatter, gather = np.zeros((nb, k)), np.zeros((nb, m))
        for b in range(nb):
            for r in range(m):
                for j in range(ptr[r], ptr[r + 1]):
                    assert row_of[j] == r
                    if rows_fired[b, r]:
                        scatter[b, idx[j]] += wj[j]
                    if cols_fired[b, idx[j]]:
                        gather[b, r] += wj[j]
        np.testing.assert_array_equal(G.ref_scatter(wj, idx, row_of, k, rows_fired), scatter)
        np.testing.assert_array_equal(G.ref_gather(wj, idx, row_of, m, cols_fired), gather)
    # the bitwise expectation: one entry per column at most
    lens, ptr, idx, row_of, perm = G.ragged(m, 5000, 3, one_per_column=True)
    bits = G.mantissa_weights(rng, idx.size)
    want = np.zeros((nb, 5000), dtype=np.int32)
    for b in range(nb):
        for j in range(idx.size):
            if rows_fired[b, row_of[j]]:
                assert want[b, idx[j]] == 0
                want[b, idx[j]] = bits[j]
    np.testing.assert_array_equal(G.expect_own_bits(bits, idx, row_of, 5000, rows_fired), want)
    assert np.isfinite(bits.view(np.float32)).all() and (bits != 0).all()


def test_case_structures():
    """The matrices and spike sets of the GPU cases are what their docstrings say (host arrays only)."""
    for nb in (1, 8):
        m, k = G.SCATTER_M[nb], G.SCATTER_K[nb]
        lens, ptr, idx, row_of, perm = G.ragged(m, k, 40 + nb)
        assert set(lens.tolist()) == set(G.ROW_LENS) and ptr[-1] == idx.size == lens.sum() and idx.min() >= 0 and idx.max() < k
        assert np.bincount(idx, minlength=k).max() <= -(-idx.size // k)
        assert np.array_equal(np.sort(perm), np.arange(idx.size))
        fired = G.active_rows(m, 40 + nb, nb, G.SCATTER_ACTIVE[nb])
        assert (fired.sum(1) == G.SCATTER_ACTIVE[nb]).all() and (fired[:, lens == 0].sum(1) == 2).all()
        # the bound of the exactness argument holds for the widest weights of every dtype on every structure of the scatter cases
        for dt in G.DTYPES:
            assert -(-idx.size // k) * G.W_UNITS[dt] * 0.5 <= G.EXACT_MAX[dt]
            assert -(-m * 65 // k) * G.W_UNITS[dt] * 0.5 <= G.EXACT_MAX[dt]
        m1, k1, _, _, idx1, _, _ = G.one_per_column_case(nb)
        assert m1 == m and np.bincount(idx1, minlength=k1).max() == 1
