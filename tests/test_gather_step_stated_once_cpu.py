"""The gather kernels (csrc/be_csr.hip: k_csrmv_nt_wave, k_csrmv_nt_vec, k_csrmm_nt_fused, k_csrmm_nt_fused_vec) are a skeleton
each plus shared parts: bitmap staging, the per-entry accumulate ladder, the reduce, the whole-wave walk of a long row, the
guarded four-entry load, the fused slots' bit visit / clear / wavefront sync and the 64-row batch header are written once; the host
picks the lanes per row in two chooser functions and launches through one function.  No GPU needed: the source is read as text.
A second spelling of any of these is a second copy that a fix to the spike test or to the end-of-array handling would miss."""
import re
from pathlib import Path

import pytest

from test_plan_step_stated_once_cpu import _code, _top_level_blocks

SRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc' / 'be_csr.hip'

# what the four kernels used to repeat, by the text that has to appear in any copy of it
ONCE = {
    'bitmap staging': 'bits_s[i] = src[i];',
    'accumulate: count': 'cnt += on ? 1 : 0;',
    'accumulate: streamed weight': 'acc += on ? (ACC)__uint_as_float(',
    'accumulate: load if on': 'else if (on) acc += (ACC)WTraits<W>::load(',
    'reduce: counts': 'cnt += __shfl_down(cnt, off,',
    'reduce: sums': 'acc += __shfl_down(acc, off,',
    'long-row walk: valid mask': 'valid |= (j0 + 256 * u + 4 * lane + q < plen ? 1u : 0u)',
    'long-row walk: spike test': 'spike_mask<IN_LDS, 8, AT0>(',
    'long-row walk: piece': 'p0 += (1ll << 30)',
    'guarded load: condition': 'b + j + 4 <= nnz_end',
    'guarded load: scalar fallback': '= (uint32_t)indices[b + j + e];',
    'fused: bit visit': 'bits &= bits - 1;',
    'fused: count slot': '[b] += 1u;',
    'fused: weight of an entry': 'VECW ? __uint_as_float(wbits) :',
    'fused: slot clear': 'for (int b = 0; b < 32; ++b)',
    'batch header': 't.rl = t.valid ? rp.at(rc + 1) - t.rb : 0;',
    'static-LDS guard': 'be_static_lds_bytes(',
}
FENCE_TRIPLE = (r'__builtin_amdgcn_fence\(__ATOMIC_RELEASE, "wavefront"\);\s*__builtin_amdgcn_wave_barrier\(\);\s*'
                r'__builtin_amdgcn_fence\(__ATOMIC_ACQUIRE, "wavefront"\);')
GONE = ['BE_NT_VEC', 'BE_NT_VEC_AT0']
THRESHOLDS = {'gather_lpr_of': ['kGatherLpr2MaxRow', 'kGatherLpr4MaxRow', 'kGatherLpr8MaxRow', 'kGatherLpr16MaxRow',
                                'kGatherLpr8MaxFixed', 'kGatherLpr16MaxFixed'],
              'fused_lpr_of': ['kFusedLpr8MaxRow', 'kFusedLpr16MaxRow']}
KERNELS = ['k_csrmv_nt_wave', 'k_csrmv_nt_vec', 'k_csrmm_nt_fused', 'k_csrmm_nt_fused_vec']


@pytest.fixture(scope='module')
def code():
    return _code(SRC.read_text())


@pytest.mark.parametrize('what', sorted(ONCE))
def test_each_shared_part_is_spelled_once(code, what):
    assert code.count(ONCE[what]) == 1, f"{what}: {ONCE[what]!r} occurs {code.count(ONCE[what])} times in be_csr.hip"


def test_the_wavefront_fence_triple_is_spelled_once(code):
    assert len(re.findall(FENCE_TRIPLE, code)) == 1
    assert code.count('wave_lds_sync();') >= 3          # the fused-vec kernel's rounds, before and after its fold


def test_the_launch_macros_are_gone():
    text = SRC.read_text()
    for name in GONE:
        assert not re.search(re.escape(name) + r'\b', text), f"{name} is back: use gather_lpr_of + be_dispatch_int + launch_gather"


def _users(code, name):
    """Headers of the top-level blocks that use `name` (its definition does not count); `name` is defined once."""
    assert len(re.findall(r'\b' + name + r' = \d+[,;]', code)) == 1, name
    blocks, inside = _top_level_blocks(code), set()
    for m in re.finditer(r'\b' + name + r'\b(?! = \d)', code):
        owner = [h for s, e, h in blocks if s <= m.start() < e]
        assert owner, f"{name} is used outside any function"
        inside.add(owner[0])
    return inside


def test_each_lanes_per_row_threshold_is_applied_in_its_chooser_only(code):
    for chooser, names in THRESHOLDS.items():
        for name in names:
            users = _users(code, name)
            assert len(users) == 1 and chooser in next(iter(users)), f"{name} is applied in {sorted(users)}"
    users = _users(code, 'kGatherVecMaxRow')                # the end of the lanes-per-row range: both choosers, nothing else
    assert len(users) == 2 and all(any(c in u for c in THRESHOLDS) for u in users), sorted(users)


@pytest.mark.parametrize('kernel', KERNELS)
def test_each_kernel_is_defined_once(code, kernel):
    defs = [h for _, _, h in _top_level_blocks(code) if '__global__' in h and re.search(r'\b' + kernel + r'\s*\(', h)]
    assert len(defs) == 1, f"{kernel}: {len(defs)} __global__ definitions"
