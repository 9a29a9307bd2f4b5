"""The planned scatter step (csrc/be_csr_plan.hip) is a skeleton plus a decoder per layout: the workgroup -> task mapping, the
in-kernel active-row list, the position range of the pre-gathered table, the lane -> list position arithmetic and the rotation of
the pointer pipeline are written once (PlanTask / PlanRows) and used by k_plan_accumulate, k_plan_accumulate_d8 and
k_plan_accumulate_h8; the host picks the kernel in one function (plan_variant_of) and launches it through one integral-constant
dispatch.  No GPU needed: the sources are read as text.  A second spelling of any of these is a second copy that only a full GPU
parity run over all 60 instances would tell apart."""
import re
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc'
PLAN = CSRC / 'be_csr_plan.hip'

# what the three step kernels used to repeat, by the text that has to appear in any copy of it
ONCE = {
    'XCD task mapping': '(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3)',
    'in-kernel active-row list': 'build_part_list<FUSED>(',
    'FUSED 3 position range': 'const uint32_t npp = (n_active + (uint32_t)parts - 1u) / (uint32_t)parts;',
    'a0': 'const uint64_t a0 =',
    'a0, fused': ': FUSED  ? (uint64_t)wave + (uint64_t)nw * lane',
    'a0, pre-gathered': '(uint64_t)pos_lo + (uint64_t)wave * 64 + lane',
    'a0, listed': '(uint64_t)part + (uint64_t)parts * (',
    'a_step': '(uint64_t)nw * 64 : (uint64_t)parts * nw * 64',
    'rotation: block starts': 'st_v = sgn.x;',
    'rotation: lengths': 'n4_v = v_n ? sgn.y : 0u;',
    'rotation: validity': 'v_n = v_nn;',
    'rotation: row ids': 'r_n = r_nn;',
}
GONE = ['#define COMMA', 'BE_PLAN_BY_FUSED', 'BE_PLAN_LAUNCH', 'BE_FUSED_ARGS', 'BE_SINGLE', 'BE_SINGLE_W']
THRESHOLDS = ['kD8QuarterMaxBlock', 'kD8EighthMaxBlock', 'kSub4MaxBlock', 'kSub8MaxBlock', 'kSub16MaxBlock', 'kSub32MaxBlock',
              'kSubW4MaxBlock', 'kSubW8MaxBlock', 'kSubW16MaxBlock', 'kSubW32MaxBlock', 'kD8NtMinBlock']
KERNELS = ['k_plan_accumulate', 'k_plan_accumulate_d8', 'k_plan_accumulate_h8', 'k_plan_single', 'k_gather_seg', 'k_compact_gather_seg']


def _code(text):
    """The text without comments (line structure kept)."""
    text = re.sub(r'/\*.*?\*/', lambda m: re.sub(r'[^\n]', ' ', m.group(0)), text, flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def _top_level_blocks(code):
    """(start, end, header) of every brace block that is not nested in another one; `namespace {` and `extern "C" {` do not count
    as nesting.  The header is the text between the previous block (or `;`) and the opening brace."""
    blocks, depth, start, last_end = [], 0, None, 0
    for m in re.finditer(r'[{}]', code):
        if m.group(0) == '{':
            head = code[last_end:m.start()]
            if depth == 0 and re.search(r'(namespace\s*\w*|extern\s+"C")\s*$', head):
                last_end = m.end()
                continue                                   # transparent: its members are top level
            if depth == 0:
                start = m.start()
            depth += 1
        else:
            if depth == 0:                                 # closes a namespace / extern "C"
                last_end = m.end()
                continue
            depth -= 1
            if depth == 0:
                blocks.append((start, m.end(), code[last_end:start].strip()))
                last_end = m.end()
    assert depth == 0
    return blocks


@pytest.fixture(scope='module')
def plan_code():
    return _code(PLAN.read_text())


@pytest.mark.parametrize('what', sorted(ONCE))
def test_each_piece_of_the_skeleton_is_spelled_once(plan_code, what):
    assert plan_code.count(ONCE[what]) == 1, f"{what}: {ONCE[what]!r} occurs {plan_code.count(ONCE[what])} times in be_csr_plan.hip"


def test_the_launch_macros_are_gone():
    for p in sorted(CSRC.iterdir()):
        if p.suffix in ('.hip', '.h'):
            text = p.read_text()
            for name in GONE:
                assert not re.search(re.escape(name) + r'\b', text), f"{name} is back in {p.name}: use plan_variant_of + be_dispatch_int"


def test_each_block_length_threshold_is_applied_in_one_function(plan_code):
    blocks = _top_level_blocks(plan_code)
    users = {}
    for name in THRESHOLDS:
        assert len(re.findall(r'constexpr int ' + name + r' = \d+;', plan_code)) == 1, name
        inside = set()
        for m in re.finditer(r'\b' + name + r'\b', plan_code):
            if re.match(r'constexpr int ' + name + r' = ', plan_code[m.start() - len('constexpr int '):]):
                continue                                   # the definition
            owner = [h for s, e, h in blocks if s <= m.start() < e]
            assert owner, f"{name} is used outside any function"
            inside.add(owner[0])
        assert len(inside) == 1, f"{name} is applied in {len(inside)} functions: {sorted(inside)}"
        users[name] = inside.pop()
    assert len(set(users.values())) == 1, f"the thresholds are applied in more than one function: {sorted(set(users.values()))}"
    assert 'plan_variant_of' in next(iter(users.values()))


@pytest.mark.parametrize('kernel', KERNELS)
def test_each_kernel_is_defined_once(plan_code, kernel):
    blocks = _top_level_blocks(plan_code)
    defs = [h for _, _, h in blocks if '__global__' in h and re.search(r'\b' + kernel + r'\s*\(', h)]
    assert len(defs) == 1, f"{kernel}: {len(defs)} __global__ definitions"
