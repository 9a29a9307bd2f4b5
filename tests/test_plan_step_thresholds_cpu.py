"""What tests/test_plan_step_exact_gpu.py sizes its cases by (the CONSTS table of tests/plan_step_cases.py and the host's choice restated
from it) is what csrc/be_csr_plan.hip says, and the case tables that module iterates cover every kernel instance the host can launch.
No GPU needed: the source is read as text, and be_binary_csrmm_t_plan_workspace_bytes / _for are host functions.  When a constant
test fails after a retune, move the table with the source and re-size the GPU cases the failure message lists."""
import re
from pathlib import Path

import numpy as np
import pytest

import plan_layout_cases as L
import plan_step_cases as P
from plan_step_cases import CONSTS

SOURCE = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc' / 'be_csr_plan.hip'
TEXT = SOURCE.read_text()

DEC = 'test_decoders (the hints at both ends of every class)'
TABLE = 'test_decoders (FUSED 3), pipeline-*-table, gather-*, compact-*'
LIST = 'list-* (test_skeleton)'


def _prod(*g):
    v = 1
    for x in g:
        v *= int(x)
    return v


def _at(i):
    return lambda *g: int(g[i])


def _same(*g):
    return int(g[0]) if len(set(g)) == 1 else -1


RGRID = r'const int rgrid = grid_for\(k, (\d+), n_batch >= (\d+) \? (\d+) : (\d+)\);'

# table key -> (regular expression, its groups -> the value, how often the source holds it, the GPU cases sized by it)
PATTERNS = {
    'u16c.lpb4': (r'constexpr int kSub4MaxBlock = (\d+);', _prod, 1, DEC),
    'u16c.lpb8': (r'constexpr int kSub8MaxBlock = (\d+);', _prod, 1, DEC),
    'u16c.lpb16': (r'constexpr int kSub16MaxBlock = (\d+);', _prod, 1, DEC),
    'u16c.lpb32': (r'constexpr int kSub32MaxBlock = (\d+);', _prod, 1, DEC),
    'u16w.lpb4': (r'constexpr int kSubW4MaxBlock = (\d+);', _prod, 1, DEC),
    'u16w.lpb8': (r'constexpr int kSubW8MaxBlock = (\d+);', _prod, 1, DEC),
    'u16w.lpb16': (r'constexpr int kSubW16MaxBlock = (\d+);', _prod, 1, DEC),
    'u16w.lpb32': (r'constexpr int kSubW32MaxBlock = (\d+);', _prod, 1, DEC),
    'd8.lpb8': (r'constexpr int kD8EighthMaxBlock = (\d+);', _prod, 1, DEC),
    'd8.lpb16': (r'constexpr int kD8QuarterMaxBlock = (\d+);', _prod, 1, DEC),
    'd8.nt_min': (r'constexpr int kD8NtMinBlock = (\d+);', _prod, 1, DEC),
    'd8.block_aux': (r'#define BE_BLOCK_AUX (\d+) ', _prod, 1, DEC),
    'pregather.max_block': (r'constexpr int kPreGatherMaxBlock = (\d+);', _prod, 1, TABLE),
    'pregather.min_slices': (r'constexpr int kPreGatherMinSlices = (\d+);', _prod, 1, f'{TABLE}: the 40 slices of the decoder matrices'),
    'pregather.max_bytes': (r'bytes <= \((\d+)ll << (\d+)\)\) \? be_align_up\(bytes, 256\) : 0;', lambda a, b: int(a) << int(b), 1, TABLE),
    'fused.min_list': (r'constexpr size_t kFusedMinList = (\d+);', _prod, 1, f'{LIST}; reduce-* (d8 at 19999 columns does not fuse)'),
    'single.chunk': (r'constexpr int kSingleChunk = (\d+);', _prod, 1, 'test_single_launch (SINGLE_M)'),
    'single.lds_extra': (r'lds \+ kSingleChunk \* 4 \+ (\d+) <= 160 \* 1024\) \{', _prod, 1, 'test_single_launch'),
    'list.stripe': (r'return \(\(n_stripes \+ parts - 1\) / parts\) \* (\d+);', _prod, 1, f'{LIST}; pipeline-*'),
    'list.words': (r'for \(int64_t u0 = 0; u0 < my_words; u0 \+= (\d+)\) \{', _prod, 1, LIST),
    'rows.batch': (r'a_step = FUSED \? \(uint64_t\)nw \* (\d+) : \(uint64_t\)parts \* nw \* (\d+);', _same, 1, 'pipeline-*'),
    'rows.waves': (r'hipLaunchKernelGGL\(kern, grid, dim3\((\d+)\), lds, st, args\.\.\.\);', lambda g: int(g) // 64, 1, 'pipeline-*'),
    'lds.cap_ids': (r'std::min<size_t>\(lds_room / 4, (\d+)\) : 0u;', _prod, 1, LIST),
    'lds.bytes': (r'const size_t lds_room = (160) \* (1024) - \d+ - lds;', _prod, 1, f'{LIST}; test_single_launch'),
    'lds.reserve': (r'const size_t lds_room = 160 \* 1024 - (\d+) - lds;', _prod, 1, LIST),
    'gather.grid': (r'hipLaunchKernelGGL\(k_gather_seg, dim3\((\d+)\), dim3\(256\), 0, st,', _prod, 1, 'gather-65-slices-grid-stride'),
    'gather.tile': (r'__shared__ uint2 tile\[(\d+)\]\[65\];', _prod, 2, 'gather-*'),
    'compact.rows': (r'__shared__ uint32_t ids_s\[(\d+)\];', _prod, 1, 'compact-*'),
    'reduce.threads': (RGRID, _at(0), 1, 'reduce-*'),
    'reduce.batch_from': (RGRID, _at(1), 1, 'reduce-batch8-*'),
    'reduce.grid_batch': (RGRID, _at(2), 1, 'reduce-batch8-*'),
    'reduce.grid': (RGRID, _at(3), 1, 'reduce-vector-*'),
    'sum.unroll': (r'for \(; q \+ (\d+) <= parts; q \+= (\d+)\) s \+= sum_n<A, (\d+)>\(', _same, 1, 'parts-*'),
    'd8.max_width': (r'constexpr int kD8MaxWidth = (\d+);', _prod, 1, 'reduce-*-d8-*, list-d8-*'),
    'h8.max_width': (r'constexpr int kH8MaxWidth = (\d+);', _prod, 1, 'reduce-*-h8-*, list-h8-*'),
    'active.extra': (r'return active_stride_of\(m \+ (\d+) \* (\d+) \+ (\d+)\);', lambda a, b, c: int(a) * int(b) + int(c), 1,
                     'every case (the workspace size)'),
}


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, value, count, cases = PATTERNS[key]
    found = re.findall(pattern, TEXT)
    assert len(found) == count, f"{key}: be_csr_plan.hip holds /{pattern}/ {len(found)} times — the GPU cases sized by it need a look: {cases}"
    values = {value(*([g] if isinstance(g, str) else g)) for g in found}
    assert values == {CONSTS[key]}, f"{key}: be_csr_plan.hip says {sorted(values)}, tests/plan_step_cases.py assumes {CONSTS[key]}: re-size {cases}"


def test_shapes_around_the_constants():
    """What the restated choice takes for granted besides the numbers."""
    one = lambda pat: len(re.findall(pat, TEXT)) == 1       # noqa: E731
    assert one(r'if \(!fused_off && lds \+ 1024 <= 160 \* 1024 && lds_room >= kFusedMinList \* 4\) \{')
    assert one(r'u0 = -1024;') and CONSTS['list.words'] == 1024
    assert one(r'const unsigned cg_grid = \(unsigned\)\(\(\(m \+ 15\) / 16 \+ 255\) / 256\);') and CONSTS['compact.rows'] == 16 * 256
    assert one(r'const PlanVariant var = plan_variant_of\(layout, homo, block_hint\);')
    assert one(r'be_dispatch_int<0, 4, 8, 16, 32>\(var\.lpb,') and len(re.findall(r'be_dispatch_int<0, 8, 16>\(var\.lpb,', TEXT)) == 2
    assert one(r'if \(!q8 && n_slices == 1 && parts == 1 && n_batch == 1 && wdtype != BE_F64 &&')
    assert one(r'else if \(spike_dtype == BE_SPIKE_BOOL && \(reinterpret_cast<uintptr_t>\(spikes\) & 15\) == 0 && \(n_batch == 1 \|\| m % 16 == 0\)\) fused = 2;')
    assert one(r'const dim3 grid\(\(unsigned\)\(\(n_tasks \+ 7\) / 8 \* 8\), \(unsigned\)n_batch\);')
    assert one(r'for \(uint32_t c = blockIdx\.x; \(uint64_t\)c \* 64 < n_active; c \+= gridDim\.x\) \{')
    assert one(r'for \(int s0 = 0; s0 < n_slices; s0 \+= 64\) \{')
    # the four instances the ledger lists as compiled but never launched are exactly what the sweep of instance_of leaves out
    assert P.ALL_INSTANCES - P.REACHABLE == {('acc', 'u16c', 32, 3, 0), ('acc', 'u16c', 0, 3, 0), ('acc', 'u16w', 0, 3, 0),
                                            ('acc', 'd8', 0, 3, CONSTS['d8.block_aux'])}
    assert len(P.ALL_INSTANCES) == 60 + 4 + 8 + 24 and P.REACHABLE <= P.ALL_INSTANCES


# ------------------------------------------------------------------------------------------------- the library's host functions
@pytest.fixture(scope='module')
def lib():
    from brainevent_amd import _lib
    return _lib


def test_workspace_bytes_match_the_library(lib):
    base, sized = lib.fn('be_binary_csrmm_t_plan_workspace_bytes'), lib.fn('be_binary_csrmm_t_plan_workspace_bytes_for')
    keys = {c.ws_args() for c in P.all_cases()}
    keys |= {(m, k, nb, shift, width, parts, homo) for m in (1, 300, 4097, 70001) for k in (50, 2400, 65539, 524291) for nb in (1, 3, 8)
             for shift, width in ((6, 60), (6, 0), (4, 19999), (14, 0), (15, 39999)) for parts in (1, 3, 64) for homo in (0, 1)}
    for key in sorted(keys):
        assert base(*key) == P.workspace_bytes(*key), key
        for hint in (0, 1, 64, 65, 100000):
            assert sized(*key, hint) == P.workspace_bytes_for(*key, hint), (key, hint)
    for c in P.all_cases():
        # what the accumulate kernels write fits what the library asks for (the step checks the same on entry)
        mx = c.matrix
        assert P.counts_bytes(c.n_batch) + c.n_batch * P.plan_active_stride(mx.m) * 4 + \
            P.partial_bytes(mx.k, c.n_batch, mx.slice_shift, mx.slice_width, c.parts, c.layout, c.homo) <= P.workspace_bytes(*c.ws_args())


# ------------------------------------------------------------------------------------------------------ the generator's claims
ALL = P.all_cases()


@pytest.mark.parametrize('case', ALL, ids=[c.id for c in ALL])
def test_case_is_exact(case):
    """check_exact at the pinned exponent and at exponents from the bound the case states; the f64 reference equals the sums taken in
    integers, so it is THE value whatever the order of the additions, and survives the cast to the output dtype unless that dtype
    rounds it (once)."""
    case.check_exact()
    for e in (case.min_exp(), case.min_exp() + 1, 36):
        if e >= case.min_exp():
            case.check_exact(e)
    mx = case.matrix
    assert mx.indices.flags.writeable is False and case.active(0).flags.writeable is False
    if not case.homo and mx.frac is None:
        rows = mx.rows_of_entries
        act = case.active(0)
        ref, _ = case.sums(act)
        for b in range(min(case.n_batch, 2)):
            sel = act[b][rows]
            exact = np.zeros(mx.k, np.int64)
            np.add.at(exact, mx.indices[sel], mx.units[sel])
            assert np.array_equal(exact / 64.0, ref[b]) and np.abs(exact).max(initial=0) < 2 ** 24
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    if not case.homo:
        with pytest.raises(AssertionError):
            case.check_exact(case.min_exp() - 1)


def test_coverage():
    """The union of `instance_of` over the GPU module's parametrisation is REACHABLE: every accumulate instance, table form, reduce and
    single-launch instance the host can launch at default settings is run by some case — and a case dropped there fails here."""
    cov = P.covered()
    assert cov == P.REACHABLE, (sorted(P.REACHABLE - cov, key=str), sorted(cov - P.REACHABLE, key=str))
    for c in ALL:
        inst = c.instance()
        assert set(c.want) <= P.parts_of_instance(inst), (c.id, c.want, inst)
    # every reachable accumulate instance is some decoder case's declared purpose, at a hint on each side of its class
    dec = P.tables()['decoder']
    assert {w for c in dec for w in c.want} == {i for i in P.REACHABLE if i[0] == 'acc'}
    for kind in P.KINDS:
        for (lpb, aux), (lo, hi) in P.hint_classes(kind).items():
            hints = {c.hint for c in dec if c.kind == kind and c.want[0][2] == lpb and c.want[0][4] == aux}
            assert lo in hints and (hi if hi is not None else 100000) in hints, (kind, lpb, aux, sorted(hints))
    # the table forms, each with every FUSED 3 decoder
    for acc in {i for i in P.REACHABLE if i[0] == 'acc' and i[3] == 3}:
        assert {c.instance()[1] for c in dec if c.want == (acc,)} == {'list', 'compact1', 'compact2'}, acc


@pytest.mark.parametrize('kind', P.KINDS)
def test_long_blocks_are_long(kind):
    """The decoder matrices hold, in rows every pattern keeps active, blocks of more lane-groups than every LPB and than 64."""
    mx = P._decoder_matrix(kind)
    enc = mx.encoded(kind)
    groups = (enc.groups & 0xffff if kind in L.SORTED else enc.groups).reshape(mx.m, mx.n_slices)
    active = P.pattern(mx, 'half')[0]
    longest = int(groups[active].max())
    assert longest > 64 and longest > max(lpb for lpb, _ in P.hint_classes(kind))
    assert (np.diff(mx.indptr)[::17] == 0).all() and mx.n_slices == CONSTS['pregather.min_slices']
    # duplicate columns inside a block
    rows = mx.rows_of_entries
    key = rows.astype(np.int64) * mx.k + mx.indices
    assert np.unique(key).size < key.size
    if kind.startswith('u16'):
        assert mx.slice_width < 1 << mx.slice_shift and (enc.count < enc.groups * L.GROUP[kind]).any(), 'no pad at slot 2^shift'


@pytest.mark.parametrize('kind', ('d8', 'h8'))
def test_crafted_blocks_are_what_they_are_named_for(kind):
    mx = P.sorted_matrix()
    enc = mx.encoded(kind)
    G = L.GROUP[kind]
    seen = 0
    for (kd, g, eg, ne), (r, s) in mx.note['crafted'].items():
        if kd != kind:
            continue
        seen += 1
        b = r * mx.n_slices + s
        assert int(enc.seg[r, s, 1]) & 0xffff == g and int(enc.seg[r, s, 1]) >> 16 == 5, (kd, g, eg, ne)
        blk = np.frombuffer(enc.block(r, s), np.uint8)
        codes = blk[:G * g] if kind == 'h8' else blk[16 * g:16 * g + 4 * g]
        esc = np.flatnonzero(codes == 255)
        if ne:
            first = eg * G + G - 1
            assert esc[:ne].tolist() == list(range(first, first + ne)), 'the escape run is not where the case says'
            assert first // G != (first + ne - 1) // G or ne == 1           # a run of two or more straddles the lane-group boundary
            if kind == 'd8':
                assert not np.frombuffer(enc.block(r, s), np.uint32)[:4 * g][esc[:ne]].any()           # escapes weigh nothing
        if g % 2 and kind == 'h8':
            assert codes[-3:].tolist() == [255] * 3 and enc.count[b] + ne == G * g - 3                # tail pads
        assert P.pattern(mx, 'half')[0][r]
    assert seen == len(P.CRAFTED_GROUPS) + len(P.CRAFTED_ESCAPES)
    assert set(P.CRAFTED_GROUPS) >= {n for lpb, _ in P.hint_classes(kind) if lpb for n in (lpb, lpb + 1)} | {64, 65}
    assert {(eg, ne) for _, eg, ne in P.CRAFTED_ESCAPES} >= {(7, 2), (15, 2), (63, 2)}


def test_blob_of_puts_the_blocks_at_their_starts():
    mx = P.sorted_matrix()
    for kind in ('d8', 'h8'):
        enc = mx.encoded(kind)
        blob = P.blob_of(enc)
        assert np.array_equal(L.defined_bytes(kind, enc.seg, blob), enc.data) and blob.size == enc.units * 128 + 128
        assert (blob[-128:] == 0xA5).all()
    enc = P.u16_matrix().encoded('u16w')
    assert np.array_equal(L.defined_bytes('u16w', enc.seg, P.blob_of(enc)), enc.data)


TRIPPED = [c for c in ALL if c.trips]


@pytest.mark.parametrize('case', TRIPPED, ids=[c.id for c in TRIPPED])
def test_loop_cases_reach_their_trip_count(case):
    for name, got, need in case.trips:
        assert got >= need >= 2, f'{case.id}: {name}: {got} trips, the case is for {need}'


def test_every_part_of_the_parts_cases_holds_something():
    """The parts-* cases run FUSED 0, where list position p belongs to part p % parts: every part's rows add to some column, in every
    step that has spikes — so a term that sum_parts drops changes the result."""
    seen = set()
    for c in ALL:
        if not c.id.startswith('parts-'):
            continue
        seen.add(c.parts)
        assert c.instance()[2][3] == 0 and c.matrix.n_slices == 2
        lens = np.diff(c.matrix.indptr)
        for step in (0, 1):
            rows = np.flatnonzero(c.active(step)[0])                          # the compacted list ascends
            for p in range(c.parts):
                sub = np.zeros((1, c.matrix.m), bool)
                sub[0, rows[p::c.parts]] = True
                assert lens[rows[p::c.parts]].sum() > 0 and c.sums(sub)[0].any(), (c.id, step, p)
    assert seen == {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 64}


def test_list_cases_restart_where_they_say():
    """The LDS list of the list-* cases holds a few thousand ids; the three patterns fit it, outgrow it in the first iteration of
    build_part_list, and outgrow it in the second after a first that fit (the restart with base > 0)."""
    for c in ALL:
        if not c.id.startswith('list-'):
            continue
        mx = c.matrix
        cap = P.lds_cap_of(mx.slice_shift, mx.slice_width, c.layout, c.homo)
        assert CONSTS['fused.min_list'] <= cap < 3072 and c.instance()[2][3] in (1, 2)
        act = c.active(0)[0]
        stripe = np.arange(mx.m) // CONSTS['list.stripe']
        mine = act & (stripe % c.parts == 0)                                   # part 0
        first = int(mine[:32 * CONSTS['list.stripe'] * c.parts].sum())
        total = int(mine.sum())
        assert mx.m % 32 and mx.m % 16 and total > first
        kind = {'40:40': 'fits', '4:4': 'first', '16:1': 'second'}[c.pat.split(':', 1)[1]]
        assert {'fits': total <= cap, 'first': first > cap, 'second': first <= cap < total}[kind], (c.id, first, total, cap)


def test_single_cases_cover_both_sides_of_the_chunk():
    ch = CONSTS['single.chunk']
    assert P.SINGLE_M == (1, ch - 1, ch, ch + 1, 2 * ch + 1)
    for c in P.tables()['single']:
        for m in P.SINGLE_M:
            sub = P.Case(c.id, P.head_of(c.matrix, m), c.kind, c.spikes, c.pat, 1, 1, c.hint, c.wdtype)
            assert sub.instance() == c.want[0]
    # k_plan_single refuses f64 by design: the same shape with an f64 output takes the sliced path
    f = [c for c in P.tables()['f64'] if 'one-slice' in c.id][0]
    assert f.matrix.n_slices == 1 and f.parts == 1 and f.n_batch == 1 and f.instance()[0] == 'sliced'
    assert P.Case('x', f.matrix, f.kind, f.spikes, f.pat, 1, 1, f.hint, 'f32').instance()[0] == 'single'
