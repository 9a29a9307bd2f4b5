"""The restated exponent rules of tests/exponent_cases.py against plain integer / rational arithmetic, and the constants that
module (and the sizes of tests/test_exponent_exact_gpu.py) are made of against the source text.  No GPU needed.

When a constant fails after a retune, move exponent_cases.CONSTS with the source and re-size the GPU cases the message names."""
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import exponent_cases as X
from exponent_cases import C, RANGE

PKG = Path(__file__).resolve().parent.parent / 'brainevent_amd'
FIXED_POINT, PLAN, CSR_PY = PKG / 'csrc' / 'be_fixed_point.hip', PKG / 'csrc' / 'be_csr_plan.hip', PKG / '_csr.py'


def _colstats_text():
    text = PLAN.read_text()
    return text[text.index('template <int MODE> struct StatAcc'):text.index('// plastic plans:')]


def _plan_exponent_text():
    text = PLAN.read_text()
    return text[text.index('int be_scatter_plan_exponent('):text.index('static inline int64_t plan_active_stride')]


def _product(groups):
    v = 1
    for g in ([groups] if isinstance(groups, str) else groups):
        v *= int(g)
    return v


# key -> [(text, pattern, matches expected, value of a match)], the GPU cases sized by it
SOURCES = {
    'entry.block': ([(FIXED_POINT.read_text, r'__launch_bounds__\((\d+)\) k_fp_(?:colsum|colmax|reduce)\(', 3, _product),
                     (FIXED_POINT.read_text, r'dim3\((\d+)\), 0, st', 7, _product)],
                    'test_weight_stats_sizes, test_entry_pass_past_one_trip, test_reduce_past_one_trip'),
    'entry.grid_cap': ([(FIXED_POINT.read_text, r'grid_for\(n(?:nz)?, 256, (\d+) \* (\d+)\)', 2, _product)],
                       'test_weight_stats_sizes, test_entry_pass_past_one_trip (exponent_cases.big_nnz_case)'),
    'reduce.grid_cap': ([(FIXED_POINT.read_text, r'grid_for\(k, 256, (\d+)\)', 2, _product)],
                        'test_reduce_past_one_trip (exponent_cases.big_k_case)'),
    'margin': ([(FIXED_POINT.read_text, r'bits_to_float\(h\[2\]\) \* ([\d.]+) :', 1, float),
                (CSR_PY.read_text, r'bound = colsum_max \* ([\d.]+) if', 1, float)],
               'every boundary case (exponent_cases.crossing_units)'),
    'headroom': ([(FIXED_POINT.read_text, r'int need = (\d+) - eb;', 1, _product), (_plan_exponent_text, r'int need = (\d+) - eb;', 1, _product),
                  (CSR_PY.read_text, r'need = (\d+) - \(math\.frexp\(bound\)', 1, _product)], 'every case'),
    'clamp.lo': ([(FIXED_POINT.read_text, r'need = need < (-\d+) \? -90 : \(need > 150 \? 150 : need\);', 1, _product),
                  (_plan_exponent_text, r'need = need < (-\d+) \? -90 : \(need > 150 \? 150 : need\);', 1, _product),
                  (_plan_exponent_text, r'e0 = e0 < (-\d+) \? -90 : \(e0 > 150 \? 150 : e0\);', 1, _product),
                  (CSR_PY.read_text, r'need = max\((-\d+), min\(150, need\)\)', 1, _product)], 'test_the_lower_clamp (CPU)'),
    'clamp.hi': ([(FIXED_POINT.read_text, r'need = need < -90 \? -90 : \(need > (\d+) \? 150 : need\);', 1, _product),
                  (_plan_exponent_text, r'need = need < -90 \? -90 : \(need > (\d+) \? 150 : need\);', 1, _product),
                  (_plan_exponent_text, r'e0 = e0 < -90 \? -90 : \(e0 > (\d+) \? 150 : e0\);', 1, _product),
                  (CSR_PY.read_text, r'need = max\(-90, min\((\d+), need\)\)', 1, _product)], 'clamp-hi in test_degenerate_and_clamp_*'),
    'min_bits.entry': ([(FIXED_POINT.read_text, r'min_weight_bits >= 0 && min_weight_bits <= (\d+)', 1, _product)],
                       'test_entry_refusals, test_gate_edges_entry'),
    'min_bits.plan': ([(_plan_exponent_text, r'min_weight_bits >= 0 && min_weight_bits <= (\d+)', 1, _product)],
                      'test_plan_refusals, test_gate_edges_plan (GATE_PU_PLAN)'),
    'plan.e0': ([(_plan_exponent_text, r'int e0 = (\d+) - ew - en;', 1, _product)], 'every plan case'),
    'plan.block': ([(_colstats_text, r'__launch_bounds__\((\d+)\) k_plan_colstats\(', 1, _product),
                    (_plan_exponent_text, r'dim3\(n_slices\), dim3\((\d+)\), lds, st', 1, _product)],
                   'the boundary structure (M = 1025: row 1024 on the second trip)'),
    'plan.u': ([(_colstats_text, r'constexpr int U = (\d+);', 1, _product)], 'the boundary structure (rows 0 ... 3 share a group of U)'),
    'plan.pass_items': ([(_colstats_text, r'for \(uint32_t g0 = 0; g0 < ngs\[u\]; g0 \+= (\d+)\)', 1, lambda g: 4 * int(g))],
                        'the boundary structure (row 3: PASS_ROW_ENTRIES)'),
    'steps.min_nnz': ([(CSR_PY.read_text, r'STATS_BY_STEPS_MIN_NNZ = (\d+) << (\d+)', 1, lambda g: int(g[0]) << int(g[1]))],
                      'test_binned_by_steps_* (they patch it to 1)'),
}


def test_every_constant_has_a_source():
    assert set(SOURCES) == set(C)


@pytest.mark.parametrize('key', sorted(SOURCES))
def test_constant_matches_the_source(key):
    places, cases = SOURCES[key]
    for text, pattern, n, value in places:
        found = re.findall(pattern, text())
        assert len(found) == n, f"{key}: /{pattern}/ found {len(found)} times, not {n} — the GPU cases sized by it need a look: {cases}"
        assert {value(g) for g in found} == {C[key]}, (f"{key}: the source says {sorted({value(g) for g in found})}, "
                                                       f"tests/exponent_cases.py assumes {C[key]}: re-size {cases}")


def test_what_the_cases_take_for_granted_besides_the_numbers():
    """The wave loop of k_plan_colstats takes 64 rows per wave and trip, an item group is a be_v4u, the entry pass filters zeros out
    of the minimum and non-finite values out of the sums, and the three sources share one candidate rule."""
    ks = _colstats_text()
    assert len(re.findall(r'for \(int64_t r0 = \(int64_t\)wave \* 64; r0 < m; r0 \+= \(int64_t\)nw \* 64\)', ks)) == 1
    assert X.PLAN_ROW_TRIP == C['plan.block'] // 64 * 64 and X.M == X.PLAN_ROW_TRIP + 1
    assert X.PASS_ROW_ENTRIES > C['plan.pass_items']
    fp = FIXED_POINT.read_text()
    assert len(re.findall(r'if \(ab != 0u\) my_min = ab < my_min \? ab : my_min;', fp)) == 1
    assert len(re.findall(r'ab != 0u && ab < 0x7f800000u\) atomicAdd\(&colsum\[indices\[j\]\], a\);', fp)) == 1
    rule = r'for \(int c = \(keep_exp != INT_MIN && keep_exp <= need\) \? 0 : 1; c < 2; \+\+c\)'
    assert len(re.findall(rule, fp)) == 1 and len(re.findall(rule, _plan_exponent_text())) == 1
    assert len(re.findall(r'for e in \(\[keep\] if keep is not None and keep <= need else \[\]\) \+ \[need\]:', CSR_PY.read_text())) == 1
    # the statistics steps ask for their f32 sums back unrounded (f16 / bf16 weights): BE_BINNED_ABS | BE_BINNED_OUT_F32
    header = (PKG.parent / 'include' / 'brainevent_amd.h').read_text()
    assert len(re.findall(r'#define BE_BINNED_ABS 4 ', header)) == 1 and len(re.findall(r'#define BE_BINNED_OUT_F32 16 ', header)) == 1
    assert len(re.findall(r'\(\(4 \| 16, flat, wcode, colsum\), \(1, one, A\.BE_F32, count\)\)', CSR_PY.read_text())) == 1
    assert len(re.findall(r'const bool out_f32 = wdtype == BE_F32 \|\| \(homo & 16\) != 0;', (PKG / 'csrc' / 'be_csr_binned.hip').read_text())) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# the rules against rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def _eb_of(x: Fraction):
    """Smallest E with x < 2^E, by comparison (no frexp)."""
    assert x > 0
    e = 0
    while x >= Fraction(2) ** e:
        e += 1
    while x < Fraction(2) ** (e - 1):
        e -= 1
    return e


def _entry_by_fractions(n_units, j):
    """need of the entry pass: the f64 product ``fl(N q * fl(1.001))`` taken as a correctly rounded Fraction."""
    prod = float(Fraction(n_units) * Fraction(2) ** j * Fraction(C['margin']))      # float(Fraction) rounds to nearest even
    return X.clamp(C['headroom'] - _eb_of(Fraction(prod)))


SWEEP = [(pu, j, n) for pu in (3, 10, 12, 16, 23) for j in (-20, -6, 0, 12)
         for n in sorted({(1 << pu) + d for d in (-2, -1, 0, 1)} | set(X.crossing_units(pu, j)) | {X.crossing_units(pu, j)[0] - 1})]


def _one_column(n_units):
    """Entries of at most 64 units on column 0 summing to n_units."""
    full, rem = divmod(n_units, X.MAX_UNITS)
    return np.concatenate([np.full(full, X.MAX_UNITS, np.int64), [rem] if rem else []]).astype(np.int64)


def test_entry_rule_over_the_sweep():
    for pu, j, n in SWEEP:
        q = math.ldexp(1.0, j)
        e = X.entry_rule(n * q, 64 * q, q, q, 1 << 20, True, 16, None)
        assert e == _entry_by_fractions(n, j), (pu, j, n)
        assert Fraction(n) * Fraction(2) ** (j + e) < (1 << 62)                       # the invariant ...
        assert Fraction(n) * Fraction(2) ** (j + e + 1) * Fraction(C['margin']) >= (1 << 62) - 1      # ... and no exponent wasted
    lo, hi = X.crossing_units(16, -6)
    assert (lo, hi) == (65470, 65471)
    assert X.entry_rule(lo / 64, 1.0, 1 / 64, 1 / 64, 10, True, 16, None) == X.entry_rule(hi / 64, 1.0, 1 / 64, 1 / 64, 10, True, 16, None) + 1


def _plan_by_python_ints(units, j, cols, k, nnz):
    """plan_bound in Python integers and Fractions, entry by entry."""
    w = [Fraction(abs(int(u))) * Fraction(2) ** j for u in units]
    wmax = max(w)
    ew, en = _eb_of(wmax) if wmax > 0 else 0, _eb_of(Fraction(nnz))
    e0 = X.clamp(C['plan.e0'] - ew - en)
    sums = [0] * k
    for x, c in zip(w, cols):
        if x > 0:
            sums[c] += int(x * Fraction(2) ** e0) + 1
    smax = max(sums)
    return math.ldexp(float(smax) + 1.0, -e0), e0, smax


def test_plan_rule_over_the_sweep_and_the_cross_relation():
    """`plan_bound` (vectorised int64) equals the same sums in Python integers; the bound is a true upper bound; and away from the
    clamps ``entry <= plan <= entry + 1``, with ``plan == entry + 1`` exactly in the 1.001 band."""
    seen_band = 0
    for pu, j, n in SWEEP:
        if pu > 16 or n < 1:
            continue
        units = _one_column(n)
        cols = np.zeros(units.size, np.int32)
        a32 = np.ldexp(units.astype(np.float64), j).astype(np.float32)
        got = X.plan_bound(a32, cols, 3, units.size)
        assert got == _plan_by_python_ints(units, j, cols, 3, units.size), (pu, j, n)
        assert Fraction(got[0]) >= Fraction(n) * Fraction(2) ** j      # (equal where the f64 of smax rounds the + 1 away: frexp's bound is strict)
        plan = X.plan_rule(a32, cols, 3, units.size, 16, None)
        entry = X.entry_rule(float(np.float32(n * math.ldexp(1.0, j))), float(a32.max()), float(a32.min()), float(a32.max()),
                             units.size, True, 16, None)
        assert entry <= plan <= entry + 1, (pu, j, n, entry, plan)
        in_band = Fraction(n) * Fraction(2) ** j < Fraction(2) ** (C['headroom'] - entry - 1)       # S itself fits one exponent more
        assert (plan == entry + 1) == in_band, (pu, j, n, entry, plan)
        seen_band += in_band
        assert Fraction(n) * Fraction(2) ** (j + plan) < (1 << 62)
    assert seen_band >= 10
    # the split of an f64 weight: twice the entries, every lo zero for an exact case — the same exponent
    c = X.build('edge-below-mixed-j-6')
    assert c.plan(split=True) == c.plan()


def test_fixed_floor_is_a_floor():
    rng = np.random.default_rng(0)
    a = np.abs(rng.normal(0, 1, 200)).astype(np.float32)
    for e0 in (-3, 0, 5, 20, 30):
        assert [int(v) for v in X.fixed_floor(a, e0)] == [math.floor(Fraction(float(x)) * Fraction(2) ** e0) for x in a]


def test_keep_and_gate_edges_of_the_rule():
    q, need = 1.0, 62 - 13                                                           # 4095 * 1.001 < 2^13
    args = (4095.0, 64.0, 2.0, 2.0, 100, True)
    assert X.entry_rule(*args, 16, None) == need == X.entry_rule(*args, 16, X.INT_MIN)
    assert X.entry_rule(*args, 16, need) == need and X.entry_rule(*args, 16, need - 1) == need - 1
    assert X.entry_rule(*args, 16, need + 1) == need                                  # would overflow: not kept
    assert X.entry_rule(*args, 16, need - 40) == need                                 # kept only if fine enough: 2^(16 - 9) > 2
    mb = need + 1                                                                     # threshold 2^(mb - need) = 2 = wmin: `>=` passes
    assert X.entry_rule(*args, mb, None) == need and X.entry_rule(*args, mb + 1, None) == RANGE
    assert X.entry_rule(4095.0, 64.0, 1.0, 2.0, 100, True, mb, None) == need          # wmin below: the column maxima pass
    assert X.entry_rule(4095.0, 64.0, 1.0, 2.0, 100, False, mb, None) == RANGE        # ... which a call without indices has not
    assert X.entry_rule(4095.0, 64.0, 1.0, 1.0, 100, True, mb, need - 3) == RANGE     # both candidates
    assert X.entry_rule(0.0, 0.0, None, float('inf'), 5, True, 60, None) == 62 == X.entry_rule(0.0, 0.0, None, float('inf'), 0, False, 0, 70)
    assert X.entry_rule(0.0, 0.0, None, float('inf'), 0, True, 0, 13) == 13
    assert X.entry_rule(1.0, float('inf'), 1.0, 1.0, 5, True, 16, None) == RANGE == X.entry_rule(1.0, float('nan'), 1.0, 1.0, 5, True, 16, None)


def test_the_lower_clamp_and_the_overflowing_sum():
    """-90 is reached by the rules only (module docstring of exponent_cases); a column sum that f32 cannot hold takes the bound
    without structure — never frexp's 0 for inf, which would give 62."""
    big = math.ldexp(1.0, 127)
    assert X.entry_rule(0.0, big, big, big, 1 << 25, False, 0, None) == C['clamp.lo']
    assert X.entry_rule(0.0, big, big, big, (1 << 24) - 2, False, 0, None) == C['clamp.lo'] + 1
    c = X.overflow_case()
    s = c.stats()
    assert s['colsum_max'] == float('inf') and X.frexp_exp(float('inf') * C['margin']) == 0
    assert c.entry() == c.plan() == c.steps()[0] == -67 == c.entry(has_indices=False)
    assert X.true_bound_holds(c, -67) and not X.true_bound_holds(c, -66) and not X.true_bound_holds(c, 62)
    assert X.clamp_case().entry() == X.clamp_case().plan() == C['clamp.hi']


def test_steps_rule_gate_variants():
    """The mean decides where it can, the entry pass where it cannot (exponent_cases.gate_case)."""
    want = {'wmin-at': (50, False), 'wmin-below': (50, True), 'colmax-below': (RANGE, True), 'mean-pass': (50, False), 'mean-fail': (50, True)}
    for v in X.GATE_VARIANTS:
        c, mb = X.gate_case(v, X.GATE_PU_ENTRY), X.gate_min_bits(X.GATE_PU_ENTRY)
        assert c.steps(min_bits=mb) == want[v], v
        assert c.entry(min_bits=mb) == want[v][0] and c.entry(min_bits=mb - 1) == 50 and c.entry(min_bits=mb, keep=30) == want[v][0]
        p = X.gate_case(v, X.GATE_PU_PLAN)
        mbp = X.gate_min_bits(X.GATE_PU_PLAN)
        assert mbp == C['min_bits.plan'] and p.plan(min_bits=mbp) == (RANGE if v == 'colmax-below' else 39) == p.entry(min_bits=mbp)


def _all_cases():
    out = [X.build(n) for n in X.CASES] + X.degenerate_cases() + [X.clamp_case(), X.subnormal_case(), X.overflow_case()]
    out += [X.gate_case(v, pu) for v in X.GATE_VARIANTS for pu in (X.GATE_PU_ENTRY, X.GATE_PU_PLAN)]
    out += [X.big_nnz_case(), X.big_k_case('sum'), X.big_k_case('max')]
    out += [X.fixed_rows_case(w, s, -6) for w in X.WHERE for s in ('pos', 'mixed')]
    return out


def test_every_case_is_exact_and_every_rule_holds_the_invariant():
    names = set()
    for c in _all_cases():
        assert c.name not in names
        names.add(c.name)
        c.check_exact()
        assert not c.units.flags.writeable and not c.indices.flags.writeable
        s = c.stats()
        col = np.zeros(c.k)
        np.add.at(col, c.indices, np.abs(c.weights))
        if math.isfinite(s['colsum_max']):
            assert s['colsum_max'] == col.max(initial=0.0)                 # the f32 sum IS the sum
        got = {'entry': c.entry(), 'flat': c.entry(has_indices=False), 'plan': c.plan(), 'steps': c.steps()[0]}
        for src, e in got.items():
            assert e == RANGE or X.true_bound_holds(c, e), (c.name, src, e)
        if RANGE not in (got['entry'], got['plan']) and C['clamp.lo'] < got['entry'] < C['clamp.hi']:
            assert got['entry'] <= got['plan'] <= got['entry'] + 1, (c.name, got)
        assert got['steps'] == got['entry']
    for where, band in (('pow2', False), ('below', True), ('cross-lo', False), ('cross-hi', True)):
        for n in X.boundary_cases(where=where):
            c = X.build(n)
            assert (c.plan() == c.entry() + 1) == band, n
    w = X.wide_f64_case()
    assert not w.exact and w.dtypes() == ['f64'] and X.true_bound_holds(w, w.entry()) and X.true_bound_holds(w, w.plan(split=True))


def test_check_exact_refuses_a_case_that_breaks_its_own_condition():
    ok = X.small_case('ok', 2, 4, [64, -64, 1], 0, [[0, 1], [3]])
    assert ok.check_exact() == 64
    with pytest.raises(AssertionError):
        X.small_case('units', 2, 4, [65, 1, 1], 0, [[0, 1], [3]])                   # bf16 does not hold 65
    with pytest.raises(AssertionError):
        X.small_case('index', 2, 4, [1, 1, 1], 0, [[0, 1], [4]])                    # a column outside [0, k)
    with pytest.raises(AssertionError):
        X.small_case('negative-index', 2, 4, [1, 1, 1], 0, [[0, -1], [3]])
    n = X.EXACT_SUM // X.MAX_UNITS
    X.small_case('just-below', 1, 2, [64] * (n - 1) + [63], 0, [[1] * n])
    with pytest.raises(AssertionError):
        X.small_case('sum', 1, 2, [64] * n, 0, [[1] * n])                           # 2^24 units in one column
    with pytest.raises(AssertionError):
        X.boundary_case('too-light', 20, 'pos', 0)                                   # fewer units than the ways H is reached
    with pytest.raises(ValueError):
        ok.units[0] = 1                                                              # read-only
