"""The three sources of the fixed-point exponent — be_fixed_point_exponent / be_weight_stats (csrc/be_fixed_point.hip),
be_scatter_plan_exponent (k_plan_colstats in csrc/be_csr_plan.hip) and BinnedScatter._exponent_by_steps — compared EXACTLY with the
rules restated in tests/exponent_cases.py, on cases whose every partial sum is exact (that module's docstring), at the smallest
sizes that reach each path.  Every comparison is an equality, and `true_bound_holds` — the largest column sum of |w| times 2^e stays
below 2^62, in integers — is asserted for every exponent any source returns.

What reaches what (tests/test_exponent_rule_cpu.py holds the sizes to the source):
  * test_weight_stats_*            k_fp_colsum without indices: 0 ... 257 elements, one element past the capped grid's first trip
                                   (the maximum there, then the minimum), bit patterns of zeros, subnormals, inf, nan, f64 outside f32
  * test_entry_boundaries          the heaviest column sum at 2^p, 2^p - q and both sides of the 1.001 crossing; signs; four dtypes;
                                   with and without indices
  * test_entry_pass_past_one_trip  nnz = 256 * 16 * 256 + 257, the heavy column on both trips
  * test_reduce_past_one_trip      k = 1024 * 256 + 1: the largest sum, then the smallest column maximum, in column k - 1
  * test_entry_keep_edges, test_entry_gate_edges, test_entry_degenerate_and_clamp, test_entry_refusals, test_entry_wide_f64
  * test_overflowing_column_sum_*  four weights of 2^126 in one column: never 62
  * test_plan_*                    u16 and d8 on the boundary structure (two slices, m = 1025, a block of more than 256 items, an
                                   escape chain, duplicates), the f64 split, the colmax mode, keep through a refresh, refusals
  * test_binned_by_steps*          fixed-length and indptr rows, 64- and 32-bit sums, f16 / bf16 weights (the steps' sums come back
                                   as f32: BE_BINNED_OUT_F32), the fall-back to the entry pass
  * test_binned_step_returns_f32_sums_on_request    the flag behind that, by direct call
  * test_three_sources_on_one_case, test_end_to_end_at_the_boundary"""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import exponent_cases as X
from exponent_cases import BE_ERR_INVALID, BE_ERR_RANGE, BE_ERR_WORKSPACE, BE_OK, C, INT_MIN, RANGE

pytestmark = pytest.mark.gpu

TORCH_DT = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
MB = 16                                  # ScatterPlan.MIN_WEIGHT_BITS
_DEV = {}


def bits(x):
    return int(np.asarray([x], np.float32).view(np.uint32)[0])


def on_device(case, wdt='f32'):
    """(weights in `wdt`, indices, indptr) of a case on the device, uploaded once; the weights are exact in `wdt`."""
    key = (case.name, wdt)
    if key not in _DEV:
        w = torch.tensor(case.weights).to(TORCH_DT[wdt])
        assert np.array_equal(w.double().numpy(), case.weights), key
        _DEV[key] = (w.cuda(), torch.tensor(case.indices).cuda(), torch.tensor(np.ascontiguousarray(case.ptr)).cuda())
    return _DEV[key]


def lib():
    from brainevent_amd import _array as A, _lib
    return A, _lib


def weight_stats(w, n=None, scratch_bytes=256, wcode=None, null=()):
    """be_weight_stats by direct call -> (rc, max bits, min bits)."""
    A, L = lib()
    mx, mn = ctypes.c_uint32(0xdead), ctypes.c_uint32(0xbeef)
    scr = torch.empty(256, dtype=torch.uint8, device='cuda')
    rc = L.fn('be_weight_stats')(None if 'weights' in null else A.ptr(w), A.wcode(w) if wcode is None else wcode,
                                 w.numel() if n is None else n, None if 'max' in null else ctypes.byref(mx),
                                 None if 'min' in null else ctypes.byref(mn), None if 'scratch' in null else A.ptr(scr), scratch_bytes,
                                 A.stream_ptr())
    return rc, mx.value, mn.value


def entry_call(w, idx, k, min_bits=MB, keep=None, nnz=None, short=0, wcode=None, null=(), scratch=None):
    """be_fixed_point_exponent by direct call -> the exponent, RANGE, or the (negative) status of another refusal."""
    A, L = lib()
    need = int(L.fn('be_fixed_point_scratch_bytes')(int(k)))
    assert need == 256 + (max(int(k), 1) * 4 + 255) // 256 * 256
    scr = torch.empty(need, dtype=torch.uint8, device='cuda') if scratch is None else scratch
    out = ctypes.c_int(-12345)
    rc = L.fn('be_fixed_point_exponent')(None if 'weights' in null else A.ptr(w), A.wcode(w) if wcode is None else wcode, A.ptr(idx),
                                         w.numel() if nnz is None else nnz, int(k), int(min_bits), INT_MIN if keep is None else int(keep),
                                         None if 'scratch' in null else A.ptr(scr), need - short,
                                         None if 'out' in null else ctypes.byref(out), A.stream_ptr())
    if rc == BE_OK:
        return int(out.value)
    assert out.value == -12345
    return RANGE if rc == BE_ERR_RANGE else rc


def holds(case, e):
    assert e == RANGE or X.true_bound_holds(case, e), (case.name, e)
    return e


def entry_of(case, wdt, has_indices=True, **kw):
    w, idx, _ = on_device(case, wdt)
    return holds(case, entry_call(w, idx if has_indices else None, case.k, **kw))


# ---------------------------------------------------------------------------------------------------------------------------
# be_weight_stats
# ---------------------------------------------------------------------------------------------------------------------------
def _stats_reference(w64):
    a = np.abs(w64.astype(np.float32))
    nz = a[a > 0]
    return bits(a.max(initial=0.0)), (bits(nz.min()) if nz.size else 0xffffffff)


@pytest.mark.parametrize('wdt', X.DTYPES)
def test_weight_stats_sizes(wdt):
    """0 ... 257 elements; then one element past the first trip of the capped grid, holding the maximum, then the minimum."""
    rng = np.random.default_rng(1)
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        w64 = rng.integers(2, 60, max(n, 1)) * rng.choice([-1.0, 1.0], max(n, 1)) / 8.0
        if n > 2:
            w64[n // 2], w64[n - 1] = 0.0, -0.0
        w = torch.tensor(w64).to(TORCH_DT[wdt]).cuda()
        want = _stats_reference(w64[:n]) if n else (0, 0xffffffff)
        assert weight_stats(w, n=n) == (BE_OK,) + want, (n, wdt)
    n = X.ENTRY_TRIP + 1
    w64 = (rng.integers(8, 33, n) * rng.choice([-1.0, 1.0], n)) / 8.0
    for last, want in ((-60.0 / 8, (bits(7.5), bits(1.0))), (3.0 / 8, (bits(4.0), bits(0.375)))):
        w64[-1] = last
        w = torch.tensor(w64).to(TORCH_DT[wdt]).cuda()
        assert weight_stats(w) == (BE_OK,) + want, (last, wdt)
        assert _stats_reference(w64[:-1]) == (bits(4.0), bits(1.0))          # without the last element: neither figure


def test_weight_stats_bit_patterns():
    f32 = lambda *v: torch.tensor(np.asarray(v, np.float32)).cuda()
    raw32 = lambda *b: torch.tensor(np.asarray(b, np.uint32).view(np.float32)).cuda()
    for wdt in X.DTYPES:
        z = torch.tensor([0.0, -0.0, 0.0, -0.0, 0.0]).to(TORCH_DT[wdt]).cuda()
        assert weight_stats(z) == (BE_OK, 0, 0xffffffff), wdt
        for bad, name in ((float('inf'), 'inf'), (float('-inf'), '-inf'), (float('nan'), 'nan')):
            rc, mx, mn = weight_stats(torch.tensor([0.5, bad, -2.0]).to(TORCH_DT[wdt]).cuda())
            assert rc == BE_OK and mx >= 0x7f800000 and mn == bits(0.5), (wdt, name, hex(mx))
    # f32 subnormals: the pass orders bit patterns as integers, so they come back unflushed
    assert weight_stats(raw32(0x00000003, 0x80400000, 0, 0x80000001)) == (BE_OK, 0x00400000, 0x00000001)
    assert weight_stats(raw32(0x00000003, 0x3f800000)) == (BE_OK, 0x3f800000, 0x00000003)
    # f16 subnormals are normal f32 values: 2^-24 and 3 * 2^-24
    h = torch.tensor(np.asarray([1, 0x8003, 0], np.uint16).view(np.float16)).cuda()
    assert weight_stats(h) == (BE_OK, bits(3 * 2.0 ** -24), bits(2.0 ** -24))
    # f64 beyond the f32 range becomes inf; below the f32 subnormals it counts as zero
    d = lambda *v: torch.tensor(np.asarray(v, np.float64)).cuda()
    assert weight_stats(d(1.0, -1e300)) == (BE_OK, 0x7f800000, bits(1.0))
    assert weight_stats(d(1e-60, -1e-300)) == (BE_OK, 0, 0xffffffff)
    assert weight_stats(d(1e-60, -0.25, 0.0)) == (BE_OK, bits(0.25), bits(0.25))
    assert weight_stats(f32(3.0)) == (BE_OK, bits(3.0), bits(3.0))


def test_weight_stats_refusals():
    w = torch.tensor([1.0, -2.0, 0.5]).cuda()
    clean = lambda: weight_stats(w) == (BE_OK, bits(2.0), bits(0.5))
    assert clean()
    for kw in ({'null': ('weights',)}, {'null': ('max',)}, {'null': ('min',)}, {'null': ('scratch',)}, {'scratch_bytes': 255}, {'n': -1},
               {'wcode': 7}, {'wcode': -1}):
        rc, mx, mn = weight_stats(w, **kw)
        assert rc == BE_ERR_INVALID and (mx, mn) == (0xdead, 0xbeef), kw
        assert clean(), kw


# ---------------------------------------------------------------------------------------------------------------------------
# be_fixed_point_exponent
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wdt', X.DTYPES)
def test_entry_boundaries(wdt):
    n = 0
    for name in X.CASES:
        c = X.build(name)
        if wdt not in c.dtypes():
            continue
        n += 1
        assert entry_of(c, wdt) == c.entry(), (name, wdt)
        assert entry_of(c, wdt, has_indices=False) == c.entry(has_indices=False), (name, wdt)
    assert n >= (25 if wdt == 'f16' else 49)


@pytest.mark.parametrize('wdt', X.DTYPES)
def test_entry_degenerate_and_clamp(wdt):
    for c in X.degenerate_cases() + [X.clamp_case()]:
        if wdt not in c.dtypes():
            continue
        for has in (True, False):
            for keep in (None, 70, 13):
                assert entry_of(c, wdt, has_indices=has, keep=keep) == c.entry(has_indices=has, keep=keep), (c.name, wdt, has, keep)
    # no entry at all: the bound is 0, nothing limits the exponent but `keep`
    w, idx, _ = on_device(X.degenerate_cases()[3], wdt)
    for keep, want in ((None, 62), (62, 62), (63, 62), (-5, -5)):
        assert entry_call(w, idx, 6, nnz=0, keep=keep) == want == X.entry_rule(0.0, 0.0, None, float('inf'), 0, True, MB, keep)
        assert entry_call(w, None, 6, nnz=0, keep=keep, min_bits=60) == want
    assert X.clamp_case().entry() == C['clamp.hi']


def test_entry_all_subnormal_weights():
    """Whether the device's global float atomicAdd keeps f32 subnormals is observed, not assumed (DESIGN.md records it): a refusal,
    or an exponent that holds the invariant.  With min_weight_bits = 0 the gate passes on the smallest weight, the column sums stay
    in the scratch, and the test prints what they became."""
    c = X.subnormal_case()
    w, idx, _ = on_device(c, 'f32')
    assert weight_stats(w) == (BE_OK,) + _stats_reference(c.weights)
    assert entry_of(c, 'f32') in (RANGE, c.entry())
    A, L = lib()
    scr = torch.zeros(int(L.fn('be_fixed_point_scratch_bytes')(c.k)), dtype=torch.uint8, device='cuda')
    e = holds(c, entry_call(w, idx, c.k, min_bits=0, scratch=scr))
    sums = scr[256:256 + 4 * c.k].view(torch.float32).cpu().numpy()
    exact = np.zeros(c.k)
    np.add.at(exact, c.indices, np.abs(c.weights))
    print(f"\n[subnormal column sums] device bits {[hex(b) for b in sums.view(np.uint32)]} exact bits "
          f"{[hex(b) for b in exact.astype(np.float32).view(np.uint32)]} exponent {e} "
          f"({'kept' if np.array_equal(sums, exact.astype(np.float32)) else 'flushed or altered'})")
    assert e in (c.entry(min_bits=0), RANGE)        # 150 from the exact sums; sums flushed to zero give 62, which the gate then refuses


@pytest.mark.parametrize('wdt', X.DTYPES)
def test_entry_pass_past_one_trip(wdt):
    c = X.big_nnz_case()
    assert c.nnz == X.ENTRY_TRIP + 257 and wdt in c.dtypes()
    assert entry_of(c, wdt) == c.entry() == 47
    assert entry_of(c, wdt, has_indices=False) == c.entry(has_indices=False)
    # the column maxima past one trip too: a threshold of 2 units against fillers of 1 unit sends the gate to k_fp_colmax, where every
    # filler column fails it: RANGE; one bit less passes on the smallest weight
    assert entry_of(c, wdt, min_bits=47 + 1) == c.entry(min_bits=48) == RANGE
    assert entry_of(c, wdt, min_bits=47) == 47


@pytest.mark.parametrize('wdt', ['f32', 'bf16'])
def test_reduce_past_one_trip(wdt):
    mb = X.gate_min_bits(X.PU)
    s, m = X.big_k_case('sum'), X.big_k_case('max')
    assert s.k == X.REDUCE_TRIP + 1 == m.k
    assert entry_of(s, wdt) == s.entry() == 49                       # 51 if column k - 1 were missed
    assert entry_of(m, wdt) == m.entry() == 50
    assert entry_of(m, wdt, min_bits=mb) == m.entry(min_bits=mb) == RANGE          # 50 if column k - 1 were missed
    assert entry_of(m, wdt, min_bits=mb - 1) == 50


def test_entry_keep_edges():
    for name in ('edge-below-mixed-j-6', 'edge-pow2-neg-j12'):
        c = X.build(name)
        need = c.entry()
        far = need - 40                                                  # 2^(16 - far) is above every filler column's largest weight
        assert c.entry(keep=far) == need and c.entry(has_indices=False, keep=c.entry(has_indices=False) - 40) == c.entry(has_indices=False)
        for keep in (need, need + 1, need - 1, far, INT_MIN, None, need - 7):
            for wdt in ('f32', 'f64'):
                assert entry_of(c, wdt, keep=keep) == c.entry(keep=keep), (name, keep)
                assert entry_of(c, wdt, has_indices=False, keep=keep) == c.entry(has_indices=False, keep=keep), (name, keep)
        assert entry_of(c, 'f32', keep=need - 1) == need - 1 and entry_of(c, 'f32', keep=need + 1) == need


@pytest.mark.parametrize('wdt', X.DTYPES)
def test_entry_gate_edges(wdt):
    mb = X.gate_min_bits(X.GATE_PU_ENTRY)
    want = {'wmin-at': 50, 'wmin-below': 50, 'colmax-below': RANGE, 'mean-pass': 50, 'mean-fail': 50}
    for v in X.GATE_VARIANTS:
        c = X.gate_case(v, X.GATE_PU_ENTRY)
        assert entry_of(c, wdt, min_bits=mb) == c.entry(min_bits=mb) == want[v], v
        assert entry_of(c, wdt, min_bits=mb - 1) == 50
        assert entry_of(c, wdt, min_bits=mb + 1) == c.entry(min_bits=mb + 1), v
        for keep in (50, 49, 30):                                        # a lower exponent only raises the threshold
            assert entry_of(c, wdt, min_bits=mb, keep=keep) == c.entry(min_bits=mb, keep=keep), (v, keep)
        assert entry_of(c, wdt, has_indices=False, min_bits=mb) == c.entry(has_indices=False, min_bits=mb)


def test_entry_refusals():
    c = X.build('edge-below-pos-j0')
    w, idx, _ = on_device(c, 'f32')
    clean = lambda: entry_call(w, idx, c.k) == c.entry()
    assert clean()
    assert entry_call(w, idx, c.k, min_bits=0) == c.entry(min_bits=0)
    assert entry_call(w, idx, c.k, min_bits=C['min_bits.entry']) == c.entry(min_bits=60) == RANGE
    light = X.degenerate_cases()[3]                                       # one entry: 60 bits are there
    lw, lidx, _ = on_device(light, 'f32')
    assert entry_call(lw, lidx, light.k, min_bits=60) == light.entry(min_bits=60) != RANGE
    for kw in ({'min_bits': -1}, {'min_bits': C['min_bits.entry'] + 1}, {'nnz': -1}, {'null': ('weights',)}, {'null': ('out',)},
               {'null': ('scratch',)}, {'wcode': 7}):
        assert entry_call(w, idx, c.k, **kw) == BE_ERR_INVALID, kw
        assert clean(), kw
    for k in (0, -1, 1 << 32):
        A, L = lib()
        out = ctypes.c_int(-1)
        scr = torch.empty(4096, dtype=torch.uint8, device='cuda')
        rc = L.fn('be_fixed_point_exponent')(A.ptr(w), X.BE_F32, A.ptr(idx), w.numel(), k, MB, INT_MIN, A.ptr(scr), 1 << 40,
                                             ctypes.byref(out), A.stream_ptr())
        assert rc == BE_ERR_INVALID and out.value == -1 and clean(), k
    assert entry_call(w, idx, c.k, short=1) == BE_ERR_WORKSPACE and clean()
    for wdt in X.DTYPES:
        for bad in (float('inf'), float('-inf'), float('nan')):
            wb = torch.tensor(c.weights).to(TORCH_DT[wdt])
            wb[c.nnz - 3] = bad
            assert entry_call(wb.cuda(), idx, c.k) == RANGE and entry_call(wb.cuda(), None, c.k) == RANGE, (wdt, bad)
    assert entry_call(torch.tensor([1.0, 1e300], dtype=torch.float64).cuda(), idx[:2], c.k) == RANGE       # inf once it is an f32
    assert clean()


def test_entry_wide_f64():
    """f64 weights that no f32 holds: the f32 sums round, the invariant holds."""
    c = X.wide_f64_case()
    for has in (True, False):
        assert entry_of(c, 'f64', has_indices=has) != RANGE


@pytest.mark.parametrize('wdt', ['f32', 'f64', 'bf16'])
def test_overflowing_column_sum_entry(wdt):
    """Four weights of 2^126 in one column: the f32 column sum is inf, which frexp leaves alone — the exponent must come from the
    bound without the structure (never 62, at which the step converts 2^156 to an integer)."""
    c = X.overflow_case()
    e = entry_of(c, wdt)
    assert e != 62 and e == c.entry() == -67 and X.true_bound_holds(c, e) and not X.true_bound_holds(c, 62)
    assert entry_of(c, wdt, has_indices=False) == -67 and entry_of(c, wdt, keep=-70) == -70 and entry_of(c, wdt, keep=0) == -67


# ---------------------------------------------------------------------------------------------------------------------------
# be_scatter_plan_exponent
# ---------------------------------------------------------------------------------------------------------------------------
def build_plan(case, wdt, layout, geometry=True):
    from brainevent_amd._csr import ScatterPlan
    w, idx, ptr = on_device(case, wdt)
    kw = {'slice_shift': X.SLICE_SHIFT, 'slice_width': X.SLICE_WIDTH} if geometry else {}
    plan = ScatterPlan.build(w, idx, ptr, shape=(case.m, case.k), layout=layout, **kw)
    assert plan.layout == {'u16': ScatterPlan.LAYOUT_U16, 'd8': ScatterPlan.LAYOUT_D8}['u16' if wdt == 'f64' else layout]
    assert plan.split_f64 == (wdt == 'f64')
    return plan


@pytest.mark.parametrize('layout', ['u16', 'd8'])
def test_plan_boundaries(layout):
    """Two slices, m = 1025, the heavy column reached five ways (exponent_cases.boundary_case).  f32 on every case; f16 / bf16 and
    the f64 split (u16 only: the sorted layout does not take f64) on the j = -6 cases."""
    for name in X.CASES:
        c = X.build(name)
        for wdt in ['f32'] + (['f16', 'bf16'] + (['f64'] if layout == 'u16' else []) if name.endswith('j-6') else []):
            plan = build_plan(c, wdt, layout)
            assert plan.n_slices == 2 and c.m == X.PLAN_ROW_TRIP + 1
            assert holds(c, plan.scale_exp) == c.plan(split=wdt == 'f64'), (name, wdt, layout)
            assert c.entry() <= plan.scale_exp <= c.entry() + 1


@pytest.mark.parametrize('layout', ['u16', 'd8'])
def test_plan_keep_through_a_refresh(layout):
    """A refresh passes the plan's exponent as `keep`: kept while it cannot overflow and is fine enough, else `need`."""
    from brainevent_amd._csr import ScatterPlan
    c = X.build('edge-below-mixed-j-6')
    w, idx, ptr = on_device(c, 'f32')
    plan = build_plan(c, 'f32', layout)
    e = plan.scale_exp
    assert e == c.plan()
    a32 = c.stats()['a32']
    kept = []
    for s in (-1, 0, 1, -1, 5, -45, 0):                                   # halved: kept; doubled: moves; 2^-45: too coarse to keep
        want = X.plan_rule(np.ldexp(a32, s), c.indices, c.k, c.nnz, MB, e)
        plan.refresh_weights(w * (2.0 ** s), idx, ptr)                    # (a power of two: exact)
        assert plan.scale_exp == want, (s, e, want)
        assert Fraction(int(c.col_units().max())) * Fraction(2) ** (c.j + s + want) < (1 << 62)
        kept.append(want == e)
        e = want
    assert kept == [True, True, False, True, False, False, False], kept


@pytest.mark.parametrize('layout', ['u16', 'd8'])
def test_plan_gate_edges(layout, monkeypatch):
    """The colmax mode (MODE 1 of k_plan_colstats), forced by one weight a quantum under the threshold; rows of 8192 entries on one
    column: blocks of 32 passes.  min_weight_bits = 40, the limit."""
    from brainevent_amd._csr import ScatterPlan, MathError
    mb = X.gate_min_bits(X.GATE_PU_PLAN)
    monkeypatch.setattr(ScatterPlan, 'MIN_WEIGHT_BITS', mb)
    for v in X.GATE_VARIANTS:
        c = X.gate_case(v, X.GATE_PU_PLAN)
        want = c.plan(min_bits=mb)
        assert want == (RANGE if v == 'colmax-below' else 39)
        if want == RANGE:
            with pytest.raises(MathError):
                build_plan(c, 'f32', layout, geometry=False)
        else:
            assert holds(c, build_plan(c, 'f32', layout, geometry=False).scale_exp) == want, v
    monkeypatch.setattr(ScatterPlan, 'MIN_WEIGHT_BITS', mb - 1)
    assert build_plan(X.gate_case('colmax-below', X.GATE_PU_PLAN), 'f32', layout, geometry=False).scale_exp == 39


@pytest.mark.parametrize('layout', ['u16', 'd8'])
def test_plan_degenerate_clamp_and_overflowing_sum(layout):
    for c in X.degenerate_cases() + [X.clamp_case(), X.overflow_case()]:
        if c.nnz == 1:
            continue                    # (a weight array of one element is the library's form of ONE SHARED weight: no exponent)
        for wdt in ('f32', 'bf16'):
            plan = build_plan(c, wdt, layout, geometry=False)
            assert holds(c, plan.scale_exp) == c.plan(), (c.name, wdt)
    c = X.overflow_case()
    assert c.plan() == -67 == c.entry() and build_plan(c, 'f64', 'u16', geometry=False).scale_exp == c.plan(split=True) == -67


def test_plan_refusals():
    """min_weight_bits 41 is refused by the entry point itself; 40 and 0 are served."""
    from brainevent_amd._csr import ScatterPlan
    A, L = lib()
    c = X.build('edge-below-pos-j0')
    plan = build_plan(c, 'f32', 'd8')
    s = c.stats()
    maxabs = torch.tensor(np.asarray([bits(s['wmax']), bits(s['wmin'])], np.uint32).view(np.int32)).cuda()
    scr = torch.empty(256, dtype=torch.uint8, device='cuda')

    def call(min_bits, scratch_bytes=256, layout=None, keep=INT_MIN):
        out = ctypes.c_int(-12345)
        rc = L.fn('be_scatter_plan_exponent')(A.ptr(plan.blob), A.ptr(plan.seg), plan.m, plan.k, plan.slice_shift, plan.slice_width,
                                              plan.layout if layout is None else layout, plan.nnz, A.ptr(maxabs), min_bits, keep,
                                              A.ptr(scr), scratch_bytes, ctypes.byref(out), A.stream_ptr())
        return rc, out.value
    assert call(MB) == (BE_OK, c.plan())
    assert call(C['min_bits.plan'] + 1) == (BE_ERR_INVALID, -12345) == call(-1)
    assert call(MB, layout=ScatterPlan.LAYOUT_H8)[0] == BE_ERR_INVALID and call(MB, scratch_bytes=255)[0] == BE_ERR_WORKSPACE
    assert call(0) == (BE_OK, c.plan(min_bits=0)) and call(C['min_bits.plan']) == (BE_OK, c.plan(min_bits=C['min_bits.plan']))
    assert call(MB, keep=c.plan() - 2) == (BE_OK, c.plan() - 2) and call(MB) == (BE_OK, c.plan())


# ---------------------------------------------------------------------------------------------------------------------------
# BinnedScatter by steps
# ---------------------------------------------------------------------------------------------------------------------------
def binned(case, wdt, acc32, monkeypatch, fallbacks=None):
    """A BinnedScatter whose exponent comes from binned steps (STATS_BY_STEPS_MIN_NNZ patched to 1); `fallbacks` collects the calls
    of the entry pass."""
    from brainevent_amd import _csr
    monkeypatch.setattr(_csr.BinnedScatter, 'STATS_BY_STEPS_MIN_NNZ', 1)
    if fallbacks is not None:
        real = _csr.fixed_point_exponent
        monkeypatch.setattr(_csr, 'fixed_point_exponent', lambda *a, **k: (fallbacks.append(k), real(*a, **k))[1])
    w, idx, ptr = on_device(case, wdt)
    ws = _csr.BinnedScatter(w, case.m, case.k, case.nnz, indices=idx, indptr=None if case.indptr is None else ptr, row_len=case.row_len,
                            acc32=acc32)
    assert ws._stats is not None
    return ws


def check_steps(case, wdt, acc32, monkeypatch):
    from brainevent_amd._csr import MathError
    mb = 50 if acc32 else MB                                             # ACC32_MIN_WEIGHT_BITS + 32
    want, by_entry = case.steps(min_bits=mb)
    calls = []
    if want == RANGE:
        with pytest.raises(MathError):
            binned(case, wdt, acc32, monkeypatch, calls)
        return None
    ws = binned(case, wdt, acc32, monkeypatch, calls)
    assert ws.acc32 == acc32 and ws.scale_exp == want - (32 if acc32 else 0), (case.name, wdt, acc32, ws.scale_exp, want)
    assert bool(calls) == by_entry, (case.name, calls)
    s = case.stats()
    if s['wmax'] == 0.0:
        assert ws._stats == (0.0, float('inf'), 0.0, float('inf'))
    else:
        assert (ws._stats[0], ws._stats[2], ws._stats[3]) == (s['colsum_max'], s['wmax'], s['wmin'])
        # the smallest column mean is one f32 division by torch, not by this library: held to the correctly rounded quotient's neighbours
        mean = np.float32(s['mean_min'])
        assert np.nextafter(mean, np.float32(0)) <= np.float32(ws._stats[1]) <= np.nextafter(mean, np.float32(np.inf)), (ws._stats, s['mean_min'])
    holds(case, ws.scale_exp + (32 if acc32 else 0))
    return ws


@pytest.mark.parametrize('acc32', [False, True])
@pytest.mark.parametrize('rows', ['fixed', 'indptr'])
def test_binned_by_steps(rows, acc32, monkeypatch):
    from brainevent_amd._csr import BinnedScatter
    assert BinnedScatter.ACC32_MIN_WEIGHT_BITS == 18
    if rows == 'fixed':
        cases = [X.fixed_rows_case(w, s, -6) for w in X.WHERE for s in ('pos', 'mixed')]
    else:
        cases = [X.build(n) for n in X.boundary_cases(j=-6) + X.boundary_cases(where='below', j=12)]
    for c in cases:
        # f16 / bf16: the steps' f32 sums must come back unrounded (BE_BINNED_OUT_F32) — 4095 units do not fit 8 or 11 bits
        for wdt in ('f32', 'bf16', 'f16') if c.name.endswith('pos-j-6') else ('f32',):
            check_steps(c, wdt, acc32, monkeypatch)


def test_binned_by_steps_gate_and_the_fall_back(monkeypatch):
    """A column whose mean passes while the smallest weight fails: decided without the entry pass; one whose mean fails: the atomic
    pass decides (its maximum passes, or RANGE)."""
    from brainevent_amd import _csr
    mb = X.gate_min_bits(X.GATE_PU_ENTRY)
    for v in X.GATE_VARIANTS:
        c = X.gate_case(v, X.GATE_PU_ENTRY)
        calls = []
        ws = binned(c, 'f32', False, monkeypatch, calls)
        assert ws.scale_exp == c.steps()[0] == 50 and not calls
        w, idx, _ = on_device(c, 'f32')
        want, by_entry = c.steps(min_bits=mb)
        for keep in (None, 50, 45):
            del calls[:]
            if want == RANGE:
                with pytest.raises(_csr.MathError):
                    ws._exponent(w, idx, min_bits=mb, keep=keep)
            else:
                assert ws._exponent(w, idx, min_bits=mb, keep=keep) == c.steps(min_bits=mb, keep=keep)[0], (v, keep)
            assert bool(calls) == c.steps(min_bits=mb, keep=keep)[1], (v, keep)
        assert by_entry == (v in ('wmin-below', 'colmax-below', 'mean-fail'))


def test_binned_step_returns_f32_sums_on_request():
    """BE_BINNED_OUT_F32 (what the statistics steps pass): f16 / bf16 weights, `out` f32 — the exact sums of tests/binned_cases.py,
    not their 16-bit rounding (which differs in some column of the |w| sums of the bf16 cases), nothing written past k."""
    import binned_cases as B
    from test_binned_kernels_exact_gpu import Device, cast_reference
    OUT_F32, rounding_shows = 16, 0
    for name in ('mixed-acc64-bf16', 'mixed-acc64-f16', 'mixed-acc32-bf16', 'mixed-counted-f16'):
        c = B.build(name)
        d = Device(c)
        A, L = d.A, d.lib
        ev, sd = d.events(c.spikes, 'bool')
        rows, live = c.rows_of_entries, c.spikes[0][c.rows_of_entries] & (c.indices < c.k)
        for flags in (OUT_F32,) + ((OUT_F32 | B.BE_BINNED_ABS,) if c.kind != 1 else ()):
            ref = np.zeros(c.k)
            np.add.at(ref, c.indices[live], c.entry_weights(absolute=bool(flags & B.BE_BINNED_ABS))[live])
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
            rounding_shows += bool((cast_reference(ref, c.wdtype) != ref).any())
            raw = torch.full((c.k + 8,), 7.0, dtype=torch.float32, device='cuda')
            is64 = int(c.indptr is not None and c.indptr.dtype == np.int64)
            rc = L.fn('be_binary_csrmm_t_binned')(A.ptr(d.w), c.kind | flags, A.wcode(d.w), A.ptr(d.indices), A.ptr(d.indptr), is64, c.row_len,
                                                  A.ptr(ev), sd, A.ptr(raw), c.m, c.k, 1, c.slice_shift, c.bin_capacity, B.SCALE_EXP[c.kind],
                                                  A.ptr(d.ws), d.ws_bytes, A.stream_ptr())
            torch.cuda.synchronize()
            assert rc == BE_OK, L.last_error()
            assert np.array_equal(raw[:c.k].cpu().numpy().astype(np.float64), ref), (name, flags)
            assert bool((raw[c.k:] == 7.0).all())
    assert rounding_shows >= 2


def test_overflowing_column_sum_by_steps(monkeypatch):
    c = X.overflow_case()
    ws = check_steps(c, 'f32', False, monkeypatch)
    print(f"\n[overflowing column sum by steps] statistics {ws._stats} exponent {ws.scale_exp}")
    assert ws.scale_exp == -67 != 62 and ws._stats[0] == float('inf')
    for c in X.degenerate_cases() + [X.clamp_case()]:
        if c.nnz > 1:                   # (one element is the library's form of one shared weight: no exponent)
            check_steps(c, 'f32', False, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# the three sources on one case; end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_three_sources_on_one_case(monkeypatch):
    """Each source equals its own rule; the plan is the entry pass's exponent or one above it, and one above exactly in the 0.1 %
    band under a power of two."""
    for where, band in (('pow2', False), ('below', True), ('cross-lo', False), ('cross-hi', True)):
        for signs in X.SIGNS:
            c = X.build(f'edge-{where}-{signs}-j-6')
            e = entry_of(c, 'f32')
            p = {lay: build_plan(c, 'f32', lay).scale_exp for lay in ('u16', 'd8')}
            s = binned(c, 'f32', False, monkeypatch).scale_exp
            assert (e, p['u16'], p['d8'], s) == (c.entry(), c.plan(), c.plan(), c.steps()[0]), c.name
            assert e <= p['d8'] <= e + 1 and (p['d8'] == e + 1) == band and s == e
            for x in (e, p['d8'], s):
                holds(c, x)


@pytest.mark.parametrize('signs', ['pos', 'neg'])
@pytest.mark.parametrize('where', ['below', 'pow2'])
def test_end_to_end_at_the_boundary(be, where, signs, monkeypatch):
    """S = 2^p - q and S = 2^p, all of one sign, every row active: the planned step (both layouts) and the binned step (64- and
    32-bit sums), each at the exponent its own source chose, give the dense f64 sums cast once — exact by construction, so a wrap
    of the integer sums shows."""
    for j in (-6, 12):
        c = X.build(f'edge-{where}-{signs}-j{j}')
        w, idx, ptr = on_device(c, 'f32')
        ref = torch.tensor(c.reference().astype(np.float32))
        assert abs(float(ref[X.H])) == math.ldexp(c.extra['heavy'], j)
        v = torch.ones(c.m, dtype=torch.bool, device='cuda')
        for lay in ('u16', 'd8'):
            plan = build_plan(c, 'f32', lay)
            assert plan.scale_exp == c.plan()
            out = be.binary_csrmv(w, idx, ptr, v, shape=(c.m, c.k), transpose=True, workspace=plan)
            assert torch.equal(out.cpu(), ref), (c.name, lay)
        for acc32 in (False, True):
            ws = check_steps(c, 'f32', acc32, monkeypatch)
            out = be.binary_csrmv(w, idx, ptr, v, shape=(c.m, c.k), transpose=True, workspace=ws)
            assert torch.equal(out.cpu(), ref), (c.name, acc32)
