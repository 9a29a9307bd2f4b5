"""The fixed-point exponent rule restated in plain Python, and the exact cases it is tested on — shared by
tests/test_exponent_rule_cpu.py (the rules against integer arithmetic, CONSTS against the source text) and
tests/test_exponent_exact_gpu.py (the three device sources against the rules).  numpy only: nothing here needs a device.

Every fast scatter route accumulates ``round(w * 2^e)`` in integers.  Three sources choose ``e`` by one rule:
  1. `entry_rule`  be_fixed_point_exponent (csrc/be_fixed_point.hip): f32 atomic column sums of |w| over the raw entries, times 1.001;
  2. `plan_rule`   be_scatter_plan_exponent (csrc/be_csr_plan.hip, k_plan_colstats): 64-bit integer column sums at a safe exponent
                   e0, every addend rounded up: a true upper bound with no margin;
  3. `steps_rule`  BinnedScatter._exponent_by_steps (_csr.py): column sums and counts from binned steps, the column MEAN as a
                   sufficient gate, the entry pass as the fall-back.
Each returns the exponent or `RANGE` (BE_ERR_RANGE / MathError).

The relation between 1 and 2.  With S the largest column sum, source 1 takes the smallest power of two above ``1.001 S``,
source 2 the smallest above ``S + (n_c + 1) 2^-e0`` (n_c: the non-zero entries of the column; ``(n_c + 1) 2^-e0 <= 2^-34 S`` at
the e0 it picks, module `plan_rule`).  ``S < S + eps < 1.001 S`` gives ``eb_plan <= eb_entry`` and, 1.001 being below 2,
``eb_entry <= eb_plan + 1``: away from the clamps ``entry <= plan <= entry + 1``, and ``plan == entry + 1`` exactly when a
power of two lies in ``(S + eps, 1.001 S]`` — the 0.1 % band under every power of two.  Both are safe; the plan is never lower.

Exactness (the argument of tests/binned_cases.py).  Weights are ``n * q`` with integer ``|n| <= 64`` and ``q = 2^j``: exact in f32,
f16 (j kept inside its normal range), bf16 (8 significant bits: the reason for 64) and f64.  Every case asserts
``sum_c |n| < 2^24`` over every column (`Case.check_exact`).  Then every partial sum of a column, in any order, is ``N q`` with
N < 2^24: the f32 atomic sums of source 1 are the same bits whatever the order, and the f32 outputs of the binned steps of source 3
(integer sums at a provisional exponent e0 with ``j + e0 > 0``, converted once) and their f32 accumulation over the chunks are
exact.  Source 2 works in integers throughout.  So every comparison of the GPU module is an equality.

Clamps.  Weights of 2^-120 reach the upper clamp, 150.  The lower clamp, -90, needs a bound of 2^152 or more: with indices a column
sum that f32 cannot hold, without them ``wmax * (nnz + 1) >= 2^152``, i.e. 2^24 entries of about 2^127 — not reachable at test
size, and no case pretends to; the CPU module drives the restated rules through it."""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Optional

import numpy as np

RANGE = 'RANGE'
INT_MIN = -(1 << 31)
BE_OK, BE_ERR_INVALID, BE_ERR_WORKSPACE, BE_ERR_RANGE = 0, -1, -2, -4
BE_F32, BE_F64, BE_F16, BE_BF16 = 0, 1, 2, 3
WCODE = {'f32': BE_F32, 'f64': BE_F64, 'f16': BE_F16, 'bf16': BE_BF16}
DTYPES = ('f32', 'f64', 'f16', 'bf16')

# what the rules and the sizes of the GPU cases are made of (tests/test_exponent_rule_cpu.py holds every entry to the source)
CONSTS = {
    'entry.block': 256,                  # threads of k_fp_colsum / k_fp_colmax / k_fp_reduce
    'entry.grid_cap': 256 * 16,          # grid_for(nnz, 256, 256 * 16): workgroups of the entry passes
    'reduce.grid_cap': 1024,             # grid_for(k, 256, 1024): workgroups of k_fp_reduce
    'margin': 1.001,                     # the entry pass's (and the binned steps') factor on the column sum
    'headroom': 62,                      # need = 62 - eb
    'clamp.lo': -90,
    'clamp.hi': 150,
    'min_bits.entry': 60,                # be_fixed_point_exponent accepts 0 ... 60
    'min_bits.plan': 40,                 # be_scatter_plan_exponent accepts 0 ... 40
    'plan.e0': 61,                       # e0 = 61 - ew - en
    'plan.block': 1024,                  # k_plan_colstats: 16 waves, 64 rows each per trip
    'plan.u': 4,                         # ... four blocks in flight per wave
    'plan.pass_items': 256,              # ... a 64-lane pass covers 64 groups of 4 items
    'steps.min_nnz': 1 << 24,            # BinnedScatter.STATS_BY_STEPS_MIN_NNZ
}
C = CONSTS
ENTRY_TRIP = C['entry.block'] * C['entry.grid_cap']            # entries one trip of the capped grid covers
REDUCE_TRIP = C['entry.block'] * C['reduce.grid_cap']          # columns one trip of k_fp_reduce covers
PLAN_ROW_TRIP = C['plan.block']                                # rows one trip of k_plan_colstats's wave loop covers
MAX_UNITS = 64
EXACT_SUM = 1 << 24


def frexp_exp(x):
    """eb with x < 2^eb (0 for x <= 0 — and for inf, which C's frexp leaves alone: the hole the fall-back closes)."""
    return math.frexp(x)[1] if x > 0 else 0


def clamp(e):
    return max(C['clamp.lo'], min(C['clamp.hi'], e))


def candidates(keep, need):
    return ([keep] if keep is not None and keep != INT_MIN and keep <= need else []) + [need]


def _thr(min_bits, e):
    return math.ldexp(1.0, min_bits - e)


def entry_rule(colsum_max_f32, wmax, wmin, colmax_min, nnz, has_indices, min_bits, keep):
    """be_fixed_point_exponent.  `colsum_max_f32`: the largest f32 column sum of |w|; `wmax` / `wmin`: largest and smallest
    non-zero |w| as f32 values (`wmin` None when every weight is zero); `colmax_min`: the smallest of the columns' largest |w|
    over the live columns.  A column sum that f32 cannot hold falls back to the bound without structure."""
    if not math.isfinite(wmax):
        return RANGE
    s = float(np.float32(colsum_max_f32))
    if has_indices and math.isfinite(s):
        bound = s * C['margin']
    else:
        bound = float(wmax) * float(nnz + 1)
    need = clamp(C['headroom'] - frexp_exp(bound))
    for e in candidates(keep, need):
        thr = _thr(min_bits, e)
        if wmin is None or float(wmin) >= thr:
            return e
        if has_indices and float(colmax_min) >= thr:
            return e
    return RANGE


def fixed_floor(absw_f32, e0):
    """fixed_from_f32(|w|, 2^(e0 - 32)) for f32 values, as int64.  The device computes ``t = w * 2^(e0 - 32)`` (a power-of-two
    scaling: exact), ``hi = floor(t)``, ``lo = (unsigned)((t - hi) * 2^32)``: ``t - hi`` is exact (no more significant bits than
    t), so is its scaling by 2^32, and the conversion to unsigned drops what lies below one unit: ``hi * 2^32 + lo`` is
    ``floor(|w| * 2^e0)`` — truncated, never rounded.  Here: the 24-bit significand shifted."""
    a = np.asarray(absw_f32, np.float64)
    mant, ex = np.frexp(a)
    mant = (mant * (1 << 24)).astype(np.int64)                 # exact: an f32 has 24 significant bits
    shift = ex.astype(np.int64) - 24 + e0
    assert np.all((shift + 24 <= 62) | (mant == 0)), "the caller's e0 keeps every addend below 2^62"
    return np.where(shift >= 0, mant << np.maximum(shift, 0), mant >> np.minimum(-np.minimum(shift, 0), 63))


def plan_bound(absw_f32, cols, k, nnz):
    """(bound, e0, smax) of be_scatter_plan_exponent: integer column sums of ``floor(|w| 2^e0) + 1`` over the NON-ZERO stored
    weights (padding, escapes and zero weights add nothing), ``bound = ((double)smax + 1) * 2^-e0``.  e0 makes
    ``nnz * (wmax 2^e0 + 1) < 2^61 + 2^en``: int64 holds every sum.  `nnz` is what the plan was built with (an f64 split doubles it)."""
    a = np.abs(np.asarray(absw_f32, np.float32))
    wmax = float(a.max(initial=0.0))
    if not (wmax > 0.0 and nnz > 0):
        return 0.0, None, 0
    ew, en = math.frexp(wmax)[1], math.frexp(float(nnz))[1]
    e0 = clamp(C['plan.e0'] - ew - en)
    live = a > 0
    add = fixed_floor(a[live], e0) + 1
    sums = np.zeros(k, np.int64)
    np.add.at(sums, np.asarray(cols)[live], add)
    assert int(add.max()) * int(live.sum()) < (1 << 63)
    smax = int(sums.max())
    return math.ldexp(float(smax) + 1.0, -e0), e0, smax


def plan_rule(absw_f32, cols, k, nnz, min_bits, keep):
    """be_scatter_plan_exponent on the f32 weights the blocks hold."""
    a = np.abs(np.asarray(absw_f32, np.float32))
    wmax = float(a.max(initial=0.0))
    if not math.isfinite(wmax):
        return RANGE
    nz = a[a > 0]
    wmin = float(nz.min()) if nz.size else None
    bound = plan_bound(a, cols, k, nnz)[0]
    need = clamp(C['headroom'] - frexp_exp(bound))
    colmax_min = None
    for e in candidates(keep, need):
        thr = _thr(min_bits, e)
        if wmin is None or wmin >= thr:
            return e
        if colmax_min is None:
            colmax_min = column_max_min(a, cols, k)
        if colmax_min >= thr:
            return e
    return RANGE


def steps_rule(colsum_max_f32, mean_min_f32, wmax, wmin, colmax_min, nnz, min_bits, keep):
    """BinnedScatter._exponent_by_steps -> (exponent or RANGE, whether the entry pass decided).  `mean_min_f32`: the smallest f32
    quotient colsum / count over the columns that hold an entry (inf without one)."""
    if not math.isfinite(wmax):
        return RANGE, False
    s = float(np.float32(colsum_max_f32))
    bound = s * C['margin'] if math.isfinite(s) else float(wmax) * float(nnz + 1)
    need = clamp(C['headroom'] - frexp_exp(bound))
    wmin_f = float('inf') if wmin is None else float(wmin)
    for e in candidates(keep, need):
        thr = _thr(min_bits, e)
        if wmin_f >= thr or float(mean_min_f32) >= thr:
            return e, False
    return entry_rule(colsum_max_f32, wmax, wmin, colmax_min, nnz, True, min_bits, keep), True


def column_max_min(absw, cols, k):
    """The smallest of the columns' largest |w| over the columns that hold a non-zero weight (inf without one)."""
    cm = np.zeros(k, np.float64)
    np.maximum.at(cm, np.asarray(cols), np.asarray(absw, np.float64))
    live = cm > 0
    return float(cm[live].min()) if live.any() else float('inf')


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
F16_J = (-14, 9)                         # n * 2^j with 1 <= |n| <= 64 stays a normal f16 for j in this range


@dataclass
class Case:
    """One matrix: ``weights = units * 2^j`` (f64 values, exact in every weight dtype the case allows), CSR structure.  Read-only."""
    name: str
    m: int
    k: int
    units: np.ndarray                      # int64, signed
    j: int
    indices: np.ndarray                    # int32
    indptr: Optional[np.ndarray]           # int32; None: rows of `row_len` entries
    row_len: int = -1
    negzero: Optional[np.ndarray] = None   # entries that are -0.0
    exact: bool = True                     # False: units beyond 64 (f64 values no f32 holds): the invariant only
    extra: dict = field(default_factory=dict)

    @property
    def nnz(self):
        return int(self.units.size)

    @property
    def weights(self):
        w = np.ldexp(self.units.astype(np.float64), self.j)
        if self.negzero is not None:
            w[self.negzero] = -0.0
        return w

    @property
    def ptr(self):
        return np.arange(0, self.m * self.row_len + 1, self.row_len, dtype=np.int32) if self.indptr is None else self.indptr

    def dtypes(self):
        if not self.exact:
            return ['f64']
        top = int(np.abs(self.units).max(initial=1)) or 1
        fits = self.j + top.bit_length() <= 128
        out = ['f64']
        if fits and self.j >= -149:
            out.append('f32')                                  # (down to the subnormals: multiples of 2^-149)
        if fits and self.j >= -126:
            out.append('bf16')
        if F16_J[0] <= self.j <= F16_J[1]:
            out.append('f16')
        return out

    def col_units(self):
        s = np.zeros(self.k, np.int64)
        np.add.at(s, self.indices, np.abs(self.units))
        return s

    def check_exact(self):
        """The generator's claim: ``|n| <= 64``, ``sum_c |n| < 2^24`` over every column, every index in [0, k)."""
        assert self.indices.size == self.units.size and (self.indices.size == 0 or (0 <= self.indices.min() and self.indices.max() < self.k))
        assert int(self.ptr[-1]) == self.nnz and len(self.ptr) == self.m + 1, self.name
        if self.exact:
            assert np.abs(self.units).max(initial=0) <= MAX_UNITS, self.name
            top = int(self.col_units().max(initial=0))
            assert top < EXACT_SUM, (self.name, top)
            return top
        return None

    def stats(self):
        """What the sources reduce, in the formats they reduce it in (exact cases: every figure is exact)."""
        w = self.weights
        a32 = np.abs(w.astype(np.float32))
        colsum = np.zeros(self.k, np.float64)
        np.add.at(colsum, self.indices, a32.astype(np.float64))
        count = np.bincount(self.indices, minlength=self.k)
        nz = a32[a32 > 0]
        live = count > 0
        with np.errstate(over='ignore'):
            cs32 = colsum.astype(np.float32)
        mean = (cs32[live] / count[live].astype(np.float32)) if live.any() else np.zeros(0, np.float32)
        return {'colsum_max': float(cs32.max(initial=0.0)), 'wmax': float(a32.max(initial=0.0)),
                'wmin': float(nz.min()) if nz.size else None, 'colmax_min': column_max_min(a32, self.indices, self.k),
                'mean_min': float(mean.min()) if mean.size else float('inf'), 'a32': a32}

    def entry(self, has_indices=True, min_bits=16, keep=None):
        s = self.stats()
        return entry_rule(s['colsum_max'], s['wmax'], s['wmin'], s['colmax_min'], self.nnz, has_indices, min_bits, keep)

    def plan(self, min_bits=16, keep=None, split=False):
        """`split`: per-entry f64 weights are stored as (hi, lo) f32 pairs on the same column: twice the entries; for an exact
        case every lo is zero."""
        a32 = self.stats()['a32']
        if split:
            w = self.weights
            hi = w.astype(np.float32)
            lo = (w - hi.astype(np.float64)).astype(np.float32)
            return plan_rule(np.stack([hi, lo], 1).reshape(-1), np.repeat(self.indices, 2), self.k, 2 * self.nnz, min_bits, keep)
        return plan_rule(a32, self.indices, self.k, self.nnz, min_bits, keep)

    def steps(self, min_bits=16, keep=None):
        s = self.stats()
        return steps_rule(s['colsum_max'], s['mean_min'], s['wmax'], s['wmin'], s['colmax_min'], self.nnz, min_bits, keep)

    def reference(self):
        """Dense f64 product with every row active: the signed column sums (exact: multiples of q below 2^24 q)."""
        out = np.zeros(self.k, np.float64)
        np.add.at(out, self.indices, self.weights)
        return out


def true_bound_holds(case, e):
    """The invariant, in integers: ``max_c sum_c |w| * 2^e < 2^62`` with the sums taken as exact multiples of the case's quantum."""
    top = max((int(x) for x in case.col_units()), default=0)
    return Fraction(top) * Fraction(2) ** (case.j + int(e)) < (1 << 62)


def _finish(name, m, k, units, j, rows_cols, *, row_len=-1, negzero=None, exact=True, extra=None):
    """`rows_cols`: the columns row by row (a list of arrays), or one flat array with `row_len`."""
    if row_len >= 0:
        indices, indptr = np.ascontiguousarray(rows_cols, np.int32).reshape(-1), None
    else:
        indices = np.concatenate([np.asarray(r, np.int32) for r in rows_cols] + [np.zeros(0, np.int32)]).astype(np.int32)
        indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows_cols])]).astype(np.int32)
    c = Case(name, m, k, np.ascontiguousarray(units, np.int64), j, indices, indptr, row_len, negzero, exact, extra or {})
    c.check_exact()
    for a in (c.units, c.indices, c.indptr, c.negzero):
        if a is not None:
            a.setflags(write=False)
    return c


def crossing_units(pu, j=0):
    """(N, N + 1): the two neighbours of the 1.001 crossing under 2^pu units — ``f64(N q) * 1.001 < 2^(pu + j) <= f64((N + 1) q) *
    1.001`` as the entry pass evaluates it (q = 2^-6, pu = 16: 65470 and 65471)."""
    n = int((1 << pu) / C['margin'])
    while frexp_exp(math.ldexp(float(n + 1), j) * C['margin']) <= pu + j:
        n += 1
    while frexp_exp(math.ldexp(float(n), j) * C['margin']) > pu + j:
        n -= 1
    return n, n + 1


# --- the boundary structure: k = 1000 in two slices of 512 columns, m = 1025 rows, the heavy column H = 900
K, H, SLICE_SHIFT, SLICE_WIDTH, M = 1000, 900, 9, 512, PLAN_ROW_TRIP + 1
DUP, PASS_ROW_ENTRIES, SPECIAL_SLOTS = 40, 300, 1 + 40 + 1 + 1 + 1
PU = 12
WHERE = ('pow2', 'below', 'cross-lo', 'cross-hi')
SIGNS = ('pos', 'neg', 'mixed')
SCALES = (-20, -6, 0, 12)


def heavy_units(where, pu=PU, j=0):
    lo, hi = crossing_units(pu, j)
    return {'pow2': 1 << pu, 'below': (1 << pu) - 1, 'cross-lo': lo, 'cross-hi': hi}[where]


def boundary_case(name, n_heavy, signs, j, seed=0, filler_units=(2, 3)):
    """The heaviest column sum is exactly ``n_heavy`` units, and column H is reached a different way in every row that holds it, so a
    decode slip in k_plan_colstats SPLITS the sum (it cannot move it whole to another column):
      row 0     H as the first entry of the row, in front of lower columns (the raw order is not the sorted one);
      row 1     H listed DUP times in one row;
      row 2     H behind a gap of 385 columns inside its slice: a d8 escape chain;
      row 3     H behind PASS_ROW_ENTRIES entries of its slice: a block of more than 256 items, H in the second 64-lane pass;
      row 1024  H alone in the last row: the second trip of the wave loop (m = 1025);
      rows 4 ...  H listed DUP times per row until ``n_heavy`` is reached (every entry 1 ... 64 units).
    Rows 40 ... 200 hold 0 ... 6 filler entries of 2 or 3 units on other columns; every other row is empty."""
    rng = np.random.default_rng(seed)
    n_slots = max(SPECIAL_SLOTS, -(-n_heavy // MAX_UNITS))
    assert n_heavy >= n_slots
    base, rem = divmod(n_heavy, n_slots)
    slots = np.full(n_slots, base, np.int64)
    slots[:rem] += 1
    assert slots.max() <= MAX_UNITS and slots.min() >= 1 and int(slots.sum()) == n_heavy
    sgn = {'pos': lambda n: np.ones(n, np.int64), 'neg': lambda n: -np.ones(n, np.int64),
           'mixed': lambda n: rng.choice(np.asarray([-1, 1], np.int64), n)}[signs]
    slots = slots * (np.where(np.arange(n_slots) % 2 == 0, 1, -1) if signs == 'mixed' else sgn(n_slots))
    fill = lambda n: rng.choice(np.asarray(filler_units, np.int64), n) * sgn(n)
    others = lambda n, lo, hi: rng.integers(lo, hi, n).astype(np.int32)          # H = 900 lies outside every range used
    rows = [np.zeros(0, np.int32) for _ in range(M)]
    units = [np.zeros(0, np.int64) for _ in range(M)]
    it = iter(range(n_slots))
    take = lambda n: slots[[next(it) for _ in range(n)]]
    rows[0], units[0] = np.asarray([H, 3, 600, 20], np.int32), np.concatenate([take(1), fill(3)])
    rows[1], units[1] = np.concatenate([np.full(DUP, H, np.int32), [5, 700]]), np.concatenate([take(DUP), fill(2)])
    rows[2], units[2] = np.asarray([100, 515, H], np.int32), np.concatenate([fill(2), take(1)])
    rows[3], units[3] = np.concatenate([others(PASS_ROW_ENTRIES, 512, H), [H]]), np.concatenate([fill(PASS_ROW_ENTRIES), take(1)])
    rows[M - 1], units[M - 1] = np.asarray([H], np.int32), take(1)
    left, r = n_slots - SPECIAL_SLOTS, 4
    while left > 0:
        n = min(DUP, left)
        rows[r], units[r] = np.concatenate([[7], np.full(n, H, np.int32)]).astype(np.int32), np.concatenate([fill(1), take(n)])
        left, r = left - n, r + 1
    assert r <= 40
    for r in range(40, 201):
        n = int(rng.integers(0, 7))
        rows[r] = np.where(rng.random(n) < 0.5, others(n, 0, H), others(n, H + 1, K)).astype(np.int32)
        units[r] = fill(n)
    c = _finish(name, M, K, np.concatenate(units), j, rows, extra={'heavy': n_heavy, 'signs': signs})
    cu = c.col_units()
    assert int(cu[H]) == n_heavy and int(np.delete(cu, H).max()) < n_heavy // 4
    return c


CASES = {}


def _register_boundaries():
    for where in WHERE:
        for signs in SIGNS:
            for j in SCALES:
                name = f'edge-{where}-{signs}-j{j}'
                CASES[name] = functools.partial(boundary_case, name, heavy_units(where, PU, j), signs, j, seed=len(CASES))
    name = 'edge-cross-hi-pos-pu16'        # the crossing of the issue's example: 65471 / 64 under 2^10
    CASES[name] = functools.partial(boundary_case, name, crossing_units(16, -6)[1], 'pos', -6, seed=99)


_register_boundaries()


def boundary_cases(where=None, signs=None, j=None):
    return [n for n in CASES if n.startswith('edge-') and (where is None or f'-{where}-' in n) and
            (signs is None or f'-{signs}-' in n) and (j is None or n.endswith(f'-j{j}'))]


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASES[name]()
    assert c.name == name
    return c


# --- gate edges: the threshold 2^(min_bits - e) is GATE_T units; the heavy column holds 3/4 * 2^pu units, so e = 62 - pu - j
GATE_T = 2
GATE_VARIANTS = ('wmin-at', 'wmin-below', 'colmax-below', 'mean-pass', 'mean-fail')


def gate_case(variant, pu, j=0, k=8):
    """Column 0 holds ``3/4 * 2^pu`` units (outside the 1.001 band) in entries of 64, listed row by row.  The other columns, in units:
      wmin-at       {2}, {2, 3}: the smallest weight sits exactly at the threshold — the cheap test passes, no second pass;
      wmin-below    {1, 2}: one quantum below — the column maxima decide, the smallest of them (2) exactly at the threshold;
      colmax-below  {1}: a column whose largest weight is below the threshold — RANGE at `need`, and at any `keep` below it;
      mean-pass     {1, 3}: wmin fails, the column's mean (2) passes: source 3 decides without the entry pass;
      mean-fail     {1, 2}, {1, 2, 2}: mean 1.5 / 1.67 fails, the maximum 2 passes: the entry pass decides.
    ``min_bits = gate_min_bits(pu)`` puts the threshold at GATE_T units."""
    tails = {'wmin-at': [[2], [2, 3]], 'wmin-below': [[1, 2]], 'colmax-below': [[1], [2, 2]], 'mean-pass': [[1, 3]],
             'mean-fail': [[1, 2], [1, 2, 2]]}[variant]
    n_heavy = 3 << (pu - 2)
    hu = np.full(n_heavy // MAX_UNITS, MAX_UNITS, np.int64)
    per_row = 8192                                             # rows of at most 8192 entries (the d8 layout sorts up to 16384)
    rows = [np.zeros(min(per_row, hu.size - s), np.int32) for s in range(0, hu.size, per_row)]
    units = [hu]
    for c, t in enumerate(tails, start=2):
        rows.append(np.full(len(t), c, np.int32))
        units.append(np.asarray(t, np.int64))
    case = _finish(f'gate-{variant}-pu{pu}-j{j}', len(rows), k, np.concatenate(units), j, rows, extra={'pu': pu})
    assert case.entry(min_bits=0) == C['headroom'] - pu - j
    return case


def gate_min_bits(pu):
    """min_bits with ``2^(min_bits - e) == GATE_T`` units at ``e = 62 - pu - j``."""
    return C['headroom'] - pu + (GATE_T.bit_length() - 1)


GATE_PU_ENTRY, GATE_PU_PLAN = PU, 23      # min_bits 51 (the entry pass takes up to 60) and 40 (the plan's limit)


# --- degenerate cases and clamps
def small_case(name, m, k, units, j, rows, **kw):
    return _finish(name, m, k, np.asarray(units, np.int64), j, [np.asarray(r, np.int32) for r in rows], **kw)


def degenerate_cases():
    z = np.zeros(5, bool)
    z[[1, 3]] = True
    return [
        small_case('all-zero', 3, 6, [0, 0, 0, 0, 0], 0, [[0, 2], [2], [5, 1]]),
        small_case('neg-zero', 3, 6, [0, 0, 0, 0, 0], 0, [[0, 2], [2], [5, 1]], negzero=z),
        small_case('zero-among', 3, 6, [0, 5, 0, -7, 0], -3, [[0, 2], [2], [2, 1]], negzero=z & False),
        small_case('one-entry', 1, 6, [-37], 4, [[4]]),
        small_case('k-is-1', 4, 1, [3, -64, 9, 1, 1], -2, [[0], [0, 0], [], [0, 0]]),
    ]


def clamp_case():
    """Weights of 2^-120 (normal in f32 and bf16): need = 62 + 117 clamps to 150."""
    return small_case('clamp-hi', 3, 6, [1, -1, 1, 1], -120, [[0, 2], [2], [2]])


def subnormal_case():
    """Every weight an f32 subnormal (n * 2^-140): whether the device's global float atomicAdd flushes them is recorded, not
    assumed — the case asserts a refusal or an exponent that holds the invariant (150 does, whatever the sums became)."""
    return small_case('all-subnormal', 3, 6, [3, -5, 64, 1], -140, [[0, 2], [2], [2]])


def overflow_case():
    """Four weights of 2^126 in one column: the f32 column sum is +inf."""
    return small_case('colsum-overflows', 4, 6, [1, 1, -1, 1, 1], 126, [[2, 0], [2], [2], [2]])


def wide_f64_case():
    """f64 weights no f32 holds (41 significant bits): the f32 sums round, so only the invariant is asserted."""
    units = np.asarray([(1 << 40) + 1, -((1 << 40) - 3), (1 << 39) + 5, 12345678901, 1], np.int64)
    return small_case('f64-wide', 3, 6, units, -30, [[2, 0], [2, 2], [1]], exact=False)


# --- past one trip of the capped grids
def big_nnz_case():
    """nnz = 256 * 16 * 256 + 257: the last 257 entries lie on the second trip of the entry passes' grid.  The heavy column (0)
    holds 2^14 - 1 units, 57 x 64 of them among those last entries: a pass that stops after one trip sees 12735 units and
    returns an exponent one higher.  The fillers put 1 unit each on columns 1 ... 4095."""
    nnz, k = ENTRY_TRIP + 257, 4096
    rng = np.random.default_rng(7)
    idx = rng.integers(1, k, nnz).astype(np.int32)
    units = np.ones(nnz, np.int64) * rng.choice(np.asarray([-1, 1], np.int64), nnz)
    n_heavy, tail = (1 << 14) - 1, 57
    head = -(-(n_heavy - tail * MAX_UNITS) // MAX_UNITS)
    pos = np.concatenate([np.arange(1000, 1000 + head), np.arange(nnz - tail, nnz)])
    u = np.full(head + tail, MAX_UNITS, np.int64)
    u[0] -= int(u.sum()) - n_heavy
    idx[pos], units[pos] = 0, u
    m = 1024
    lens = np.full(m, nnz // m, np.int64)
    lens[-1] += nnz - int(lens.sum())
    rows = np.split(idx, np.cumsum(lens)[:-1])
    c = _finish('big-nnz', m, k, units, 0, rows, extra={'tail_units': tail * MAX_UNITS})
    assert 1 <= u[0] <= MAX_UNITS and int(c.col_units()[0]) == n_heavy and pos[head] >= ENTRY_TRIP
    lost = float(n_heavy - tail * MAX_UNITS)
    assert frexp_exp(lost * C['margin']) < frexp_exp(float(n_heavy) * C['margin'])       # losing the second trip moves the exponent
    return c


def big_k_case(which):
    """k = 1024 * 256 + 1: column k - 1 lies on the second trip of k_fp_reduce.  `sum`: it holds the largest column sum
    (2^12 - 1 units against 2^10 elsewhere); `max`: the heavy column holds 3/4 * 2^12 units and column k - 1 the smallest column maximum — 1 unit, under the threshold of
    `gate_min_bits(PU)` while every other column passes: RANGE, where a reduce that stops after one trip answers."""
    k = REDUCE_TRIP + 1
    if which == 'sum':
        rows = [np.full(64, k - 1, np.int32), np.full(16, 5, np.int32), np.asarray([k - 2, 0, 77], np.int32)]
        units = np.concatenate([np.full(63, 64), [63], np.full(16, 64), [2, 3, 2]]).astype(np.int64)
    else:
        rows = [np.full(48, 5, np.int32), np.asarray([k - 1, 0, 77], np.int32)]
        units = np.concatenate([np.full(48, 64), [1, 2, 3]]).astype(np.int64)
    return _finish(f'big-k-{which}', len(rows), k, units, 0, rows)


# --- fixed-length rows for the binned steps: the boundary structure's heavy column inside rows of one length
def fixed_rows_case(where, signs, j, row_len=8, m=600, k=K):
    rng = np.random.default_rng(len(where) + len(signs) + j)
    n_heavy = heavy_units(where, PU, j)
    idx = rng.integers(0, H, (m, row_len)).astype(np.int32)
    sg = {'pos': 1, 'neg': -1}.get(signs)
    units = rng.choice(np.asarray([2, 3], np.int64), (m, row_len)) * (sg if sg else rng.choice(np.asarray([-1, 1], np.int64), (m, row_len)))
    n_slots = -(-n_heavy // MAX_UNITS) + 1
    base, rem = divmod(n_heavy, n_slots)
    slots = np.full(n_slots, base, np.int64)
    slots[:rem] += 1
    flat_pos = rng.choice(m * row_len, n_slots, replace=False)
    idx.reshape(-1)[flat_pos] = H
    units.reshape(-1)[flat_pos] = slots * (sg if sg else np.where(np.arange(n_slots) % 2 == 0, 1, -1))
    c = _finish(f'fixed-{where}-{signs}-j{j}', m, k, units.reshape(-1), j, idx, row_len=row_len, extra={'heavy': n_heavy})
    cu = c.col_units()
    assert int(cu[H]) == n_heavy and int(np.delete(cu, H).max()) < n_heavy // 4
    return c
