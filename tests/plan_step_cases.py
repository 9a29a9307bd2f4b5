"""The planned scatter *step* (csrc/be_csr_plan.hip: the accumulate kernels, the table gathers, the reduce, the single-launch kernel and
the host's choice among them) restated in numpy — shared by tests/test_plan_step_exact_gpu.py and
tests/test_plan_step_thresholds_cpu.py (which ties CONSTS to the source text and the restated sizes to the library's host functions).
numpy only: nothing here needs a device.

The host's choice.  `cap_of`, `lds_slots_of`, `lds_bytes`, `plan_variant_of`, `fused_region_of`, `plan_active_stride`,
`plan_dense_seg_bytes`, `workspace_bytes` and `workspace_bytes_for` restate the host functions of the same names from CONSTS alone;
`instance_of` restates `plan_step::be_binary_csrmm_t_plan` at default settings (none of BE_PLAN_FUSED, BE_PLAN_PREGATHER_SLICES,
BE_PLAN_PREGATHER_MAX set) and names the kernels a call launches.

The ledger.  ALL_INSTANCES is what the source instantiates: 40 k_plan_accumulate + 16 _d8 + 4 _h8, the four ways a step comes by
its table (none, k_gather_seg over the compacted list, k_compact_gather_seg<1>, <2>), 8 k_plan_reduce, 24 k_plan_single.  REACHABLE is
what `instance_of` returns over a sweep of its arguments.  Compiled but never launched at default settings, because FUSED 3 (the
pre-gathered table) needs ``block_hint <= 64`` and these decoders are chosen above it:
  k_plan_accumulate<true, 32, 3>       counted u16 at 32 lanes        (hints 97 ... 210)
  k_plan_accumulate<true, 0, 3>        counted u16 by the wave        (hints > 210)
  k_plan_accumulate<false, 0, 3>       weighted u16 by the wave       (hints > 96)
  k_plan_accumulate_d8<0, 3, BE_BLOCK_AUX>   d8 by the wave with the cache policy (hints >= 160)

Exactness.  Per-entry weights are ``n / 64`` with integer ``|n| <= 64``, both signs (exact in f32, f16 and bf16); one shared weight
is a small positive integer, or 1.5.  `Case.check_exact(e)` asserts ``64 * sum |w| < 2^24`` over every output column and every batch
row, that ``2^e * w`` is an integer for every stored weight and that ``2^e * sum |w| < 2^62``.  Then
  * fixed_from_f32 rounds nothing: ``t = w * 2^(e - 32)`` is a product with a power of two, ``floor(t)`` fits an int, ``t - floor(t)``
    is exact and its product with 2^32 is the integer ``2^e w - 2^32 floor(t)``;
  * the 64-bit sums in LDS, the partial sums and sum_parts wrap nowhere and are exact in any order; counted entries are integers;
  * ``(double)(long long)sum * 2^-e`` is exact: the sum is ``2^(e - 6)`` times an integer below 2^24;
  * store_d rounds once to the output dtype (through f32, which holds the value exactly); a count times the shared weight is an
    integer (or a multiple of 1/2) below 2^24 in f32, rounded once.
f64 weights are stored as two f32 entries (`split_f64`): their weights carry a second dyadic term ``t * 2^-40``, below the 24 bits of
the first, so ``hi = n / 64`` and ``lo = t * 2^-40`` exactly; the integer condition bounds the exponent from below (e >= 40), and the
case asserts ``2^40 * sum |w| < 2^53`` instead, so the f64 reference and the conversion of the sum are exact.
So every comparison of the GPU module is an equality with `Case.reference`: dense f64 accumulation with ``np.add.at`` over the active
rows, cast once (numpy for f32, f16 and f64; torch on the CPU for bf16).  tests/binned_cases.py argues the same way for the binned
route.

Plans from the host.  `plan_layout_cases.encode` states ``seg`` and the defined bytes of every block; `blob_of` lays them out at the
``seg`` starts into a poisoned blob.  The step then runs on blocks the host wrote, at SCALE_EXP.  The crafted rows of `sorted_matrix`
(escape runs at chosen item positions, a first local column above 0, blocks of exactly LPB, LPB + 1, 64 and 65 lane-groups) become
crafted blocks through the same encoder."""
import functools
import itertools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import plan_layout_cases as L

# ---------------------------------------------------------------------------------------------------------------------------
# what the cases are sized by (tests/test_plan_step_thresholds_cpu.py holds every entry to the source)
# ---------------------------------------------------------------------------------------------------------------------------
CONSTS = {
    'u16c.lpb4': 18,                 # kSub4MaxBlock: counted u16, 4 lanes per block up to this hint
    'u16c.lpb8': 43,                 # kSub8MaxBlock
    'u16c.lpb16': 96,                # kSub16MaxBlock
    'u16c.lpb32': 210,               # kSub32MaxBlock
    'u16w.lpb4': 7,                  # kSubW4MaxBlock: weighted u16
    'u16w.lpb8': 18,                 # kSubW8MaxBlock
    'u16w.lpb16': 43,                # kSubW16MaxBlock
    'u16w.lpb32': 96,                # kSubW32MaxBlock
    'd8.lpb8': 18,                   # kD8EighthMaxBlock
    'd8.lpb16': 43,                  # kD8QuarterMaxBlock
    'd8.nt_min': 160,                # kD8NtMinBlock: d8 by the wave loads with BE_BLOCK_AUX from this hint
    'd8.block_aux': 2,               # BE_BLOCK_AUX
    'pregather.max_block': 64,       # kPreGatherMaxBlock
    'pregather.min_slices': 40,      # kPreGatherMinSlices
    'pregather.max_bytes': 8 << 30,  # plan_dense_seg_bytes: no table above 8 GiB
    'fused.min_list': 2048,          # kFusedMinList
    'single.chunk': 4096,            # kSingleChunk
    'single.lds_extra': 64,          # the single-launch kernel's static LDS besides its list
    'list.stripe': 1024,             # rows per stripe (fused_region_of)
    'list.words': 1024,              # words per iteration of build_part_list
    'rows.batch': 64,                # rows a wave of PlanRows takes per batch
    'rows.waves': 16,                # waves of an accumulate workgroup (1024 threads)
    'lds.cap_ids': 32768,            # ceiling of lds_cap
    'lds.bytes': 160 * 1024,         # the LDS budget
    'lds.reserve': 1024,             # ... less this for the static arrays of the fused step
    'gather.grid': 512,              # workgroups of k_gather_seg
    'gather.tile': 64,               # rows (and slices) per tile
    'compact.rows': 4096,            # rows per workgroup of k_compact_gather_seg (256 threads x 16)
    'reduce.grid': 2048,             # grid cap of k_plan_reduce
    'reduce.grid_batch': 256,        # ... for batches
    'reduce.batch_from': 8,          # ... of this many rows
    'reduce.threads': 256,
    'sum.unroll': 8,                 # loads in flight in sum_parts
    'd8.max_width': 20000,           # kD8MaxWidth
    'h8.max_width': 40000,           # kH8MaxWidth
    'active.extra': 64 * 1024 + 1024,    # ids plan_active_stride adds to m
}
C = CONSTS

KINDS = ('u16w', 'u16c', 'd8', 'h8')
KIND = {('u16', False): 'u16w', ('u16', True): 'u16c', ('d8', False): 'd8', ('h8', True): 'h8'}
LAYOUT_OF = {'u16w': ('u16', False), 'u16c': ('u16', True), 'd8': ('d8', False), 'h8': ('h8', True)}
LAYOUT_CODE = {'u16': 0, 'd8': 1, 'h8': 2}                       # BE_PLAN_U16 / _D8 / _H8
SINGLE_LAYOUT = {'u16w': 0, 'u16c': 1, 'd8': 2, 'h8': 3}         # k_plan_single's LAYOUT
WDTYPES = ('f32', 'f64', 'f16', 'bf16')
SPIKES = ('bool', 'float', 'bits')
SCALE_EXP = 30                      # what the host-encoded calls pass (module docstring: any e >= 6 with 2^e sum |w| < 2^62)
SCALE_EXP_F64 = 46                  # ... with the second dyadic term of the f64 cases (e >= 40)
F64_FRAC = 40


def align_up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------------------------------------------------------
# the host's sizes, restated
# ---------------------------------------------------------------------------------------------------------------------------
def width_of(slice_shift, slice_width):
    return slice_width if slice_width > 0 else 1 << slice_shift


def n_slices_of(k, slice_shift, slice_width=0):
    return -(-k // width_of(slice_shift, slice_width))


def cap_of(slice_shift, slice_width, layout, homo):
    """Accumulators per task = stride of a task's partial sums."""
    w = width_of(slice_shift, slice_width)
    if layout == 'd8':
        return (w + 1) & ~1
    if layout == 'h8':
        return (w + 3) & ~3
    return (w + 3) & ~3 if homo else (w + 1) & ~1


def lds_slots_of(slice_shift, slice_width, layout, homo):
    return 1 << slice_shift if layout == 'u16' else cap_of(slice_shift, slice_width, layout, homo)


def lds_bytes(slice_shift, slice_width, layout, homo):
    return ((lds_slots_of(slice_shift, slice_width, layout, homo) + 1) * (4 if homo else 8) + 15) & ~15


def lds_cap_of(slice_shift, slice_width, layout, homo):
    """Row ids the fused step's list holds in LDS (0: the step does not fuse)."""
    lds = lds_bytes(slice_shift, slice_width, layout, homo)
    if lds + C['lds.reserve'] > C['lds.bytes']:
        return 0
    room = C['lds.bytes'] - C['lds.reserve'] - lds
    return min(room // 4, C['lds.cap_ids']) if room >= C['fused.min_list'] * 4 else 0


def hint_classes(kind):
    """lanes per block (and, d8 by the wave, the cache policy) -> (first, last) hint that selects it; last None: no upper end.
    Hint 0 (unknown) selects the wave per block without the policy."""
    if kind == 'h8':
        return {(0, 0): (1, None)}
    if kind == 'd8':
        return {(8, 0): (1, C['d8.lpb8']), (16, 0): (C['d8.lpb8'] + 1, C['d8.lpb16']),
                (0, 0): (C['d8.lpb16'] + 1, C['d8.nt_min'] - 1), (0, C['d8.block_aux']): (C['d8.nt_min'], None)}
    t = [C[f'{kind}.lpb{n}'] for n in (4, 8, 16, 32)]
    return {(4, 0): (1, t[0]), (8, 0): (t[0] + 1, t[1]), (16, 0): (t[1] + 1, t[2]), (32, 0): (t[2] + 1, t[3]), (0, 0): (t[3] + 1, None)}


def plan_variant_of(layout, homo, block_hint):
    """(lanes per block, AUX)."""
    def upto(max_block):
        return 0 < block_hint <= max_block
    if layout == 'h8':
        return 0, 0
    if layout == 'd8':
        if upto(C['d8.lpb8']):
            return 8, 0
        if upto(C['d8.lpb16']):
            return 16, 0
        return 0, C['d8.block_aux'] if block_hint >= C['d8.nt_min'] else 0
    kind = 'u16c' if homo else 'u16w'
    for n in (4, 8, 16, 32):
        if upto(C[f'{kind}.lpb{n}']):
            return n, 0
    return 0, 0


def fused_region_of(m, parts):
    n_stripes = (((m + 31) >> 5) + 31) >> 5
    return -(-n_stripes // parts) * C['list.stripe']


def counts_bytes(n_batch):
    return align_up(n_batch * 4, 256)


def plan_active_stride(m):
    return align_up((m + C['active.extra']) * 4, 256) // 4


def plan_dense_seg_bytes(m, n_slices, n_batch):
    nbytes = n_slices * plan_active_stride(m) * 8
    ok = n_batch == 1 and n_slices >= max(C['pregather.min_slices'], 2) and nbytes <= C['pregather.max_bytes']
    return align_up(nbytes, 256) if ok else 0


def workspace_bytes(m, k, n_batch, slice_shift, slice_width, parts, homo):
    ns = n_slices_of(k, slice_shift, slice_width)
    task = max(1 << slice_shift, (width_of(slice_shift, slice_width) + 3) & ~3)
    return counts_bytes(n_batch) + n_batch * plan_active_stride(m) * 4 + align_up(n_batch * ns * parts * task * (4 if homo else 8), 256)


def workspace_bytes_for(m, k, n_batch, slice_shift, slice_width, parts, homo, block_hint):
    base = workspace_bytes(m, k, n_batch, slice_shift, slice_width, parts, homo)
    pre = 0 < block_hint <= C['pregather.max_block']
    return base + (plan_dense_seg_bytes(m, n_slices_of(k, slice_shift, slice_width), n_batch) if pre else 0)


def partial_bytes(k, n_batch, slice_shift, slice_width, parts, layout, homo):
    """What the accumulate kernels of a call write behind the active lists."""
    return n_batch * n_slices_of(k, slice_shift, slice_width) * parts * cap_of(slice_shift, slice_width, layout, homo) * (4 if homo else 8)


# ---------------------------------------------------------------------------------------------------------------------------
# the host's choice, restated
# ---------------------------------------------------------------------------------------------------------------------------
def fused_of(layout, homo, n_slices, n_batch, m, spike_dtype, spikes_aligned16, block_hint, slice_shift, slice_width, workspace_has_table):
    fused = 0
    if lds_cap_of(slice_shift, slice_width, layout, homo) > 0:
        if spike_dtype == 'bits':
            fused = 1
        elif spike_dtype == 'bool' and spikes_aligned16 and (n_batch == 1 or m % 16 == 0):
            fused = 2
    if plan_dense_seg_bytes(m, n_slices, n_batch) > 0 and 0 < block_hint <= C['pregather.max_block'] and workspace_has_table:
        fused = 3
    return fused


def instance_of(layout, homo, wdtype, n_slices, parts, n_batch, m, spike_dtype, spikes_aligned16, block_hint, slice_shift, slice_width,
                workspace_has_table):
    """The kernels ``be_binary_csrmm_t_plan`` launches for these arguments at default settings:
    ``('single', LAYOUT, SP, W)`` or ``('sliced', table form, ('acc', kind, LPB, FUSED, AUX), ('reduce', W, HOMO))`` with the table
    form one of 'none', 'list' (k_gather_seg over the compacted list), 'compact1', 'compact2' (k_compact_gather_seg<1 | 2>)."""
    assert (layout, bool(homo)) in KIND and wdtype in WDTYPES and spike_dtype in SPIKES
    homo = bool(homo)
    kind = KIND[(layout, homo)]
    lds = lds_bytes(slice_shift, slice_width, layout, homo)
    assert lds <= C['lds.bytes'], 'the step refuses this slice'
    if n_slices == 1 and parts == 1 and n_batch == 1 and wdtype != 'f64' and spike_dtype in ('bool', 'float') and \
            lds + C['single.chunk'] * 4 + C['single.lds_extra'] <= C['lds.bytes']:
        return 'single', SINGLE_LAYOUT[kind], spike_dtype, wdtype
    fused = fused_of(layout, homo, n_slices, n_batch, m, spike_dtype, spikes_aligned16, block_hint, slice_shift, slice_width,
                     workspace_has_table)
    form = 'none'
    if fused == 3:
        form = 'compact1' if spike_dtype == 'bits' else 'compact2' if (spike_dtype == 'bool' and spikes_aligned16) else 'list'
    lpb, aux = plan_variant_of(layout, homo, block_hint)
    return 'sliced', form, ('acc', kind, lpb, fused, aux), ('reduce', wdtype, homo)


def _all_instances():
    acc = {('acc', kind, lpb, fused, 0) for kind in ('u16w', 'u16c') for lpb in (0, 4, 8, 16, 32) for fused in range(4)}
    acc |= {('acc', 'd8', lpb, fused, aux) for lpb, aux in ((0, 0), (0, C['d8.block_aux']), (8, 0), (16, 0)) for fused in range(4)}
    acc |= {('acc', 'h8', 0, fused, 0) for fused in range(4)}
    assert len(acc) == 40 + 16 + 4
    forms = {('table', f) for f in ('none', 'list', 'compact1', 'compact2')}
    red = {('reduce', w, h) for w in WDTYPES for h in (False, True)}
    single = {('single', lay, sp, w) for lay in range(4) for sp in ('bool', 'float') for w in ('f32', 'f16', 'bf16')}
    assert len(red) == 8 and len(single) == 24
    return acc | forms | red | single


ALL_INSTANCES = frozenset(_all_instances())


def parts_of_instance(inst):
    """The ledger entries an `instance_of` result stands for."""
    if inst[0] == 'single':
        return {inst}
    _, form, acc, red = inst
    return {('table', form), acc, red}


@functools.lru_cache(None)
def _reachable():
    out = set()
    hints = sorted({0, 100000} | {h + d for kind in KINDS for lo, hi in hint_classes(kind).values() for h in (lo, hi or lo) for d in (0, 1)}
                   | {C['pregather.max_block'], C['pregather.max_block'] + 1})
    for kind in KINDS:
        layout, homo = LAYOUT_OF[kind]
        for (ns, width, shift), (parts, nb), m, wd, sp, al, hint, table in itertools.product(
                ((1, 60, 6), (2, 60, 6), (40, 60, 6)), ((1, 1), (2, 1), (1, 3)), (600, 608), WDTYPES, SPIKES, (False, True), hints,
                (False, True)):
            out |= parts_of_instance(instance_of(layout, homo, wd, ns, parts, nb, m, sp, al, hint, shift, width, table))
    return frozenset(out)


def reachable():
    return _reachable()


# ---------------------------------------------------------------------------------------------------------------------------
# matrices (built once, shared, read-only)
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class Matrix:
    """Rows of columns with per-entry weights in units of 1/64 (``units``, non-zero integers in [-64, 64]) and the geometry the plan
    of every layout it serves is cut by.  ``zero_col``: a column whose entries, all in always-active rows, sum to zero."""
    name: str
    m: int
    k: int
    slice_shift: int
    slice_width: int
    indices: np.ndarray
    indptr: np.ndarray
    units: np.ndarray
    kinds: tuple = KINDS
    zero_col: Optional[int] = None
    always: tuple = ()                     # rows every non-trivial spike pattern keeps active
    frac: Optional[np.ndarray] = None      # f64 cases: the second dyadic term, integers t of t * 2^-40
    note: dict = field(default_factory=dict)

    @property
    def n_slices(self):
        return n_slices_of(self.k, self.slice_shift, self.slice_width)

    @property
    def rows_of_entries(self):
        return np.repeat(np.arange(self.m), np.diff(self.indptr.astype(np.int64)))

    def weights(self):
        """f64 values of the per-entry weights."""
        w = self.units / 64.0
        return w if self.frac is None else w + np.ldexp(self.frac.astype(np.float64), -F64_FRAC)

    @functools.lru_cache(None)
    def encoded(self, kind) -> L.Encoded:
        assert kind in self.kinds
        w = self.weights().astype(np.float32)
        assert self.frac is not None or np.array_equal(w.astype(np.float64), self.weights())
        return L.encode(kind, w, self.indices, self.indptr, self.m, self.k, self.slice_shift, self.slice_width)


def blob_of(enc: L.Encoded, poison=0xA5) -> np.ndarray:
    """The blocks of `enc` at their ``seg`` starts; every byte no block defines (the padding to 128 and the 128 spare bytes the
    library allocates behind the last block) is ``poison``."""
    blob = np.full(enc.units * 128 + 128, poison, np.uint8)
    start = enc.seg.reshape(-1, 2)[:, 0].astype(np.int64) * 128
    at = np.repeat(start - enc.byte_off, enc.nbytes) + np.arange(enc.data.size, dtype=np.int64)
    assert at.size == 0 or at.max() < enc.units * 128
    blob[at] = enc.data
    return blob


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False


def _finish(name, m, k, shift, width, rows, rng, kinds=KINDS, zero=None, always=(), note=None, frac=False):
    """rows: list of int arrays of columns.  ``zero`` = (column, row a, row b): the column is cleared everywhere else, row a gets it
    twice at +32/64, row b once at -64/64."""
    rows = [np.asarray(r, np.int64).reshape(-1) for r in rows]
    forced = {}
    if zero is not None:
        c0, ra, rb = zero
        other = c0 + 1 if (c0 + 1) % width else c0 - 1
        rows = [np.where(r == c0, other, r) for r in rows]
        forced = {ra: (np.array([c0, c0]), np.array([32, 32])), rb: (np.array([c0]), np.array([-64]))}
    idx, units, lens = [], [], []
    for r, cols in enumerate(rows):
        u = rng.integers(1, 65, cols.size) * rng.choice([-1, 1], cols.size)
        if r in forced:
            at = int(rng.integers(0, cols.size + 1))
            cols = np.concatenate([cols[:at], forced[r][0], cols[at:]])
            u = np.concatenate([u[:at], forced[r][1], u[at:]])
        idx.append(cols)
        units.append(u)
        lens.append(cols.size)
    idx = np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)
    units = np.concatenate(units).astype(np.int64) if units else np.zeros(0, np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    fr = None
    if frac:
        fr = rng.integers(-1000, 1001, units.size).astype(np.int64)
    _freeze(idx, units, ptr, fr)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < k)
    return Matrix(name, m, k, shift, width, idx, ptr, units, tuple(kinds), None if zero is None else zero[0],
                  tuple(always) + (() if zero is None else (zero[1], zero[2])), fr, note or {})


DEC_SLICES = 40


@functools.lru_cache(None)
def u16_matrix():
    """40 slices of 60 columns at slice_shift 6 (pads go to slot 64 > the width), rows of 0 ... 40 entries, every 17th empty, a tenth
    with 300 ... 1100 more entries (duplicate columns) inside one slice: blocks past a 64-lane pass in both u16 layouts."""
    rng = np.random.default_rng(600)
    m, width = 600, 60
    k = DEC_SLICES * width
    long_rows = np.flatnonzero(rng.random(m) < 0.1)
    long_rows = long_rows[(long_rows % 17 != 0) & (long_rows > 2)]
    rows = []
    for r in range(m):
        cols = rng.integers(0, k, int(rng.integers(0, 41))) if r % 17 else np.zeros(0, np.int64)
        if r in long_rows:
            n = 1100 if r == long_rows[0] else int(rng.integers(300, 701))
            cols = np.concatenate([cols, int(rng.integers(0, k // width)) * width + rng.integers(0, width, n)])
            rng.shuffle(cols)
        rows.append(cols)
    return _finish('u16', m, k, 6, width, rows, rng, ('u16w', 'u16c'), zero=(7, 1, 2), always=tuple(long_rows[:4]))


SORTED_WIDTH = 1000
#: lane-groups of the crafted blocks: every LPB and LPB + 1 of a sub-wave decoder, 64, 65 and two full passes and a bit
CRAFTED_GROUPS = (4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130)
#: (lane-groups, lane-group the escape run starts in, escapes): inside the first 8, straddling the 8th | 9th, the 16th | 17th and the
#: 64th | 65th lane-group (the run's first escape is the last item of one lane-group, its second the first item of the next)
CRAFTED_ESCAPES = ((20, 3, 1), (20, 7, 2), (40, 15, 2), (70, 63, 2), (70, 66, 3))


def crafted_block(kind, groups, esc_group=None, escapes=0, base=5, pads=0):
    """Local columns of a block of exactly `groups` lane-groups (less `pads` tail pads): duplicates and steps of one from `base`, and,
    with `escapes`, one gap bridged by that many escape items of which the first is the LAST item of lane-group `esc_group`."""
    G = L.GROUP[kind]
    items = groups * G - pads
    n = items - escapes                                # stored entries
    step = (np.arange(n) % 8 == 1).astype(np.int64)     # 0, 1, 0, 0, ...: duplicate columns and neighbours
    step[0] = 0
    if escapes:
        e = esc_group * G + G - 1                       # item position of the first escape = index of the entry behind the run
        assert 0 < e < n
        step[e] = 255 * escapes + (3 if kind == 'd8' else 0)       # h8: a gap of exactly 255 x escapes ends in code 0
    cols = base + np.cumsum(step)
    assert cols[-1] < SORTED_WIDTH
    return cols


@functools.lru_cache(None)
def sorted_matrix():
    """40 slices of 1000 columns for d8 and h8: random short rows, every 17th empty, random long rows (300 ... 700 entries in one slice)
    and the crafted rows, one crafted block each, at a first local column of 5."""
    rng = np.random.default_rng(601)
    m, width = 400, SORTED_WIDTH
    k = DEC_SLICES * width
    rows = []
    crafted = {}
    specs = [(g, None, 0) for g in CRAFTED_GROUPS] + list(CRAFTED_ESCAPES)
    for r in range(m):
        cols = rng.integers(0, k, int(rng.integers(0, 41))) if r % 17 else np.zeros(0, np.int64)
        rows.append(cols)
    free = [r for r in range(3, m) if r % 17]
    at = 0
    for kind in ('d8', 'h8'):
        for g, eg, ne in specs:
            r = free[at]
            at += 1
            s = int(rng.integers(1, DEC_SLICES))
            blk = crafted_block(kind, g, eg, ne, pads=3 if g % 2 else 0)
            keep = rows[r][rows[r] // width != s]
            cols = np.concatenate([keep, s * width + blk])
            rng.shuffle(cols)
            rows[r] = cols
            crafted[(kind, g, eg, ne)] = (r, s)
    for r in free[at:at + 12]:
        s = int(rng.integers(0, DEC_SLICES))
        cols = np.concatenate([rows[r], s * width + rng.integers(0, width, int(rng.integers(300, 701)))])
        rng.shuffle(cols)
        rows[r] = cols
    always = tuple(sorted({r for r, _ in crafted.values()}))
    return _finish('sorted', m, k, 6, width, rows, rng, ('d8', 'h8'), zero=(7, 1, 2), always=always, note={'crafted': crafted})


def _short_rows(rng, m, k, lo, hi, empty_every=17):
    return [rng.integers(0, k, int(rng.integers(lo, hi + 1))) if (empty_every == 0 or r % empty_every) else np.zeros(0, np.int64)
            for r in range(m)]


@functools.lru_cache(None)
def small_matrix(m, n_slices, width=60, ragged=True, no_empty_row=False):
    """A few slices of `width` columns (the last one narrower when `ragged`), rows of 0 ... 12 entries (1 ... 12 with `no_empty_row`)
    and one long row."""
    rng = np.random.default_rng(700 + m + n_slices + width)
    k = n_slices * width - (7 if ragged and n_slices > 1 else 0)
    rows = _short_rows(rng, m, k, 1, 12, empty_every=0) if no_empty_row else _short_rows(rng, m, k, 0, 12)
    if m > 5:
        rows[5] = rng.integers(0, min(k, width), 600)
    return _finish(f'small-{m}-{n_slices}-{width}{"-dense" if no_empty_row else ""}', m, k, 6 if width <= 64 else 4, width, rows, rng,
                   KINDS if width <= 64 else ('d8', 'h8'), always=(5,) if m > 5 else ())


@functools.lru_cache(None)
def two_entry_matrix(m, n_slices, width=60, ragged=False):
    """Two entries per row (a row is empty every 17th): many rows, few blocks — what the loops over rows and positions need."""
    rng = np.random.default_rng(800 + m + n_slices)
    k = n_slices * width - (13 if ragged else 0)
    rows = _short_rows(rng, m, k, 2, 2)
    return _finish(f'two-{m}-{n_slices}-{width}', m, k, 6 if width <= 64 else 4, width, rows, rng, KINDS if width <= 64 else ('d8', 'h8'))


def wide_width(kind, target_ids):
    """The widest slice of a d8 / h8 plan that still leaves `target_ids` row ids of LDS to the fused step's list — derived from the
    restated LDS arithmetic."""
    layout, homo = LAYOUT_OF[kind]
    w = C['d8.max_width'] if kind == 'd8' else C['h8.max_width']
    while lds_cap_of(4, w, layout, homo) < target_ids:
        w -= 1
    return w - 1          # (an odd width below the widest: the partial-sum stride exceeds it)


LIST_CAP_TARGET = 2560


@functools.lru_cache(None)
def list_matrix(kind, parts):
    """build_part_list past one iteration: m just past 32 x 1024 x parts rows (not a multiple of 32 or 16), two wide slices (the
    second narrower) whose accumulators leave a list of ~2560 ids to LDS.  One or two entries per row."""
    rng = np.random.default_rng(900 + parts)
    width = wide_width(kind, LIST_CAP_TARGET)
    m = 32 * C['list.stripe'] * parts + C['list.stripe'] + 37
    k = 2 * width - 11
    rows = _short_rows(rng, m, k, 1, 2, empty_every=0)
    return _finish(f'list-{kind}-{parts}', m, k, 4, width, rows, rng, (kind,))


@functools.lru_cache(None)
def reduce_matrix(kind, k):
    """The reduce's column loop: k outputs in the widest slices of d8 / h8 less one (odd: the partial-sum stride exceeds the width; the
    last slice is narrower), a few entries per row."""
    rng = np.random.default_rng(1000 + k)
    width = (C['d8.max_width'] if kind == 'd8' else C['h8.max_width']) - 1
    m = 200
    rows = _short_rows(rng, m, k, 0, 10)
    rows[3] = np.array([0, 1, k - 1, k - 2, width - 1, width, width + 1, k - 1])
    return _finish(f'reduce-{kind}-{k}', m, k, 4, width, rows, rng, (kind,), always=(3,))


@functools.lru_cache(None)
def single_matrix():
    """One slice of 50 columns, 2 x 4096 + 1 rows of 0 ... 3 entries and two long rows (past a 64-lane pass in every layout); the
    matrices of fewer rows are its first rows."""
    rng = np.random.default_rng(1100)
    m, k = 2 * C['single.chunk'] + 1, 50
    rows = _short_rows(rng, m, k, 0, 3)
    rows[0] = rng.integers(0, k, 5)
    rows[4094] = rng.integers(0, k, 700)
    rows[4096] = rng.integers(0, k, 530)
    return _finish('single', m, k, 6, 50, rows, rng)


@functools.lru_cache(None)
def head_of(matrix: Matrix, m: int) -> Matrix:
    """The first m rows."""
    n = int(matrix.indptr[m])
    idx, ptr, units = matrix.indices[:n].copy(), matrix.indptr[:m + 1].copy(), matrix.units[:n].copy()
    _freeze(idx, ptr, units)
    return Matrix(f'{matrix.name}[:{m}]', m, matrix.k, matrix.slice_shift, matrix.slice_width, idx, ptr, units, matrix.kinds,
                  None, tuple(r for r in matrix.always if r < m))


@functools.lru_cache(None)
def f64_matrix():
    """Three slices, per-entry weights ``n / 64 + t * 2^-40``."""
    rng = np.random.default_rng(1200)
    m, width = 300, 60
    k = 3 * width - 7
    rows = _short_rows(rng, m, k, 0, 12)
    rows[5] = rng.integers(0, width, 300)
    return _finish('f64', m, k, 6, width, rows, rng, ('u16w', 'd8'), always=(5,), frac=True)


# ---------------------------------------------------------------------------------------------------------------------------
# spike patterns
# ---------------------------------------------------------------------------------------------------------------------------
def pattern(matrix: Matrix, name: str, n_batch: int = 1, seed: int = 0) -> np.ndarray:
    """bool [n_batch, m].  'half' / 'tenth': random; 'all'; 'none'; 'silent-row': random with batch row 1 silent;
    'tail-heavy:<a>:<b>': every a-th of the rows up to the last multiple of 32 x 1024 and every b-th of the rest; 'hole': nothing in the first
    compact.rows rows, everything behind them."""
    m = matrix.m
    rng = np.random.default_rng(1 + seed)
    if name == 'all':
        v = np.ones((n_batch, m), bool)
    elif name == 'none':
        v = np.zeros((n_batch, m), bool)
    elif name in ('half', 'tenth', 'silent-row'):
        v = rng.random((n_batch, m)) < (0.1 if name == 'tenth' else 0.5)
        for r in matrix.always:
            v[:, r] = True
        if name == 'silent-row':
            v[1 % n_batch] = False
    elif name.startswith('tail-heavy'):
        a, b = (int(x) for x in name.split(':')[1:])
        cut = m - m % (32 * C['list.stripe'])              # the rows behind the parts' first iteration of build_part_list
        v = np.zeros((n_batch, m), bool)
        v[:, :cut:a] = True
        v[:, cut::b] = True
    elif name == 'hole':
        v = np.ones((n_batch, m), bool)
        v[:, :C['compact.rows']] = False
    else:
        raise KeyError(name)
    v.flags.writeable = False
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# a case: one matrix in one layout, one call shape
# ---------------------------------------------------------------------------------------------------------------------------
NP_DTYPE = {'f32': np.float32, 'f16': np.float16, 'f64': np.float64}


@dataclass(frozen=True)
class Case:
    """One call of the step: a matrix in one layout, the spikes' encoding and pattern, the batch, the parts, the hint, the output
    dtype and whether the workspace has room for the pre-gathered table.  ``shared`` is the one weight of the counted layouts."""
    id: str
    matrix: Matrix
    kind: str
    spikes: str = 'bits'                   # 'bits' | 'float' | 'bool' (16-byte aligned) | 'bool_off' (one byte off)
    pat: str = 'half'
    n_batch: int = 1
    parts: int = 3
    hint: int = 100000
    wdtype: str = 'f32'
    table: bool = True
    shared: float = 3.0
    want: tuple = ()                       # ledger entries the case is for (asserted against instance_of)
    trips: tuple = ()                      # (name of the loop, trips it reaches, trips it has to reach)

    @property
    def layout(self):
        return LAYOUT_OF[self.kind][0]

    @property
    def homo(self):
        return LAYOUT_OF[self.kind][1]

    @property
    def spike_dtype(self):
        return 'bool' if self.spikes.startswith('bool') else self.spikes

    @property
    def aligned_by_design(self):
        return self.spikes != 'bool_off'

    def active(self, step=0):
        """bool [n_batch, m] of step 0 (the case's pattern), step 1 (another draw) and step 2 (nothing)."""
        if step == 0:
            return pattern(self.matrix, self.pat, self.n_batch)
        return pattern(self.matrix, 'none' if step == 2 else 'half', self.n_batch, seed=17 * step)

    def instance(self, aligned16=None):
        mx = self.matrix
        al = self.aligned_by_design if aligned16 is None else aligned16
        return instance_of(self.layout, self.homo, self.wdtype, mx.n_slices, self.parts, self.n_batch, mx.m, self.spike_dtype, al,
                           self.hint, mx.slice_shift, mx.slice_width, self.table)

    def ws_args(self):
        mx = self.matrix
        return mx.m, mx.k, self.n_batch, mx.slice_shift, mx.slice_width, self.parts, int(self.homo)

    def ws_bytes(self):
        return workspace_bytes_for(*self.ws_args(), self.hint) if self.table else workspace_bytes(*self.ws_args())

    def entry_weights(self):
        return np.full(self.matrix.indices.size, self.shared) if self.homo else self.matrix.weights()

    def scale_exp(self):
        return SCALE_EXP_F64 if self.matrix.frac is not None else SCALE_EXP

    def min_exp(self):
        """The smallest exponent at which 2^e w is an integer for every stored weight."""
        return 0 if self.homo else (F64_FRAC if self.matrix.frac is not None else 6)

    def sums(self, spikes):
        """f64 [n_batch, k] of the signed sums and of the sums of |w|."""
        mx = self.matrix
        rows, w = mx.rows_of_entries, self.entry_weights()
        out = np.zeros((spikes.shape[0], mx.k), np.float64)
        mag = np.zeros_like(out)
        for b in range(spikes.shape[0]):
            sel = spikes[b][rows]
            np.add.at(out[b], mx.indices[sel], w[sel])
            np.add.at(mag[b], mx.indices[sel], np.abs(w[sel]))
        return out, mag

    def reference(self, spikes=None):
        """[n_batch, k] in the output dtype (a torch tensor for bf16)."""
        out, _ = self.sums(self.active(0) if spikes is None else np.atleast_2d(spikes))
        if self.wdtype == 'bf16':
            import torch
            return torch.from_numpy(out).to(torch.bfloat16)
        return out.astype(NP_DTYPE[self.wdtype])

    def check_exact(self, scale_exp=None):
        """The conditions of the module docstring, at the exponent the call passes."""
        e = self.scale_exp() if scale_exp is None else int(scale_exp)
        mx = self.matrix
        assert self.kind in mx.kinds
        if self.homo:
            assert self.shared > 0 and self.shared * 2 == int(self.shared * 2) and self.shared <= 8
        else:
            assert e >= self.min_exp()
            w = mx.weights()
            scaled = np.ldexp(w, e)
            assert np.array_equal(scaled, np.round(scaled)), 'a stored weight is no integer at this exponent'
            assert (mx.units != 0).all() and (np.abs(mx.units) <= 64).all()
        for step in (0, 1):
            out, mag = self.sums(self.active(step))
            if mx.frac is None:
                assert 64 * mag.max(initial=0) < 2 ** 24
            else:
                assert self.wdtype == 'f64' and 2.0 ** F64_FRAC * mag.max(initial=0) < 2 ** 53
            if not self.homo:
                assert np.ldexp(mag.max(initial=0), e) < 2 ** 62, 'the 64-bit sums could wrap'
            if self.wdtype == 'f16':
                assert np.abs(out).max(initial=0) < 65504
        if mx.zero_col is not None and not self.homo and self.pat in ('half', 'tenth', 'all', 'silent-row'):
            out, mag = self.sums(self.active(0))
            b = 0
            assert out[b, mx.zero_col] == 0.0 and mag[b, mx.zero_col] == 2.0, 'the zero-sum column'
        return True


# ---------------------------------------------------------------------------------------------------------------------------
# the case tables (the GPU module's parametrisation: both test modules iterate these)
# ---------------------------------------------------------------------------------------------------------------------------
def _hint_ends(kind, cls, fused3):
    lo, hi = hint_classes(kind)[cls]
    hi = 100000 if hi is None else hi
    if fused3:
        hi = min(hi, C['pregather.max_block'])
        if lo > hi:
            return None
    return lo, hi


def _decoder_matrix(kind):
    return u16_matrix() if kind.startswith('u16') else sorted_matrix()


def _decoder_cases():
    """One or more cases per accumulate instance `instance_of` can name: every LPB class of each layout by the hints at both ends of
    its range, FUSED 0 (float spikes; a bool buffer one byte off alignment), 1, 2 and 3 through each of its table forms; each as a
    vector, and FUSED 0 ... 2 as a 3-row batch too (a batch never gets a table)."""
    out = []
    for kind in KINDS:
        mx = _decoder_matrix(kind)
        for cls in hint_classes(kind):
            lpb, aux = cls
            for fused in range(4):
                ends = _hint_ends(kind, cls, fused == 3)
                if ends is None:
                    continue
                lo, hi = ends
                want = (('acc', kind, lpb, fused, aux),)
                # a hint <= 64 on 40 slices takes the table whenever the workspace has room for it: FUSED 0 ... 2 then run on the
                # smaller workspace (`table=False`), as a caller that sized it with ..._workspace_bytes does
                forms = {0: (('float', lo), ('bool_off', hi)), 1: (('bits', lo), ('bits', hi)), 2: (('bool', lo), ('bool', hi)),
                         3: (('float', lo), ('bits', hi), ('bool', lo), ('bool_off', hi))}[fused]
                for sp, hint in dict.fromkeys(forms):
                    out.append(Case(f'{kind}-lpb{lpb}-aux{aux}-fused{fused}-{sp}-hint{hint}', mx, kind, sp, 'half', 1, 3, hint,
                                    table=fused == 3, shared=1.5 if (kind, lpb, fused) in (('u16c', 8, 1), ('h8', 0, 2)) else 3.0, want=want))
                if fused < 3:
                    m16 = mx.m % 16 == 0
                    sp = {0: 'float', 1: 'bits', 2: 'bool'}[fused]
                    if fused == 2 and not m16:
                        continue             # (a batch of bool rows with m % 16 != 0 is compacted: the batch cases below)
                    out.append(Case(f'{kind}-lpb{lpb}-aux{aux}-fused{fused}-{sp}-batch3-hint{hi}', mx, kind, sp, 'half', 3, 3, hi,
                                    table=False, want=want))
    return out


def _skeleton_cases():
    out = []
    # tasks: n_slices * parts below 8, equal to 8 and 8 j + 1 — idle workgroups next to working ones
    for kind in KINDS:
        for ns, parts in ((2, 3), (2, 4), (3, 3), (3, 11)):
            out.append(Case(f'tasks-{kind}-{ns}x{parts}', small_matrix(300, ns), kind, 'bits', 'half', 1, parts, 30))
    # every arm of sum_parts' switch and two full rounds of 8, both accumulator types
    for kind in ('u16w', 'h8'):
        for parts in (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 64):
            rounds = parts // C['sum.unroll']
            # (FUSED 0: list position p belongs to part p % parts, so every part holds rows; the in-kernel lists deal stripes of 1024
            # rows, which would leave all but part 0 of these 300 rows empty — and a lost term of sum_parts unseen)
            out.append(Case(f'parts-{kind}-{parts}', small_matrix(300, 2, no_empty_row=True), kind, 'bool_off' if parts % 2 else 'float', 'half', 1, parts, 30,
                            trips=(('sum_parts rounds of 8', rounds, 2),) if parts in (16, 64) else ()))
    # the pointer pipeline: more rows in a part than 3 x 16 x 64
    per_pass = C['rows.waves'] * C['rows.batch']
    mx = two_entry_matrix(12 * C['list.stripe'] + 6, DEC_SLICES)
    for kind, parts in (('u16w', 3), ('u16c', 4), ('d8', 3), ('h8', 4)):
        for sp, table, hint in (('float', False, 8), ('bits', False, 8), ('bool', False, 8), ('bits', True, 8), ('float', True, 8)):
            if kind in ('d8', 'h8'):
                mxk = two_entry_matrix(12 * C['list.stripe'] + 6, DEC_SLICES, SORTED_WIDTH)
            else:
                mxk = mx
            fused = fused_of(*LAYOUT_OF[kind], DEC_SLICES, 1, mxk.m, 'bool' if sp == 'bool' else sp, True, hint, mxk.slice_shift,
                             mxk.slice_width, table)
            stripes = -(-mxk.m // C['list.stripe'])
            rows_in_part0 = {0: -(-mxk.m // parts), 3: -(-mxk.m // parts)}.get(
                fused, min(mxk.m, sum(min(C['list.stripe'], mxk.m - s * C['list.stripe']) for s in range(0, stripes, parts))))
            out.append(Case(f'pipeline-{kind}-{sp}-{"table" if table else "plain"}-parts{parts}', mxk, kind, sp, 'all', 1, parts, hint,
                            table=table, trips=((f'PlanRows batches (FUSED {fused})', -(-rows_in_part0 // per_pass), 4),)))
    # build_part_list: a second iteration; a list that outgrows LDS in the first; one that fits the first and outgrows in the second
    for kind, parts, sp, pat in (('d8', 1, 'bits', 'tail-heavy:40:40'), ('d8', 1, 'bool', 'tail-heavy:4:4'),
                                 ('d8', 1, 'bits', 'tail-heavy:16:1'), ('d8', 1, 'bool', 'tail-heavy:16:1'),
                                 ('d8', 2, 'bits', 'tail-heavy:16:1'), ('h8', 1, 'bool', 'tail-heavy:4:4'),
                                 ('h8', 1, 'bits', 'tail-heavy:16:1')):
        mxl = list_matrix(kind, parts)
        n_stripes = -(-(-(-mxl.m // 32)) // 32)
        words = -(-n_stripes // parts) * 32
        out.append(Case(f'list-{kind}-parts{parts}-{sp}-{pat}', mxl, kind, sp, pat, 1, parts, 100000,
                        trips=(('build_part_list iterations', -(-words // C['list.words']), 2),)))
    # k_gather_seg: 65 and 130 slices, more than 512 x 64 listed rows, a last tile of fewer than 64
    g_rows = C['gather.grid'] * C['gather.tile']
    mxg = two_entry_matrix(g_rows + C['gather.tile'] + 7, 65, ragged=True)
    out.append(Case('gather-65-slices-grid-stride', mxg, 'u16c', 'float', 'all', 1, 2, 8,
                    trips=(('k_gather_seg tiles per workgroup', -(-(-(-mxg.m // C['gather.tile'])) // C['gather.grid']), 2),
                           ('gather_tile s0 trips', -(-65 // C['gather.tile']), 2))))
    mxg2 = two_entry_matrix(200, 130, ragged=True)
    for kind in ('u16w', 'u16c'):
        out.append(Case(f'gather-130-slices-{kind}', mxg2, kind, 'float', 'half', 1, 1, 8,
                        trips=(('gather_tile s0 trips', -(-130 // C['gather.tile']), 3),)))
    out.append(Case('gather-130-slices-bool-off', mxg2, 'u16w', 'bool_off', 'half', 1, 2, 8,
                    trips=(('gather_tile s0 trips', -(-130 // C['gather.tile']), 3),)))
    # k_compact_gather_seg<1 | 2>: m below, at and past 4096 rows per workgroup; a workgroup without a spike; all; none
    R = C['compact.rows']
    for m in (R - 6, R, 2 * R + 5):
        mxc = two_entry_matrix(m, DEC_SLICES)
        for sp in ('bits', 'bool'):
            for pat in ('tenth', 'all', 'none') + (('hole',) if m > R else ()):
                out.append(Case(f'compact-{sp}-m{m}-{pat}', mxc, 'u16w', sp, pat, 1, 2, 8,
                                trips=(('k_compact_gather_seg workgroups', -(-m // R), 3),) if m > R else ()))
    out.append(Case('compact-130-slices-bits', mxg2, 'u16c', 'bits', 'half', 1, 2, 8))
    # the reduce's column loop: every W for both HOMO, a vector and a batch of 8
    kv = C['reduce.grid'] * C['reduce.threads'] + 3
    kb = C['reduce.grid_batch'] * C['reduce.threads'] + 3
    for kind in ('d8', 'h8'):
        for wd in WDTYPES:
            out.append(Case(f'reduce-vector-{kind}-{wd}', reduce_matrix(kind, kv), kind, 'bits', 'half', 1, 2, 100000, wd,
                            trips=(('k_plan_reduce column trips', -(-(-(-kv // C['reduce.threads'])) // C['reduce.grid']), 2),)))
            out.append(Case(f'reduce-batch8-{kind}-{wd}', reduce_matrix(kind, kb), kind, 'bits', 'half', C['reduce.batch_from'], 1, 100000, wd,
                            trips=(('k_plan_reduce column trips', -(-(-(-kb // C['reduce.threads'])) // C['reduce.grid_batch']), 2),)))
    # u16: a width that is no multiple of 4 (counted) or 2 (weighted): the partial-sum stride exceeds it; a narrower last slice
    for kind in ('u16w', 'u16c'):
        for wd in WDTYPES:
            out.append(Case(f'reduce-odd-width-{kind}-{wd}', small_matrix(300, 3, 61), kind, 'bool', 'half', 1, 2, 30, wd))
    # batches
    for kind in KINDS:
        for nb in (2, 3, 8):
            out.append(Case(f'batch{nb}-{kind}-silent-row-bits', small_matrix(301, 3), kind, 'bits', 'silent-row', nb, 2, 30))
        out.append(Case(f'batch3-{kind}-bool-unaligned-m', small_matrix(301, 3), kind, 'bool', 'half', 3, 2, 30,
                        want=(('acc', kind) + plan_variant_of(*LAYOUT_OF[kind], 30)[:1] + (0,) + plan_variant_of(*LAYOUT_OF[kind], 30)[1:],)))
        out.append(Case(f'batch3-{kind}-bool-aligned-m', small_matrix(304, 3), kind, 'bool', 'silent-row', 3, 2, 30,
                        want=(('acc', kind) + plan_variant_of(*LAYOUT_OF[kind], 30)[:1] + (2,) + plan_variant_of(*LAYOUT_OF[kind], 30)[1:],)))
    return out


def _single_cases():
    """All 24 k_plan_single instances; each runs m in SINGLE_M with no, some and all rows active."""
    out = []
    for kind in KINDS:
        for sp in ('bool', 'float'):
            for wd in ('f32', 'f16', 'bf16'):
                out.append(Case(f'single-{kind}-{sp}-{wd}', single_matrix(), kind, sp, 'tenth', 1, 1, 100000, wd,
                                want=(('single', SINGLE_LAYOUT[kind], sp, wd),)))
    return out


SINGLE_M = (1, C['single.chunk'] - 1, C['single.chunk'], C['single.chunk'] + 1, 2 * C['single.chunk'] + 1)


def _f64_cases():
    """f64 through ScatterPlan.build: per-entry weights split in two f32 entries, and one shared f64 weight — on the sliced path, and
    what would be the single-launch shape (one slice, one part, bool spikes), which f64 does not take."""
    out = []
    for kind in ('u16w', 'd8'):
        out.append(Case(f'f64-weighted-{kind}', f64_matrix(), kind, 'bits', 'half', 1, 2, 30, 'f64', want=(('reduce', 'f64', False),)))
    for kind in ('u16c', 'h8'):
        out.append(Case(f'f64-shared-{kind}', small_matrix(300, 3), kind, 'bool', 'half', 1, 2, 30, 'f64', shared=1.5,
                        want=(('reduce', 'f64', True),)))
    out.append(Case('f64-one-slice-takes-the-sliced-path', head_of(single_matrix(), 300), 'u16w', 'bool', 'half', 1, 1, 30, 'f64',
                    want=(('reduce', 'f64', False),)))
    return out


def _library_cases():
    """Plans from ScatterPlan.build at the library's exponent, through _plan_call."""
    out = []
    for kind in KINDS:
        for sp, hint in (('bits', 100000), ('float', 8)):
            out.append(Case(f'library-{kind}-{sp}-hint{hint}', _decoder_matrix(kind), kind, sp, 'half', 1, 3, hint))
    return out


@functools.lru_cache(None)
def tables():
    t = {'decoder': _decoder_cases(), 'skeleton': _skeleton_cases(), 'single': _single_cases(), 'f64': _f64_cases(),
         'library': _library_cases()}
    ids = [c.id for cases in t.values() for c in cases]
    assert len(ids) == len(set(ids))
    return t


def all_cases():
    return [c for cases in tables().values() for c in cases]


def covered():
    """The union of the ledger entries of every call the GPU module makes (by design alignment: the GPU module asserts the real
    one gives the same instance)."""
    out = set()
    for c in all_cases():
        if c.id.startswith('single-'):
            for m in SINGLE_M:
                out |= parts_of_instance(Case(c.id, head_of(c.matrix, m), c.kind, c.spikes, c.pat, 1, 1, c.hint, c.wdtype).instance())
        else:
            out |= parts_of_instance(c.instance())
    return out


REACHABLE = reachable()
