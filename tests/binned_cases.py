"""The binned scatter route (csrc/be_csr_binned.hip) restated in numpy — shared by tests/test_binned_kernels_exact_gpu.py and
tests/test_binned_kernels_thresholds_cpu.py (which ties CONSTS to the source text and the restated geometry to the library's
host functions).  numpy only: nothing here needs a device.

The geometry.  `stream_cap`, `geometry`, `geometry_batch`, `cap_blocks`, `parts` and `workspace_bytes` restate the host functions
of the same names from CONSTS alone; `class_bounds` derives from them the bin counts at which pass B's block size changes.

Exactness.  Per-entry weights are ``n / 64`` with integer ``|n| <= 64`` (exact in f32, f16 and bf16), one shared weight is a small
integer.  Every case asserts ``64 * sum |w| < 2^24`` over every output column (`Case.check_exact`), so every partial sum of a
column, in any order, is a multiple of 1/64 below 2^18: exact in f32.  Then
  * the 64-bit sums are exact: fixed_from_f32 splits ``w * 2^e`` into floor and fraction without rounding when ``w * 2^e`` is an
    integer, i.e. for every exponent ``e >= 6`` (the direct calls pass SCALE_EXP[0]; the library derives far larger ones);
  * the 32-bit sums are exact for the same reason (``__float2int_rn`` of an integer), and ``2^e * sum |w| < 2^31`` at SCALE_EXP[2];
  * the float atomics of the overflow image and of the merge of a bin's parts add exactly;
  * an f16 / bf16 output is the exact f32 value rounded once.
So every comparison of the GPU module is an equality with `Case.reference`: dense f64 accumulation with ``np.add.at``, cast once.
tests/delay_cases.py (`exact_case`) argues the same way for the delayed products."""
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------
# what the cases are sized by (tests/test_binned_kernels_thresholds_cpu.py holds every entry to the source)
# ---------------------------------------------------------------------------------------------------------------------------
CONSTS = {
    'lds.bytes': 160 * 1024,             # the LDS budget of pass B and pass C
    'stream.margin': 512,                # ... less this margin in pass B
    'stream.waves': 16,                  # kStreamWaves
    'stream.threads': 1024,              # BE_STREAM_THREADS
    'fixed.table_words': 64 * 2 + 66 + 64,   # kStreamWl per wave: row starts (int64), prefix sums, row lengths
    'fixed.list_words': 128,             # kStreamFixedWords: a wave's flush list
    'fixed.ticket_words': 12,            # ... the task ticket and three conservation sums
    'fixed.dummy_words': 256,            # ... the dummies
    'fixed.align_words': 4,              # ... the blocks start 16-byte aligned
    'ring': 2,                           # kRing (BE_RING)
    'per_bin.entry_bytes_weighted': 6,   # stream_cap: bytes of an entry with a weight of its own
    'per_bin.entry_bytes_counted': 2,    # ... of a counted entry
    'per_bin.words_bytes': 8,            # ... ticket + flag
    'per_bin.ring_bytes': 8,             # ... commit count + generation per ring slot
    'cap.largest': 128,                  # stream_cap tries blocks of 128 entries first
    'cap.smallest': 8,                   # ... and gives up below 8
    'max_bins': 2048,                    # kMaxBins
    'stream.grid': 256,                  # kStreamGrid: workgroups of pass B = regions per bin
    'acc.static_bytes': 4 * (256 + 256 + 1 + 16) + 512,   # kAccStaticBytes
    'acc.local_column_max': 65535,       # local columns are uint16
    'geo.small_k': 256 * 256,            # up to this many outputs the bins are 256 columns wide
    'geo.small_width': 256,
    'geo.pow2_shift': 14,                # weighted entries over many outputs: bins of 2^14 columns at most
    'cap_blocks.num': 5,                 # stream_cap_blocks: bin_capacity / kStreamGrid * 5 / 4 + 64 ...
    'cap_blocks.den': 4,
    'cap_blocks.add': 64,
    'cap_blocks.extra': 2,               # ... in blocks, + 2
    'batch.pass': 32,                    # batch rows per pass at most
    'batch.floor_weighted': 16,          # ... as long as pass B keeps blocks of this many weighted entries
    'batch.floor_counted': 32,           # ... counted entries
    'batch.capacity_add': 64,            # batch_bin_capacity
    'short_row': 256,                    # kShortRow
    'task.rows_floor': 4,                # kTaskRowsFloor
    'task.groups_cap': 1024,             # kTaskGroupsCap
    'stream.u': 2,                       # BE_STREAM_U
    'bin.u': 4,                          # BE_BIN_U (held to the source for the record: no case is sized by it)
    'parts.total': 256,                  # parts = 256 / n_vbins ...
    'parts.max': 16,                     # ... clipped to [1, 16]
    'audit.off': 256,                    # kBinAuditOff
    'audit.grid_c': 2048,                # kBinAuditGridC
}
C = CONSTS

KINDS = (0, 1, 2)                        # 64-bit sums, one shared weight (counts), 32-bit sums (BE_BINNED_ACC32)
KIND_NAME = {0: 'acc64', 1: 'counted', 2: 'acc32'}
BE_BINNED_ABS, BE_BINNED_SHORT_ROWS = 4, 8
BE_OK, BE_ERR_RANGE = 0, -4
SCALE_EXP = {0: 30, 1: 0, 2: 8}          # what the direct calls pass (module docstring)
HOMO_W = 3.0
CAPS = (128, 64, 32, 16, 8)


def align_up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------------------------------------------------------
# the geometry, restated
# ---------------------------------------------------------------------------------------------------------------------------
def stream_fixed_words():
    return C['stream.waves'] * (C['fixed.table_words'] + C['fixed.list_words']) + C['fixed.ticket_words'] + C['fixed.dummy_words'] + \
        C['fixed.align_words']


def stream_budget():
    return C['lds.bytes'] - C['stream.margin'] - 4 * stream_fixed_words()


def entry_bytes(kind):
    return C['per_bin.entry_bytes_counted'] if kind == 1 else C['per_bin.entry_bytes_weighted']


def acc_bytes(kind):
    return 8 if kind == 0 else 4


def per_bin_bytes(cap, kind):
    return C['ring'] * cap * entry_bytes(kind) + C['per_bin.words_bytes'] + C['per_bin.ring_bytes'] * C['ring']


def stream_cap(n_bins, kind):
    """Entries per write-combining block: the largest the LDS of pass B holds for this many bins (0: none)."""
    cap = C['cap.largest']
    while cap >= C['cap.smallest']:
        if per_bin_bytes(cap, kind) * n_bins <= stream_budget():
            return cap
        cap >>= 1
    return 0


def class_bounds(kind):
    """block size -> (first, last) bin count that gets it, derived from the budget (never written down)."""
    out, first = {}, 1
    for cap in CAPS:
        last = min(stream_budget() // per_bin_bytes(cap, kind), C['max_bins'])
        out[cap] = (first, last)
        first = last + 1
    for cap, (lo, hi) in out.items():
        assert stream_cap(lo, kind) == cap == stream_cap(hi, kind) and (hi == C['max_bins'] or stream_cap(hi + 1, kind) != cap)
    return out


def max_width(slice_shift, kind):
    w = (C['lds.bytes'] - C['acc.static_bytes']) // acc_bytes(kind)
    return min(w, 1 << slice_shift, C['acc.local_column_max']) & ~3


def map_cap_of(width, kind):
    v = C['lds.bytes'] - C['acc.static_bytes'] - ((width * acc_bytes(kind) + 15) & ~15)
    return 0 if v < 0 else v & ~15


def geometry_branch(k, slice_shift, kind):
    max_w = max_width(slice_shift, kind)
    if k <= C['geo.small_k']:
        return 'small'
    if kind == 0 and k > 256 * min(max_w, 1 << C['geo.pow2_shift']):
        return 'pow2'
    return 'rounds'


def geometry(k, slice_shift, kind):
    """(width, n_bins, cap, map_cap) of a single vector; n_bins == 0 past kMaxBins, cap == 0 when pass B's LDS does not hold it."""
    max_w = max_width(slice_shift, kind)
    branch = geometry_branch(k, slice_shift, kind)
    if branch == 'small':
        width = min(C['geo.small_width'], max_w)
    elif branch == 'pow2':
        sh = C['geo.pow2_shift']
        while (1 << sh) > max_w:
            sh -= 1
        width = 1 << sh
    else:
        rounds = (k + 256 * max_w - 1) // (256 * max_w)
        width = ((k + 256 * rounds - 1) // (256 * rounds) + 3) & ~3
    nb = (k + width - 1) // width
    if nb > C['max_bins']:
        return width, 0, 0, 0
    return width, nb, stream_cap(nb, kind), map_cap_of(width, kind)


def bins(k, slice_shift, kind):
    """be_binned_bins."""
    if k <= 0 or not 4 <= slice_shift <= 16:
        return 0
    _, nb, cap, _ = geometry(k, slice_shift, kind)
    return nb if cap > 0 else 0


def geometry_batch(k, slice_shift, kind, n_batch):
    """(width, n_bins per batch row, cap, map_cap, gb): gb batch rows share a pass (gb == 1: the single-vector geometry)."""
    single = geometry(k, slice_shift, kind) + (1,)
    if n_batch <= 1:
        return single
    max_w = max_width(slice_shift, kind)
    nbb = (k + max_w - 1) // max_w
    width = ((k + nbb - 1) // nbb + 3) & ~3
    floor = C['batch.floor_counted'] if kind == 1 else C['batch.floor_weighted']
    gb = min(n_batch, C['batch.pass'])
    while gb > 1 and (nbb * gb > C['max_bins'] or stream_cap(nbb * gb, kind) < floor):
        gb -= 1
    if gb <= 1:
        return single
    return width, nbb, stream_cap(nbb * gb, kind), map_cap_of(width, kind), gb


def batch_bin_capacity(k, slice_shift, kind, bin_capacity, n_batch):
    width, nbb, cap, _, gb = geometry_batch(k, slice_shift, kind, n_batch)
    if gb <= 1:
        return bin_capacity
    n1 = geometry(k, slice_shift, kind)[1]
    c = int(float(bin_capacity) * (n1 if n1 > 0 else 1) / (nbb if nbb > 0 else 1)) + C['batch.capacity_add']
    return min(c, (1 << 31) - 1)


def cap_blocks(bin_capacity, cap):
    per_region = bin_capacity // C['stream.grid'] * C['cap_blocks.num'] // C['cap_blocks.den'] + C['cap_blocks.add']
    return (per_region + cap - 1) // cap + C['cap_blocks.extra']


def parts(n_vbins):
    return max(1, min(C['parts.max'], C['parts.total'] // max(n_vbins, 1)))


def workspace_layout(m, k, n_batch, slice_shift, bin_capacity):
    """binned_ws_layout: byte offsets of the overflow image and of the f32 image behind it, and the total."""
    n_batch = max(1, n_batch)
    blocks_bytes = dir_bytes = 0
    gb_max = 1
    for kind in KINDS:
        width, nbb, cap, _, gb = geometry_batch(k, slice_shift, kind, n_batch)
        if cap == 0:
            continue
        vb = nbb * gb
        cb = cap_blocks(batch_bin_capacity(k, slice_shift, kind, bin_capacity, n_batch), cap)
        blocks_bytes = max(blocks_bytes, vb * C['stream.grid'] * cb * cap * entry_bytes(kind))
        dir_bytes = max(dir_bytes, vb * C['stream.grid'] * 4)
        gb_max = max(gb_max, gb)
    audit_bytes = (3 * C['stream.grid'] + C['audit.grid_c']) * 8
    active = C['audit.off'] + align_up(audit_bytes, 256)
    masks = active + align_up(m * 4, 256)
    dirs = masks + (align_up(m * 4, 256) if n_batch > 1 else 0)
    regions = dirs + align_up(dir_bytes, 256)
    ovf = regions + align_up(blocks_bytes, 256)
    out32 = ovf + align_up(gb_max * k * 4, 256)
    return {'ovf': ovf, 'out32': out32, 'total': out32 + align_up(n_batch * k * 4, 256)}


def workspace_bytes(m, k, n_batch, slice_shift, bin_capacity):
    return workspace_layout(m, k, n_batch, slice_shift, bin_capacity)['total']


def room(bin_capacity, cap):
    """Entries one workgroup of pass B can put into one bin's region before the overflow path takes over."""
    return cap_blocks(bin_capacity, cap) * cap


def task_rows(avg_len, n_active, task_groups, min_tasks):
    """Rows per task of pass B (k_bin_stream's `R`): about `task_groups` groups of four entries, at least task.rows_floor rows
    while those stay within task.groups_cap groups, no fewer than `min_tasks` tasks.  `avg_len`: row_len, or nnz // m of an indptr.
    One row per task means that a lane's group index never leaves row 0 of the task's table: the division by the row's groups
    (`fixdiv`), the search over the prefix sums, the rows' starts past the first and a wave that holds short and long rows at once
    are reached only where this is above 1."""
    g4 = max(1, (avg_len + 3) >> 2)
    rshift = 6
    while rshift > 0 and (g4 << rshift) > task_groups:
        rshift -= 1
    while (1 << rshift) < C['task.rows_floor'] and (g4 << (rshift + 1)) <= C['task.groups_cap']:
        rshift += 1
    while rshift > 0 and (n_active >> rshift) < min_tasks:
        rshift -= 1
    return 1 << rshift


#: be_binned_set_tuning(task_groups, min_tasks) under which the cases below pack several rows into a task (the persisted tuning asks
#: for 2048 tasks at least: with fewer than 4096 active rows every task is ONE row, whatever the case)
PACKED_TUNING = (256, 1)
#: entries a wave of pass B appends per round: 64 lanes x 4 entries x BE_STREAM_U steps
ROUND_ENTRIES = 64 * 4 * C['stream.u']
FLUSH_LIST = 64                          # blocks a wave's flush list holds (one pass of stream_append's flush loop)


# ---------------------------------------------------------------------------------------------------------------------------
# row structures (built once, shared, read-only)
# ---------------------------------------------------------------------------------------------------------------------------
MIXED_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 257)      # 5, 7, 65, 257: the last group of four is partial (the window moves back)
SHORT_RUN = 70                                              # consecutive rows of 1 ... 3 entries: more than one wave of them
# row_len without an indptr: short rows (1, 3), the rows' groups of four a power of two (1, 1, 1, 2 and 64: `fixdiv` is a shift) or not
# (100 -> 25, kShortRow + 1 -> 65: a multiply-high), both sides of kShortRow
FIXED_LENS = (1, 3, 4, 6, 100, C['short_row'], C['short_row'] + 1)


def mixed_lens(seed, reps=6):
    rng = np.random.default_rng(seed)
    lens = np.tile(np.asarray(MIXED_LENS, np.int64), reps)
    rng.shuffle(lens)
    return np.concatenate([lens, rng.integers(1, 4, SHORT_RUN)])


@dataclass
class Case:
    """One matrix, one set of event vectors and the shape the step is called with.  ``weights`` holds f64 values that are exact in
    every weight dtype; ``spikes`` is bool ``[n_batch, m]``."""
    name: str
    m: int
    k: int
    slice_shift: int
    kind: int
    indices: np.ndarray
    indptr: Optional[np.ndarray]           # None: rows of `row_len` entries
    row_len: int
    weights: np.ndarray
    spikes: np.ndarray
    bin_capacity: int
    wdtype: str = 'f32'
    flags: int = 0
    overflow: bool = False                 # sized so that some region overflows (else: sized with room)
    cap: int = 0                           # the block size the case is named for (0: not about the block size)
    note: str = ''
    extra: dict = field(default_factory=dict)

    @property
    def n_batch(self):
        return self.spikes.shape[0]

    @property
    def lens(self):
        return np.full(self.m, self.row_len, np.int64) if self.indptr is None else np.diff(self.indptr.astype(np.int64))

    @property
    def rows_of_entries(self):
        return np.repeat(np.arange(self.m), self.lens)

    def entry_weights(self, absolute=False):
        w = np.broadcast_to(self.weights, self.indices.shape) if self.kind == 1 else self.weights
        return np.abs(w) if absolute or (self.flags & BE_BINNED_ABS) else w

    def reference(self, spikes=None):
        """f64 ``[n_batch, k]``: ``out[b, col(e)] += w_e`` over the entries of the rows active in batch row ``b``; entries with a
        column ``>= k`` are dropped; BE_BINNED_ABS sums ``|w|``."""
        spikes = self.spikes if spikes is None else np.atleast_2d(spikes)
        rows, w = self.rows_of_entries, self.entry_weights()
        out = np.zeros((spikes.shape[0], self.k), np.float64)
        for b in range(spikes.shape[0]):
            sel = spikes[b][rows] & (self.indices < self.k)
            np.add.at(out[b], self.indices[sel], w[sel])
        return out

    def counts(self, spikes=None):
        """(entries in the active rows summed over the batch rows, those among them with a column >= k, those with a column past
        the last bin's end).  Tickets are drawn per bin: a column >= k inside the width of a partial last bin draws one and is
        dropped where the outputs are written; one past the last bin draws none."""
        spikes = self.spikes if spikes is None else np.atleast_2d(spikes)
        rows = self.rows_of_entries
        width, n_bins = self.geometry()[:2]
        n = sum(int(spikes[b][rows].sum()) for b in range(spikes.shape[0]))
        bad = sum(int((spikes[b][rows] & (self.indices >= self.k)).sum()) for b in range(spikes.shape[0]))
        past = sum(int((spikes[b][rows] & (self.indices >= width * n_bins)).sum()) for b in range(spikes.shape[0]))
        return n, bad, past

    def geometry(self):
        return geometry_batch(self.k, self.slice_shift, self.kind, self.n_batch)

    def rows_per_task(self, task_groups, min_tasks, spikes=None):
        """`task_rows` of a step of this case (a batch pass lists the rows active in any of its batch rows: the first pass here)."""
        spikes = self.spikes if spikes is None else np.atleast_2d(spikes)
        gb = self.geometry()[4]
        n_active = int(spikes[:gb].any(axis=0).sum())
        avg = self.row_len if self.indptr is None else max(int(self.indices.size), 0) // self.m
        return task_rows(avg, n_active, task_groups, min_tasks)

    def ws_key(self):
        return self.m, self.k, self.n_batch, self.slice_shift, self.bin_capacity

    def check_exact(self):
        """The generator's claim: weights are multiples of 1/64 (one shared weight: an integer), exact in the weight dtype, and
        ``64 * sum |w| < 2^24`` over every column with EVERY row active — so any subset, in any order, is exact in f32 — and the
        32-bit sums hold it at SCALE_EXP[2]."""
        w = np.asarray(self.weights, np.float64)
        assert np.array_equal(w * 64, np.round(w * 64)) and np.abs(w).max(initial=0) <= (HOMO_W if self.kind == 1 else 1.0)
        if self.kind == 1:
            assert w.size == 1 and w[0] == round(w[0])
        ok = self.indices < self.k
        col_abs = np.zeros(self.k, np.float64)
        np.add.at(col_abs, self.indices[ok], self.entry_weights(absolute=True)[ok])
        top = float(col_abs.max(initial=0.0))                          # (batch rows have outputs of their own)
        assert 64 * top < 2 ** 24, (self.name, top)
        assert top * 2.0 ** SCALE_EXP[2] < 2 ** 31 and top * 2.0 ** SCALE_EXP[0] < 2 ** 62
        assert np.array_equal(col_abs.astype(np.float32).astype(np.float64), col_abs)
        return top


def _ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _weights(rng, n, kind, min_units=0):
    if kind == 1:
        return np.asarray([HOMO_W])
    mag = rng.integers(min_units, 65, n)
    return mag * rng.choice([-1.0, 1.0], n) / 64.0


def _columns(rng, lens, k, lo=0, hi=None, avoid=None):
    """Uniform columns in [lo, hi) (default: all k), outside `avoid = (a, b)`."""
    hi = k if hi is None else hi
    n = int(np.sum(lens))
    if avoid is None:
        return rng.integers(lo, hi, n).astype(np.int32)
    a, b = avoid
    c = rng.integers(lo, hi - (b - a), n)
    return np.where(c >= a, c + (b - a), c).astype(np.int32)


def need_capacity(case_indices, rows, spikes, k, slice_shift, kind):
    """A small `bin_capacity` with which NO region can overflow, however the rows are dealt to the workgroups: a region then
    holds every active entry of its bin (a batch scales the capacity by the bins a batch row loses: batch_bin_capacity)."""
    n_batch = spikes.shape[0]
    width, n_bins, cap, _, gb = geometry_batch(k, slice_shift, kind, n_batch)
    top = 0
    for b in range(n_batch):
        sel = spikes[b][rows] & (case_indices < k)
        if sel.any():
            top = max(top, int(np.bincount(case_indices[sel] // width, minlength=n_bins).max()))
    scale = max(geometry(k, slice_shift, kind)[1], 1) // n_bins if gb > 1 else 1
    bc = max(8, C['stream.grid'] * top // max(scale, 1))
    while room(batch_bin_capacity(k, slice_shift, kind, bc, n_batch), cap) < top:
        bc = bc * 5 // 4 + C['stream.grid']
    return bc


def _finish(name, m, k, shift, kind, indices, indptr, row_len, weights, spikes, *, wdtype='f32', flags=0, bin_capacity=None, cap=0,
            note='', i64=False, extra=None):
    spikes = np.atleast_2d(np.asarray(spikes, bool))
    c = Case(name, m, k, shift, kind, np.ascontiguousarray(indices, np.int32),
             None if indptr is None else indptr.astype(np.int64 if i64 else np.int32), row_len, weights, spikes, 0, wdtype, flags,
             bin_capacity is not None, cap, note, extra or {})
    width, nbb, gcap, _, gb = c.geometry()
    if bin_capacity is None and gcap > 0:
        bin_capacity = need_capacity(c.indices, c.rows_of_entries, spikes, k, shift, kind)        # with room
    c.bin_capacity = 8 if bin_capacity is None else bin_capacity
    for a in (c.indices, c.indptr, c.weights, c.spikes):
        if a is not None:
            a.setflags(write=False)
    return c


def simple_case(name, m, row_len, k, shift, kind, seed):
    """m rows of `row_len` entries behind an indptr, uniform columns, every row firing (test_no_geometry's matrix)."""
    rng = np.random.default_rng(seed)
    lens = np.full(m, row_len)
    return _finish(name, m, k, shift, kind, rng.integers(0, k, m * row_len), _ptr(lens), -1, _weights(rng, m * row_len, kind),
                   np.ones((1, m), bool))


def structured(name, k, shift, kind, seed, *, long_rows=(), fire=0.5, n_batch=1, dup=True, all_columns=True, reps=6, **kw):
    """The mixed row structure (MIXED_LENS shuffled, a run of rows shorter than four, a row listing every column once, a row of
    duplicate columns) behind `long_rows` leading rows; the leading rows, the all-columns row and the duplicates row always fire."""
    rng = np.random.default_rng(seed)
    min_units = kw.pop('min_units', 0)
    lens = np.concatenate([np.asarray(long_rows, np.int64), mixed_lens(seed, reps)])
    cols = [_columns(rng, lens, k)]
    special = list(range(len(long_rows)))
    if all_columns:
        special.append(len(lens))
        lens = np.append(lens, k)
        cols.append(rng.permutation(k).astype(np.int32))
    if dup:
        special.append(len(lens))
        lens = np.append(lens, 41)
        cols.append(rng.choice(rng.integers(0, k, 3), 41).astype(np.int32))
    m = len(lens)
    indices = np.concatenate(cols)
    spikes = rng.random((n_batch, m)) < fire
    spikes[:, special] = True
    return _finish(name, m, k, shift, kind, indices, _ptr(lens), -1, _weights(rng, indices.size, kind, min_units), spikes,
                   **kw)


def long_len(cap, n_bins):
    """A row that alone completes two blocks in about every bin of its workgroup (2.5 blocks' worth per bin on average)."""
    return 2 * cap * n_bins + cap * n_bins // 2 + 37


# ---------------------------------------------------------------------------------------------------------------------------
# the cases (name -> builder); both test modules build every one of them
# ---------------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name):
    def deco(f):
        assert name not in CASES, name
        CASES[name] = f
        return f
    return deco


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASES[name]()
    assert c.name == name
    return c


def _register_block_sizes():
    """Block sizes: shift 4 (bins of 16 columns), the first and the last bin count of every class for f32 weights, the first for
    f16 / bf16.  Under the persisted tuning (at least 2048 tasks) fewer than 4096 active rows make every task ONE row, and the tasks
    are dealt one or a few per workgroup: only a row of `long_len` entries completes blocks inside its workgroup, so four of them lead.
    At 8 entries per block a round of ROUND_ENTRIES = 512 entries completes about FLUSH_LIST = 64 blocks — EXPECTED to be more than the
    flush list holds about every other round (its second pass); no counter says so, it is not guaranteed.  The GPU module runs every
    case a second time with BE_BINNED_SHORT_ROWS (the one-step-in-flight instance of the same block size)."""
    assert ROUND_ENTRIES // C['cap.smallest'] >= FLUSH_LIST
    for kind in KINDS:
        for cap, (first, last) in class_bounds(kind).items():
            for wdt, which in (('f32', 'first'), ('f32', 'last'), ('f16', 'first'), ('bf16', 'first')):
                nb = first if which == 'first' else last
                name = f'cap-{KIND_NAME[kind]}-{cap}-{which}-{wdt}'

                def make(name=name, kind=kind, cap=cap, nb=nb, wdt=wdt):
                    return structured(name, 16 * nb, 4, kind, seed=cap + 7 * kind + nb, long_rows=[long_len(cap, nb)] * 3 + [long_len(cap, nb) - 2],
                                      wdtype=wdt, cap=cap, reps=3, all_columns=nb <= 512)
                CASES[name] = make


_register_block_sizes()


def block_size_cases(wdt=None):
    return [n for n in CASES if n.startswith('cap-') and (wdt is None or n.endswith('-' + wdt))]


def unserved_shapes():
    """(k, slice_shift, kind) one bin past the last class: no geometry (be_binned_bins == 0, the step returns BE_ERR_RANGE).  For
    counted entries the last class ends at kMaxBins itself."""
    return [(16 * (class_bounds(kind)[C['cap.smallest']][1] + 1), 4, kind) for kind in KINDS]


# --- geometry branches
K_BRANCH = C['geo.small_k'] + 1


def _register_geometry():
    for shift in (8, 16):
        for kind in KINDS:
            name = f'geo-{K_BRANCH}-shift{shift}-{KIND_NAME[kind]}'
            CASES[name] = functools.partial(structured, name, K_BRANCH, shift, kind, seed=shift + kind, long_rows=[6000] * 2, reps=3,
                                            all_columns=False)
    for k in (7, 16 * 5 + 3):             # fewer columns than one bin; a partial last bin
        for kind in KINDS:
            name = f'geo-{k}-shift4-{KIND_NAME[kind]}'
            CASES[name] = functools.partial(structured, name, k, 4, kind, seed=k + kind, reps=2)


_register_geometry()

# --- parts: bin counts of 1, 2, 16, 17, 128, 129 -> 16, 16, 16, 15, 2, 1 parts per bin; k % 4 == 1
PARTS_BINS = (1, 2, 16, 17, 128, 129)


def _register_parts():
    for nb in PARTS_BINS:
        for kind in KINDS:
            name = f'parts-{nb}-{KIND_NAME[kind]}'
            CASES[name] = functools.partial(structured, name, 16 * nb - 3, 4, kind, seed=nb + kind, long_rows=[2000], reps=2)


_register_parts()

# --- overflow: bin_capacity 8; 640 or more active rows whose entries all fall into one bin, next to ordinary rows that avoid that bin
OVERFLOW_HOT_ROWS = 640


def overflow_hot_rows(cap, hot_len):
    """At least 640, and more entries than all 256 regions of the hot bin hold together: some region overflows however the rows
    are dealt to the workgroups (blocks of 128 entries: 256 regions of 384 take 983 rows of 100)."""
    return max(OVERFLOW_HOT_ROWS, C['stream.grid'] * room(8, cap) // hot_len + 40)
OVERFLOW_ROW_LENS = {'ragged': 100, 'full': 128}


def overflow_case(name, kind, cap, hot_len, wdtype='f32', slack=False):
    """`full`: rows of 128 entries — whatever rows a workgroup is dealt, its count in the hot bin is a multiple of every block size:
    full blocks only, through the flush list, nothing left at the drain (guaranteed).  `ragged`: rows of 100 entries — a workgroup with
    n of them holds 100 n entries, no multiple of 32 / 64 / 128 for n < 8 and none of 8 / 16 for odd n: a partly filled block of a full
    region at the drain is EXPECTED (for blocks of 8 and 16 it needs a workgroup with an odd number of hot rows, which depends on the
    order of the active list), not guaranteed, and no counter tells the two slow paths apart.
    Either way the hot rows hold more entries than all regions of the hot bin together.  `slack`: k is one short of the bins' end and
    the hot bin is the last one, so one in sixteen of the hot entries has the column k — inside the bin, past the outputs."""
    first, last = class_bounds(kind)[cap]
    nb = first + 1
    k, rng = 16 * nb - int(slack), np.random.default_rng(cap + kind)
    hot = nb - 1 if slack else nb // 2
    ordinary = mixed_lens(cap + kind, reps=3)
    n_hot = overflow_hot_rows(cap, hot_len)
    lens = np.concatenate([np.full(n_hot, hot_len, np.int64), ordinary])
    indices = np.concatenate([_columns(rng, lens[:n_hot], k, 16 * hot, 16 * hot + 16),
                              _columns(rng, ordinary, k, avoid=(16 * hot, 16 * hot + 16))])
    m = len(lens)
    spikes = rng.random((1, m)) < 0.5
    spikes[0, :n_hot] = True
    c = _finish(name, m, k, 4, kind, indices, _ptr(lens), -1, _weights(rng, indices.size, kind), spikes, wdtype=wdtype, bin_capacity=8,
                cap=cap, extra={'hot_bin': hot, 'hot_len': hot_len})
    assert n_hot * hot_len > C['stream.grid'] * room(8, cap)
    return c


def _register_overflow():
    for kind in KINDS:
        for cap in CAPS:
            for variant, hot_len in OVERFLOW_ROW_LENS.items():
                name = f'overflow-{KIND_NAME[kind]}-{cap}-{variant}'
                CASES[name] = functools.partial(overflow_case, name, kind, cap, hot_len)
    CASES['overflow-acc64-32-ragged-f16'] = functools.partial(overflow_case, 'overflow-acc64-32-ragged-f16', 0, 32, 100, 'f16')
    for kind in KINDS:
        name = f'overflow-slack-{KIND_NAME[kind]}'
        CASES[name] = functools.partial(overflow_case, name, kind, 64, 100, slack=True)


_register_overflow()

# --- encodings, flags, task size, the Python path: the mixed structure over 150 bins (one part per bin, blocks of 64 entries)
MIXED_K = 16 * 150 - 1


@case('mixed-acc64')
def _mixed_acc64():
    return structured('mixed-acc64', MIXED_K, 4, 0, seed=11, long_rows=[3000, 1001], min_units=2)


@case('mixed-counted')
def _mixed_counted():
    return structured('mixed-counted', MIXED_K, 4, 1, seed=12, long_rows=[3000, 1001])


@case('mixed-acc32')
def _mixed_acc32():
    return structured('mixed-acc32', MIXED_K, 4, 2, seed=13, long_rows=[3000, 1001], min_units=2)


def _register_mixed_dtypes():
    for kind in KINDS:
        for wdt in ('f16', 'bf16'):
            name = f'mixed-{KIND_NAME[kind]}-{wdt}'
            CASES[name] = functools.partial(structured, name, MIXED_K, 4, kind, seed=20 + kind, long_rows=[3000, 1001], wdtype=wdt)


_register_mixed_dtypes()


@case('mixed-acc64-i64')
def _mixed_i64():
    return structured('mixed-acc64-i64', MIXED_K, 4, 0, seed=14, long_rows=[3000, 1001], i64=True)


@case('mixed-abs')
def _mixed_abs():
    return structured('mixed-abs', MIXED_K, 4, 0, seed=15, long_rows=[3000, 1001], flags=BE_BINNED_ABS)


@case('mixed-encodings')
def _mixed_enc():                       # m % 32 != 0 and m % 256 != 0 (asserted by the GPU module)
    return structured('mixed-encodings', MIXED_K, 4, 0, seed=16, long_rows=[500])


def _register_fixed():
    for n in FIXED_LENS:
        for kind in (0, 1):
            name = f'fixed-{n}-{KIND_NAME[kind]}'

            def make(name=name, n=n, kind=kind):
                rng = np.random.default_rng(n + kind)
                m = 301
                indices = rng.integers(0, MIXED_K, m * n).astype(np.int32)
                return _finish(name, m, MIXED_K, 4, kind, indices, None, n, _weights(rng, m * n, kind), rng.random((1, m)) < 0.6)
            CASES[name] = make


_register_fixed()


def column_past_k_case(name, k):
    """Every 50th entry has a column in [k, k + 40): the caller's error, such entries are dropped."""
    c = structured(name, k, 4, 0, seed=17, long_rows=[2000])
    idx = c.indices.copy()
    idx[::50] = k + (np.arange(idx[::50].size) % 40)
    return _finish(name, c.m, k, 4, 0, idx, c.indptr, -1, c.weights.copy(), c.spikes.copy())


CASES['column-past-k'] = functools.partial(column_past_k_case, 'column-past-k', MIXED_K + 1)            # the last bin is full
CASES['column-past-k-slack'] = functools.partial(column_past_k_case, 'column-past-k-slack', MIXED_K)    # column k sits in the last bin


# --- batches
BATCH_SIZES = (1, 2, 5, 32, 33, 70)
BATCH_K = 16 * 8 - 3                      # 8 bins per batch row: 32 batch rows share a pass for every kind
BATCH_K_64_COUNTED = 16 * 10 - 3          # 10 bins per batch row: 320 virtual bins, counted blocks of 64 entries
BATCH_K_CUT = 16 * 70                     # weighted: the block-size floor cuts a pass to 9 batch rows


def batch_case(name, k, shift, kind, n_batch, seed, fire=0.3, silent_row=None, **kw):
    c = structured(name, k, shift, kind, seed=seed, n_batch=n_batch, fire=fire, **kw)
    if silent_row is not None:
        s = c.spikes.copy()
        s[silent_row] = False
        c = _finish(name, c.m, k, shift, kind, c.indices, c.indptr, -1, c.weights.copy(), s, wdtype=c.wdtype)
    return c


def _register_batches():
    for nbatch in BATCH_SIZES:
        for kind in KINDS:
            name = f'batch-{nbatch}-{KIND_NAME[kind]}'
            CASES[name] = functools.partial(batch_case, name, BATCH_K, 4, kind, nbatch, seed=nbatch + kind, long_rows=[700], reps=2,
                                            silent_row=1 if nbatch >= 5 else None)
    for kind in KINDS:
        name = f'batch-cut-{KIND_NAME[kind]}'
        CASES[name] = functools.partial(batch_case, name, BATCH_K_CUT, 4, kind, 20, seed=70 + kind, long_rows=[3000], reps=2)
    # blocks of 64 entries in the batch kernel: 12 x 8 = 96 virtual bins (weighted), 32 x 10 = 320 (counted)
    for kind in (0, 2):
        name = f'batch-12-{KIND_NAME[kind]}'
        CASES[name] = functools.partial(batch_case, name, BATCH_K, 4, kind, 12, seed=12 + kind, long_rows=[700], reps=2, silent_row=1)
    CASES['batch-32x10-counted'] = functools.partial(batch_case, 'batch-32x10-counted', BATCH_K_64_COUNTED, 4, 1, 32, seed=10, long_rows=[700], reps=2)
    CASES['batch-5-acc64-f16'] = functools.partial(batch_case, 'batch-5-acc64-f16', BATCH_K, 4, 0, 5, seed=5, long_rows=[700], reps=2, wdtype='f16')
    CASES['batch-5-acc32-bf16'] = functools.partial(batch_case, 'batch-5-acc32-bf16', BATCH_K, 4, 2, 5, seed=6, long_rows=[700], reps=2, wdtype='bf16')


_register_batches()


def unmapped_k(kind, below=0):
    """One bin per batch row as wide as pass C's accumulators allow: the block map is left `map_cap` = a few bytes."""
    return max_width(16, kind) - below


UNMAPPED_BELOW = 16                       # this much narrower, the map holds a quiet call's blocks and not a busy one's


def unmapped_case(name, kind, below, quiet):
    """n_batch = 2 at slice_shift 16: one bin per batch row, blocks of 128 entries.  `quiet`: so few active entries that the
    bin's blocks fit the map whatever the dealing (a block holds at least one entry); else every row fires and the bin's entries
    alone need more blocks than the map has bytes."""
    k = unmapped_k(kind, below)
    c = structured(name, k, 16, kind, seed=kind + below, n_batch=2, fire=1.0, long_rows=[2000], reps=5, all_columns=True)
    width, nbb, cap, map_cap, gb = c.geometry()
    assert (nbb, gb) == (1, 2) and cap == C['cap.largest']
    spikes = c.spikes.copy()
    if quiet:
        spikes[:] = False
        order = np.argsort(c.lens, kind='stable')
        order = order[c.lens[order] > 0]
        take = order[:int(np.searchsorted(np.cumsum(c.lens[order]), map_cap, side='right'))]
        assert len(take) >= 2
        spikes[0, take] = True
        spikes[1, take[::2]] = True
    c = _finish(name, c.m, k, 16, kind, c.indices, c.indptr, -1, c.weights.copy(), spikes, extra={'quiet': quiet})
    per_row = [int(c.lens[spikes[b]].sum()) for b in range(2)]
    if quiet:
        assert 0 < max(per_row) <= map_cap, (per_row, map_cap)                 # blocks <= entries <= map_cap: mapped
    else:
        assert min(per_row) // cap > map_cap, (per_row, map_cap)               # blocks >= entries / cap > map_cap: the search
    return c


def _register_unmapped():
    for kind in KINDS:
        CASES[f'unmapped-{KIND_NAME[kind]}'] = functools.partial(unmapped_case, f'unmapped-{KIND_NAME[kind]}', kind, 0, False)
        for quiet in (True, False):
            name = f'near-unmapped-{KIND_NAME[kind]}-{"quiet" if quiet else "busy"}'
            CASES[name] = functools.partial(unmapped_case, name, kind, UNMAPPED_BELOW, quiet)


_register_unmapped()


def check_derived():
    """What the cases take from the table: five classes per kind that end where the budget says, the geometry branches at
    K_BRANCH, the batch passes, the parts, and the map sizes of the unmapped cases."""
    for kind in KINDS:
        b = class_bounds(kind)
        assert list(b) == list(CAPS) and b[128][0] == 1
        assert b[8][1] == min(stream_budget() // per_bin_bytes(8, kind), C['max_bins'])
        assert bins(16 * (b[8][1] + 1), 4, kind) == 0 and bins(16 * b[8][1], 4, kind) == b[8][1]
    assert class_bounds(0) == class_bounds(2)
    assert class_bounds(1)[8][1] == C['max_bins'] < stream_budget() // per_bin_bytes(8, 1)
    # k = 65537: shift 8 — weighted: the power-of-two branch; counted / ACC32: the rounds branch; shift 16: 260 columns, no power of two
    assert [geometry_branch(K_BRANCH, 8, kind) for kind in KINDS] == ['pow2', 'rounds', 'rounds']
    assert [geometry_branch(K_BRANCH, 16, kind) for kind in KINDS] == ['rounds'] * 3
    assert geometry(K_BRANCH, 8, 0)[0] == 256 and geometry(K_BRANCH, 8, 1)[0] == geometry(K_BRANCH, 8, 2)[0] == 132
    assert geometry(K_BRANCH, 16, 0)[0] == 260 and 260 & 259
    assert geometry_branch(C['geo.small_k'], 8, 0) == 'small'
    assert [parts(n) for n in PARTS_BINS] == [16, 16, 16, 15, 2, 1]
    for kind in KINDS:
        assert [geometry_batch(BATCH_K, 4, kind, n)[4] for n in BATCH_SIZES] == [1, 2, 5, 32, 32, 32]
        k = unmapped_k(kind)
        width, nbb, cap, map_cap, gb = geometry_batch(k, 16, kind, 2)
        assert (width, nbb, gb) == (k, 1, 2) and map_cap < 32
        assert geometry_batch(k + 1, 16, kind, 2)[1] == 2          # one column more is a second bin
        assert 32 < geometry_batch(k - UNMAPPED_BELOW, 16, kind, 2)[3] < 256
    assert geometry_batch(BATCH_K_CUT, 4, 0, 20)[4] == geometry_batch(BATCH_K_CUT, 4, 2, 20)[4] == \
        class_bounds(0)[C['batch.floor_weighted']][1] // 70 < 20
    assert geometry_batch(BATCH_K_CUT, 4, 1, 20)[4] == class_bounds(1)[C['batch.floor_counted']][1] // 70 < 20
    # the batch kernel's block sizes: every one a shared pass can have (the floors keep it at 16 weighted / 32 counted entries or more)
    reached = {kind: set() for kind in KINDS}
    for name in CASES:
        if name.startswith('batch-'):
            kind = {v: k for k, v in KIND_NAME.items()}[name.split('-')[2]]
            nb = 20 if 'cut' in name else int(name.split('-')[1].split('x')[0])
            k = {'cut': BATCH_K_CUT, '32x10': BATCH_K_64_COUNTED}.get(name.split('-')[1], BATCH_K)
            g = geometry_batch(k, 4, kind, nb)
            if g[4] > 1:
                reached[kind].add(g[2])
    assert reached[0] == reached[2] == {c for c in CAPS if c >= C['batch.floor_weighted']}, reached
    assert reached[1] == {c for c in CAPS if c >= C['batch.floor_counted']}, reached
    # packed tasks: under PACKED_TUNING the fixed-length rows go 64, 64, 64, 64, 8, 4, 4 to a task (200 active rows)
    assert [task_rows(n, 200, *PACKED_TUNING) for n in FIXED_LENS] == [64, 64, 64, 64, 8, 4, 4]
    assert [task_rows(n, 200, 256, 2048) for n in FIXED_LENS] == [1] * 7
    assert task_rows(50, 200, 1, 1) == C['task.rows_floor'] and task_rows(50, 200, 1 << 20, 1) == 64
