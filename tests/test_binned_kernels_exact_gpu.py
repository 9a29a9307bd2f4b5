"""The binned scatter route (csrc/be_csr_binned.hip: k_bin_stream, k_bin_accumulate, k_bin_reset, k_bin_union, k_bin_round behind
be_binary_csrmv_t_binned / be_binary_csrmm_t_binned) compared EXACTLY with the dense f64 reference of tests/binned_cases.py, at the
smallest shapes that reach each kernel instance.  Every comparison is an equality of bits (binned_cases: why every partial sum is
exact), every output buffer starts as a sentinel, and after every step the workspace's conservation counters are read:
entries in the active rows == tickets == accumulated + overflowed, the first equal to the count numpy takes from the case, the
last zero in every case sized with room and positive in every overflow case — a case cannot silently miss the path it is named for.

What reaches what (the CPU module tests/test_binned_kernels_thresholds_cpu.py holds the sizes to the source):
  * test_block_sizes             k_bin_stream<W, HOMO, CAP> / k_bin_accumulate<HOMO, CAP, ACC32> for CAP in 128 ... 8, the three kinds,
                                 the first and last bin count of each class (f32), the first (f16, bf16)
  * test_no_geometry             one bin past the last class / past kMaxBins: BE_ERR_RANGE, nothing written
  * test_geometry_branches       k = 65537 at shift 8 (power-of-two and rounds branch) and 16 (bins of 260 columns: the multiply-high
                                 division), k < 16, a partial last bin
  * test_parts                   16, 16, 16, 15, 2, 1 parts per bin, `out` 16-byte aligned and not, k % 4 == 1 (both branches of k_bin_reset)
  * test_overflow                bin_capacity 8, 640+ rows into one bin: the flush path through float atomics with full blocks and
                                 with a partly filled block at the drain, every block size and kind; the image reads zero afterwards
  * test_encodings               bool, float, bit-packed (bits past m set), BE_SPIKE_IDS; no spike, one spike, every row
  * test_batch*                  k_bin_stream<..., BATCH = true>, k_bin_union x 3, passes of 32 with a partial last pass, a pass cut
                                 to 9 / 12 batch rows by the block-size floor, a silent batch row
  * test_unmapped_directory      pass C's binary search over the directory (more blocks than the map has bytes), and the mapped /
                                 unmapped switch between a quiet and a busy call of one shape
  * test_fixed_length_rows, test_packed_tasks, test_task_size
                                 several rows in one task (be_binned_set_tuning): `fixdiv` as a shift and as a multiply-high, the search
                                 over the prefix sums, short and long rows in one wave — see below
  * test_abs_flag, test_short_rows_hint, test_int64_indptr, test_column_past_k
  * test_python_path             BinnedScatter (acc32 True / False) and binned_batch give the bits of the direct call

Rows per task.  The persisted tuning asks for at least 2048 tasks, so a step with fewer than 4096 active rows — every case here —
makes each task ONE row: a lane's group index stays inside row 0 of the task's table, `fixdiv.div` returns 0 for any divisor and the
search over the prefix sums never moves.  The cases named above therefore run under be_binned_set_tuning(*PACKED_TUNING) too
(`tuned`, restored in a finally), where binned_cases.task_rows — restated from kTaskRowsFloor / kTaskGroupsCap — says 4 to 64 rows
share a task, and each asserts that it does.  All other cases (block sizes, overflow, parts, encodings, geometry) run one row per task.

Not reached: rows of 2^26 entries or more (the "huge" piece loop of k_bin_stream) need 2^26 stored entries in one row — no test-size
case has them, and nothing here pretends to.  The batch kernel has no instance with blocks of 8 entries (16, counted) to reach: a
shared pass keeps blocks of 16 (32) entries or more, else the batch falls back to single vectors.  Expected, not guaranteed (no
counter tells): more than 64 blocks completed in one append round at blocks of 8 entries, and a partly filled block of a FULL region
at the drain in the `ragged` overflow cases of 8 and 16 entries (binned_cases.overflow_case)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import binned_cases as B
from binned_cases import BE_BINNED_ABS, BE_BINNED_SHORT_ROWS, BE_ERR_RANGE, BE_OK, KIND_NAME, KINDS, SCALE_EXP

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
TORCH_DT = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}
SPIKE_BOOL, SPIKE_FLOAT, SPIKE_BITS, SPIKE_IDS = 0, 1, 2, 3


def cast_reference(ref, wdt):
    """The f64 reference cast ONCE to the output dtype (numpy for f32 / f16, torch on the CPU for bf16), back as f64."""
    if wdt == 'bf16':
        return torch.from_numpy(ref.astype(np.float32)).to(torch.bfloat16).double().numpy()      # (f64 -> f32 is exact here)
    return ref.astype({'f32': np.float32, 'f16': np.float16}[wdt]).astype(np.float64)


def pack_bits(spikes, garbage=True):
    """bool [nb, m] -> int32 words [nb, ceil(m / 32)], the bits past m SET (a packer may leave anything there)."""
    nb, m = spikes.shape
    nw = (m + 31) // 32
    padded = np.full((nb, nw * 32), garbage, dtype=bool)
    padded[:, :m] = spikes
    words = (padded.reshape(nb, nw, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return words.view(np.int32)


class Device:
    """A case's matrix on the device, a workspace of its own, and the direct C calls on them."""

    def __init__(self, case, n_batch=None):
        from brainevent_amd import _array as A, _lib
        self.A, self.lib, self.c = A, _lib, case
        self.n_batch = case.n_batch if n_batch is None else n_batch
        dt = TORCH_DT[case.wdtype]
        self.w = torch.tensor(np.asarray(case.weights, np.float64)).to(dt).cuda()
        assert np.array_equal(self.w.double().cpu().numpy(), case.weights)           # exact in the weight dtype
        self.indices = torch.tensor(case.indices).cuda()
        self.indptr = None if case.indptr is None else torch.tensor(case.indptr).cuda()
        key = (case.m, case.k, self.n_batch, case.slice_shift, case.bin_capacity)
        self.ws_bytes = int(_lib.fn('be_binary_csrmm_t_binned_workspace_bytes')(*key))
        assert self.ws_bytes == B.workspace_bytes(*key), key                           # pins the restated cap, gb and cap_blocks
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device='cuda')
        rc = _lib.fn('be_binary_csrmm_t_binned_workspace_init')(A.ptr(self.ws), self.ws_bytes, *key, A.stream_ptr())
        assert rc == BE_OK, _lib.last_error()
        self.total = [0, 0, 0, 0]

    def events(self, spikes, enc):
        spikes = np.atleast_2d(spikes)
        if enc == 'bool':
            return torch.tensor(spikes).cuda(), SPIKE_BOOL
        if enc == 'float':          # active: > 0 only — zeros, negatives and -0.0 are silent
            rng = np.random.default_rng(3)
            v = np.where(spikes, rng.choice([0.25, 1.0, 3.5], spikes.shape), rng.choice([0.0, -0.0, -1.0, -7.5], spikes.shape))
            return torch.tensor(v.astype(np.float32)).cuda(), SPIKE_FLOAT
        if enc == 'bits':
            return torch.tensor(pack_bits(spikes)).cuda(), SPIKE_BITS
        assert enc == 'ids' and spikes.shape[0] == 1
        ids = np.nonzero(spikes[0])[0].astype(np.int32)
        buf = torch.full((self.c.m + 1,), -1, dtype=torch.int32, device='cuda')          # (past the count: never read)
        buf[:ids.size] = torch.tensor(ids).cuda()
        count = torch.tensor([ids.size], dtype=torch.int32, device='cuda')
        return self.A.ActiveIds(buf, count, self.c.m), SPIKE_IDS

    def out_buffer(self, nb, misalign=0):
        dt = TORCH_DT[self.c.wdtype]
        raw = torch.full((nb * self.c.k + 8,), SENTINEL, dtype=dt, device='cuda')
        return raw, raw[misalign:misalign + nb * self.c.k]

    def step_rc(self, spikes=None, enc='bool', flags=None, misalign=0, scale_exp=None):
        """One step through be_binary_csrmm_t_binned (be_binary_csrmv_t_binned for an id list) -> (rc, raw buffer, output view)."""
        c, A = self.c, self.A
        spikes = c.spikes if spikes is None else np.atleast_2d(spikes)
        nb = spikes.shape[0]
        ev, sd = self.events(spikes, enc)
        raw, out = self.out_buffer(nb, misalign)
        homo = c.kind | (c.flags if flags is None else flags)
        e = SCALE_EXP[c.kind] if scale_exp is None else scale_exp
        is64 = int(c.indptr is not None and c.indptr.dtype == np.int64)
        head = (A.ptr(self.w), homo, A.wcode(self.w), A.ptr(self.indices), A.ptr(self.indptr), is64, c.row_len, A.ptr(ev), sd, A.ptr(out),
                c.m, c.k)
        tail = (c.slice_shift, c.bin_capacity, e, A.ptr(self.ws), self.ws_bytes, A.stream_ptr())
        if sd == SPIKE_IDS:
            assert self.n_batch == 1
            rc = self.lib.fn('be_binary_csrmv_t_binned')(*head, *tail)
        else:
            assert nb == self.n_batch
            rc = self.lib.fn('be_binary_csrmm_t_binned')(*head, nb, *tail)
        torch.cuda.synchronize()
        return rc, raw, out

    def audit(self):
        a = (ctypes.c_uint64 * 4)()
        assert self.lib.fn('be_binned_workspace_audit')(self.A.ptr(self.ws), a, self.A.stream_ptr()) == BE_OK
        return [int(x) for x in a]

    def status(self, clear=0):
        return self.lib.fn('be_binned_workspace_status')(self.A.ptr(self.ws), clear, self.A.stream_ptr())

    def step(self, spikes=None, enc='bool', flags=None, misalign=0, overflow=None, dropped=False):
        """A step that must succeed, write every output and nothing else, equal the reference and conserve its entries."""
        c = self.c
        spikes = c.spikes if spikes is None else np.atleast_2d(spikes)
        rc, raw, out = self.step_rc(spikes, enc, flags, misalign)
        assert rc == BE_OK, self.lib.last_error()
        n = spikes.shape[0] * c.k
        edge = torch.cat([raw[:misalign], raw[misalign + n:]])
        assert bool((edge == SENTINEL).all()), 'the step wrote outside its output'
        got = out.double().cpu().numpy().reshape(spikes.shape[0], c.k)
        want = cast_reference(c.reference(spikes), c.wdtype)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (c.name, enc, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        # conservation: this step's share of the counters
        before, now = self.total, self.audit()
        a, b, cc, d = (x - y for x, y in zip(now, before))
        self.total = now
        n_entries, n_bad, n_past = c.counts(spikes)
        assert a == n_entries, (c.name, 'entries in the active rows', a, n_entries)
        assert b == cc + d and a - b == n_past, (c.name, (a, b, cc, d), n_past)
        assert (n_bad > 0) == dropped, (c.name, 'entries with a column >= k', n_bad)
        overflow = c.overflow if overflow is None else overflow
        assert (d > 0) == overflow, (c.name, 'overflowed entries', d, 'expected some' if overflow else 'expected none')
        if a == b:
            assert self.status() == BE_OK, self.lib.last_error()
        return out

    def overflow_image(self):
        lay = B.workspace_layout(self.c.m, self.c.k, self.n_batch, self.c.slice_shift, self.c.bin_capacity)
        return self.ws[lay['ovf']:lay['out32']]


def persisted_tuning():
    """(task_groups, min_tasks) the package hands the library for this device."""
    from brainevent_amd import _csr, _tuning
    _tuning.ensure_resolved()
    t = getattr(_csr, '_TUNING', None) or _tuning.get_scatter_tuning()
    return int(t.binned_task_groups), int(t.binned_min_tasks)


@contextlib.contextmanager
def tuned(pair):
    """be_binned_set_tuning(*pair) for the block; the persisted pair afterwards, whatever happens inside."""
    from brainevent_amd import _lib
    back = persisted_tuning()
    try:
        assert _lib.fn('be_binned_set_tuning')(*pair) == BE_OK
        yield
    finally:
        assert _lib.fn('be_binned_set_tuning')(*back) == BE_OK


def run(name, **kw):
    c = B.build(name)
    d = Device(c)
    return d, d.step(**kw)


# ================================================================================================================ block sizes
@pytest.mark.parametrize('name', B.block_size_cases())
def test_block_sizes(name):
    c = B.build(name)
    assert c.geometry()[2] == c.cap and c.geometry()[4] == 1
    d, two_ahead = run(name, flags=0)
    one_ahead = d.step(flags=BE_BINNED_SHORT_ROWS)             # k_bin_stream<..., U = 1> of the same block size
    assert torch.equal(two_ahead.view(torch.uint8), one_ahead.view(torch.uint8))


@pytest.mark.parametrize('k,shift,kind', B.unserved_shapes())
def test_no_geometry(k, shift, kind):
    """One bin past the last class: be_binned_bins returns 0, the step returns BE_ERR_RANGE and writes nothing; a clean call of a
    served shape follows on the same process."""
    from brainevent_amd import _lib
    assert _lib.fn('be_binned_bins')(k, shift, kind) == 0 and _lib.fn('be_binned_bins')(k - 16, shift, kind) == (k - 16) // 16
    c = B.simple_case(f'unserved-{kind}', 64, 8, k, shift, kind, seed=k)
    d = Device(c)
    rc, raw, out = d.step_rc()
    assert rc == BE_ERR_RANGE
    assert bool((raw == SENTINEL).all())
    assert d.audit() == [0, 0, 0, 0] and d.status() == BE_OK
    run(f'geo-7-shift4-{KIND_NAME[kind]}')


# ========================================================================================================== geometry branches
@pytest.mark.parametrize('name', [n for n in B.CASES if n.startswith('geo-')])
def test_geometry_branches(name):
    run(name)


# ===================================================================================================================== parts
@pytest.mark.parametrize('misalign', [0, 1])
@pytest.mark.parametrize('name', [n for n in B.CASES if n.startswith('parts-')])
def test_parts(name, misalign):
    c = B.build(name)
    assert c.k % 4 == 1 and B.parts(c.geometry()[1]) == dict(zip(B.PARTS_BINS, (16, 16, 16, 15, 2, 1)))[c.geometry()[1]]
    d = Device(c)
    out = d.step(misalign=misalign)
    assert (out.data_ptr() % 16 == 0) == (misalign == 0)


# ================================================================================================================== overflow
@pytest.mark.parametrize('name', [n for n in B.CASES if n.startswith('overflow-')])
def test_overflow(name):
    c = B.build(name)
    assert c.bin_capacity == 8 and c.geometry()[2] == c.cap and int(c.spikes[0, :640].sum()) == 640
    slack = 'slack' in name           # one hot entry in sixteen has the column k: inside the last bin, past the outputs — dropped
    assert (c.counts()[1] > 1000) == slack and c.counts()[2] == 0
    d = Device(c)
    assert not bool(d.overflow_image().any())
    first = d.step(dropped=slack).clone()
    assert not bool(d.overflow_image().any()), 'the step left part of the overflow image behind'
    second = d.step(dropped=slack)
    assert torch.equal(first.view(torch.uint8), second.view(torch.uint8))
    assert not bool(d.overflow_image().any())


# ================================================================================================================= encodings
@pytest.mark.parametrize('pattern', ['none', 'one', 'all', 'random'])
@pytest.mark.parametrize('enc', ['bool', 'float', 'bits', 'ids'])
def test_encodings(enc, pattern):
    c = B.build('mixed-encodings')
    assert c.m % 32 != 0 and c.m % 256 != 0
    s = {'none': np.zeros(c.m, bool), 'all': np.ones(c.m, bool), 'random': c.spikes[0]}.get(pattern)
    if s is None:
        s = np.zeros(c.m, bool)
        s[c.m - 1] = True                 # the last row: the one next to the bits past m
        assert c.lens[c.m - 1] > 0
    Device(c).step(s, enc=enc)


def test_encodings_share_a_workspace():
    """The spike counter in the workspace head is re-armed by every step for the next, whichever encoding either uses."""
    c = B.build('mixed-encodings')
    d = Device(c)
    for enc in ('bits', 'ids', 'bool', 'ids', 'float', 'bits'):
        d.step(enc=enc)


# ===================================================================================================================== batch
@pytest.mark.parametrize('name', [n for n in B.CASES if n.startswith('batch-')])
def test_batch(name):
    c = B.build(name)
    assert c.m % 256 != 0
    tag = name.split('-')
    if len(tag) == 3 and tag[1].isdigit() and int(tag[1]) >= 5:
        assert not c.spikes[1].any() and c.spikes[0].any()            # a batch row without a spike
    run(name)


@pytest.mark.parametrize('enc', ['float', 'bits'])
@pytest.mark.parametrize('kind', KINDS)
def test_batch_union_encodings(kind, enc):
    """k_bin_union<BE_SPIKE_FLOAT> and <BE_SPIKE_BITS> (test_batch runs <BE_SPIKE_BOOL>), a partial last pass of one batch row."""
    run(f'batch-33-{KIND_NAME[kind]}', enc=enc)


@pytest.mark.parametrize('name', [n for n in B.CASES if 'unmapped-' in n])
def test_unmapped_directory(name):
    run(name)


# ===================================================================================================================== flags
def test_abs_flag():
    c = B.build('mixed-abs')
    assert c.flags == BE_BINNED_ABS and (c.weights < 0).any()
    d, out = run('mixed-abs')
    assert float(out.min()) >= 0.0


@pytest.mark.parametrize('name', ['mixed-acc64', 'mixed-counted', 'mixed-acc32'])
def test_short_rows_hint(name):
    """BE_BINNED_SHORT_ROWS set and clear: one step of loads in flight or two, the same bits."""
    d = Device(B.build(name))
    a = d.step(flags=0).clone()
    b = d.step(flags=BE_BINNED_SHORT_ROWS)
    assert torch.equal(a, b)


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('name', [n for n in B.CASES if n.startswith('fixed-')])
def test_fixed_length_rows(name, packed):
    """row_len without an indptr: the short-row load path (1, 3), one step in flight up to kShortRow entries and two past it.
    `packed`: 64 (rows of up to 6 entries), 8 (100) or 4 (kShortRow, kShortRow + 1) rows share a task, so a lane finds its row by
    `fixdiv` — a shift for 1 group per row (1, 3, 4), 2 (6) and 64 (kShortRow), a multiply-high for 25 (100) and 65 (kShortRow + 1)."""
    c = B.build(name)
    assert c.indptr is None and c.row_len in B.FIXED_LENS
    pair = B.PACKED_TUNING if packed else persisted_tuning()
    rows = c.rows_per_task(*pair)
    groups = (c.row_len + 3) // 4
    if packed:
        assert rows == {1: 64, 2: 64, 25: 8, 64: 4, 65: 4}[groups] and (groups & (groups - 1) == 0) == (groups not in (25, 65))
    with tuned(pair):
        run(name)


PACKED = [n for n in B.CASES if n.startswith('mixed-')] + ['batch-33-acc64', 'batch-33-counted', 'batch-33-acc32', 'batch-12-acc64',
                                                           'batch-cut-acc32', 'column-past-k-slack']


@pytest.mark.parametrize('name', PACKED)
def test_packed_tasks(name):
    """Several rows in one task, rows behind an indptr: the prefix scan of the rows' groups, the search over it, row starts past the
    first, and waves that hold rows of 0 ... 257 entries and the run of rows shorter than four at once (the entry-by-entry load path
    for the whole wave) — every kind and weight type, int64 row pointers, |w|, a column >= k, and the batch kernel."""
    c = B.build(name)
    assert c.rows_per_task(*B.PACKED_TUNING) >= 16
    with tuned(B.PACKED_TUNING):
        d = Device(c)
        d.step(dropped=c.counts()[1] > 0)
        if c.n_batch == 1:
            d.step(enc='ids', dropped=c.counts()[1] > 0)


def test_int64_indptr():
    c = B.build('mixed-acc64-i64')
    assert c.indptr.dtype == np.int64
    run('mixed-acc64-i64')


def test_task_size():
    """be_binned_set_tuning: 4 rows per task (the floor), the persisted size, and 64 rows per task — the same bits."""
    outs = {}
    for pair, rows in (((1, 1), B.C['task.rows_floor']), (persisted_tuning(), None), ((1 << 20, 1), 64)):
        for name in ('mixed-acc64', 'mixed-counted'):
            if rows is not None:
                assert B.build(name).rows_per_task(*pair) == rows
            with tuned(pair):
                outs.setdefault(name, []).append(run(name)[1].clone())
    for name, (first, *rest) in outs.items():
        assert len(rest) == 2 and all(torch.equal(first, o) for o in rest), name


@pytest.mark.parametrize('name', ['column-past-k', 'column-past-k-slack'])
def test_column_past_k(name):
    """Entries with a column >= k are dropped: the output is the reference without them and the counters say how many — entries
    in the active rows minus tickets (`Device.step`; with a partial last bin, minus those whose column lies inside that bin: they
    draw a ticket and are dropped where the outputs are written).  The status call names the cause and clears the counters."""
    c = B.build(name)
    n_entries, n_bad, n_past = c.counts()
    assert n_bad > 20 and (n_past == n_bad) == (name == 'column-past-k') and n_past > 0
    d = Device(c)
    d.step(dropped=True)
    assert d.status(clear=1) == BE_ERR_RANGE and 'column ids >= k' in d.lib.last_error()
    assert d.audit() == [0, 0, 0, 0] and d.status() == BE_OK


# =========================================================================================================== the Python path
@pytest.mark.parametrize('name,acc32', [('mixed-acc64', False), ('mixed-acc32', True)])
def test_python_path(be, name, acc32):
    """BinnedScatter derives the exponent and the capacity itself; exact sums do not depend on either: the bits of the direct call."""
    from brainevent_amd import _array as A, _csr
    c = B.build(name)
    d = Device(c)
    direct = d.step()
    ws = _csr.BinnedScatter(d.w, c.m, c.k, c.indices.size, slice_shift=c.slice_shift, indices=d.indices, acc32=acc32, indptr=d.indptr)
    assert ws.acc32 == acc32 and ws.kind == c.kind and ws.scale_exp >= 6
    key = (c.m, c.k, 1, c.slice_shift, ws.bin_capacity)
    assert ws.workspace(1).numel() == B.workspace_bytes(*key)
    spikes = torch.tensor(c.spikes[0]).cuda()
    out = torch.full((c.k,), SENTINEL, dtype=torch.float32, device='cuda')
    _csr._binned_call(ws, d.w, d.indices, d.indptr, -1, spikes, A.BE_SPIKE_BOOL, out)
    assert torch.equal(out, direct)
    a, b, cc, dd = ws.audit()
    assert a == b == cc + dd == c.counts()[0]
    ws.check_status()


@pytest.mark.parametrize('name', ['batch-33-acc64', 'batch-5-counted'])
def test_python_batch_path(be, name):
    from brainevent_amd import _array as A, _csr
    c = B.build(name)
    d = Device(c)
    direct = d.step()
    ws = _csr.BinnedScatter(d.w, c.m, c.k, c.indices.size, slice_shift=c.slice_shift, indices=d.indices, acc32=False, indptr=d.indptr)
    key = (c.m, c.k, c.n_batch, c.slice_shift, ws.bin_capacity)
    assert ws.workspace(c.n_batch).numel() == B.workspace_bytes(*key)
    out = torch.full((c.n_batch, c.k), SENTINEL, dtype=torch.float32, device='cuda')
    _csr.binned_batch(ws, d.w, d.indices, d.indptr, -1, torch.tensor(c.spikes).cuda(), A.BE_SPIKE_BOOL, out)
    assert torch.equal(out.reshape(-1), direct)
    a, b, cc, dd = ws.audit(c.n_batch)
    assert a == b == cc + dd == c.counts()[0]
    ws.check_status()
