"""``events @ Float8CSR`` on the device, every comparison bit for bit against the numpy restatement (tests/csr_f8_cases.py): the two
routes by direct C call (be_binary_csrm*_t_f8: global 64-bit integer atomics; be_scatter_plan_q8_* + be_binary_csrm*_t_plan_f8:
the q8 layout), and the container through Python.  The sums are integers at a fixed exponent, so equality — with the restatement,
between the routes, between geometries, between calls — is the contract, not a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import brainevent_amd as be
from brainevent_amd import _array as A
from brainevent_amd import _csr as C
from brainevent_amd import _csr_f8 as F
from brainevent_amd._lib import fn, last_error
import csr_f8_cases as K

pytestmark = pytest.mark.gpu
FMTS = sorted(K.E)
OK, INVALID, WORKSPACE, RANGE, UNSUPPORTED = 0, -1, -2, -4, -5
SENTINEL = 0xA5
HINTS = list(K.LPB_VARIANTS.values())        # block hints that select 8 lanes, 16 lanes and a wave per block


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Mat:
    """A CSR matrix of FP8 codes, on the host (for the restatement) and on the device (for the calls)."""

    def __init__(self, codes, indices, indptr, m, k, fmt, i64=False):
        self.codes, self.indices, self.indptr, self.m, self.k, self.fmt = codes, indices, indptr, m, k, fmt
        self.d_codes, self.d_indices = dev(codes), dev(indices)
        self.d_indptr = dev(indptr.astype(np.int64) if i64 else indptr.astype(np.int32))
        self.is64 = int(i64)
        self.nnz = len(indices)
        self._plans = {}

    def expected(self, active, scale=1.0):
        return K.expected(self.codes, self.indices, self.indptr, active, self.k, self.fmt, scale)

    def plan(self, shift, width):
        """(seg, blob) of the q8 plan at this geometry, or the status of the refusing call."""
        key = (shift, width)
        if key not in self._plans:
            n_slices = -(-self.k // (width or (1 << shift)))
            seg = torch.empty(max(1, n_slices * self.m * 2), dtype=torch.int32, device='cuda')
            scratch = A.workspace(fn('be_scatter_plan_q8_scratch_bytes')(self.m, self.k, shift, width))
            order = torch.empty(max(1, self.nnz), dtype=torch.int16, device='cuda')
            nbytes = ctypes.c_int64(-1)
            rc = fn('be_scatter_plan_q8_count')(A.ptr(self.d_indices), A.ptr(self.d_indptr), self.is64, -1, self.m, self.k, shift, width,
                                                A.ptr(seg), A.ptr(scratch), scratch.numel(), ctypes.byref(nbytes), A.ptr(order),
                                                A.stream_ptr())
            if rc != OK:
                return rc
            blob = torch.full((int(nbytes.value) + 128,), SENTINEL, dtype=torch.uint8, device='cuda')
            # the order is used by half of the builds: the fill sorts again without it, and writes the same blocks
            use_order = (shift + width + self.m) % 2 == 0
            rc = fn('be_scatter_plan_q8_fill')(A.ptr(self.d_codes), A.ptr(self.d_indices), A.ptr(self.d_indptr), self.is64, -1, self.m,
                                               self.k, shift, width, A.ptr(seg), A.ptr(blob), A.ptr(order if use_order else None),
                                               A.stream_ptr())
            assert rc == OK, last_error()
            torch.cuda.synchronize()
            assert bool((blob[int(nbytes.value):] == SENTINEL).all()), "the fill wrote past the blob"
            self._plans[key] = (seg, blob)
        return self._plans[key]


def spikes_of(kind, active):
    """(keep-alive object, pointer, spike dtype code) of a bool vector [m] or batch [nb, m] in the encoding ``kind``."""
    active = np.asarray(active, dtype=bool)
    if kind == 'bool':
        t = dev(active.astype(np.uint8) * 3)
        return t, A.ptr(t), A.BE_SPIKE_BOOL
    if kind == 'float':
        v = np.where(active, np.float32(0.5), np.float32(0.0)).astype(np.float32)
        off = np.flatnonzero(~active.reshape(-1))
        v.reshape(-1)[off[0::3]] = -2.0             # a negative value and a NaN are inactive
        v.reshape(-1)[off[1::3]] = np.nan
        assert np.array_equal(K.active_of(v), active)
        t = dev(v)
        return t, A.ptr(t), A.BE_SPIKE_FLOAT
    if kind == 'bits':
        t = dev(K.pack_bits(active).view(np.int32))
        return t, A.ptr(t), A.BE_SPIKE_BITS
    assert kind == 'ids' and active.ndim == 1
    ids = np.flatnonzero(active)[::-1].astype(np.int32)          # (in no particular order)
    ids_t = dev(np.concatenate([ids, np.zeros(4, np.int32)]))
    holder = A.ActiveIds(ids_t, dev(np.array([len(ids)], np.int32)), len(active))
    return holder, ctypes.c_void_p(holder.data_ptr()), A.BE_SPIKE_IDS


def guarded(nbytes, fill=None):
    """A byte buffer of ``nbytes`` (zeroed, or ``fill``) with a sentinel tail of 256 bytes behind it."""
    t = torch.full((nbytes + 256,), SENTINEL, dtype=torch.uint8, device='cuda')
    if nbytes:
        t[:nbytes] = 0 if fill is None else fill
    return t


def tail_ok(t, nbytes):
    return bool((t[nbytes:] == SENTINEL).all())


def run_direct(M, kind, active, scale=1.0, expect=OK):
    active = np.asarray(active, dtype=bool)
    nb = 1 if active.ndim == 1 else active.shape[0]
    keep, sp, sd = spikes_of(kind, active)
    need = fn('be_binary_csrmm_t_f8_workspace_bytes')(M.m, M.k, nb)
    ws, out = guarded(need, fill=0x5A), guarded(nb * M.k * 4, fill=0xFF)
    rc = fn('be_binary_csrmm_t_f8')(A.ptr(M.d_codes), K.FMT_CODE[M.fmt], scale, A.ptr(M.d_indices), A.ptr(M.d_indptr), M.is64, -1, M.nnz,
                                    sp, sd, A.ptr(out), M.m, M.k, nb, A.ptr(ws), need, A.stream_ptr())
    assert rc == expect, (rc, last_error())
    torch.cuda.synchronize()
    assert tail_ok(ws, need) and tail_ok(out, nb * M.k * 4), "wrote past the workspace / the output"
    del keep
    r = out[:nb * M.k * 4].view(torch.float32).cpu().numpy().reshape(nb, M.k)
    return r[0] if active.ndim == 1 else r


def run_plan(M, kind, active, shift, width, parts=1, hint=0, scale=1.0):
    active = np.asarray(active, dtype=bool)
    nb = 1 if active.ndim == 1 else active.shape[0]
    seg, blob = M.plan(shift, width)
    keep, sp, sd = spikes_of(kind, active)
    need = fn('be_binary_csrmm_t_plan_f8_workspace_bytes')(M.m, M.k, nb, shift, width, parts, hint)
    ws, out = guarded(need), guarded(nb * M.k * 4, fill=0xFF)
    rc = fn('be_binary_csrmm_t_plan_f8')(A.ptr(blob), A.ptr(seg), K.FMT_CODE[M.fmt], scale, sp, sd, A.ptr(out), M.m, M.k, nb, shift, width,
                                         hint, parts, A.ptr(ws), need, A.stream_ptr())
    assert rc == OK, (rc, last_error())
    torch.cuda.synchronize()
    assert tail_ok(ws, need) and tail_ok(out, nb * M.k * 4), "wrote past the workspace / the output"
    assert not bool(ws[:4 * nb].any()), "the spike counters are zero again after the call"
    del keep
    r = out[:nb * M.k * 4].view(torch.float32).cpu().numpy().reshape(nb, M.k)
    return r[0] if active.ndim == 1 else r


def geometries(k):
    """(slice_shift, slice_width) giving 1, 2 and 5 slices (as many as k allows) at the smallest capacity the entry points accept,
    and that capacity itself — 16 columns per slice — where it stays within the slice limit."""
    out = []
    for n in (1, 2, 5):
        w = -(-k // min(n, k))
        if (4, w) not in out:
            out.append((4, w))
    if -(-k // 16) <= K.MAX_SLICES and (4, 0) not in out and (4, 16) not in out:
        out.append((4, 0))
    return out


# ------------------------------------------------------------------------------------------------- by direct C call
@pytest.mark.parametrize('m', [1, 3, 257])
@pytest.mark.parametrize('k', [1, 63, 64, 65, 300, 1025])
def test_sizes_geometries_and_parts(k, m):
    rng = np.random.default_rng(1000 * k + m)
    kinds = ['bool', 'bits', 'float', 'ids']
    n = 0
    for fmt in FMTS:
        M = Mat(*K.random_matrix(m, k, fmt, seed=k + m), m, k, fmt, i64=(k + m) % 2 == 1)
        acts = [rng.random(m) < 0.5, np.ones(m, dtype=bool), np.zeros(m, dtype=bool)]
        wants = [M.expected(a) for a in acts]
        for a, want in zip(acts, wants):
            assert bits_equal(run_direct(M, kinds[n % 4], a), want)
            n += 1
        for shift, width in geometries(k):
            for parts in (1, 3):
                for a, want in zip(acts, wants):
                    got = run_plan(M, kinds[n % 4], a, shift, width, parts, HINTS[n % 3])
                    assert bits_equal(got, want), (fmt, shift, width, parts, kinds[n % 4], HINTS[n % 3])
                    n += 1


@pytest.mark.parametrize('fmt', FMTS)
def test_an_all_empty_matrix(fmt):
    m, k = 5, 70
    M = Mat(np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(m + 1, np.int32), m, k, fmt)
    a = np.ones(m, dtype=bool)
    assert bits_equal(run_direct(M, 'bool', a), np.zeros(k, np.float32))
    for shift, width in geometries(k):
        assert bits_equal(run_plan(M, 'bits', a, shift, width, 3, 10), np.zeros(k, np.float32))


@pytest.fixture(scope='module', params=FMTS)
def long_blocks(request):
    """Two slices of 1300 columns.  Row 0: two entries 599 columns apart in slice 0 (two escape entries between them).  Row 1: a block
    of 300 entries in slice 0 (more than one wave pass of 256) and one of 1100 in slice 1 (more than one tail chunk after any first
    pass).  Row 2: empty.  Row 3: short blocks in both slices."""
    fmt = request.param
    rng = np.random.default_rng(7)
    fc = K.finite_codes(fmt)
    rows = [([604, 5], rng.choice(fc, 2)),
            (np.concatenate([rng.integers(0, 1300, 300), rng.integers(1300, 2600, 1100)]), rng.choice(fc, 1400)),
            ([], []),
            (rng.permutation(2600)[:9], rng.choice(fc, 9))]
    M = Mat(*K.from_rows(rows, 2600), 4, 2600, fmt)
    acts = {'all': np.ones(4, bool), 'row0': np.array([1, 0, 0, 0], bool), 'row1': np.array([0, 1, 0, 0], bool),
            'none': np.zeros(4, bool)}
    return M, acts, {n: M.expected(a) for n, a in acts.items()}


@pytest.mark.parametrize('lpb', sorted(K.LPB_VARIANTS))
def test_escapes_long_blocks_and_tails_at_every_lanes_per_block_variant(long_blocks, lpb):
    M, acts, wants = long_blocks
    hint = K.LPB_VARIANTS[lpb]
    n = 0
    for name, a in acts.items():
        assert bits_equal(run_direct(M, 'bool', a), wants[name])
        for parts in (1, 3):
            for kind in ('bool', 'bits', 'float', 'ids'):
                # 2 slices of 1300; one slice of 2600 (the escapes of row 0 and both long blocks in one block of 1400)
                for shift, width in ((4, 1300), (4, 2600)) if n % 2 == 0 else ((4, 1300),):
                    got = run_plan(M, kind, a, shift, width, parts, hint)
                    assert bits_equal(got, wants[name]), (name, parts, kind, shift, width)
                n += 1


@pytest.mark.parametrize('fmt', FMTS)
def test_the_row_limit_of_the_sorted_layout(fmt):
    """16384 entries in a row are planned, 16385 are refused by the plan build with BE_ERR_RANGE — and served by the direct route."""
    rng = np.random.default_rng(11)
    fc = K.finite_codes(fmt)
    k = 20000
    for n, planned in ((K.MAX_ROW, True), (K.MAX_ROW + 1, False)):
        rows = [(rng.integers(0, k, n), rng.choice(fc, n)), (rng.integers(0, k, 5), rng.choice(fc, 5))]
        M = Mat(*K.from_rows(rows, k), 2, k, fmt)
        a = np.ones(2, bool)
        want = M.expected(a)
        assert bits_equal(run_direct(M, 'bool', a), want)
        if planned:
            assert bits_equal(run_plan(M, 'bool', a, 4, k // 4, 3, 100), want)
            assert bits_equal(run_plan(M, 'ids', a, 4, k, 1, 100), want)
        else:
            assert M.plan(4, k // 4) == RANGE and 'be_scatter_plan_q8_count' in last_error() and '16384' in last_error()
            assert bits_equal(run_direct(M, 'bits', a), want)          # a clean call after the refusal


@pytest.mark.parametrize('fmt', FMTS)
def test_every_finite_code_cancellation_and_the_carry_of_the_64_bit_sum(fmt):
    fc = K.finite_codes(fmt)
    k = 300
    pmax, nmax = (0x7e, 0xfe) if fmt == 'e4m3' else (0x7b, 0xfb)
    assert K.q_table(fmt)[pmax] == K.Q_MAX[fmt] == -K.q_table(fmt)[nmax]
    assert {0x00, 0x80, 0x01, 0x81, pmax, nmax} <= set(fc.tolist())         # both zeros, the smallest subnormals, +-max
    rows = [(fc.astype(np.int32), fc),                                     # code c at column c: every finite code once
            (np.full(len(fc), 7), fc),                                     # every finite code on column 7: the sum cancels to 0
            ([10, 10, 11, 11, 299, 299], [pmax, pmax, nmax, nmax, pmax, nmax]),
            ([10, 11], [pmax, nmax])]
    M = Mat(*K.from_rows(rows, k), 4, k, fmt)
    R = K.column_sums(M.codes, M.indices, M.indptr, np.array([0, 1, 1, 0], bool), k, fmt)
    assert R[7] == 0 and R[299] == 0 and R[10] == 2 * K.Q_MAX[fmt] == -R[11]
    if fmt == 'e5m2':
        assert R[10] > 1 << 32                                              # the carry into, and the sign of, the high word
    for a in (np.ones(4, bool), np.array([0, 1, 1, 0], bool), np.array([1, 0, 0, 1], bool)):
        for scale in (1.0, 0.25, 0.3):
            want = M.expected(a, scale)
            assert bits_equal(run_direct(M, 'bool', a, scale), want)
            for i, (shift, width) in enumerate(geometries(k)):
                assert bits_equal(run_plan(M, 'bits', a, shift, width, 1 + 2 * (i % 2), HINTS[i % 3], scale), want), (scale, shift, width)


@pytest.mark.parametrize('m', [256, 257])
@pytest.mark.parametrize('fmt', FMTS)
def test_spike_encodings_batches_and_repeatability(fmt, m):
    k = 300
    rng = np.random.default_rng(m)
    M = Mat(*K.random_matrix(m, k, fmt, seed=m), m, k, fmt)
    a1 = rng.random(m) < 0.3
    want1 = M.expected(a1)
    for kind in ('bool', 'float', 'bits', 'ids'):
        d = run_direct(M, kind, a1)
        assert bits_equal(d, want1) and bits_equal(run_direct(M, kind, a1), d)             # two identical calls: identical bits
        p = run_plan(M, kind, a1, 4, 60, 3, 10)
        assert bits_equal(p, d) and bits_equal(run_plan(M, kind, a1, 4, 60, 3, 10), p)
    for nb in (1, 3, 33):
        act = rng.random((nb, m)) < 0.3
        act[nb // 2] = False                                                            # a batch row without a spike
        want = M.expected(act)
        for kind in ('bool', 'float', 'bits'):
            d = run_direct(M, kind, act)
            assert bits_equal(d, want)
            assert bits_equal(d, np.stack([run_direct(M, kind, act[b]) for b in range(nb)]))  # = nb one-vector calls
            for shift, width, parts, hint in ((4, 60, 2, 10), (4, 0, 1, 30), (4, 300, 3, 100)):
                p = run_plan(M, kind, act, shift, width, parts, hint)
                assert bits_equal(p, d), (nb, kind, shift, width)
                if nb == 3:
                    assert bits_equal(p, np.stack([run_plan(M, kind, act[b], shift, width, parts, hint) for b in range(nb)]))


def test_every_error_code_is_followed_by_a_clean_call():
    m, k, fmt = 9, 70, 'e4m3'
    M = Mat(*K.random_matrix(m, k, fmt, seed=3), m, k, fmt)
    a = np.ones(m, bool)
    want = M.expected(a)
    seg, blob = M.plan(4, 0)
    keep, sp, sd = spikes_of('bool', a)
    out = guarded(k * 4 * 2, fill=0xFF)
    wsd = guarded(fn('be_binary_csrmm_t_f8_workspace_bytes')(m, k, 2))
    wsp = guarded(fn('be_binary_csrmm_t_plan_f8_workspace_bytes')(m, k, 2, 4, 0, 3, 0))
    st = A.stream_ptr()

    def direct(codes=A.ptr(M.d_codes), f=0, scale=1.0, spikes=sp, sdt=sd, o=A.ptr(out), mm=m, kk=k, nb=1, ws=A.ptr(wsd), wb=wsd.numel() - 256):
        return fn('be_binary_csrmm_t_f8')(codes, f, scale, A.ptr(M.d_indices), A.ptr(M.d_indptr), 0, -1, M.nnz, spikes, sdt, o, mm, kk, nb,
                                          ws, wb, st)

    def plan(f=0, scale=1.0, spikes=sp, sdt=sd, o=A.ptr(out), mm=m, kk=k, nb=1, shift=4, width=0, parts=3, ws=A.ptr(wsp),
             wb=wsp.numel() - 256, b=A.ptr(blob)):
        return fn('be_binary_csrmm_t_plan_f8')(b, A.ptr(seg), f, scale, spikes, sdt, o, mm, kk, nb, shift, width, 0, parts, ws, wb, st)

    ids_keep, ids_ptr, _ = spikes_of('ids', a)
    null = ctypes.c_void_p(0)
    refusals = [
        (direct, dict(f=2), INVALID), (direct, dict(scale=float('nan')), INVALID), (direct, dict(sdt=7), INVALID),
        (direct, dict(o=null), INVALID), (direct, dict(spikes=null), INVALID), (direct, dict(codes=null), INVALID),
        (direct, dict(mm=1 << 33), INVALID), (direct, dict(nb=-1), INVALID), (direct, dict(nb=70000), INVALID),
        (direct, dict(wb=16), WORKSPACE), (direct, dict(ws=null), WORKSPACE),
        (direct, dict(spikes=ids_ptr, sdt=A.BE_SPIKE_IDS, nb=2), UNSUPPORTED),
        (plan, dict(f=-1), INVALID), (plan, dict(scale=float('inf')), INVALID), (plan, dict(sdt=4), INVALID), (plan, dict(shift=3), INVALID),
        (plan, dict(shift=16), INVALID), (plan, dict(width=-1), INVALID), (plan, dict(width=K.MAX_WIDTH + 1), INVALID),
        (plan, dict(parts=0), INVALID), (plan, dict(parts=65), INVALID), (plan, dict(o=null), INVALID), (plan, dict(b=null), INVALID),
        (plan, dict(kk=1 << 33), INVALID), (plan, dict(nb=70000), INVALID),
        (plan, dict(wb=64), WORKSPACE), (plan, dict(ws=null), WORKSPACE),
        (plan, dict(shift=15, width=0), RANGE),                                   # 32768 64-bit sums do not fit LDS
        (plan, dict(kk=16 * (K.MAX_SLICES + 1)), RANGE),                          # 1025 slices
        (plan, dict(spikes=ids_ptr, sdt=A.BE_SPIKE_IDS, nb=2), UNSUPPORTED),
    ]
    for call, kw, code in refusals:
        rc = call(**kw)
        assert rc == code, (call.__name__, kw, rc, last_error())
        assert ('be_binary_csrmm_t_f8:' if call is direct else 'be_binary_csrmm_t_plan_f8:') in last_error(), last_error()
        torch.cuda.synchronize()
        assert bool((out[:k * 8] == 0xFF).all()) and tail_ok(out, k * 8), "a refused call wrote to the output"
        assert bits_equal(run_direct(M, 'bool', a) if call is direct else run_plan(M, 'bool', a, 4, 0, 3), want)
    # the build's own refusals
    nbytes = ctypes.c_int64(0)
    scratch = A.workspace(fn('be_scatter_plan_q8_scratch_bytes')(m, 16 * (K.MAX_SLICES + 1), 4, 0))

    def count(kk=k, shift=4, width=0, sb=scratch.numel(), sg=A.ptr(seg)):
        return fn('be_scatter_plan_q8_count')(A.ptr(M.d_indices), A.ptr(M.d_indptr), 0, -1, m, kk, shift, width, sg, A.ptr(scratch), sb,
                                              ctypes.byref(nbytes), None, st)
    for kw, code in ((dict(shift=3), INVALID), (dict(width=K.MAX_WIDTH + 1), INVALID), (dict(sg=null), INVALID), (dict(sb=8), WORKSPACE),
                     (dict(kk=16 * (K.MAX_SLICES + 1)), RANGE), (dict(shift=15), RANGE)):
        assert count(**kw) == code and 'be_scatter_plan_q8_count' in last_error(), (kw, last_error())
    assert fn('be_scatter_plan_q8_fill')(A.ptr(M.d_codes), A.ptr(M.d_indices), A.ptr(M.d_indptr), 0, -1, m, k, 4, 0, A.ptr(seg), null, None,
                                         st) == INVALID
    assert fn('be_scatter_plan_q8_scratch_bytes')(m, k, 3, 0) == INVALID
    assert fn('be_binary_csrmm_t_plan_f8_workspace_bytes')(m, k, 1, 4, 0, 0, 0) == INVALID
    assert fn('be_binary_csrmm_t_f8_workspace_bytes')(-1, k, 1) == INVALID
    assert bits_equal(run_plan(M, 'bool', a, 4, 0, 3), want)
    # m, k or n_batch of zero: BE_OK and nothing else
    for kw in (dict(mm=0), dict(kk=0), dict(nb=0)):
        assert direct(**kw) == OK and plan(**kw) == OK
    torch.cuda.synchronize()
    assert bool((out[:k * 8] == 0xFF).all()) and tail_ok(out, k * 8)
    assert fn('be_binary_csrmv_t_f8_workspace_bytes')(m, k) == fn('be_binary_csrmm_t_f8_workspace_bytes')(m, k, 1)
    assert fn('be_binary_csrmv_t_plan_f8_workspace_bytes')(m, k, 4, 0, 3, 0) == fn('be_binary_csrmm_t_plan_f8_workspace_bytes')(m, k, 1, 4, 0, 3, 0)
    del keep, ids_keep


def test_the_one_vector_entry_points():
    m, k, fmt = 33, 130, 'e5m2'
    M = Mat(*K.random_matrix(m, k, fmt, seed=8), m, k, fmt)
    a = np.random.default_rng(8).random(m) < 0.5
    keep, sp, sd = spikes_of('bool', a)
    seg, blob = M.plan(4, 0)
    out = torch.empty(k, dtype=torch.float32, device='cuda')
    ws = A.workspace(fn('be_binary_csrmv_t_f8_workspace_bytes')(m, k))
    assert fn('be_binary_csrmv_t_f8')(A.ptr(M.d_codes), 1, 0.3, A.ptr(M.d_indices), A.ptr(M.d_indptr), 0, -1, M.nnz, sp, sd, A.ptr(out), m,
                                      k, A.ptr(ws), ws.numel(), A.stream_ptr()) == OK
    assert bits_equal(out.cpu().numpy(), M.expected(a, 0.3))
    ws = A.workspace(fn('be_binary_csrmv_t_plan_f8_workspace_bytes')(m, k, 4, 0, 2, 10)).zero_()
    out.fill_(-1.0)
    assert fn('be_binary_csrmv_t_plan_f8')(A.ptr(blob), A.ptr(seg), 1, 0.3, sp, sd, A.ptr(out), m, k, 4, 0, 10, 2, A.ptr(ws), ws.numel(),
                                           A.stream_ptr()) == OK
    assert bits_equal(out.cpu().numpy(), M.expected(a, 0.3))
    del keep


# ------------------------------------------------------------------------------------------------- through Python
def _csr(m, k, seed, values):
    """A CSR without duplicate positions whose weights are drawn from ``values``."""
    rng = np.random.default_rng(seed)
    dense = np.where(rng.random((m, k)) < 0.15, rng.choice(np.asarray(values, np.float32), (m, k)), np.float32(0)).astype(np.float32)
    dense[m // 2] = 0                                                                      # an empty row
    return be.CSR.fromdense(dense), dense


@pytest.fixture(params=['plan', 'direct'])
def route(request, monkeypatch):
    monkeypatch.setattr(C, 'PLAN_MIN_NNZ', 1 if request.param == 'plan' else 1 << 40)
    return request.param


@pytest.mark.parametrize('fmt', FMTS)
def test_quantize_fp8_holds_the_dense_quantisation_at_the_stored_positions(fmt):
    csr, dense = _csr(40, 70, 1, np.random.default_rng(2).standard_normal(64) * 3)
    W8 = csr.quantize_fp8(fmt)
    assert isinstance(W8, be.Float8CSR) and W8.fmt == fmt and W8.shape == (40, 70) and W8.nse == csr.nse
    assert W8.indices.data_ptr() == csr.indices.data_ptr() and W8.indptr.data_ptr() == csr.indptr.data_ptr()
    D8 = be.quantize_fp8(csr.todense(), fmt, scale=W8.scale)
    assert D8.scale == W8.scale == be.quantize_fp8(dense, fmt).scale
    rows, cols = np.nonzero(dense)
    assert np.array_equal(W8.codes.view(torch.uint8).cpu().numpy(), D8.codes.view(torch.uint8).cpu().numpy()[rows, cols])
    # tocsr() round-trips: the dequantised CSR quantises back to the same codes, and todense() is its dense form
    back = W8.tocsr()
    assert isinstance(back, be.CSR) and back.dtype == torch.float32 and back.shape == W8.shape
    deq = W8.codes.to(torch.float32).cpu() * torch.tensor(W8.scale, dtype=torch.float32)
    assert torch.equal(back.data.cpu(), deq)
    assert torch.equal(back.quantize_fp8(fmt, scale=W8.scale).codes.view(torch.uint8).cpu(), W8.codes.view(torch.uint8).cpu())
    assert np.array_equal(np.asarray(W8.todense()), back.todense())
    assert W8.tocsr(torch.float16).dtype == torch.float16
    with pytest.raises(TypeError, match='one shared weight'):
        be.CSR((np.ones(1, np.float32), csr.indices.cpu().numpy(), csr.indptr.cpu().numpy()), shape=(40, 70)).quantize_fp8(fmt)


@pytest.mark.parametrize('fmt', FMTS)
def test_the_product_equals_the_float8dense_product_on_exact_sums(fmt, route):
    """Small dyadic weights (multiples of 1/4 up to 3, exact in both formats) and a dyadic scale: every active column sum is exact in
    f32, so the Float8Dense product (an f32 sum times the scale, rounded) and this one (an integer sum times scale * 2^-E in f64,
    rounded) are each one rounding of the same number — and here not even that."""
    csr, dense = _csr(130, 300, 3, [-3, -1.5, -1, -0.5, -0.25, 0.25, 0.5, 0.75, 1, 1.25, 2, 3])
    W8 = csr.quantize_fp8(fmt, scale=0.25)
    assert np.array_equal(np.asarray(W8.todense()), dense)                                  # the quantisation is exact here
    D8 = be.quantize_fp8(W8.todense(), fmt=W8.fmt, scale=W8.scale)
    rng = np.random.default_rng(4)
    s1 = torch.from_numpy(rng.random(130) < 0.4).cuda()
    sb = torch.from_numpy(rng.random((5, 130)) < 0.4).cuda()
    for s in (s1, sb):
        got, want = be.BinaryArray(s) @ W8, be.BinaryArray(s) @ D8
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.shape == want.shape
        assert bits_equal(got.cpu().numpy(), want.cpu().numpy())
        assert bits_equal(got.cpu().numpy(), K.expected(W8.codes.view(torch.uint8).cpu().numpy(), W8.indices.cpu().numpy(),
                                                        W8.indptr.cpu().numpy(), s.cpu().numpy(), 300, fmt, 0.25))
    assert (W8._plan is not None) == (route == 'plan')


@pytest.mark.parametrize('fmt', FMTS)
def test_event_containers_numpy_results_prepare_and_the_two_routes(fmt, monkeypatch):
    m, k = 200, 500
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=9)
    rng = np.random.default_rng(9)
    s = rng.random(m) < 0.3
    sb = rng.random((3, m)) < 0.3
    want, wantb = (K.expected(codes, indices, indptr, x, k, fmt, 0.3) for x in (s, sb))
    results = {}
    for name, min_nnz in (('plan', 1), ('direct', 1 << 40)):
        monkeypatch.setattr(C, 'PLAN_MIN_NNZ', min_nnz)
        W = be.Float8CSR((codes, indices, indptr), shape=(m, k), scale=0.3, fmt=fmt)
        Wp = be.Float8CSR((codes, indices, indptr), shape=(m, k), scale=0.3, fmt=fmt).prepare()
        assert (Wp._plan is not None) == (name == 'plan') and W._plan is None
        if name == 'plan':
            assert isinstance(Wp._plan, be.Q8Plan) and Wp._plan.nbytes() > 0 and Wp._plan.n_slices >= 1
        r = be.BinaryArray(s) @ W                                                       # numpy in -> numpy out
        assert isinstance(r, np.ndarray) and bits_equal(r, want)
        assert bits_equal(be.BinaryArray(s) @ Wp, r)                                    # prepare() changes nothing but the time
        rb = be.BinaryArray(sb) @ W
        assert isinstance(rb, np.ndarray) and bits_equal(rb, wantb)
        st = torch.from_numpy(s).cuda()
        rt = be.BinaryArray(st) @ W
        assert isinstance(rt, torch.Tensor) and rt.is_cuda and bits_equal(rt.cpu().numpy(), want)
        assert bits_equal((be.BitPackedBinary(st) @ W).cpu().numpy(), want)             # packed words
        assert bits_equal((be.CompactBinary.from_array(st) @ W).cpu().numpy(), want)    # the compacted id list
        assert bits_equal((be.BinaryArray(torch.from_numpy(np.where(s, 2.0, -1.0).astype(np.float32)).cuda()) @ W).cpu().numpy(), want)
        ring = be.SpikeRing(m, 4)
        ring.push(st)
        ring.push(torch.zeros_like(st))
        assert bits_equal((ring.events(1) @ W).cpu().numpy(), want)                     # the spikes of one step ago
        results[name] = rt.cpu().numpy()
        Wt = be.Float8CSR((torch.from_numpy(codes).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(indptr).cuda()),
                          shape=(m, k), scale=0.3, fmt=fmt)
        assert isinstance(be.BinaryArray(s) @ Wt, torch.Tensor)
        with pytest.raises(NotImplementedError, match='gather direction'):
            W @ be.BinaryArray(np.ones(k, bool))
    assert bits_equal(results['plan'], results['direct'])
    E = be.Float8CSR((np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(m + 1, np.int32)), shape=(m, k), fmt=fmt)
    assert not (be.BinaryArray(s) @ E).any()


@pytest.mark.parametrize('fmt', FMTS)
def test_a_captured_product_replays_with_new_spikes(fmt, route):
    m, k = 300, 700
    codes, indices, indptr = K.random_matrix(m, k, fmt, seed=12)
    W = be.Float8CSR((torch.from_numpy(codes).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(indptr).cuda()), shape=(m, k),
                     scale=0.5, fmt=fmt)
    rng = np.random.default_rng(12)
    s = torch.zeros(m, dtype=torch.bool, device='cuda')
    step = be.capture_step(lambda: be.BinaryArray(s) @ W)
    for _ in range(3):
        a = rng.random(m) < 0.3
        s.copy_(torch.from_numpy(a))
        got = step().cpu().numpy()
        assert bits_equal(got, K.expected(codes, indices, indptr, a, k, fmt, 0.5))
    assert (W._plan is not None) == (route == 'plan')
