"""The planned scatter step — the accumulate kernels, the table gathers, the reduce and the single-launch kernel of
``csrc/be_csr_plan.hip`` — against ``plan_step_cases.Case.reference``, bit for bit, in every kernel instance the host can launch at
default settings.  Every comparison is an equality of the output's bits (integers of the element size); there is no tolerance in this
file.  Why equality is the right bar is argued in the docstring of ``tests/plan_step_cases.py``; ``tests/test_plan_step_thresholds_cpu.py``
holds the constants the cases are sized by to the source and proves, without a GPU, that the tables below cover the ledger.

The plans are host-encoded (``plan_layout_cases.encode`` laid out by ``plan_step_cases.blob_of`` into a poisoned blob) and stepped
through the C entry point at a pinned exponent, except where a test says it builds with ``ScatterPlan.build``.

After every step, through `step_and_check`: the output equals the reference; the 8 spare elements behind it still hold the sentinel;
the 4096 bytes of 0xAB behind the workspace size the library asked for are intact (the workspace itself starts as 32-bit ones); the per-batch spike counters read zero; and two more steps
on the same workspace — other spikes, then none — are exact too (stale lists, stale table entries, stale partial sums).

Which test reaches what (`instance_of` names the instance at the top of each test, with the real alignment of the spike buffer):

  test_decoders            every accumulate instance of REACHABLE (56 of the 60 compiled): each LPB class of each layout by the hints
                           at both ends of its range; FUSED 0 (float spikes; a bool buffer one byte off 16-byte alignment), 1
                           (bit-packed, the bits past m set), 2 (aligned bool), 3 through k_gather_seg, k_compact_gather_seg<1> and <2>;
                           vectors and 3-row batches; blocks longer than LPB and than 64 lane-groups; duplicate columns; u16 pads at
                           slot 64 of 60-column slices; the crafted d8 / h8 blocks (escape runs inside the first lane-groups and across
                           the 8th, 16th and 64th lane-group boundary, a first local column of 5, blocks of exactly 4, 5, 8, 9, 16, 17,
                           32, 33, 64, 65 and 130 lane-groups, tail pads) — under every hint class, so each falls into the pipelined
                           pass in one case and into the serial tail in another
  test_skeleton  tasks-*   idle workgroups (6, 8, 9 and 33 tasks)
                 parts-*   every arm of sum_parts' switch, two and eight rounds of 8, both accumulator types
                 pipeline-*  the third rotation of PlanRows' pointers in FUSED 0, 1, 2 and 3
                 list-*    build_part_list: a second iteration, a list that outgrows LDS in the first, and one that fits the first
                           and restarts from the second with base > 0; bit-packed and byte spikes; m % 32 != 0 and m % 16 != 0
                 gather-*  gather_tile's s0 loop (65, 130 slices), k_gather_seg's grid stride, a last tile of 7 rows
                 compact-* k_compact_gather_seg<1 | 2> below, at and past 4096 rows; a workgroup without a spike; all; none
                 reduce-*  the column loop of k_plan_reduce<W, HOMO> past its grid for every W and both HOMO (vector and batch of 8);
                           partial-sum strides above the slice width; a narrower last slice
                 batch*    2, 3 and 8 rows, a silent row, bool rows with m % 16 != 0 (FUSED 0) and == 0 (FUSED 2), bit-packed rows
                           whose last word ends in set bits
  test_single_launch       all 24 k_plan_single instances at m = 1, 4095, 4096, 4097 and 8193 with no, some and all rows active
  test_f64                 f64 through ScatterPlan.build: split per-entry weights, one shared f64 weight, and the one-slice shape the
                           single-launch kernel leaves to the sliced path
  test_library_plans       ScatterPlan.build + _plan_call at the library's exponent (check_exact holds there too)

Compiled but not reached at default settings (FUSED 3 needs a hint <= 64, these decoders are chosen above it; they are not reached
through the environment either): k_plan_accumulate<true, 32, 3>, <true, 0, 3>, <false, 0, 3> and k_plan_accumulate_d8<0, 3, BE_BLOCK_AUX>.

Expected but not proven by a counter: that the list-* cases take the LDS -> workspace restart (the test only knows the list lengths
and the restated ``lds_cap``), that the idle workgroups of tasks-* are the ones the restated task mapping names, and the trip counts
of the loops, which are computed from CONSTS (the CPU module asserts them), not read back from the device.

Sizes: every case is the smallest that reaches its trip count.  The largest are forced by constants of the source: gather-65-slices
(512 x 64 listed rows x 65 slices of table: `k_gather_seg`'s grid), list-* (32 x 1024 rows per part: one iteration of
build_part_list), reduce-vector-* (2048 x 256 columns: the reduce's grid)."""
import functools
import os

import numpy as np
import pytest
import torch

import plan_step_cases as P
from brainevent_amd import _array as A
from brainevent_amd._csr import ScatterPlan, _plan_call
from brainevent_amd._lib import call, fn

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
INT_OF = {2: np.int16, 4: np.int32, 8: np.int64}
WCODE = {'f32': A.BE_F32, 'f64': A.BE_F64, 'f16': A.BE_F16, 'bf16': A.BE_BF16}
SPIKE_CODE = {'bool': A.BE_SPIKE_BOOL, 'float': A.BE_SPIKE_FLOAT, 'bits': A.BE_SPIKE_BITS}
SENTINEL, SPARE, GUARD = 7.0, 8, 4096
TABLES = P.tables()


def _default_settings():
    assert not any(v in os.environ for v in ('BE_PLAN_FUSED', 'BE_PLAN_PREGATHER_SLICES', 'BE_PLAN_PREGATHER_MAX')), \
        'instance_of restates the default settings only'


# ------------------------------------------------------------------------------------------------------------ helpers
def bits_of(x) -> np.ndarray:
    """The elements as integers of their size (numpy array or torch tensor, any device)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        return x.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]).numpy()
    x = np.ascontiguousarray(x)
    return x.view(INT_OF[x.dtype.itemsize])


def assert_bits(got, want, tag):
    g, w = bits_of(got).reshape(-1), bits_of(want).reshape(-1)
    assert g.shape == w.shape, tag
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        j = int(bad[0])
        gv = got.detach().cpu().reshape(-1)[j].item() if isinstance(got, torch.Tensor) else got.reshape(-1)[j]
        wv = want.reshape(-1)[j].item() if isinstance(want, torch.Tensor) else want.reshape(-1)[j]
        raise AssertionError(f'{tag}: {bad.size} of {g.size} outputs differ; the first is element {j}: got {gv!r} ({g[j]:#x}), '
                             f'the reference says {wv!r} ({w[j]:#x})')


def device_spikes(case, active):
    """(tensor, spike dtype code) of bool [n_batch, m] in the case's encoding.  float: 2.5 fires, 0 and -1 do not; bits: 32 rows per
    word, the bits past m of every batch row's last word SET; bool: bytes 1 and 3 fire; bool_off: the same one byte off alignment."""
    nb, m = active.shape
    if case.spikes == 'float':
        quiet = np.where(np.arange(m) % 3 == 0, -1.0, 0.0)
        t = torch.from_numpy(np.where(active, 2.5, quiet).astype(np.float32)).cuda()
    elif case.spikes == 'bits':
        words = (m + 31) // 32
        b = np.ones((nb, words * 32), bool)
        b[:, :m] = active
        t = torch.from_numpy(np.packbits(b, axis=1, bitorder='little').view(np.int32).copy()).cuda()
    else:
        v = torch.from_numpy(np.where(active, np.where(np.arange(m) % 2 == 0, 1, 3), 0).astype(np.uint8))
        if case.spikes == 'bool':
            t = v.cuda()
        else:
            buf = torch.zeros(nb * m + 32, dtype=torch.uint8, device='cuda')
            t = buf[1:1 + nb * m].view(nb, m)
            t.copy_(v)
            assert t.data_ptr() % 16 == 1
    if case.spikes == 'bool':
        assert t.data_ptr() % 16 == 0
    assert t.is_contiguous()
    return t, SPIKE_CODE[case.spike_dtype]


@functools.lru_cache(maxsize=8)
def device_plan(matrix, kind):
    """(blob, seg) of the host-encoded plan on the device."""
    enc = matrix.encoded(kind)
    blob = torch.from_numpy(P.blob_of(enc)).cuda()
    seg = torch.from_numpy(enc.seg.reshape(-1).view(np.int32).copy()).cuda()
    return blob, seg


def check_instance(case, spikes_t):
    """`instance_of` with the real alignment names what the case was made for."""
    inst = case.instance(aligned16=spikes_t.data_ptr() % 16 == 0)
    assert inst == case.instance(), (case.id, inst, case.instance())
    assert set(case.want) <= P.parts_of_instance(inst), (case.id, case.want, inst)
    return inst


class Workspace:
    def __init__(self, case):
        args = case.ws_args()
        lib = fn('be_binary_csrmm_t_plan_workspace_bytes_for')(*args, int(case.hint)) if case.table else \
            fn('be_binary_csrmm_t_plan_workspace_bytes')(*args)
        assert lib == case.ws_bytes()
        self.need, self.n_batch = int(lib), case.n_batch
        # behind the size: 0xAB.  Inside: every 32-bit word 1 — a stale row id that is a row, a stale table entry that is a block, a
        # stale partial sum that is wrong — so a step that reads what it did not write gives a wrong number, not a wild address
        assert self.need % 4 == 0
        self.t = torch.full((self.need + GUARD,), 0xAB, dtype=torch.uint8, device='cuda')
        self.t[:self.need].view(torch.int32).fill_(1)
        self.t[:P.counts_bytes(case.n_batch)].zero_()          # the counters are zero on entry (caller contract)

    def check(self, tag):
        assert bool((self.t[self.need:] == 0xAB).all()), f'{tag}: the step wrote behind its workspace'
        counters = self.t[:4 * self.n_batch].cpu().numpy().view(np.uint32)
        assert not counters.any(), f'{tag}: spike counters left at {counters.tolist()}'


def one_step(case, blob, seg, ws, active, scale_exp, tag, first=False):
    mx = case.matrix
    sp, sd = device_spikes(case, active)
    if first:
        check_instance(case, sp)
    n = case.n_batch * mx.k
    out = torch.full((n + SPARE,), SENTINEL, dtype=TORCH[case.wdtype], device='cuda')
    w1 = torch.tensor([case.shared], dtype=TORCH[case.wdtype], device='cuda')
    call('be_binary_csrmm_t_plan', A.ptr(w1), int(case.homo), WCODE[case.wdtype], A.ptr(blob), A.ptr(seg), A.ptr(sp), sd, A.ptr(out),
         mx.m, mx.k, case.n_batch, mx.slice_shift, mx.slice_width, P.LAYOUT_CODE[case.layout], int(case.hint), case.parts,
         int(scale_exp), A.ptr(ws.t), ws.need, A.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all()), f'{tag}: the step wrote behind its output'
    assert_bits(out[:n], case.reference(active), tag)
    ws.check(tag)


def step_and_check(case):
    """Three steps on one workspace: the case's spikes, another draw, none."""
    _default_settings()
    blob, seg = device_plan(case.matrix, case.kind)
    ws = Workspace(case)
    for step in (0, 1, 2):
        one_step(case, blob, seg, ws, case.active(step), case.scale_exp(), f'{case.id}, step {step}', first=step == 0)


def ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize('case', TABLES['decoder'], ids=ids(TABLES['decoder']))
def test_decoders(case):
    step_and_check(case)


@pytest.mark.parametrize('case', TABLES['skeleton'], ids=ids(TABLES['skeleton']))
def test_skeleton(case):
    step_and_check(case)


@pytest.mark.parametrize('case', TABLES['single'], ids=ids(TABLES['single']))
def test_single_launch(case):
    """One instance of k_plan_single: m on both sides of the 4096-spike chunk, with no, some and all rows active."""
    _default_settings()
    for m in P.SINGLE_M:
        sub = P.Case(f'{case.id}-m{m}', P.head_of(case.matrix, m), case.kind, case.spikes, case.pat, 1, 1, case.hint, case.wdtype,
                     want=case.want)
        blob, seg = device_plan(sub.matrix, sub.kind)
        ws = Workspace(sub)
        for i, pat in enumerate(('none', 'tenth', 'all')):
            one_step(sub, blob, seg, ws, P.pattern(sub.matrix, pat, 1), sub.scale_exp(), f'{sub.id}, {pat}', first=i == 0)


def _library_plan(case, weights):
    mx = case.matrix
    plan = ScatterPlan.build(weights, torch.from_numpy(mx.indices.copy()), torch.from_numpy(mx.indptr.copy()), shape=(mx.m, mx.k),
                             slice_shift=mx.slice_shift, slice_width=mx.slice_width, layout=case.layout)
    assert plan.layout == P.LAYOUT_CODE[case.layout] and plan.n_slices == mx.n_slices and plan.homo == case.homo
    plan.block_hint_override = case.hint
    return plan


def _library_steps(case, plan, wd):
    case.check_exact(plan.scale_exp)
    mx = case.matrix
    n = case.n_batch * mx.k
    for step in (0, 1, 2):
        active = case.active(step)
        sp, sd = device_spikes(case, active)
        if step == 0:
            check_instance(case, sp)
        full = torch.full((n + SPARE,), SENTINEL, dtype=TORCH[case.wdtype], device='cuda')
        _plan_call(plan, wd, sp[0] if case.n_batch == 1 else sp, sd, full[:n] if case.n_batch == 1 else full[:n].view(case.n_batch, mx.k),
                   parts=case.parts)
        torch.cuda.synchronize()
        assert bool((full[n:] == SENTINEL).all())
        assert_bits(full[:n], case.reference(active), f'{case.id}, step {step}, exponent {plan.scale_exp}')


@pytest.mark.parametrize('case', TABLES['f64'], ids=ids(TABLES['f64']))
def test_f64(case):
    """f64 through ScatterPlan.build: per-entry weights as two f32 entries (`split_f64`), or one shared f64 weight.  The single-launch
    kernel has no f64 instance: `instance_of` sends the one-slice shape to the sliced path."""
    _default_settings()
    assert case.instance()[0] == 'sliced'
    w = torch.tensor([case.shared], dtype=torch.float64) if case.homo else torch.from_numpy(case.matrix.weights().copy())
    plan = _library_plan(case, w)
    assert plan.split_f64 == (not case.homo)
    _library_steps(case, plan, A.to_device(w))


@pytest.mark.parametrize('case', TABLES['library'], ids=ids(TABLES['library']))
def test_library_plans(case):
    """The build and the exponent are the library's; the result is the same reference, bit for bit."""
    _default_settings()
    w = torch.tensor([case.shared], dtype=torch.float32) if case.homo else torch.from_numpy(case.matrix.weights().astype(np.float32))
    plan = _library_plan(case, w)
    _library_steps(case, plan, A.to_device(w))
