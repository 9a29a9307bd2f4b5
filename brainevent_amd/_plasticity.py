"""Spike-triggered plasticity: the additive pair-based STDP updates of the reference
(``brainevent/_csr/plasticity_binary.py``, ``brainevent/_dense/plasticity_binary.py``, ``brainevent/_fcn/plasticity_binary.py``)
and the ``update_on_pre`` / ``update_on_post`` methods of ``CSR``, ``CSC``, ``Dense``, ``FixedNumPerPre`` and ``FixedNumPerPost``
(``_csr/main.py:1389-1455``, ``:2290-2360``; ``_dense/main.py:477-510``; ``_fcn/main.py:627-680``, ``:987-1003``, ``:1256-1272``).

Rule (the reference's order of operations):
  pre : for every active pre neuron ``i`` and every stored synapse ``(i, j)``:  ``w += post_trace[j]``
  post: for every active post neuron ``j`` and every stored synapse ``(i, j)``: ``w += pre_trace[i]``
  then ``clip(w, w_min, w_max)`` over the WHOLE weight array (``min(max(w, w_min), w_max)``; ``None`` disables a bound).
A spike is any nonzero value.  The trace is cast to the weight dtype first; f16 / bf16 add in f32 and round once.

The hot path is ``csrc/be_plasticity.hip``: ``be_plasticity_rows`` (row-driven, or through a slot -> weight permutation for the
unfavourable direction), ``be_plasticity_rows_aged`` (the permuted walk with the trace read by age from a ring of values: the
post-spike update of delayed synapses, ``DelayedCSR.update_on_post``) and ``be_plasticity_dense``.  The functional API copies
the weights, runs the kernel unclipped and clamps the whole copy.  The methods also take ``inplace=True``: the container's own ``data`` is updated and, once the container has
established that every weight lies in ``[w_min, w_max]`` (a *clip certificate* kept in ``buffers``), the kernel clips the
touched entries only, which gives the same result without a pass over the whole array.

Captured graphs (``capture_step``): the calls never synchronise the host, but a replay repeats the path chosen at capture time
(certified or not).  A step captured on the certified path assumes that nothing else writes ``data`` out of range between
replays — the same contract as :meth:`CSR.refresh_weights`.
"""
import math
import numbers
from typing import Optional

import numpy as np
import torch

from . import _array as A
from ._event import is_event, event_operand
from ._lib import check, fn      # (not `call`: every lookup goes through this module's own `fn`, which the validation tests bar)

__all__ = ['update_csr_on_binary_pre', 'update_csr_on_binary_post', 'update_csc_on_binary_pre', 'update_csc_on_binary_post',
           'update_dense_on_binary_pre', 'update_dense_on_binary_post', 'update_fixed_post_conn_on_binary_pre',
           'update_fixed_pre_conn_on_binary_post']


_HOMO_MSG = ("Plasticity updates require per-synapse (heterogeneous) weights, but received "
             "a homogeneous (size-1) weight. Materialize per-synapse weights first "
             "(e.g. broadcast to the connectivity shape) before applying a plasticity update.")

CLIP_KEY = 'plasticity_clip'        # buffers: (weights_stamp(data), w_min, w_max) while every weight lies in the bounds
INDEX_KEY = 'plasticity_index'      # buffers: (t_indptr, t_rows, perm) of the transposed structure (structure only)
PLASTIC_KEY = 'plastic'             # buffers: the state of prepare(plastic=...) while the container is armed (arm_plastic)


# =====================================================================================================
# validation (host only: nothing here touches the device)
# =====================================================================================================
def _shape_of(x):
    if is_event(x) or isinstance(x, (torch.Tensor, np.ndarray, A.PackedSpikes, A.ActiveIds)):
        return tuple(int(s) for s in x.shape)
    return tuple(np.shape(x))


def _numel(x) -> int:
    return int(np.prod(_shape_of(x), dtype=np.int64))


def _check_vec(x, n: int, what: str) -> None:
    s = _shape_of(x)
    if len(s) != 1 or s[0] != n:
        raise ValueError(f"{what} must have shape ({n},); got {s}.")


def _check_weight(weight, n_syn: int) -> None:
    if _numel(weight) == 1 and n_syn > 1:
        raise ValueError(_HOMO_MSG)
    dt = weight.dtype if isinstance(weight, (torch.Tensor, np.ndarray)) else np.asarray(weight).dtype
    ok = dt.is_floating_point if isinstance(dt, torch.dtype) else np.issubdtype(dt, np.floating)
    if not ok:
        raise ValueError(f"weights must be a floating-point array; got {dt}.")


def _bound(b, what: str):
    """``None``, a float (host value) or a one-element device tensor."""
    if b is None:
        return None
    if isinstance(b, bool) or not isinstance(b, (numbers.Number, np.generic, np.ndarray, torch.Tensor)):
        raise ValueError(f"{what} must be None, a number or a one-element array; got {type(b).__name__}.")
    if isinstance(b, (numbers.Number, np.generic)):
        return float(b)
    if b.size == 1 if isinstance(b, np.ndarray) else b.numel() == 1:
        if isinstance(b, torch.Tensor) and b.is_cuda:
            return b
        return float(np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b).reshape(()))
    raise ValueError(f"{what} must be a scalar (one element); got shape {tuple(b.shape)}.")


def _bounds(w_min, w_max):
    return _bound(w_min, 'w_min'), _bound(w_max, 'w_max')


# =====================================================================================================
# device side
# =====================================================================================================
def _spikes(x):
    """Event operand -> (buffer, spike code): ids / words / bytes / f32 (any nonzero value is a spike).  A pair that this
    function returned passes through (one conversion for the update and the plan's upkeep)."""
    if isinstance(x, tuple):
        return x
    v = event_operand(x, scatter=True) if is_event(x) else x
    if isinstance(v, A.ActiveIds):
        return v, A.BE_SPIKE_IDS
    if isinstance(v, A.PackedSpikes):
        return A.to_device(v.bits), A.BE_SPIKE_BITS
    t = A.to_device(v)
    if t.dtype in (torch.bool, torch.uint8, torch.int8):
        return t, A.BE_SPIKE_BOOL
    if t.dtype == torch.float32:
        return t, A.BE_SPIKE_FLOAT
    return (t != 0), A.BE_SPIKE_BOOL


def _rounded(b, dtype):
    """A host bound as a value of the weight dtype (the kernel compares in that dtype)."""
    return float(torch.tensor(b, dtype=torch.float64).to(dtype).to(torch.float64))


def _clip_args(w: torch.Tensor, lo, hi):
    if lo is None and hi is None:
        return 0, 0.0, 0, 0.0
    return int(lo is not None), (0.0 if lo is None else _rounded(lo, w.dtype)), int(hi is not None), \
        (0.0 if hi is None else _rounded(hi, w.dtype))


def _workspace(n: int) -> torch.Tensor:
    return A.workspace(fn('be_plasticity_workspace_bytes')(int(n)))


def _run_rows(w: torch.Tensor, col, indptr, row_len: int, perm, spikes, n_rows: int, trace, clip=(None, None)) -> None:
    """``be_plasticity_rows`` on ``w`` in place (``clip``: bounds applied to the touched entries only)."""
    sp, sd = _spikes(spikes)
    tr = A.to_device(trace).to(w.dtype).contiguous()
    ws = _workspace(n_rows)
    f = fn('be_plasticity_rows')
    lo_on, lo, hi_on, hi = _clip_args(w, *clip)
    check(f(A.ptr(w), A.wcode(w), A.ptr(col), A.ptr(indptr), int(indptr is not None and indptr.dtype == torch.int64),
            int(row_len), int(col.numel()), A.ptr(perm), int(perm is not None and perm.dtype == torch.int64), A.ptr(sp), sd,
            int(n_rows), A.ptr(tr), lo_on, lo, hi_on, hi, A.ptr(ws), ws.numel(), A.stream_ptr()), 'be_plasticity_rows')


def _run_rows_aged(w: torch.Tensor, t_rows, t_indptr, perm, spikes, n_post: int, hist, ages: int, clip=(None, None)) -> None:
    """``be_plasticity_rows_aged`` on ``w`` in place: the permuted walk over the transposed structure of a matrix stacked by
    delay, the trace read by age from ``hist`` (a :class:`~brainevent_amd.ValueRing` of ``w``'s dtype over the pre neurons)."""
    sp, sd = _spikes(spikes)
    ws = _workspace(n_post)
    f = fn('be_plasticity_rows_aged')
    lo_on, lo, hi_on, hi = _clip_args(w, *clip)
    check(f(A.ptr(w), A.wcode(w), A.ptr(t_rows), A.ptr(t_indptr), int(t_indptr.dtype == torch.int64), int(t_rows.numel()),
            A.ptr(perm), int(perm.dtype == torch.int64), A.ptr(sp), sd, int(n_post), A.ptr(hist.values), A.ptr(hist.head),
            int(hist.n), int(hist.depth), int(ages), lo_on, lo, hi_on, hi, A.ptr(ws), ws.numel(), A.stream_ptr()),
          'be_plasticity_rows_aged')


def _run_dense(w: torch.Tensor, pre: bool, spikes, trace, clip=(None, None)) -> None:
    sp, sd = _spikes(spikes)
    tr = A.to_device(trace).to(w.dtype).contiguous()
    n_rows, n_cols = int(w.shape[0]), int(w.shape[1])
    ws = _workspace(n_rows if pre else n_cols)
    f = fn('be_plasticity_dense')
    lo_on, lo, hi_on, hi = _clip_args(w, *clip)
    check(f(int(pre), A.ptr(w), A.wcode(w), n_rows, n_cols, A.ptr(sp), sd, A.ptr(tr), lo_on, lo, hi_on, hi, A.ptr(ws),
            ws.numel(), A.stream_ptr()), 'be_plasticity_dense')


def _clamp_(w: torch.Tensor, lo, hi) -> None:
    """The reference's whole-array ``clip`` (torch.clamp: ``min(max(w, lo), hi)``, NaN kept)."""
    if lo is None and hi is None:
        return
    as_arg = (lambda b: None if b is None else (b.to(device=w.device, dtype=w.dtype).reshape(()) if isinstance(b, torch.Tensor)
                                                else _rounded(b, w.dtype)))
    lo_t, hi_t = as_arg(lo), as_arg(hi)
    if isinstance(lo_t, torch.Tensor) or isinstance(hi_t, torch.Tensor):
        if lo_t is not None:
            torch.maximum(w, lo_t if isinstance(lo_t, torch.Tensor) else torch.tensor(lo_t, dtype=w.dtype, device=w.device), out=w)
        if hi_t is not None:
            torch.minimum(w, hi_t if isinstance(hi_t, torch.Tensor) else torch.tensor(hi_t, dtype=w.dtype, device=w.device), out=w)
        return
    w.clamp_(min=lo_t, max=hi_t)


def _functional(weight, run, lo, hi, *others):
    """Copy, update without clipping, clamp the whole copy; numpy in -> numpy out."""
    as_np = A.wants_numpy(weight, *others)
    w = A.to_device(weight).clone()
    run(w)
    _clamp_(w, lo, hi)
    return A.to_result(w, as_np)


def _as_index(x):
    return A.to_device(x)


# =====================================================================================================
# functional API (the reference's signatures)
# =====================================================================================================
def update_csr_on_binary_pre(weight, indices, indptr, pre_spike, post_trace, w_min=None, w_max=None, *, shape,
                             backend: Optional[str] = None):
    """``weight[e] += post_trace[indices[e]]`` for every entry ``e`` of every active row, then ``clip(weight, w_min, w_max)``
    (reference ``brainevent/_csr/plasticity_binary.py:45-173``).  Returns a new weight array.

    >>> update_csr_on_binary_pre(np.array([0.5, 0.3, 0.8, 0.2], np.float32), np.array([0, 1, 0, 2], np.int32),
    ...                          np.array([0, 2, 4], np.int32), np.array([True, False]),
    ...                          np.array([0.1, 0.2, 0.05], np.float32), shape=(2, 3))        # doctest: +SKIP
    array([0.6, 0.5, 0.8, 0.2], dtype=float32)
    """
    m, k = int(shape[0]), int(shape[1])
    nnz = _numel(indices)
    _check_weight(weight, nnz)
    if _numel(weight) != nnz:
        raise ValueError(f"weight has {_numel(weight)} entries, indices {nnz}.")
    _check_vec(indptr, m + 1, 'indptr')
    _check_vec(pre_spike, m, 'pre_spike')
    _check_vec(post_trace, k, 'post_trace')
    lo, hi = _bounds(w_min, w_max)

    def run(w):
        _run_rows(w, A.to_device(indices).to(torch.int32), _as_index(indptr), -1, None, pre_spike, m, post_trace)
    return _functional(weight, run, lo, hi, indices, indptr)


def update_csr_on_binary_post(weight, indices, indptr, weight_indices, pre_trace, post_spike, w_min=None, w_max=None, *, shape,
                              backend: Optional[str] = None):
    """``weight[weight_indices[s]] += pre_trace[indices[s]]`` for every slot ``s`` of every active column, then the whole-array
    clip; ``indices`` / ``indptr`` are the CSC arrays of the matrix and ``weight_indices`` the CSC -> CSR permutation (reference
    ``brainevent/_csr/plasticity_binary.py:477-618``).  Returns a new weight array.

    >>> update_csr_on_binary_post(np.array([1., 2., 3., 4.], np.float32), np.array([0, 1, 0, 1], np.int32),
    ...                           np.array([0, 2, 4], np.int32), np.array([0, 2, 1, 3], np.int32),
    ...                           np.array([0.5, 1.5], np.float32), np.array([False, True]), shape=(2, 2))  # doctest: +SKIP
    array([1. , 2.5, 3. , 5.5], dtype=float32)
    """
    m, k = int(shape[0]), int(shape[1])
    nnz = _numel(indices)
    _check_weight(weight, nnz)
    if not (_numel(weight) == nnz == _numel(weight_indices)):
        raise ValueError(f"weight ({_numel(weight)}), weight_indices ({_numel(weight_indices)}) and indices ({nnz}) must have "
                         "the same number of entries.")
    _check_vec(indptr, k + 1, 'indptr')
    _check_vec(post_spike, k, 'post_spike')
    _check_vec(pre_trace, m, 'pre_trace')
    lo, hi = _bounds(w_min, w_max)

    def run(w):
        p = A.to_device(weight_indices)
        p = p if p.dtype in (torch.int32, torch.int64) else p.to(torch.int64)
        _run_rows(w.reshape(-1), A.to_device(indices).to(torch.int32), _as_index(indptr), -1, p, post_spike, k, pre_trace)
    return _functional(weight, run, lo, hi, indices, indptr)


def update_csc_on_binary_pre(weight, indices, indptr, pre_spike, post_trace, w_min=None, w_max=None, *, shape,
                             backend: Optional[str] = None):
    """Pre-spike update of a CSC matrix ``(n_pre, n_post)`` (reference ``_csr/plasticity_binary.py:968-1063``): the
    unfavourable direction, through the CSC -> CSR permutation built here (``csc_to_csr_index``)."""
    from ._convert import csc_to_csr_index
    m, k = int(shape[0]), int(shape[1])
    _check_weight(weight, _numel(indices))
    if _numel(weight) != _numel(indices):
        raise ValueError(f"weight has {_numel(weight)} entries, indices {_numel(indices)}.")
    _check_vec(indptr, k + 1, 'indptr')
    _check_vec(pre_spike, m, 'pre_spike')
    _check_vec(post_trace, k, 'post_trace')
    _bounds(w_min, w_max)
    csr_indptr, csr_indices, perm = csc_to_csr_index(A.to_device(indptr), A.to_device(indices), shape=(m, k))
    out = update_csr_on_binary_post(A.to_device(weight), csr_indices, csr_indptr, perm, post_trace, pre_spike, w_min, w_max,
                                    shape=(k, m), backend=backend)
    return A.to_result(out, A.wants_numpy(weight, indices, indptr))


def update_csc_on_binary_post(weight, indices, indptr, pre_trace, post_spike, w_min=None, w_max=None, *, shape,
                              backend: Optional[str] = None):
    """Post-spike update of a CSC matrix: the favourable, row-driven direction over the stored columns (reference
    ``_csr/plasticity_binary.py:1066-1160``)."""
    return update_csr_on_binary_pre(weight, indices, indptr, post_spike, pre_trace, w_min, w_max, shape=(int(shape[1]), int(shape[0])),
                                    backend=backend)


def update_dense_on_binary_pre(weight, pre_spike, post_trace, w_min=None, w_max=None, *, backend: Optional[str] = None):
    """``W[i, :] += post_trace`` for every active pre neuron ``i``, then the whole-array clip (reference
    ``brainevent/_dense/plasticity_binary.py:42-140``)."""
    s = _shape_of(weight)
    if len(s) != 2:
        raise ValueError(f"weight must be 2-D; got shape {s}.")
    _check_weight(weight, s[0] * s[1])
    _check_vec(pre_spike, s[0], 'pre_spike')
    _check_vec(post_trace, s[1], 'post_trace')
    lo, hi = _bounds(w_min, w_max)
    return _functional(weight, lambda w: _run_dense(w, True, pre_spike, post_trace), lo, hi)


def update_dense_on_binary_post(weight, pre_trace, post_spike, w_min=None, w_max=None, *, backend: Optional[str] = None):
    """``W[:, j] += pre_trace`` for every active post neuron ``j``, then the whole-array clip (reference
    ``brainevent/_dense/plasticity_binary.py:360-458``)."""
    s = _shape_of(weight)
    if len(s) != 2:
        raise ValueError(f"weight must be 2-D; got shape {s}.")
    _check_weight(weight, s[0] * s[1])
    _check_vec(pre_trace, s[0], 'pre_trace')
    _check_vec(post_spike, s[1], 'post_spike')
    lo, hi = _bounds(w_min, w_max)
    return _functional(weight, lambda w: _run_dense(w, False, post_spike, pre_trace), lo, hi)


def _check_fcn(data, indices, n_rows: int):
    s = _shape_of(indices)
    if len(s) != 2 or s[0] != n_rows:
        raise ValueError(f"indices must have shape ({n_rows}, num_conn); got {s}.")
    _check_weight(data, s[0] * s[1])
    if _shape_of(data) != s:
        raise ValueError(f"data shape {_shape_of(data)} must match indices shape {s}.")


def update_fixed_post_conn_on_binary_pre(data, indices, pre_spike, post_trace, w_min=None, w_max=None, *, shape,
                                         backend: Optional[str] = None):
    """Pre-spike update of a ``FixedNumPerPre`` (``indices (num_pre, num_conn)`` = post ids): row-driven over the implicit
    rows (reference ``brainevent/_fcn/plasticity_binary.py:207-266``)."""
    n_pre, n_post = int(shape[0]), int(shape[1])
    _check_fcn(data, indices, n_pre)
    _check_vec(pre_spike, n_pre, 'pre_spike')
    _check_vec(post_trace, n_post, 'post_trace')
    lo, hi = _bounds(w_min, w_max)

    def run(w):
        idx = A.to_device(indices).to(torch.int32)
        _run_rows(w, idx, None, int(idx.shape[1]), None, pre_spike, n_pre, post_trace)
    return _functional(data, run, lo, hi, indices)


def update_fixed_pre_conn_on_binary_post(data, indices, pre_trace, post_spike, w_min=None, w_max=None, *, shape,
                                         backend: Optional[str] = None):
    """Post-spike update of a ``FixedNumPerPost`` (``indices (num_post, num_conn)`` = pre ids): row-driven over the implicit
    rows (reference ``brainevent/_fcn/plasticity_binary.py:269-300``)."""
    n_pre, n_post = int(shape[0]), int(shape[1])
    _check_fcn(data, indices, n_post)
    _check_vec(pre_trace, n_pre, 'pre_trace')
    _check_vec(post_spike, n_post, 'post_spike')
    lo, hi = _bounds(w_min, w_max)

    def run(w):
        idx = A.to_device(indices).to(torch.int32)
        _run_rows(w, idx, None, int(idx.shape[1]), None, post_spike, n_post, pre_trace)
    return _functional(data, run, lo, hi, indices)


# =====================================================================================================
# container methods
# =====================================================================================================
def plasticity_index(M):
    """``(t_indptr, t_rows, perm)`` of the transposed stored structure of a CSR / CSC / fixed-number container: for every
    secondary id the stored rows that hold it, and the map of those slots to positions in ``data``.  Taken from the cached
    :class:`~brainevent_amd.Mirror` when it kept its raw arrays and permutation, otherwise built once (device sort / the
    column-block kernels) and cached in ``buffers`` — structure only, so it survives weight updates and travels with
    ``update_on_*(inplace=False)``.  Memory: 4 (row id) + 4 bytes per entry (``perm`` int32), 4 + 8 above 2**31 entries
    (``perm`` int64), plus the offsets."""
    idx = M.buffers.get(INDEX_KEY)
    if idx is not None:
        return idx
    mr = M.buffers.get('mirror')
    if mr is not None and not mr.released and mr.perm is not None and mr.indices is not None and mr.indptr is not None:
        return mr.indptr, mr.indices.to(torch.int32), mr.perm
    from ._convert import csr_to_csc_index, fixed_conn_num_csc_structure
    r = M._stored_rows()
    if r.indptr is None:
        ptr, rows, perm = fixed_conn_num_csc_structure(r.indices, shape=(r.m, r.k))
    else:
        ptr, rows, perm = csr_to_csc_index(r.indptr, r.indices, shape=(r.m, r.k), include_perm=True)
    nnz = int(rows.numel())
    perm = perm.to(torch.int64 if nnz > np.iinfo(np.int32).max else torch.int32)
    idx = M.buffers[INDEX_KEY] = (ptr, rows.to(torch.int32), perm)
    return idx


def _certified(M, lo, hi) -> bool:
    from ._csr import weights_stamp
    if isinstance(lo, torch.Tensor) or isinstance(hi, torch.Tensor) or (lo is None and hi is None):
        return False
    cert = M.buffers.get(CLIP_KEY)
    return cert is not None and cert[0] == weights_stamp(M.data) and cert[1] == lo and cert[2] == hi


def _certify(M, data, lo, hi) -> None:
    from ._csr import weights_stamp
    if isinstance(lo, torch.Tensor) or isinstance(hi, torch.Tensor) or (lo is None and hi is None):
        M.buffers.pop(CLIP_KEY, None)
    else:
        M.buffers[CLIP_KEY] = (weights_stamp(data), lo, hi)


# =====================================================================================================
# plastic mode: prepare(plastic=(w_min, w_max)) — the cached scatter workspace follows in-place updates by itself
# =====================================================================================================
EXP_MIN, EXP_MAX = -90, 150          # the range of a fixed-point exponent (2^(e - 32) has to be a normal f32)
SLOT_MAX_U16_ROW = 65536             # longest stored row whose block positions fit the uint16 slot table of a u16 plan


def plastic_exponent_bound(cmax: int, bound: float) -> int:
    """The fixed-point exponent no weight in ``[-bound, bound]`` can overflow: ``62 - ceil(log2(cmax * bound))`` with ``cmax`` the
    most stored entries on one output column (duplicates counted) — every column sum then stays below ``2^62`` whatever the
    weights become.  Written like ``BinnedScatter._exponent_by_steps``: ``62 - frexp(cmax * bound * 1.001)[1]`` (the factor
    covers the roundings of the addends; a product that is an exact power of two ``2^p`` gives ``61 - p``, one below the formula:
    its sum could reach ``2^62`` itself), clamped to the range of an exponent.  ``bound == 0`` or an empty structure: nothing
    can overflow, the largest exponent.  Pure host arithmetic."""
    cmax, bound = int(cmax), abs(float(bound))
    if not math.isfinite(bound):
        raise ValueError(f"the weight bound must be finite; got {bound}.")
    if cmax <= 0 or bound == 0.0:
        return EXP_MAX
    return max(EXP_MIN, min(EXP_MAX, 62 - math.frexp(cmax * bound * 1.001)[1]))


def plastic_bounds(bounds):
    """``(w_min, w_max)`` of ``prepare(plastic=...)`` as two finite host floats with ``w_min <= w_max`` (``ValueError`` otherwise:
    a missing bound, a bound on a device — the clip certificate refuses those too —, inf / nan, a reversed pair)."""
    if not isinstance(bounds, (tuple, list)) or len(bounds) != 2:
        raise ValueError(f"plastic must be a pair (w_min, w_max); got {bounds!r}.")
    for b in bounds:
        if isinstance(b, torch.Tensor) and b.device.type != 'cpu':
            raise ValueError("plastic=(w_min, w_max) takes host numbers: bounds held in device tensors cannot be certified.")
    lo, hi = _bounds(*bounds)
    if lo is None or hi is None:
        raise ValueError("plastic=(w_min, w_max) needs both bounds: an open side lets the weights outgrow any exponent.")
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise ValueError(f"plastic=(w_min, w_max) needs finite bounds with w_min <= w_max; got ({lo}, {hi}).")
    return lo, hi


def _column_count_max(M, rows) -> int:
    """The most stored entries on one secondary id (duplicates counted): from the cached transposed structure when there is
    one, else one counted pass over the indices.  Synchronises (arming only)."""
    if rows.k <= 0 or rows.indices.numel() == 0:
        return 0
    idx = M.buffers.get(INDEX_KEY)
    mr = M.buffers.get('mirror')
    ptr = idx[0] if idx is not None else (mr.indptr if mr is not None and not mr.released and mr.indptr is not None else None)
    if ptr is not None:
        return int((ptr[1:] - ptr[:-1]).max())
    flat = rows.indices.reshape(-1)
    counts = torch.zeros(rows.k, dtype=torch.int64, device=flat.device)
    for a in range(0, int(flat.numel()), 1 << 27):
        counts += torch.bincount(flat[a:a + (1 << 27)], minlength=rows.k)
    return int(counts.max())


def arm_plastic(M, bounds) -> None:
    """``M.prepare(plastic=bounds)``: see :meth:`StoredRowsData.prepare`."""
    from . import _csr as C
    from ._error import MathError
    lo, hi = plastic_bounds(bounds)
    rows = M._stored_rows()
    nse = int(rows.indices.numel())
    w = M.data
    if w.numel() == 1 and nse > 1:
        raise ValueError(_HOMO_MSG)
    if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"prepare(plastic=...) serves per-entry f32 / f16 / bf16 weights; got {w.dtype} (f64 entries are stored "
                         "as two f32 entries each, which the touched-entries upkeep does not follow).")
    lo_r, hi_r = _rounded(lo, w.dtype), _rounded(hi, w.dtype)          # what the update kernel clips to
    if nse:
        mn, mx = torch.aminmax(w)                                      # one pass; NaN fails both comparisons
        if not (float(mn) >= lo_r and float(mx) <= hi_r):
            raise ValueError(f"prepare(plastic=({lo}, {hi})): the weights span [{float(mn)}, {float(mx)}]; clamp them into the "
                             "bounds first (arming never modifies weights).")
    bound = max(abs(lo_r), abs(hi_r))
    cmax = _column_count_max(M, rows)
    e_bound = plastic_exponent_bound(cmax, bound)

    ws = M.buffers.get('scatter_plan', False)
    if ws is False or (ws is not None and ws.is_stale(w)):
        saved, C.PLAN_KEEP_ORDER = C.PLAN_KEEP_ORDER, True             # (a plan built here keeps its rows' column order)
        try:
            ws = M._scatter_workspace()
        finally:
            C.PLAN_KEEP_ORDER = saved
    if ws is not None and bound < math.ldexp(1.0, C.ScatterPlan.MIN_WEIGHT_BITS - e_bound):
        raise MathError(f"prepare(plastic=({lo}, {hi})): at the exponent {e_bound} that {cmax} entries per column of that size "
                        f"cannot overflow, the bound itself keeps fewer than {C.ScatterPlan.MIN_WEIGHT_BITS} bits.")
    max_row = None
    if isinstance(ws, C.ScatterPlan):
        assert not ws.homo and not ws.split_f64 and ws.layout in (ws.LAYOUT_U16, ws.LAYOUT_D8)
        route = 'plan-d8' if ws.layout == ws.LAYOUT_D8 else 'plan-u16'
        if ws.layout == ws.LAYOUT_U16:
            max_row = rows.row_len if rows.indptr is None else int((rows.indptr[1:] - rows.indptr[:-1]).max())
    elif isinstance(ws, C.BinnedScatter):
        route = 'binned'
        if ws.acc32:            # the 32-bit sums' gate depends on the smallest weight, which learning moves: 64-bit bins
            ws.scale_exp += 32
            ws.acc32 = False
            ws._set_geometry()
            ws._ws = {}
            ws.ws = ws.workspace(1)
    else:
        route = 'direct'
    if ws is not None:
        ws.scale_exp = min(ws.scale_exp, e_bound)       # a launch argument of every step: from here on independent of the weights
    _certify(M, w, lo, hi)
    M.buffers[PLASTIC_KEY] = {'route': route, 'w_min': lo, 'w_max': hi, 'cmax': cmax, 'e_bound': e_bound, 'ws': ws,
                              'max_row': max_row}


def plastic_state(M):
    st = M.buffers.get(PLASTIC_KEY)
    if st is None:
        return None
    ws = st['ws']
    return {'route': st['route'], 'w_min': st['w_min'], 'w_max': st['w_max'], 'exponent': None if ws is None else ws.scale_exp,
            'cmax': st['cmax']}


def _disarm(M) -> None:
    """Leave plastic mode: the state goes, and with it the plan's slot table (2 bytes per entry that only the entry patch reads)."""
    st = M.buffers.pop(PLASTIC_KEY, None)
    if st is not None and st['route'].startswith('plan'):
        st['ws'].slot = None


def _plastic_ready(M, lo, hi):
    """The armed state when this in-place update may keep the workspace current itself — same bounds, valid certificate, the
    armed workspace still cached and fresh — else ``None``, and the container is disarmed (the next product refreshes in full)."""
    from ._csr import weights_stamp
    st = M.buffers.get(PLASTIC_KEY)
    if st is None:
        return None
    ws = M.buffers.get('scatter_plan', False)
    if (ws is st['ws'] and isinstance(lo, float) and isinstance(hi, float) and st['w_min'] == lo and st['w_max'] == hi
            and _certified(M, lo, hi) and (ws is None or ws.stamp == weights_stamp(M.data))):
        return st
    _disarm(M)
    return None


def _geom(plan):
    return plan.m, plan.k, plan.slice_shift, plan.slice_width, plan.layout, A.ptr(plan.seg), A.ptr(plan.blob)


def _rows_head(w, rows):
    return (A.ptr(w), A.wcode(w), A.ptr(rows.indices), A.ptr(rows.indptr),
            int(rows.indptr is not None and rows.indptr.dtype == torch.int64), int(rows.row_len))


def _refresh_workspace(n: int) -> torch.Tensor:
    return A.workspace(fn('be_scatter_plan_refresh_workspace_bytes')(int(n)))


def _plan_slots(plan, st, w, rows) -> bool:
    """The plan's slot table (built on first use of the permuted side, kept like ``order``); ``False`` — with the reason as a
    warning — when block positions do not fit its uint16 entries."""
    if plan.slot is not None:
        return True
    if plan.layout == plan.LAYOUT_U16 and st['max_row'] > SLOT_MAX_U16_ROW:
        import warnings
        warnings.warn(f"brainevent_amd: the permuted side of this plastic container is not kept current: a stored row of "
                      f"{st['max_row']} entries exceeds the {SLOT_MAX_U16_ROW} block positions of the u16 plan's slot table; "
                      "the container is disarmed and refreshes in full.", stacklevel=4)
        return False
    plan.slot = torch.empty(int(rows.indices.numel()), dtype=torch.int16, device=plan.blob.device)
    f = fn('be_scatter_plan_slots')
    check(f(*_rows_head(w, rows), *_geom(plan), A.ptr(getattr(plan, 'order', None)), A.ptr(plan.slot), A.stream_ptr()),
          'be_scatter_plan_slots')
    return True


def _plan_refresh_rows(plan, w, rows, sp, sd) -> None:
    """``be_scatter_plan_refresh_rows``: the blocks of the active stored rows rewritten from ``w``."""
    ws = _refresh_workspace(plan.m)
    f = fn('be_scatter_plan_refresh_rows')
    # (d8 positions follow from the structure alone: only a u16 refresh, which draws them anew, has slots to rewrite)
    slot = plan.slot if plan.layout == plan.LAYOUT_U16 else None
    check(f(*_rows_head(w, rows), *_geom(plan), A.ptr(getattr(plan, 'order', None)), A.ptr(slot), A.ptr(sp), sd,
            A.ptr(ws), ws.numel(), A.stream_ptr()), 'be_scatter_plan_refresh_rows')


def _plan_patch_entries(plan, w, index, sp, sd) -> None:
    """``be_scatter_plan_patch_entries``: the entries on the active secondary ids stored into their blocks."""
    t_ptr, t_rows, perm = index
    ws = _refresh_workspace(plan.k)
    f = fn('be_scatter_plan_patch_entries')
    check(f(A.ptr(w), A.wcode(w), A.ptr(t_ptr), int(t_ptr.dtype == torch.int64), A.ptr(t_rows), A.ptr(perm),
            int(perm.dtype == torch.int64), int(t_rows.numel()), A.ptr(plan.slot), *_geom(plan), A.ptr(sp), sd, A.ptr(ws),
            ws.numel(), A.stream_ptr()), 'be_scatter_plan_patch_entries')


def container_update(M, pre: bool, spikes, trace, w_min, w_max, inplace: bool, aged=None):
    """Shared body of the ``update_on_pre`` / ``update_on_post`` methods.  ``aged=(hist, ages)`` (``DelayedCSR.update_on_post`` on
    its stacked matrix, in place of ``trace``): the trace of stacked row ``d * n + i`` is ``hist``'s value of neuron ``i`` at age
    ``d`` — the same walk, certificate and plan upkeep, with ``be_plasticity_rows_aged`` as the update kernel."""
    from ._dense import Dense
    n_pre, n_post = int(M.shape[0]), int(M.shape[1])
    n_spk, n_tr = (n_pre, n_post) if pre else (n_post, n_pre)
    if isinstance(M, Dense):
        n_syn = n_pre * n_post
    else:
        n_syn = int(M.indices.numel())
    if M.data.numel() == 1 and n_syn > 1:
        raise ValueError(_HOMO_MSG)
    _check_vec(spikes, n_spk, 'pre_spike' if pre else 'post_spike')
    if aged is None:
        _check_vec(trace, n_tr, 'post_trace' if pre else 'pre_trace')
    else:
        assert not pre and trace is None and not isinstance(M, Dense) and not M._scatter_side(pre)
    lo, hi = _bounds(w_min, w_max)

    # which kernel: row-driven over the stored rows (the spikes are on the scatter side: pre spikes are the left operand of
    # ``spk @ M``), or permuted over the transposed structure
    rows = None if isinstance(M, Dense) else M._stored_rows()

    def run(w, clip):
        if rows is None:
            _run_dense(w, pre, spikes, trace, clip)
        elif M._scatter_side(pre):
            _run_rows(w.reshape(-1), rows.indices.reshape(-1), rows.indptr, rows.row_len, None, spikes, n_spk, trace, clip)
        else:
            t_ptr, t_rows, perm = plasticity_index(M)
            if aged is not None:
                _run_rows_aged(w.reshape(-1), t_rows, t_ptr, perm, spikes, n_spk, aged[0], aged[1], clip)
            else:
                _run_rows(w.reshape(-1), t_rows, t_ptr, -1, perm, spikes, n_spk, trace, clip)

    if inplace:
        # plastic mode (prepare(plastic=...)): the cached scatter workspace is kept current by launches of its own after the
        # update kernel — the active rows' blocks refilled, or the touched entries patched in — and never refreshed in full
        st = None if rows is None else _plastic_ready(M, lo, hi)
        plan = None
        if st is not None and st['route'].startswith('plan'):
            plan = st['ws']
            spikes = _spikes(spikes)                      # (one conversion for the update and the plan's upkeep)
            if not M._scatter_side(pre) and not _plan_slots(plan, st, M.data.reshape(-1), rows):
                _disarm(M)
                st = plan = None
        if _certified(M, lo, hi):
            run(M.data, (lo, hi))                         # untouched entries are already in range: clip the touched ones
        else:
            run(M.data, (None, None))
            _clamp_(M.data, lo, hi)
        if plan is not None:
            if M._scatter_side(pre):
                _plan_refresh_rows(plan, M.data.reshape(-1), rows, *spikes)
            else:
                _plan_patch_entries(plan, M.data.reshape(-1), plasticity_index(M), *spikes)
        # the kernel wrote through a raw pointer: move torch's version counter so that cached plans / mirrors see the change
        torch.autograd.graph.increment_version(M.data)
        _certify(M, M.data, lo, hi)
        if st is not None and st['ws'] is not None:
            from ._csr import weights_stamp
            st['ws'].stamp = weights_stamp(M.data)        # (binned: the bins are refilled from the raw arrays every step)
        return M
    w = M.data.clone()
    run(w, (None, None))
    _clamp_(w, lo, hi)
    keep = {INDEX_KEY: M.buffers[INDEX_KEY]} if M.buffers.get(INDEX_KEY) is not None else {}
    if isinstance(M, Dense):
        out = Dense(w, shape=M.shape, backend=M.backend, buffers=keep)
    else:
        out = M.with_data(w)
        out.buffers.update(keep)
    out._numpy_result = M._numpy_result
    _certify(out, w, lo, hi)
    return out


class PlasticityMixin:
    """``update_on_pre`` / ``update_on_post`` of the weight containers (reference ``_csr/main.py:1389-1455``)."""

    def update_on_pre(self, pre_spike, post_trace, w_min=None, w_max=None, *, inplace: bool = False):
        """Pre-spike STDP update: every stored synapse ``(i, j)`` of an active pre neuron ``i`` gets ``+= post_trace[j]``, then
        ``clip(W, w_min, w_max)`` over the whole array.  ``inplace=False`` (the reference's behaviour) returns a new container
        sharing the structure; ``inplace=True`` updates ``self.data`` and returns ``self`` (cached plans and mirrors refresh
        on the next product; see the module docstring for the clip certificate and captured graphs)."""
        return container_update(self, True, pre_spike, post_trace, w_min, w_max, inplace)

    def update_on_post(self, pre_trace, post_spike, w_min=None, w_max=None, *, inplace: bool = False):
        """Post-spike STDP update: every stored synapse ``(i, j)`` of an active post neuron ``j`` gets ``+= pre_trace[i]``, then
        the whole-array clip.  ``inplace`` as in :meth:`update_on_pre`."""
        return container_update(self, False, post_spike, pre_trace, w_min, w_max, inplace)
