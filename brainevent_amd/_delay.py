"""Synaptic delays on the presynaptic side: :class:`SpikeRing` and :class:`DelayedCSR`.

The last ``depth`` spike vectors are kept bit-packed (:class:`SpikeRing`); every stored row of the matrix is split by delay once
(:class:`DelayedCSR`): stored row ``d * n_pre + i`` of the *stacked* matrix holds the synapses of neuron ``i`` whose delay is ``d``.
``ring @ D`` is then one ordinary event-driven scatter over the stacked rows ``{d * n_pre + i : neuron i fired d steps ago}``: the
ring is compacted into that id list (``csrc/be_delay.hip``) and the list goes through the scatter routes that exist (planned,
binned, direct) as an :class:`~brainevent_amd._array.ActiveIds` operand.  The reference has no delays.

Delayed synapses learn: ``D.update_on_pre(ring, post_trace)`` is the row-driven update of the stacked matrix over
the same id list; ``D.update_on_post(hist, post_spike)`` reads the pre-side value each synapse saw arrive from a
:class:`ValueRing` — the history of a per-neuron quantity beside the history of spikes — by age, inside the update kernel; and
``ring @ D`` is differentiable in the weights (``D.stacked.data`` is the leaf, :meth:`DelayedCSR.stacked_to_original` moves its
gradient to the order the synapses were given in).  The delays are axonal: they sit between the pre neuron and the synapse.

Everything that can be refused is refused before the first device call (shapes, dtypes, the ``depth`` range), so the validation
runs without a GPU.

Batched rings: ``SpikeRing(n, depth, batch=B)`` holds ``B`` histories under one ``head``; ``ring @ D`` then
unrolls them by age into the bit-packed batch ``[B, depth * n_pre]`` (``be_spike_ring_unroll``) that the stacked matrix
multiplies through its own scatter route, and comes back ``[B, n_post]``."""
from typing import Optional

import numpy as np
import torch

from . import _array as A
from ._event import BinaryArray, BitPackedBinary, CompactBinary
from ._lib import call, fn

__all__ = ['SpikeRing', 'ValueRing', 'DelayedCSR', 'MAX_DELAY_DEPTH', 'check_ring_matches']

#: largest ``depth`` of a :class:`DelayedCSR` (the split kernels keep one LDS counter per delay and wave: kMaxDepth)
MAX_DELAY_DEPTH = 256
#: largest number of ages one compaction covers (its grid's second dimension)
MAX_RING_AGES = 65535
#: largest ``batch`` of a :class:`SpikeRing` (the batch row is the second grid dimension of the push and of the unroll; it is
#: also the largest batch of every batched product of the library)
MAX_RING_BATCH = 65535
_ID_LIMIT = 1 << 31


def _check_ring_size(n: int, depth: int) -> None:
    if n < 1:
        raise ValueError(f"SpikeRing: n must be >= 1; got {n}.")
    if depth < 1:
        raise ValueError(f"SpikeRing: depth must be >= 1; got {depth}.")
    if depth * n >= _ID_LIMIT:
        raise ValueError(f"SpikeRing: depth * n = {depth * n} must stay below 2^31 (the ids of the stacked rows are int32).")


def check_ring_matches(ring_n: int, ring_depth: int, shape, depth: int) -> None:
    """``ring @ D`` needs a ring over ``D``'s pre population that remembers at least ``D.depth`` steps (``ValueError``)."""
    if int(ring_n) != int(shape[0]):
        raise ValueError(f"ring @ DelayedCSR: the ring holds {int(ring_n)} neurons, the matrix has {int(shape[0])} rows.")
    if int(ring_depth) < int(depth):
        raise ValueError(f"ring @ DelayedCSR: the ring remembers {int(ring_depth)} steps, the matrix needs depth {int(depth)}.")


class SpikeRing:
    """The last ``depth`` spike vectors of ``n`` neurons, bit-packed on the device.

    ``bits`` is int32 ``[depth, ceil(n / 32)]`` (the ``BitPackedBinary`` layout per slot), ``head`` a device int32 ``[1]``.
    :meth:`push` writes the spikes of the current step into slot ``head`` and advances ``head`` on the device, so a captured step
    (``capture_step(fn, repeat=r)``) stays correct when replayed; the spikes of *age* ``a`` (0: just pushed) lie in slot
    ``(head - 1 - a) mod depth``.  History before the first push is silent.

    ``batch=None`` (the default): one vector per step.  ``batch=B`` (``1 <= B <= 65535``): ``B`` histories under the one
    ``head`` — ``bits`` is ``[depth, B, ceil(n / 32)]``, :meth:`push` takes ``[B, n]`` (batch-major, the layout ``ring @ D``
    answers in: ``[B, n_post]``), ``shape`` is ``(B, n)``; :meth:`stacked_bits` lays the histories out by age as the bit-packed
    batch the stacked matrix of a :class:`DelayedCSR` multiplies."""

    #: ``None``: one vector per step; ``B``: a batched ring
    batch: Optional[int] = None

    def __init__(self, n: int, depth: int, device=None, *, batch: Optional[int] = None):
        n, depth = int(n), int(depth)
        _check_ring_size(n, depth)
        if batch is not None:
            batch = int(batch)
            if not 1 <= batch <= MAX_RING_BATCH:
                raise ValueError(f"SpikeRing: batch must lie in [1, {MAX_RING_BATCH}]; got {batch}.")
        self.n, self.depth, self.batch = n, depth, batch
        dev = torch.device(device) if device is not None else A.device()
        self._words = (n + 31) // 32
        self.bits = torch.zeros((depth, self._words) if batch is None else (depth, batch, self._words), dtype=torch.int32,
                                device=dev)
        self._state = torch.zeros(2, dtype=torch.int32, device=dev)       # head, and the push kernel's arrival ticket
        self.head = self._state[:1]
        self._ids = None        # the id buffer (depth * n), its counter and the operands over it: built by the first ids()
        self._count = None
        self._operands = {}
        self._stacked = {}      # ages -> the unrolled words [B, ceil(ages * n / 32)]: built by the first stacked_bits(ages)
        self._numpy = True      # numpy in -> numpy out: False once a device tensor was pushed

    # -- writing --------------------------------------------------------------------------------------------------------
    def push(self, spikes) -> 'SpikeRing':
        """Store the spikes of the current step.  A tensor or numpy array of ``n`` elements (bool / integer: active when ``!= 0``;
        float: active when ``> 0``), a ``BinaryArray``, or a ``BitPackedBinary`` / ``CompactBinary`` (their packed words are
        copied, the bits past ``n`` cleared).  A batched ring takes ``[B, n]`` — a tensor or numpy array, or a ``BinaryArray``
        of one; packed words go through :meth:`push_packed`.  One launch, no host read."""
        if isinstance(spikes, SpikeRing):
            raise TypeError("SpikeRing.push takes one spike vector.")
        if self.batch is not None:
            return self._push_batch(spikes)
        if isinstance(spikes, (BitPackedBinary, CompactBinary)):
            p = spikes._packed_operand()
            v = p if p is not None else spikes.value
        elif isinstance(spikes, BinaryArray):
            v = spikes.value
        else:
            v = spikes
        if isinstance(v, A.ActiveIds):
            raise TypeError("SpikeRing.push takes spikes by position, not an id list.")
        shape = tuple(v.shape) if hasattr(v, 'shape') else np.shape(v)
        if len(shape) != 1:
            raise NotImplementedError(f"SpikeRing.push takes one 1-D spike vector; got shape {shape} (a ring of B histories is "
                                      "SpikeRing(n, depth, batch=B)).")
        if shape[0] != self.n:
            raise ValueError(f"SpikeRing.push: {shape[0]} spikes for a ring of {self.n} neurons.")
        if not A.wants_numpy(v):
            self._numpy = False
        buf, sd = A.spikes_to_device(v)
        call('be_spike_ring_push', A.ptr(buf), sd, self.n, self.depth, A.ptr(self.bits), A.ptr(self.head),
             A.ptr(self._state[1:]), A.stream_ptr())
        return self

    def _push_batch(self, spikes) -> 'SpikeRing':
        if isinstance(spikes, (BitPackedBinary, CompactBinary)):
            raise TypeError("SpikeRing.push of a batched ring takes [batch, n] spikes (or a BinaryArray of them); hand packed "
                            "words [batch, ceil(n / 32)] to push_packed.")
        v = spikes.value if isinstance(spikes, BinaryArray) else spikes
        if isinstance(v, (A.ActiveIds, A.PackedSpikes)):
            raise TypeError("SpikeRing.push of a batched ring takes spikes by position, [batch, n].")
        shape = _shape_of(v)
        if len(shape) != 2 or shape != (self.batch, self.n):
            raise ValueError(f"SpikeRing.push: a ring of batch {self.batch} over {self.n} neurons takes spikes of shape "
                             f"({self.batch}, {self.n}); got {shape}.")
        if not A.wants_numpy(v):
            self._numpy = False
        buf, sd = A.spikes_to_device(v)
        return self._push_call(buf, sd)

    def _push_call(self, buf, sd) -> 'SpikeRing':
        call('be_spike_ring_push_batch', A.ptr(buf), sd, self.n, self.depth, self.batch, A.ptr(self.bits), A.ptr(self.head),
             A.ptr(self._state[1:]), A.stream_ptr())
        return self

    def push_packed(self, words) -> 'SpikeRing':
        """Store the spikes of the current step of a batched ring from already packed words: int32 ``[B, ceil(n / 32)]`` (bit
        ``i % 32`` of word ``i // 32`` of row ``b`` = neuron ``i`` of sample ``b``).  The bits past ``n`` of every row are cleared.
        A method of its own because a ``[B, W]`` integer array given to :meth:`push` is ``B`` vectors of ``W`` spikes.  One
        launch, no host read.  (A ring without a batch takes its packed words as a ``BitPackedBinary``, through :meth:`push`.)"""
        if self.batch is None:
            raise NotImplementedError("SpikeRing.push_packed is the packed input of a batched ring; a ring without a batch takes "
                                      "push(BitPackedBinary.from_packed(words, n)).")
        want = (self.batch, self._words)
        shape = _shape_of(words)
        if shape != want:
            raise ValueError(f"SpikeRing.push_packed: the packed words of this ring have shape {want}; got {shape}.")
        if isinstance(words, torch.Tensor):
            dt, ok = words.dtype, words.dtype in (torch.int32, torch.uint32)
        else:
            dt = np.asarray(words).dtype
            ok = dt in (np.dtype(np.int32), np.dtype(np.uint32))
        if not ok:
            raise TypeError(f"SpikeRing.push_packed takes 32-bit words (int32); got {dt}.")
        if not A.wants_numpy(words):
            self._numpy = False
        if not isinstance(words, torch.Tensor):
            words = np.asarray(words).view(np.int32)
        return self._push_call(A.to_device(words), A.BE_SPIKE_BITS)

    def reset(self) -> 'SpikeRing':
        """Forget the history (``bits`` and ``head`` back to zero)."""
        self.bits.zero_()
        self._state.zero_()
        return self

    # -- reading --------------------------------------------------------------------------------------------------------
    def events(self, age: int = 0):
        """The spikes of ``age`` steps ago as a ``BitPackedBinary`` (a copy of that slot): ``ring.events(3) @ csr`` is one delay
        for a whole projection, with any container.  The slot is picked by a device-side index, so the call captures.  A
        batched ring gives a ``BinaryArray`` over a bool ``[B, n]`` tensor (unpacked with torch bit arithmetic: not a hot path);
        ``ring.events(3) @ csr`` is then ``[B, n_post]``."""
        age = int(age)
        if not 0 <= age < self.depth:
            raise ValueError(f"SpikeRing.events: age must lie in [0, {self.depth}); got {age}.")
        slot = torch.remainder(self.head - (1 + age), self.depth)
        if self.batch is not None:
            words = self.bits.index_select(0, slot).reshape(self.batch, self._words, 1)
            lanes = torch.arange(32, dtype=torch.int32, device=words.device)
            on = torch.bitwise_and(torch.bitwise_right_shift(words, lanes), 1).ne(0)
            return BinaryArray(on.reshape(self.batch, self._words * 32)[:, :self.n].contiguous())
        words = self.bits.index_select(0, slot).reshape(-1)
        return BitPackedBinary.from_packed(words, self.n)

    def ids(self, ages: Optional[int] = None, row_mask: Optional[torch.Tensor] = None) -> A.ActiveIds:
        """The ring compacted into the list ``{a * n + i : neuron i fired a steps ago, a < ages}`` (default: every age), gated by
        ``row_mask`` (int32 ``[>= ages, ceil(n / 32)]``, word for word) — an ``ActiveIds`` over ``ages * n`` positions, in no
        particular order.  The id buffer is allocated once, by the first call; the counter is zeroed on the stream by every call.
        An id list is one vector: a batched ring raises ``NotImplementedError`` (its form by age is :meth:`stacked_bits`)."""
        if self.batch is not None:
            raise NotImplementedError("SpikeRing.ids: an id list is one vector; a batched ring is laid out by age with "
                                      "stacked_bits().")
        ages = self.depth if ages is None else int(ages)
        if not 1 <= ages <= min(self.depth, MAX_RING_AGES):
            raise ValueError(f"SpikeRing.ids: ages must lie in [1, {min(self.depth, MAX_RING_AGES)}]; got {ages}.")
        if row_mask is not None:
            if row_mask.dtype != torch.int32 or row_mask.ndim != 2 or row_mask.shape[0] < ages or row_mask.shape[1] != self._words \
                    or not row_mask.is_contiguous():
                raise ValueError(f"SpikeRing.ids: row_mask must be a contiguous int32 [>= {ages}, {self._words}] tensor.")
        if self._ids is None:
            self._ids = torch.zeros(self.depth * self.n, dtype=torch.int32, device=self.bits.device)
            self._count = torch.zeros(1, dtype=torch.int32, device=self.bits.device)
        call('be_spike_ring_compact', A.ptr(self.bits), A.ptr(self.head), self.n, self.depth, ages, A.ptr(row_mask),
             A.ptr(self._ids), A.ptr(self._count), A.stream_ptr())
        op = self._operands.get(ages)
        if op is None:
            op = self._operands[ages] = A.ActiveIds(self._ids, self._count, ages * self.n)
        op.numpy_result = self._numpy
        return op

    def stacked_bits(self, ages: Optional[int] = None, row_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The histories of a batched ring by age, bit-packed: int32 ``[B, ceil(ages * n / 32)]`` whose bit
        ``a * n + i`` of row ``b`` is the spike of neuron ``i`` of sample ``b`` at age ``a < ages`` (default: every age), gated by
        ``row_mask`` (int32 ``[>= ages, ceil(n / 32)]``); the bits past ``ages * n`` are 0.  It is the ``BE_SPIKE_BITS`` batch
        operand over the ``ages * n`` rows of a stacked matrix.  Every word is written by each call (nothing is zeroed first);
        the buffer is allocated by the first call for that ``ages`` and reused: the next call overwrites what this one returned.
        A ring without a batch has :meth:`ids` instead."""
        if self.batch is None:
            raise NotImplementedError("SpikeRing.stacked_bits lays out a batched ring; a ring without a batch is compacted with ids().")
        ages = self.depth if ages is None else int(ages)
        if not 1 <= ages <= self.depth:
            raise ValueError(f"SpikeRing.stacked_bits: ages must lie in [1, {self.depth}]; got {ages}.")
        if row_mask is not None:
            if not isinstance(row_mask, torch.Tensor) or row_mask.dtype != torch.int32 or row_mask.ndim != 2 \
                    or row_mask.shape[0] < ages or row_mask.shape[1] != self._words or not row_mask.is_contiguous():
                raise ValueError(f"SpikeRing.stacked_bits: row_mask must be a contiguous int32 [>= {ages}, {self._words}] tensor.")
        out = self._stacked.get(ages)
        if out is None:
            out = self._stacked[ages] = torch.empty((self.batch, (ages * self.n + 31) // 32), dtype=torch.int32,
                                                    device=self.bits.device)
        call('be_spike_ring_unroll', A.ptr(self.bits), A.ptr(self.head), self.n, self.depth, self.batch, ages, A.ptr(row_mask),
             A.ptr(out), A.stream_ptr())
        return out

    # -- product --------------------------------------------------------------------------------------------------------
    shape = property(lambda self: (self.n,) if self.batch is None else (self.batch, self.n))
    ndim = property(lambda self: 1 if self.batch is None else 2)

    def __matmul__(self, other):
        if isinstance(other, DelayedCSR):
            return other.__rmatmul__(self)
        raise NotImplementedError("SpikeRing @ x is defined for a DelayedCSR; for one delay of a whole projection use "
                                  "ring.events(age) @ matrix.")

    def __rmatmul__(self, other):
        raise NotImplementedError("x @ SpikeRing is not defined: the delays live on the presynaptic side (ring @ D).")

    def __repr__(self):
        if self.batch is not None:
            return f"SpikeRing(n={self.n}, depth={self.depth}, batch={self.batch})"
        return f"SpikeRing(n={self.n}, depth={self.depth})"


_VALUE_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


def _float_dtype_of(x):
    """The torch float dtype of a tensor or numpy array, ``None`` for anything else (no device call)."""
    if isinstance(x, torch.Tensor):
        return x.dtype if x.dtype in _VALUE_DTYPES else None
    dt = np.asarray(x).dtype
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.float16): torch.float16}.get(dt)


class ValueRing:
    """The last ``depth`` value vectors of ``n`` neurons on the device — the history of a per-neuron quantity (a presynaptic
    trace) beside the history of spikes, for the updates of delayed synapses.

    ``values`` is ``[depth, n]`` in ``dtype`` (f32, f64, f16 or bf16), ``head`` a device int32 ``[1]`` with :class:`SpikeRing`'s
    convention: :meth:`push` writes slot ``head`` and advances ``head`` on the device (one launch, no host read, so a captured step
    replays correctly), and the vector of *age* ``a`` (0: just pushed) lies in slot ``(head - 1 - a) mod depth``.  History before the
    first push is zero.  One vector per step (no batch).  Results are device tensors."""

    def __init__(self, n: int, depth: int, dtype=torch.float32, device=None):
        n, depth = int(n), int(depth)
        if n < 1:
            raise ValueError(f"ValueRing: n must be >= 1; got {n}.")
        if depth < 1:
            raise ValueError(f"ValueRing: depth must be >= 1; got {depth}.")
        if depth * n >= _ID_LIMIT:
            raise ValueError(f"ValueRing: depth * n = {depth * n} must stay below 2^31 (the ids of the stacked rows are int32).")
        if dtype not in _VALUE_DTYPES:
            raise TypeError(f"ValueRing: dtype must be torch.float32, float64, float16 or bfloat16; got {dtype}.")
        self.n, self.depth, self.dtype = n, depth, dtype
        dev = torch.device(device) if device is not None else A.device()
        self.values = torch.zeros((depth, n), dtype=dtype, device=dev)
        self._state = torch.zeros(2, dtype=torch.int32, device=dev)       # head, and the push kernel's arrival ticket
        self.head = self._state[:1]
        self._ages = None       # 0 .. depth - 1 on the device: built by the first by_age()

    def push(self, x) -> 'ValueRing':
        """Store the values of the current step: a 1-D tensor or numpy array of ``n`` elements in any float dtype, converted to
        the ring's dtype as a cast does.  One launch, no host read."""
        shape = _shape_of(x)
        if len(shape) != 1:
            raise NotImplementedError(f"ValueRing.push takes one 1-D value vector; got shape {shape} (batched rings are not built).")
        if shape[0] != self.n:
            raise ValueError(f"ValueRing.push: {shape[0]} values for a ring of {self.n} neurons.")
        if _float_dtype_of(x) is None:
            raise TypeError(f"ValueRing.push takes a float tensor or numpy array; got {getattr(x, 'dtype', type(x).__name__)}.")
        buf = A.to_device(x)
        call('be_value_ring_push', A.ptr(buf), A.wcode(buf), self.n, self.depth, A.ptr(self.values), A.wcode(self.values),
             A.ptr(self.head), A.ptr(self._state[1:]), A.stream_ptr())
        return self

    def reset(self) -> 'ValueRing':
        """Forget the history (``values`` and ``head`` back to zero)."""
        self.values.zero_()
        self._state.zero_()
        return self

    def value(self, age: int = 0) -> torch.Tensor:
        """The vector of ``age`` steps ago (a copy of that slot).  The slot is picked by a device-side index, so the call
        captures."""
        age = int(age)
        if not 0 <= age < self.depth:
            raise ValueError(f"ValueRing.value: age must lie in [0, {self.depth}); got {age}.")
        slot = torch.remainder(self.head - (1 + age), self.depth)
        return self.values.index_select(0, slot).reshape(-1)

    def by_age(self) -> torch.Tensor:
        """``[depth, n]`` with row ``a`` = the vector of age ``a``: a gather with a device-side index (capturable), a copy of
        the whole history."""
        if self._ages is None:
            self._ages = torch.arange(1, self.depth + 1, dtype=torch.int32, device=self.values.device)
        return self.values.index_select(0, torch.remainder(self.head - self._ages, self.depth))

    shape = property(lambda self: (self.depth, self.n))

    def __repr__(self):
        return f"ValueRing(n={self.n}, depth={self.depth}, dtype={self.dtype})"


def _as_int32_delays(delays, nnz: int):
    """``delays`` checked without touching a device: an integer array (numpy or torch) with one element per stored entry."""
    if not isinstance(delays, torch.Tensor):
        delays = np.asarray(delays)
        is_int = np.issubdtype(delays.dtype, np.integer)
    else:
        is_int = delays.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    if not is_int:
        raise TypeError(f"DelayedCSR: delays must be an integer array (steps); got dtype {delays.dtype}.")
    if int(np.prod(tuple(delays.shape))) != nnz:
        raise ValueError(f"DelayedCSR: {int(np.prod(tuple(delays.shape)))} delays for {nnz} stored entries.")
    return delays


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, 'shape') else np.shape(x)


class DelayedCSR:
    """A CSR matrix whose stored entries carry a conduction delay each, in steps: ``(ring @ D)[j]`` is the sum, over the entries
    ``e`` of column ``j``, of ``w_e`` times the spike of ``row(e)`` at age ``delays[e]``.  Several entries may share ``(row, col)``
    (parallel synapses with different delays are the normal case); all of them count.

    ``DelayedCSR((data, indices, indptr, delays), shape=(n_pre, n_post), depth=depth)``: ``0 <= delays[e] < depth <= 256``, one
    integer per stored entry in the order of ``data`` (``ValueError`` naming an offending position otherwise).  ``indptr=None``:
    rows of fixed length, ``indices`` is ``[n_pre, row_len]``.  ``data`` with one element is one shared weight and stays shared.

    ``stacked`` is a plain :class:`~brainevent_amd.CSR` of shape ``(depth * n_pre, n_post)`` whose row ``d * n_pre + i`` holds the
    entries of row ``i`` with delay ``d`` in their original order; ``perm`` maps a stacked position to the original one;
    ``row_mask`` (int32 ``[depth, ceil(n_pre / 32)]``) marks the non-empty stacked rows.  ``update_on_pre`` / ``update_on_post`` are
    the spike-triggered updates; ``ring @ D`` is differentiable in the weights, with ``stacked.data`` as the leaf
    (no spike gradient: the ring holds bits).  A batched ring (``SpikeRing(n_pre, depth, batch=B)``) gives ``[B, n_post]``
    through the same stacked matrix and the same gradient, summed over the batch; the plasticity updates are
    defined for one sample.  Dendritic delays and CSC and JIT-connectivity inputs are not built."""

    def __init__(self, args, *, shape, depth: int, backend: Optional[str] = None):
        if len(args) != 4:
            raise ValueError("DelayedCSR expects (data, indices, indptr, delays).")
        data, indices, indptr, delays = args
        depth = int(depth)
        shape = (int(shape[0]), int(shape[1]))
        if not 1 <= depth <= MAX_DELAY_DEPTH:
            raise ValueError(f"DelayedCSR: depth must lie in [1, {MAX_DELAY_DEPTH}]; got {depth}.")
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"DelayedCSR: shape must be positive; got {shape}.")
        if depth * shape[0] >= _ID_LIMIT:
            raise ValueError(f"DelayedCSR: depth * n_pre = {depth * shape[0]} must stay below 2^31 (stacked row ids are int32).")
        ishape = _shape_of(indices)
        if indptr is None:
            if len(ishape) != 2 or ishape[0] != shape[0]:
                raise ValueError(f"DelayedCSR: with indptr=None indices must be [n_pre, row_len]; got shape {ishape}.")
            row_len = int(ishape[1])
        else:
            if len(ishape) != 1:
                raise ValueError(f"DelayedCSR: indices must be 1-D beside an indptr; got shape {ishape}.")
            if _shape_of(indptr) != (shape[0] + 1,):
                raise ValueError(f"DelayedCSR: indptr must have n_pre + 1 = {shape[0] + 1} elements; got shape {_shape_of(indptr)}.")
            row_len = -1
        nnz = int(np.prod(ishape))
        n_data = int(np.prod(_shape_of(data)))
        if n_data != 1 and n_data != nnz:
            raise ValueError(f"DelayedCSR: data must have one element or one per stored entry ({nnz}); got {n_data}.")
        delays = _as_int32_delays(delays, nnz)
        # ---- everything below runs on the device
        from ._misc import _as_int32_indices, _as_indptr
        self._numpy_result = A.wants_numpy(data, indices, indptr, delays)
        self.shape, self.depth, self.backend = shape, depth, backend
        self.delays = A.to_device(delays, torch.int32).reshape(-1)
        w = A.to_device(data)
        if not w.dtype.is_floating_point:
            raise TypeError('Weights must be a floating-point type.')
        idx = _as_int32_indices(A.to_device(indices), shape[1], 'DelayedCSR', check_values=True)
        ptr_ = None
        if indptr is not None:
            ptr_ = A.to_device(indptr)
            if ptr_.dtype not in (torch.int32, torch.int64):
                ptr_ = _as_indptr(ptr_, nnz, 'auto', 'DelayedCSR')
            if int(ptr_[0]) != 0 or int(ptr_[-1]) != nnz or bool((ptr_[1:] < ptr_[:-1]).any()):
                raise ValueError("DelayedCSR: indptr must start at 0, be non-decreasing and end at the number of stored entries.")
        self._data_shape = tuple(w.shape)
        indptr_s, perm, indices_s, self.row_mask = _split_by_delay(idx, ptr_, row_len, self.delays, shape[0], depth, nnz)
        self.perm = perm
        data_s = w.reshape(-1) if n_data == 1 else w.reshape(-1)[self._gather]
        self.stacked = _stacked_csr(data_s, indices_s, indptr_s, (depth * shape[0], shape[1]), backend, self._numpy_result)

    @classmethod
    def of_container(cls, M, indptr, delays, depth: int) -> 'DelayedCSR':
        """``M.with_delays``: the arrays of a ``CSR`` / ``FixedNumPerPre`` (``indptr=None``); results follow ``M``'s numpy rule."""
        obj = cls((M.data, M.indices, indptr, delays), shape=M.shape, depth=depth, backend=M.backend)
        obj._numpy_result = obj.stacked._numpy_result = M._numpy_result
        return obj

    # -- properties -----------------------------------------------------------------------------------------------------
    dtype = property(lambda self: self.stacked.data.dtype)
    ndim = property(lambda self: 2)
    nse = property(lambda self: int(self.delays.numel()))

    @property
    def _gather(self) -> torch.Tensor:
        """``perm`` as torch indexes with it (int64): made when asked for, not kept — 8 bytes per entry."""
        return self.perm if self.perm.dtype == torch.int64 else self.perm.long()

    @property
    def data(self):
        """The weights in the ORIGINAL order (gathered back from ``stacked.data``; one shared weight as it is)."""
        d = self.stacked.data
        if int(np.prod(self._data_shape)) == 1:
            return d.reshape(self._data_shape)
        out = torch.empty_like(d)
        out[self._gather] = d
        return out.reshape(self._data_shape)

    def prepare(self, **kw) -> 'DelayedCSR':
        """Build the stacked matrix's scatter workspace now (``CSR.prepare``'s keywords)."""
        self.stacked.prepare(**kw)
        return self

    def _stacked_order(self, new_data) -> torch.Tensor:
        w = A.to_device(new_data)
        old = self.stacked.data
        if int(w.numel()) != int(np.prod(self._data_shape)) or w.dtype != old.dtype:
            raise ValueError(f"DelayedCSR: new data must have {int(np.prod(self._data_shape))} elements of {old.dtype} "
                             f"(the original order); got {int(w.numel())} of {w.dtype}.")
        return w.reshape(-1) if old.numel() == 1 and w.numel() == 1 else w.reshape(-1)[self._gather]

    def with_data(self, new_data) -> 'DelayedCSR':
        """Same structure and delays, new weights, given in the original order: a new container that shares ``perm``, ``delays``,
        ``row_mask`` and the stacked structure (scatter workspaces are not shared: they embed the weights)."""
        obj = object.__new__(DelayedCSR)
        obj.__dict__.update(self.__dict__)
        obj.stacked = _stacked_csr(self._stacked_order(new_data), self.stacked.indices, self.stacked.indptr, self.stacked.shape,
                                   self.backend, self._numpy_result)
        return obj

    def set_data_(self, new_data) -> 'DelayedCSR':
        """:meth:`with_data` in place: writes ``stacked.data`` (``copy_``), under the staleness rules of ``csr.data`` — the next
        product refreshes a cached workspace by itself; between replays of a captured step call ``stacked.refresh_weights()``."""
        self.stacked.data.copy_(self._stacked_order(new_data).reshape(self.stacked.data.shape))
        return self

    @property
    def plastic_state(self):
        """``stacked.plastic_state``: ``None`` unless ``prepare(plastic=(w_min, w_max))`` armed plastic mode."""
        return self.stacked.plastic_state

    def stacked_to_original(self, t) -> torch.Tensor:
        """One value per stored entry in the order of ``stacked.data`` (``stacked.data.grad``, say) moved to the ORIGINAL order
        through ``perm``, in the shape the weights were given in — what :attr:`data` does for the weights."""
        t = A.to_device(t)
        if int(t.numel()) != int(self.stacked.data.numel()):
            raise ValueError(f"DelayedCSR.stacked_to_original: {int(t.numel())} values for {int(self.stacked.data.numel())} "
                             "stacked weights.")
        if int(np.prod(self._data_shape)) == 1:
            return t.reshape(self._data_shape)
        out = torch.empty_like(t.reshape(-1))
        out[self._gather] = t.reshape(-1)
        return out.reshape(self._data_shape)

    # -- plasticity ------------------------------------------------------------------------------------
    def _check_plastic(self, vec, vec_name: str) -> None:
        """What both updates refuse before the first device call: one shared weight, a spike / trace vector of the wrong shape."""
        from ._plasticity import _HOMO_MSG, _check_vec
        if int(np.prod(self._data_shape)) == 1 and self.nse > 1:
            raise ValueError(_HOMO_MSG)
        _check_vec(vec, self.shape[1], vec_name)

    def _updated(self, st, inplace: bool) -> 'DelayedCSR':
        if inplace:
            return self
        obj = object.__new__(DelayedCSR)
        obj.__dict__.update(self.__dict__)
        # over the stacked structure itself, as with_data (CSR.with_data would narrow an int64 indptr into a new array); the
        # clip certificate and the transposed structure of the update travel along
        obj.stacked = _stacked_csr(st.data, self.stacked.indices, self.stacked.indptr, self.stacked.shape, self.backend,
                                   self._numpy_result)
        obj.stacked.buffers.update(st.buffers)
        return obj

    def update_on_pre(self, ring: SpikeRing, post_trace, w_min=None, w_max=None, *, inplace: bool = False) -> 'DelayedCSR':
        """The update at a spike's ARRIVAL: every stored entry ``e`` whose pre neuron fired ``delays[e]`` steps ago (``ring``, as in
        ``ring @ D``) gets ``w_e += post_trace[col(e)]`` — one rounding to the weight dtype, then ``clip(W, w_min, w_max)`` over
        the whole array, as ``CSR.update_on_pre``.  ``inplace=False`` returns a new ``DelayedCSR`` sharing ``perm``, ``delays``,
        ``row_mask`` and the stacked structure; ``inplace=True`` updates ``stacked.data`` and returns ``self``, with the clip
        certificate and the plastic-mode upkeep of ``CSR.update_on_pre(inplace=True)``."""
        from ._plasticity import _bounds, container_update
        if not isinstance(ring, SpikeRing):
            raise TypeError("DelayedCSR.update_on_pre takes the SpikeRing of the pre population (the spikes by age).")
        if ring.batch is not None:
            raise NotImplementedError("DelayedCSR.update_on_pre is defined for one sample: a batched ring has no single arrival "
                                      "per synapse (batched plasticity is not built).")
        check_ring_matches(ring.n, ring.depth, self.shape, self.depth)
        self._check_plastic(post_trace, 'post_trace')
        _bounds(w_min, w_max)
        ids = ring.ids(ages=self.depth, row_mask=self.row_mask)
        return self._updated(container_update(self.stacked, True, ids, post_trace, w_min, w_max, inplace), inplace)

    def update_on_post(self, pre_history, post_spike, w_min=None, w_max=None, *, inplace: bool = False) -> 'DelayedCSR':
        """The update at a POST spike: every stored entry ``e`` of an active post neuron (``post_spike``: any encoding
        ``CSR.update_on_post`` takes, any non-zero float is a spike) gets ``w_e +=`` the pre-side value of ``row(e)`` at age
        ``delays[e]`` — what that synapse saw arrive —, then the whole-array clip; ``inplace`` as in :meth:`update_on_pre`.

        ``pre_history`` is a :class:`ValueRing` over the pre population (``n == n_pre``, ``depth >= self.depth``, the weights'
        dtype: a whole history is never converted per step), read by age inside the update kernel; or a plain ``[self.depth,
        n_pre]`` array by age (``hist.by_age()[:self.depth]``), which is the stacked matrix's pre-trace as it is."""
        from ._plasticity import _bounds, container_update
        if isinstance(pre_history, ValueRing):
            if pre_history.n != self.shape[0]:
                raise ValueError(f"DelayedCSR.update_on_post: the history holds {pre_history.n} neurons, the matrix has "
                                 f"{self.shape[0]} rows.")
            if pre_history.depth < self.depth:
                raise ValueError(f"DelayedCSR.update_on_post: the history remembers {pre_history.depth} steps, the matrix needs "
                                 f"depth {self.depth}.")
            if pre_history.dtype != self.dtype:
                raise TypeError(f"DelayedCSR.update_on_post: the history holds {pre_history.dtype}, the weights are {self.dtype}: "
                                "build the ValueRing in the weights' dtype (push converts one vector per step).")
            trace, aged = None, (pre_history, self.depth)
        else:
            if _shape_of(pre_history) != (self.depth, self.shape[0]):
                raise ValueError(f"DelayedCSR.update_on_post: a history by age must have shape ({self.depth}, {self.shape[0]}); got "
                                 f"{_shape_of(pre_history)}.")
            trace = (pre_history if isinstance(pre_history, torch.Tensor) else np.asarray(pre_history)).reshape(-1)
            aged = None
        self._check_plastic(post_spike, 'post_spike')
        _bounds(w_min, w_max)
        return self._updated(container_update(self.stacked, False, post_spike, trace, w_min, w_max, inplace, aged=aged), inplace)

    # -- product --------------------------------------------------------------------------------------------------------
    def __rmatmul__(self, ring):
        if not isinstance(ring, SpikeRing):
            raise NotImplementedError("x @ DelayedCSR is defined for a SpikeRing (a batch of histories: SpikeRing(n, depth, "
                                      "batch=B)); a 2-D array of spikes carries no history.")
        check_ring_matches(ring.n, ring.depth, self.shape, self.depth)
        if ring.batch is not None:
            return self._batched_product(ring)
        from ._csr import _csr_p_call, binary_csrmv_p
        ids = ring.ids(ages=self.depth, row_mask=self.row_mask)
        st = self.stacked
        rows = st._stored_rows()
        r = _csr_p_call(binary_csrmv_p, st.data, rows.indices, rows.indptr, ids, st._scatter_workspace(), (rows.m, rows.k), True,
                        self.backend)[0]
        return A.to_result(r, self._numpy_result and ring._numpy and not r.requires_grad)

    def _batched_product(self, ring: SpikeRing):
        """``ring @ D`` for a batched ring: the histories unrolled by age are the ``BE_SPIKE_BITS`` batch operand
        ``[B, ceil(depth * n_pre / 32)]`` of the stacked matrix's scatter step, on the matrix's own workspace."""
        from . import _autograd as _ag
        from ._csr import binary_csrmm_p, rows_step
        binary_csrmm_p.resolve(self.backend)                    # (an unknown backend is refused as the 1-D product refuses it)
        st = self.stacked
        rows = st._stored_rows()
        ws = st._scatter_workspace()
        words = ring.stacked_bits(ages=self.depth, row_mask=self.row_mask)
        weights = st.data.reshape(1) if st.data.ndim == 0 else st.data

        def run():
            return rows_step(weights.detach(), rows.indices, rows.indptr, -1, words, A.BE_SPIKE_BITS, m=rows.m, k=rows.k,
                             transpose=True, workspace=ws)

        if _ag.needed(weights):
            # the ring reuses `words` from step to step: the packed activity, not the buffer, is what backward keeps (2.16)
            spec = _ag.RowsSpec(run, rows, True, 'bm')
            spec.w_meta = (tuple(weights.shape), weights.dtype)
            spec.mask, spec.nb = _ag.packed_activity(words, rows.m, ring.batch), ring.batch
            r = _ag.RowsProduct.apply(weights, None, spec)
        else:
            r = run()
        return A.to_result(r, self._numpy_result and ring._numpy and not r.requires_grad)

    def __matmul__(self, other):
        raise NotImplementedError("DelayedCSR @ x is not defined: the delays live on the presynaptic side (ring @ D).")

    def __repr__(self):
        return f"DelayedCSR(shape={self.shape}, depth={self.depth}, nse={self.nse}, dtype={self.dtype})"


def _stacked_csr(data, indices, indptr, shape, backend, numpy_result):
    from ._csr import CSR
    st = CSR((data, indices, indptr), shape=shape, backend=backend, indptr_dtype=indptr.dtype, check_structure=False)
    st._numpy_result = numpy_result
    return st


def _split_by_delay(indices, indptr, row_len: int, delays, m: int, depth: int, nnz: int):
    """``(indptr_s, perm, indices_s, row_mask)`` of the stacked matrix (``be_delay_split_count`` -> scan -> ``_fill``).  The index
    type of ``indptr_s`` and ``perm`` is int64 whenever ``indptr`` is, or from 2^31 entries on.  Reads the error word once."""
    dev = delays.device
    is64 = int(indptr is not None and indptr.dtype == torch.int64)
    out64 = int(bool(is64) or nnz >= _ID_LIMIT)
    pt = torch.int64 if out64 else torch.int32
    if nnz == 0:
        return (torch.zeros(depth * m + 1, dtype=pt, device=dev), torch.zeros(0, dtype=pt, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros((depth, (m + 31) // 32), dtype=torch.int32, device=dev))
    counts = torch.empty(depth * m + 1, dtype=pt, device=dev)
    ws = A.workspace(fn('be_delay_split_workspace_bytes')(m, depth))
    call('be_delay_split_count', A.ptr(indptr), is64, row_len, A.ptr(delays), m, depth, A.ptr(counts), out64, A.ptr(ws), ws.numel(),
         A.stream_ptr())
    bad = int(ws[:8].view(torch.int64)[0])           # (the error word, read once: a host synchronisation, at build time)
    if bad >= 0:
        raise ValueError(f"DelayedCSR: delays[{bad}] = {int(delays[bad])} lies outside [0, depth = {depth}).")
    indptr_s = torch.cumsum(counts, 0, dtype=pt)
    del counts
    perm = torch.empty(nnz, dtype=pt, device=dev)
    indices_s = torch.empty(nnz, dtype=torch.int32, device=dev)
    row_mask = torch.zeros((depth, (m + 31) // 32), dtype=torch.int32, device=dev)
    call('be_delay_split_fill', A.ptr(indptr), is64, row_len, A.ptr(delays), A.ptr(indices), m, depth, A.ptr(indptr_s), out64,
         A.ptr(perm), A.ptr(indices_s), A.ptr(row_mask), A.stream_ptr())
    return indptr_s, perm, indices_s, row_mask
