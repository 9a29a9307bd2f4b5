"""Plasticity and weight gradients of delayed synapses restated in numpy — shared by tests/test_delay_stdp_cpu.py (which holds the
restatement to a brute-force loop over the entries) and tests/test_delay_stdp_gpu.py.  numpy only (bf16 rounds through torch on
the CPU): nothing here needs a device.

The semantics, axonal delays, age 0 = the vector pushed last, history before the first push zero / silent,
every stored entry its own synapse:

  arrival   : ``w_e += [s_row(e)(age = delays[e])] * post_trace[col(e)]``
  post spike: ``w_e += [post_spike[col(e)] != 0] * x_row(e)(age = delays[e])``
  both      : one rounding to the weight dtype (f16 / bf16 add in f32), then ``min(max(w, w_min), w_max)`` over the whole array
  gradient  : ``dL/dw_e = g[col(e)] * [s_row(e)(age = delays[e])]`` for ``y = ring @ D``

Exactness.  One call adds at most one value to an entry, so the result of a call is ``round(w_e + t_e)`` whatever the kernel's
order: every weight comparison is an equality for arbitrary float inputs.  For PRODUCTS after updates the generators draw weights,
traces and bounds as multiples of 1/64 (the rule of tests/delay_cases.py): the updated weights stay such multiples and their sums
are exact on every route and under any fixed-point exponent."""
import numpy as np

import delay_cases as DC

__all__ = ['PUSH_TILES', 'VALUE_TILE', 'DTYPES', 'to_dtype_np', 'add_clip_np', 'value_ring_np', 'brute_on_pre', 'brute_on_post',
           'stacked_on_pre', 'stacked_on_post', 'brute_grad', 'stdp_case']

#: the tile constants of k_value_ring_push (brainevent_amd/csrc/be_delay.hip; tests/test_delay_stdp_cpu.py ties them to the source)
PUSH_TILES = {'kValueThreads': 256, 'kValuePer': 16}
#: elements of the pushed vector one workgroup converts and copies
VALUE_TILE = PUSH_TILES['kValueThreads'] * PUSH_TILES['kValuePer']

#: weight dtype name -> the numpy dtype that HOLDS its values here (bf16 values live in f32 arrays)
DTYPES = {'f32': np.float32, 'f64': np.float64, 'f16': np.float16, 'bf16': np.float32}


def to_dtype_np(x, name):
    """``x`` rounded to the weight dtype ``name`` (bf16: through torch on the CPU, held as f32)."""
    x = np.asarray(x)
    if name == 'bf16':
        import torch
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()
    return x.astype(DTYPES[name])


def add_clip_np(w, t, touched, name, lo=None, hi=None):
    """``w[touched] = round(w + t)`` in the weight dtype (f16 / bf16: the sum in f32, one rounding), then the whole-array clip with
    the bounds rounded to the dtype.  ``t`` is already a value of the dtype."""
    w = np.array(w, copy=True)
    if name in ('f16', 'bf16'):
        s = to_dtype_np(w.astype(np.float32) + np.asarray(t).astype(np.float32), name)
    else:
        s = (w + np.asarray(t).astype(w.dtype)).astype(w.dtype)
    w[touched] = s[touched]
    if lo is not None:
        w = np.maximum(w, to_dtype_np(np.array(lo, dtype=np.float64), name).astype(w.dtype))
    if hi is not None:
        w = np.minimum(w, to_dtype_np(np.array(hi, dtype=np.float64), name).astype(w.dtype))
    return w


class value_ring_np:
    """A list-based value history in the dtype ``name``: ``age(a)`` is the vector pushed ``a`` pushes ago, zero before the first
    push.  ``slots`` / ``head`` restate the device layout beside it (slot ``head`` is written, then ``head`` advances): the aged
    lookup of the update kernel reads ``slots[(head - 1 - a) % depth]``."""

    def __init__(self, n, depth, name='f32'):
        self.n, self.depth, self.name, self.history = int(n), int(depth), name, []
        self.slots, self.head = np.zeros((self.depth, self.n), dtype=DTYPES[name]), 0

    def push(self, x):
        x = np.asarray(x)
        if x.dtype == np.float64 and self.name in ('f16', 'bf16'):
            x = x.astype(np.float32)                  # (the push rounds f64 to a 16-bit dtype through f32)
        v = to_dtype_np(x, self.name)
        self.history.append(v)
        self.slots[self.head] = v
        self.head = (self.head + 1) % self.depth

    def age(self, a):
        assert 0 <= a < self.depth
        return self.history[-1 - a] if a < len(self.history) else np.zeros(self.n, dtype=DTYPES[self.name])

    def by_age(self):
        return np.stack([self.age(a) for a in range(self.depth)])

    def aged(self, a, i):
        """The device's lookup, vectorised over ages ``a`` and neurons ``i``."""
        return self.slots[(self.head - 1 - np.asarray(a)) % self.depth, np.asarray(i)]


# ---------------------------------------------------------------------------------------------------------------------------
# brute force: a loop over the entries, straight from the formulas
# ---------------------------------------------------------------------------------------------------------------------------
def _rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(np.asarray(indptr, dtype=np.int64)))


def brute_on_pre(data, indices, indptr, delays, ring, post_trace, name, lo=None, hi=None):
    data = np.asarray(data).reshape(-1)
    rows, tr = _rows_of(indptr), to_dtype_np(post_trace, name)
    t, touched = np.zeros_like(data), np.zeros(data.size, dtype=bool)
    for e in range(data.size):
        if ring.age(int(delays[e]))[rows[e]]:
            t[e], touched[e] = tr[indices[e]], True
    return add_clip_np(data, t, touched, name, lo, hi)


def brute_on_post(data, indices, indptr, delays, hist, post_spike, name, lo=None, hi=None):
    data = np.asarray(data).reshape(-1)
    rows, spk = _rows_of(indptr), np.asarray(post_spike) != 0
    t, touched = np.zeros_like(data), np.zeros(data.size, dtype=bool)
    for e in range(data.size):
        if spk[indices[e]]:
            t[e], touched[e] = hist.age(int(delays[e]))[rows[e]], True
    return add_clip_np(data, t, touched, name, lo, hi)


def brute_grad(indices, indptr, delays, ring, g):
    """``g[col(e)] * bit`` per entry, f64."""
    indices, delays = np.asarray(indices).reshape(-1), np.asarray(delays).reshape(-1)
    rows, g = _rows_of(indptr), np.asarray(g, dtype=np.float64)
    out = np.zeros(indices.size, dtype=np.float64)
    for e in range(indices.size):
        if ring.age(int(delays[e]))[rows[e]]:
            out[e] = g[indices[e]]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement in stacked form (vectorised: the GPU tests use it at every size)
# ---------------------------------------------------------------------------------------------------------------------------
def _stacked(data, indices, indptr, delays, n_pre, depth):
    indptr_s, perm, row_mask = DC.split_by_delay_np(indptr, delays, n_pre, depth)
    return indptr_s, perm, row_mask, np.asarray(data).reshape(-1)[perm], np.asarray(indices).reshape(-1)[perm]


def _unstacked(ws, perm):
    out = np.empty_like(ws)
    out[perm] = ws
    return out


def stacked_on_pre(data, indices, indptr, delays, n_pre, depth, ring, post_trace, name, lo=None, hi=None):
    """On-pre over the ACTIVE stacked rows: the ring's id list (gated by the row mask) picks rows ``d * n_pre + i`` of the stacked
    matrix, each of whose entries takes ``post_trace[col]``.  Returns the weights in the original order."""
    indptr_s, perm, row_mask, ws, cols = _stacked(data, indices, indptr, delays, n_pre, depth)
    active = np.zeros(depth * n_pre, dtype=bool)
    active[ring.ids(ages=depth, row_mask=row_mask)] = True
    touched = np.repeat(active, np.diff(indptr_s))
    return _unstacked(add_clip_np(ws, to_dtype_np(post_trace, name)[cols], touched, name, lo, hi), perm)


def stacked_on_post(data, indices, indptr, delays, n_pre, depth, hist, post_spike, name, lo=None, hi=None):
    """On-post with the aged lookup: slot ``k`` of the stacked matrix lies in stacked row ``r``; ``a = r // n_pre``, ``i = r - a *
    n_pre``, and the value is ``hist.slots[(head - 1 - a) % hist.depth, i]`` (``hist`` may be deeper than the matrix)."""
    indptr_s, perm, _, ws, cols = _stacked(data, indices, indptr, delays, n_pre, depth)
    r = np.repeat(np.arange(depth * n_pre, dtype=np.int64), np.diff(indptr_s))
    a = r // n_pre
    t = hist.aged(a, r - a * n_pre)
    touched = (np.asarray(post_spike) != 0)[cols]
    return _unstacked(add_clip_np(ws, t, touched, name, lo, hi), perm)


# ---------------------------------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------------------------------
def stdp_case(seed, n_pre, n_post, depth, max_row, name='f32', *, exact=False, parallel=True, ends=False, fixed_len=None):
    """``(data, indices, indptr, delays)`` with ``data`` holding values of the weight dtype ``name``: arbitrary floats in ``[-1,
    1]``, or (``exact``) multiples of 1/64 in ``[0, 1]``.  Some rows are empty (lengths start at 0) unless ``fixed_len`` gives every
    row that many entries; ``parallel``: synapses stored twice with delays of their own; ``ends``: only the delays 0 and ``depth -
    1``."""
    _, indices, indptr, delays = DC.exact_case(seed, n_pre, n_post, depth, max_row, parallel=parallel, fixed_len=fixed_len)
    rng = np.random.default_rng(seed + 1000)
    if ends:
        delays = DC.delay_pattern('ends', seed, indptr, depth)
    nnz = indices.size
    data = rng.integers(0, 65, nnz) / 64.0 if exact else rng.uniform(-1.0, 1.0, nnz)
    return to_dtype_np(data, name), indices, indptr, delays
