"""``torch.autograd`` through the event-driven products: ``loss.backward()`` works through ``BinaryArray(s) @ csr``.

The reference defines JVP / transpose rules for every binary product (``brainevent/_csr/binary.py:656-715``, ``:1303-1360``;
``brainevent/_dense/binary.py:290-330``; ``brainevent/_fcn/binary.py:317-``); the torch counterpart is one
``torch.autograd.Function`` per family here: :class:`RowsProduct` (CSR, CSC, ``FixedNumPerPre`` / ``FixedNumPerPost``) and
:class:`DenseProduct`.  With ``a = active(s)`` (the forward kernels' rule: ``!= 0`` for bool / integer spikes, ``> 0`` for float
spikes), ``g`` the incoming gradient and ``r(j)`` / ``c(j)`` the row / column of stored entry ``j`` in the CSR reading of the
arrays:

  ``s @ A``  ->  ``dw[j] = sum_b a[b, r(j)] * g[b, c(j)]``,  ``ds = A @ g``
  ``A @ s``  ->  ``dw[j] = sum_b g[b, r(j)] * a[b, c(j)]``,  ``ds = A.T @ g``
  one shared weight: the scalar sum over ``j``;  dense: ``dW = a.T @ g`` / ``g.T @ a`` (masked outer products).

* Weight gradients use ``a``, not the spike values: the product is exactly linear in the weights, so this is the exact
  derivative (the reference's ``_csrmv_jvp_weights``).  The reference's transpose rule multiplies by the raw float values
  instead; the two agree for 0/1 spikes and differ for other float values (a spike of 0.5 counts as 1 here, as it does in the
  forward product).
* Spike gradients are straight-through: the gradient of the linear product (the reference's ``_csrmv_jvp_v``); a surrogate
  function upstream supplies d(spike)/dV.  Only float spike tensors can receive one; bool / integer spikes and the bit-packed
  and compacted containers get weight gradients only.
* Weight gradients run on ``csrc/be_grad.hip``: per entry, f32 (f64) accumulation in ascending batch order, one rounding, every
  entry written once, no atomics (bit-reproducible).  Spike gradients reuse the float-operand kernels (``_float``; through the
  container's mirror when the direction is a scatter and a mirror exists); dense spike gradients are plain GEMMs
  (``torch.matmul``: there is no event structure in them).
* The float-operand products (``csr @ x`` with a plain array, ``csrmv / csrmm / fcnmv / fcnmm``) have a Function of their own,
  :class:`FloatRowsProduct`: the weight gradient is a sampled dense-dense product (``csrc/be_sddmm.hip``), the operand gradient
  the transposed float product.  Not differentiable: ``Dense`` with a plain array, ``PlannedMatrix``.
* The JIT-connectivity products (``binary_jit{s,u,n}{mv,mm}``, ``jit{s,u,n}{mv,mm}`` and the six containers' ``@``) store no
  weights; their one or two PARAMETERS are differentiated by :class:`JitProduct`: both parameter gradients of a call come out
  of one walk of the generated edges (``csrc/be_jitc_grad.hip``), the operand gradient is the float twin of the transposed call.
* ``solve`` (``_solve``) is differentiated by :class:`Solve`: ``db = A^-T g`` is one more solve on the transposed arrays, the
  weight gradient ``-db[row] * x[col]`` the SDDMM with one batch column.  No new kernel.
* Wrapping happens only when grad mode is on and an operand requires grad; otherwise the existing path runs untouched.  The
  forward pass of the Function IS the existing path (same route, same kernels, same bits).  Higher-order gradients are not
  supported (``once_differentiable``).
"""
from typing import Callable, Optional

import torch
from torch.autograd.function import once_differentiable

from . import _array as A
from ._error import UnsupportedOperationError
from ._lib import call, fn

__all__ = ['RowsProduct', 'FloatRowsProduct', 'DenseProduct', 'JitProduct', 'SliceRows', 'Solve', 'needed']


def _value(x):
    from ._event import BinaryArray
    return x.value if isinstance(x, BinaryArray) else x


def _requires(x) -> bool:
    x = _value(x)
    return isinstance(x, torch.Tensor) and x.requires_grad


def needed(*xs) -> bool:
    """Grad mode is on and one of the operands (a tensor, or the value of a ``BinaryArray``) requires grad."""
    return torch.is_grad_enabled() and any(_requires(x) for x in xs)


def diff_spikes(x) -> Optional[torch.Tensor]:
    """The spike tensor that receives a gradient: a float tensor that requires grad, given as is or as a ``BinaryArray``."""
    v = _value(x)
    if isinstance(v, torch.Tensor) and v.requires_grad and v.dtype.is_floating_point:
        return v
    return None


# =====================================================================================================
# device calls
# =====================================================================================================
def activity(operand, layout: str):
    """The activity of a product's spike operand (as the kernels receive it: tensor, ``PackedSpikes`` or ``ActiveIds``) as the
    per-neuron bit mask ``int32 [n, ceil(nb / 32)]`` of ``be_grad_pack_activity``.  ``layout``: ``'vec'`` (``[n]``), ``'nm'``
    (``[n, nb]``) or ``'bm'`` (``[nb, n]``).  Returns ``(mask, nb)``."""
    if layout == 'nm':
        sp, sd = A.spikes_batch_major(operand)
    else:
        sp, sd = A.spikes_to_device(operand)
    if layout == 'vec':
        n, nb = int(operand.shape[0]), 1
    else:
        nb, n = (int(s) for s in (sp.shape if sd != A.BE_SPIKE_BITS else (sp.shape[0], operand.shape[-1])))
    if sd not in (A.BE_SPIKE_BITS, A.BE_SPIKE_IDS):
        sp = sp.contiguous()
    mask = torch.empty(max(fn('be_grad_mask_bytes')(n, nb), 4) // 4, dtype=torch.int32, device=A.device())
    call('be_grad_pack_activity', A.ptr(sp), sd, n, nb, A.ptr(mask), A.stream_ptr())
    return mask, nb


def packed_activity(words: torch.Tensor, n: int, nb: int) -> torch.Tensor:
    """The per-neuron mask of a bit-packed batch ``words [nb, ceil(n / 32)]`` (``BE_SPIKE_BITS`` rows over ``n`` positions): what
    :func:`activity` builds, for an operand that exists only as packed rows (the unrolled batched ring, ``_delay``)."""
    mask = torch.empty(max(fn('be_grad_mask_bytes')(int(n), int(nb)), 4) // 4, dtype=torch.int32, device=A.device())
    call('be_grad_pack_activity', A.ptr(words), A.BE_SPIKE_BITS, int(n), int(nb), A.ptr(mask), A.stream_ptr())
    return mask


def rows_weight_grad(w_meta, indices, indptr, row_len: int, n_rows: int, transpose: bool, mask, nb: int, g_nm) -> torch.Tensor:
    """``be_grad_rows``: the gradient of the weights (``w_meta``: a tensor or ``(shape, dtype)``; one value per stored entry, or
    the scalar of a shared weight).  ``g_nm``: the output gradient neuron-major ``[out_len, nb]``."""
    shape, dtype = (tuple(w_meta.shape), w_meta.dtype) if isinstance(w_meta, torch.Tensor) else w_meta
    homo = _numel(shape) == 1
    nse = int(indices.numel())
    dw = torch.empty(1 if homo else nse, dtype=dtype, device=A.device())
    g = g_nm.to(dtype).contiguous()
    ws = A.workspace(fn('be_grad_rows_workspace_bytes')(nse)) if homo else None
    is64 = int(indptr is not None and indptr.dtype == torch.int64)
    call('be_grad_rows', int(transpose), A.ptr(dw), int(homo), A.wcode(dw), A.ptr(indices), A.ptr(indptr), is64, int(row_len),
         int(n_rows), nse, A.ptr(mask), int(nb), A.ptr(g), int(nb), 1, A.ptr(ws), 0 if ws is None else ws.numel(), A.stream_ptr())
    return dw.reshape(shape)


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def dense_weight_grad(w_meta, transpose: bool, mask, nb: int, g_nm) -> torch.Tensor:
    """``be_grad_dense``: ``dW [R, C]`` (``w_meta``: a tensor or ``(shape, dtype)``).  ``g_nm``: the output gradient
    ``[out_len, nb]``."""
    shape, dtype = (tuple(w_meta.shape), w_meta.dtype) if isinstance(w_meta, torch.Tensor) else w_meta
    n_rows, n_cols = int(shape[0]), int(shape[1])
    dw = torch.empty((n_rows, n_cols), dtype=dtype, device=A.device())
    if transpose:     # lanes run over the columns = output neurons: batch-major g keeps the loads contiguous
        g = g_nm.to(dtype).T.contiguous()
        g_sn, g_sb = 1, n_cols
    else:             # one output neuron per row: neuron-major g, a broadcast per row
        g = g_nm.to(dtype).contiguous()
        g_sn, g_sb = nb, 1
    call('be_grad_dense', int(transpose), A.ptr(dw), A.wcode(dw), n_rows, n_cols, A.ptr(mask), int(nb), A.ptr(g), g_sn, g_sb,
         A.stream_ptr())
    return dw


def _to_nm(g: torch.Tensor, layout: str) -> torch.Tensor:
    return g.reshape(-1, 1) if layout == 'vec' else (g.T if layout == 'bm' else g)


def _from_nm(d: torch.Tensor, layout: str, shape, dtype) -> torch.Tensor:
    d = d.reshape(-1) if layout == 'vec' else (d.T if layout == 'bm' else d)
    return d.to(dtype).reshape(shape)


# =====================================================================================================
# the Functions
# =====================================================================================================
class RowsSpec:
    """What the backward pass of a row-stored product needs: the stored structure (``rows``: a ``_csr.StoredRows``), the
    direction (``transpose``: the scatter over the stored rows), the operand / output layout, the packed activity and, for the
    scatter-direction spike gradient, an optional mirror source."""
    __slots__ = ('run', 'rows', 'transpose', 'layout', 'mirror', 'mask', 'nb', 'w_meta', 's_meta')

    def __init__(self, run, rows, transpose, layout, mirror=None):
        self.run, self.rows, self.transpose, self.layout, self.mirror = run, rows, bool(transpose), layout, mirror
        self.mask, self.nb, self.w_meta, self.s_meta = None, 1, None, None


class RowsProduct(torch.autograd.Function):
    """CSR / CSC / fixed-number products.  Saved: the structure, the packed activity (not the spikes) and — when the spikes
    need a gradient — the weights."""

    @staticmethod
    def forward(ctx, weights, spikes, spec: RowsSpec):
        out = spec.run()
        ctx.spec = spec
        if spikes is not None:
            ctx.save_for_backward(weights)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        spec = ctx.spec
        r = spec.rows
        g_nm = _to_nm(g, spec.layout)
        dw = ds = None
        if ctx.needs_input_grad[0]:
            dw = rows_weight_grad(spec.w_meta, r.indices, r.indptr, r.row_len, r.m, spec.transpose, spec.mask, spec.nb, g_nm)
        if ctx.needs_input_grad[1]:
            ds = _from_nm(_rows_spike_grad(ctx.saved_tensors[0], spec, g_nm), spec.layout, *spec.s_meta)
        return dw, ds, None


def _rows_spike_grad(weights, spec: RowsSpec, g_nm) -> torch.Tensor:
    from ._float import _float_csr
    r = spec.rows
    if spec.transpose:            # s @ A: ds = A @ g (gather over the stored rows)
        return _float_csr(weights, r.indices, r.indptr, r.row_len, g_nm, m=r.m, k=r.k, transpose=False)
    mr = spec.mirror() if spec.mirror is not None else None
    if mr is not None:            # A @ s: ds = A.T @ g — a scatter; the mirror turns it into a gather
        return _float_csr(mr.data.detach(), mr.indices, mr.indptr, -1, g_nm, m=int(mr.shape[0]), k=int(mr.shape[1]), transpose=False)
    return _float_csr(weights, r.indices, r.indptr, r.row_len, g_nm, m=r.m, k=r.k, transpose=True)


def rows_product(run: Callable, weights, spikes_arg, operand, layout: str, rows, transpose: bool, mirror=None):
    """Run ``run()`` (the existing forward path) as a :class:`RowsProduct` over the stored ``rows``.  ``spikes_arg``: what the
    caller got (tensor or event container), ``operand``: what the kernels receive."""
    spec = RowsSpec(run, rows, transpose, layout, mirror)
    spec.w_meta = (tuple(weights.shape), weights.dtype)
    s = diff_spikes(spikes_arg)
    if s is not None:
        spec.s_meta = (s.shape, s.dtype)
    if weights.requires_grad:
        spec.mask, spec.nb = activity(operand, layout)
    return RowsProduct.apply(weights, s, spec)


class FloatRowsProduct(torch.autograd.Function):
    """The float-operand products over stored rows ``A [m, k]`` (``csrmv / csrmm / fcnmv / fcnmm`` and the containers' ``@``
    with a plain array): every element of the operand ``X`` counts.  With ``g`` the incoming gradient, both neuron-major
    ``[., nb]`` (a vector is ``nb = 1``), and ``sddmm(P, Q)[j] = sum_b P[r(j), b] Q[c(j), b]`` (``csrc/be_sddmm.hip``):

      ``A @ X``   (``transpose=False``)  ->  ``dw = sddmm(P = g, Q = X)``,  ``dX = A.T @ g``
      ``A.T @ X`` (``transpose=True``)   ->  ``dw = sddmm(P = X, Q = g)``,  ``dX = A @ g``
      one shared weight: the scalar ``sum(P * (A1 @ Q))``, ``A1`` the structure with weight 1 — the float product in the
      gather direction, then one ``torch.sum``: no float atomics.

    ``dX`` is :func:`_rows_spike_grad` (a live mirror serves the scatter direction; none is built).  The backward pass reads
    the raw stored rows only, so ``dw`` arrives in ``data``'s own order and shape whichever route the forward pass took.
    Saved: the operand when the weights need a gradient, the weights when the operand does."""

    @staticmethod
    def forward(ctx, weights, x, x_nm, spec: RowsSpec):
        out = spec.run()
        ctx.spec = spec
        ctx.save_for_backward(weights if x is not None else None, x_nm)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        spec = ctx.spec
        r = spec.rows
        weights, x_nm = ctx.saved_tensors
        g_nm = _to_nm(g, spec.layout)
        dw = dx = None
        if ctx.needs_input_grad[0]:
            dw = float_rows_weight_grad(spec.w_meta, r, (x_nm, g_nm) if spec.transpose else (g_nm, x_nm))
        if ctx.needs_input_grad[1]:
            shape, dtype, dev = spec.s_meta
            dx = _from_nm(_rows_spike_grad(weights, spec, g_nm), spec.layout, shape, dtype).to(dev)
        return dw, dx, None, None


def float_rows_weight_grad(w_meta, rows, pq) -> torch.Tensor:
    """The weight gradient of a float-operand product over ``rows``: ``sddmm(P, Q)`` per stored entry in the weights' shape, or
    the scalar of a shared weight.  ``pq = (P [m, nb], Q [k, nb])``."""
    from ._float import _float_csr
    from ._sddmm import sddmm_rows
    shape, dtype = w_meta
    P, Q = (t.to(dtype) for t in pq)
    if _numel(shape) == 1 and int(rows.indices.numel()) != 1:
        one = torch.ones(1, dtype=dtype, device=A.device())
        aq = _float_csr(one, rows.indices, rows.indptr, rows.row_len, Q, m=rows.m, k=rows.k, transpose=False)     # A1 @ Q [m, nb]
        acc = torch.float64 if dtype == torch.float64 else torch.float32
        return torch.sum(P.to(acc) * aq.to(acc)).to(dtype).reshape(shape)
    return sddmm_rows(rows.indices, rows.indptr, rows.row_len, None, rows.m, rows.k, P, Q).reshape(shape)


def float_rows_product(run: Callable, weights, x, layout: str, rows, transpose: bool, mirror=None):
    """Run ``run()`` (the existing forward path) as a :class:`FloatRowsProduct` over the stored ``rows``.  ``x``: the dense
    operand as the caller gave it (a tensor), ``layout`` as for :func:`rows_product`."""
    spec = RowsSpec(run, rows, transpose, layout, mirror)
    spec.w_meta = (tuple(weights.shape), weights.dtype)
    xd = x if (x.requires_grad and x.dtype.is_floating_point) else None
    if xd is not None:
        spec.s_meta = (x.shape, x.dtype, x.device)
    x_nm = None
    if weights.requires_grad:          # the operand by value, neuron-major in the weights' dtype
        x_nm = _to_nm(A.to_device(x.detach(), dtype=weights.dtype), layout)
    return FloatRowsProduct.apply(weights, xd, x_nm, spec)


def float_needed(weights, x) -> bool:
    """Whether a float-operand product is to be recorded: grad mode is on, the operand is a tensor (numpy operands give numpy
    results without autograd), and the weights or the operand require grad."""
    return isinstance(x, torch.Tensor) and isinstance(weights, torch.Tensor) and needed(weights, x)


def container_float_product(M, other, left: bool, run: Callable):
    """``other @ M`` (``left``) or ``M @ other`` of a CSR / CSC / fixed-number container with a dense tensor operand, as a
    :class:`FloatRowsProduct` over the container's own arrays (whichever route — direct or mirror — ``run`` takes)."""
    if other.ndim not in (1, 2):
        with torch.no_grad():
            return run()               # (raises: the forward path's own error)
    t = M._scatter_side(left)
    layout = 'vec' if other.ndim == 1 else ('bm' if left else 'nm')
    return float_rows_product(run, M.data, other, layout, M._stored_rows(), t, mirror=None if t else (lambda: _live_mirror(M)))


class DenseSpec:
    __slots__ = ('run', 'transpose', 'layout', 'mask', 'nb', 's_meta')

    def __init__(self, run, transpose, layout):
        self.run, self.transpose, self.layout = run, bool(transpose), layout
        self.mask, self.nb, self.s_meta = None, 1, None


class DenseProduct(torch.autograd.Function):
    """``binary_densemv/mm``.  ``transpose=True``: ``s @ W``; ``False``: ``W @ s``.  Spike gradients are plain GEMMs."""

    @staticmethod
    def forward(ctx, weights, spikes, spec: DenseSpec):
        out = spec.run()
        ctx.spec = spec
        ctx.save_for_backward(weights if spikes is not None else None)
        ctx.w_meta = (tuple(weights.shape), weights.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        spec = ctx.spec
        g_nm = _to_nm(g, spec.layout)
        dw = ds = None
        if ctx.needs_input_grad[0]:
            dw = dense_weight_grad(ctx.w_meta, spec.transpose, spec.mask, spec.nb, g_nm)
        if ctx.needs_input_grad[1]:
            w = ctx.saved_tensors[0]
            gw = g_nm.to(w.dtype)
            d = torch.matmul(w, gw) if spec.transpose else torch.matmul(w.T, gw)
            ds = _from_nm(d, spec.layout, *spec.s_meta)
        return dw, ds, None


def dense_product(run: Callable, weights, spikes_arg, operand, layout: str, *, transpose: bool):
    spec = DenseSpec(run, transpose, layout)
    s = diff_spikes(spikes_arg)
    if s is not None:
        spec.s_meta = (s.shape, s.dtype)
    if weights.requires_grad:
        spec.mask, spec.nb = activity(operand, layout)
    return DenseProduct.apply(weights, s, spec)


class JitSpec:
    """What the backward pass of a JITC product needs besides the saved tensors: the generator ``(family, clen, seed, shape,
    transpose, corder, rank)``, the operand / output layout, the product's dtype, the parameters that are no inputs of the node
    (python / numpy values, tensors that need no gradient) and the operand's ``(shape, dtype, device)``."""
    __slots__ = ('run', 'family', 'clen', 'seed', 'shape', 'transpose', 'corder', 'rank', 'layout', 'dtype', 'consts', 's_meta')

    def __init__(self, run, family, clen, seed, shape, transpose, corder, rank, layout, dtype):
        self.run, self.family, self.clen, self.seed = run, family, int(clen), int(seed)
        self.shape, self.transpose, self.corder = (int(shape[0]), int(shape[1])), bool(transpose), bool(corder)
        self.rank, self.layout, self.dtype = int(rank), layout, dtype
        self.consts, self.s_meta = (None, None), None


class JitProduct(torch.autograd.Function):
    """The JIT-connectivity products, event and float operands alike.  The generator of a call — fixed by ``(shape, transpose,
    corder, seed, prob, rank)``; rows = walk owners — carries ``w = w0 + t(r, j) w1`` on edge ``(r, j)`` (scalar: ``w = w0``).
    With ``X`` the operand (event products: the 0/1 activity), ``g`` the incoming gradient, both neuron-major ``[., nb]``, and
    ``(P, Q) = (g, X)`` when ``corder`` else ``(X, g)``:

      ``S0 = sum_edges sum_b P[r, b] Q[j, b]``,  ``S1 = sum_edges t(r, j) sum_b P[r, b] Q[j, b]``   (``be_jit_param_grad``)
      scalar: ``d weight = S0``;  uniform: ``d w_low = S0 - S1``, ``d w_high = S1``;  normal: ``d w_loc = S0``, ``d w_scale = S1``
      ``dX = M.T @ g``: the float twin of the same family and rank with ``transpose`` and ``corder`` both flipped (the same
      generator, so the same matrix), on the parameter values the forward pass read.

    Inputs: the two parameters (``None`` where they are no size-1 floating tensors that require grad) and the differentiable
    operand (``None`` otherwise).  Saved: those, and — when a parameter needs a gradient — the operand neuron-major in the
    product's dtype.  The forward pass is ``spec.run()``: the existing path, the stored twin of ``prepare()`` included."""

    @staticmethod
    def forward(ctx, a, b, x, x_nm, spec: JitSpec):
        out = spec.run()
        ctx.spec = spec
        ctx.save_for_backward(a, b, x_nm)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import _jitc as J
        spec = ctx.spec
        a, b, x_nm = ctx.saved_tensors
        g_nm = _to_nm(g, spec.layout).to(spec.dtype).contiguous()
        da = db = dx = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            P, Q = jit_pq(spec.corder, g_nm, x_nm)
            sums = J.jit_param_sums(spec.family, P, Q, clen=spec.clen, seed=spec.seed, shape1=spec.shape[1],
                                    stride=32 if spec.rank == 1 else 4)
            ga, gb = jit_param_grads(spec.family, sums[0], sums[1])
            if ctx.needs_input_grad[0]:
                da = ga.to(a.dtype).reshape(a.shape).to(a.device)
            if ctx.needs_input_grad[1]:
                db = gb.to(b.dtype).reshape(b.shape).to(b.device)
        if ctx.needs_input_grad[2]:
            pa, pb = (a if a is not None else spec.consts[0]), (b if b is not None else spec.consts[1])
            twin = getattr(J, f"jit{spec.family}{'mv' if spec.rank == 1 else 'mm'}_p_call")
            t_transpose, t_corder = jit_twin_flags(spec.transpose, spec.corder)
            d = twin(*((pa,) if spec.family == 's' else (pa, pb)), spec.clen, g_nm[:, 0] if spec.rank == 1 else g_nm, spec.seed,
                     shape=spec.shape, transpose=t_transpose, corder=t_corder)[0]
            shape, dtype, dev = spec.s_meta
            dx = _from_nm(d, spec.layout, shape, dtype).to(dev)
        return da, db, dx, None, None


def jit_pq(corder: bool, g_nm, x_nm):
    """``(P, Q)`` of the two sums: ``P`` is indexed by generator row, ``Q`` by walk position."""
    return (g_nm, x_nm) if corder else (x_nm, g_nm)


def jit_param_grads(family: str, s0, s1):
    """The gradients of the family's parameters from ``S0`` / ``S1``: ``w = w0 + t w1`` with ``w1 = high - low`` (uniform)."""
    if family == 's':
        return s0, None
    return (s0 - s1, s1) if family == 'u' else (s0, s1)


def jit_twin_flags(transpose: bool, corder: bool):
    """``(transpose, corder)`` of the float twin that computes ``M.T @ g`` on the same ``shape``: both flipped — the same
    generator rows and walk, so the same matrix."""
    return (not transpose, not corder)


def _jit_param(p) -> bool:
    """A differentiable JITC parameter: a size-1 floating tensor that requires grad (``prob`` and ``seed`` never are)."""
    return isinstance(p, torch.Tensor) and p.requires_grad and p.dtype.is_floating_point and p.numel() == 1


def jit_needed(params, x) -> bool:
    """Whether a JITC product is to be recorded: grad mode is on and a parameter, or a float tensor operand (given as is or as
    the value of an event container), requires grad."""
    return torch.is_grad_enabled() and (any(_jit_param(p) for p in params) or diff_spikes(x) is not None)


def _jit_operand_nm(x, source, layout: str, event: bool, dtype) -> torch.Tensor:
    """The operand of a JITC product by value, neuron-major ``[in_len, nb]`` in the product's dtype; for an event product its
    0/1 activity (the forward kernels' rule), built from the container's value where the kernels received packed words."""
    if isinstance(x, A.PackedSpikes):
        if source is not None:
            x = source.value
        else:
            bits, n = x.bits, x.n
            x = torch.empty(n, dtype=torch.bool, device=A.device())
            call('be_unpack_spikes', A.ptr(A.to_device(bits)), n, A.ptr(x), A.stream_ptr())
    elif isinstance(x, A.ActiveIds):
        raise UnsupportedOperationError("a JIT-connectivity product takes no compacted id list.")
    t = A.to_device(x.detach() if isinstance(x, torch.Tensor) else x)
    if event:
        t = (t > 0) if t.dtype.is_floating_point else (t != 0)
    return _to_nm(t.to(dtype), layout).contiguous()


def jit_product(run: Callable, family: str, a, b, clen, x, seed, *, shape, transpose: bool, corder: bool, rank: int, layout: str,
                event: bool, dtype, source=None):
    """Run ``run()`` (the existing forward path) as a :class:`JitProduct`.  ``x``: the operand as the product receives it (a
    tensor, a numpy array, packed words — ``source`` is then the event container they came out of — or an event container's
    value); ``layout`` as for :func:`rows_product`."""
    spec = JitSpec(run, family, clen, seed, shape, transpose, corder, rank, layout, dtype)
    pa, pb = (a if _jit_param(a) else None), (b if _jit_param(b) else None)
    spec.consts = (None if pa is not None else a, None if pb is not None else b)
    xd = diff_spikes(x)
    if xd is not None:
        spec.s_meta = (xd.shape, xd.dtype, xd.device)
    x_nm = _jit_operand_nm(x, source, layout, event, dtype) if (pa is not None or pb is not None) else None
    return JitProduct.apply(pa, pb, xd, x_nm, spec)


class SliceRows(torch.autograd.Function):
    """``W[rows]`` (``_slice``: CSR, CSC, ``FixedNumPerPre`` / ``FixedNumPerPost`` and the functional ``csr_slice_rows``).  The
    read is linear in the weights; its transpose is ``be_slice_rows_grad``: per stored entry of a selected row the sum of the
    incoming gradient over the selections of that row, ascending, one rounding, no atomics.  ``run`` is the existing forward
    path; ``grad(g)`` returns the gradient in ``data``'s shape (for the containers that store the transpose: moved back from
    the mirror's order through its permutation).  Nothing is saved: the structure lives in the two closures."""

    @staticmethod
    def forward(ctx, data, run: Callable, grad: Callable):
        ctx.grad = grad
        return run()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ctx.grad(g), None, None


def slice_rows(data, run: Callable, grad: Callable):
    """Run ``run()`` as a :class:`SliceRows` node whose backward is ``grad``."""
    return SliceRows.apply(data, run, grad)


class Solve(torch.autograd.Function):
    """``x = A^-1 b`` (``_solve``: ``CSR.solve`` / ``CSC.solve`` / ``csr_solve``) over the CSR arrays ``(data, indices, indptr)`` of
    ``A``.  With ``g`` the incoming gradient: ``db = A^-T g`` — one more solve, on the CSR arrays of ``A.T`` (the arrays of
    ``tocsc()``), to the forward call's ``rtol`` and ``maxiter`` — and ``ddata[e] = -db[row(e)] * x[col(e)]``, the SDDMM of
    ``csrc/be_sddmm.hip`` with one batch column; one shared weight receives the sum.  ``spec = (run, indices, indptr, n, rtol,
    maxiter, who)``; ``run()`` is the existing forward path and returns ``(x, info)``; ``info`` is handed back through
    ``spec``.  A backward solve that does not converge raises ``MathError``.  ``x0`` is not differentiated.  ``run`` is dropped
    once it has run, so that the node does not keep its closure (``b``, ``x0``) alive until the backward.  The backward
    rebuilds the index of ``A.T`` (``csr_to_csc_index``) on every call: nothing is cached on the node."""

    @staticmethod
    def forward(ctx, data, b, spec: dict):
        x, spec['info'] = spec.pop('run')()
        ctx.spec = spec
        ctx.save_for_backward(data, x)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from ._convert import csr_to_csc_index
        from ._sddmm import sddmm_rows
        from ._solve import solve_arrays, _raise_unless_converged
        spec = ctx.spec
        data, x = ctx.saved_tensors
        idx, ptr_, n = spec['indices'], spec['indptr'], spec['n']
        w = data.detach().reshape(-1)
        nse = int(idx.numel())
        shared = w.numel() == 1 and nse != 1
        tptr, tidx, perm = csr_to_csc_index(ptr_, idx, shape=(n, n))
        tw = w.expand(nse).contiguous() if shared else w
        db, info = solve_arrays(tw[perm.long()], tidx, tptr.to(ptr_.dtype), A.to_device(g.detach(), dtype=w.dtype), n,
                                rtol=spec['rtol'], maxiter=spec['maxiter'])
        _raise_unless_converged(info, spec['rtol'], spec['who'] + ' (backward)')
        dw = None
        if ctx.needs_input_grad[0]:
            dw = -sddmm_rows(idx, ptr_, -1, None, n, n, db.reshape(n, 1), x.reshape(n, 1))
            dw = (dw.sum() if shared else dw).reshape(data.shape)
        return dw, (db if ctx.needs_input_grad[1] else None), None


def solve(run: Callable, data, b, indices, indptr, n: int, *, rtol: float, maxiter: int, who: str):
    """Run ``run()`` (the existing solve, ``(x, info)``) as a :class:`Solve` node; returns ``(x, info)``."""
    spec = dict(run=run, indices=indices, indptr=indptr, n=int(n), rtol=rtol, maxiter=maxiter, who=who, info=None)
    x = Solve.apply(data, b, spec)
    return x, spec['info']


def refuse_planned() -> None:
    raise UnsupportedOperationError(
        "PlannedMatrix holds no raw structure to differentiate against: a gradient through it cannot be computed. Keep the "
        "container (prepare(release_raw=False)) or run the product under torch.no_grad().")


def _live_mirror(M):
    """The container's mirror when it exists and still holds its raw arrays (a gather for the scatter-direction spike
    gradient), else ``None``; never builds one."""
    if M.buffers.get('mirror') is None:
        return None
    mr = M._fresh_mirror(auto=False)
    if mr is None or mr.released or mr.indices is None or mr.indptr is None:
        return None
    return mr


def container_product(M, other, left: bool, run: Callable):
    """``other @ M`` (``left``) or ``M @ other`` of a CSR / CSC / fixed-number container with an event operand, as a
    :class:`RowsProduct` over the container's own arrays (whichever route — direct, plan, binned, mirror — ``run`` takes).
    A numpy operand gives a numpy result, without autograd."""
    from ._event import event_operand
    operand = event_operand(other, scatter=True)
    if A.wants_numpy(operand):
        with torch.no_grad():
            return run()
    t = M._scatter_side(left)
    layout = 'vec' if operand.ndim == 1 else ('bm' if left else 'nm')
    return rows_product(run, M.data, other, operand, layout, M._stored_rows(), t,
                        mirror=None if t else (lambda: _live_mirror(M)))
