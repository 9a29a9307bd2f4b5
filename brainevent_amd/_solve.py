"""``solve``: ``A x = b`` for CSR / CSC / Dense — the step after ``diag_add``: an implicit Euler step ``(I - dt L) v' = v`` of a
cable or compartment model, the fixed point of a linearised rate network.

Reference surface (read as text): ``CSR.solve`` (``brainevent/_csr/main.py:1778-1814``), ``CSC.solve`` (``:2698-2734``),
``Dense.solve`` (``_dense/main.py:408-424``) and ``csr_solve`` (``_csr/spsolve.py``: cuSOLVER sparse QR).  Names, positional
parameters and the two assertions are the reference's.  Differences, all this project's own:

* **the method is iterative**: right-preconditioned BiCGSTAB with the Jacobi preconditioner (``csrc/be_solve.hip``), five
  launches per iteration and no host synchronisation inside one.  ``tol`` and ``reorder`` (the singularity tolerance and the
  fill-reducing ordering of the reference's QR) are accepted and unused, exactly as the reference's own ``Dense.solve`` treats
  them;
* the contract is a residual: on return ``|b - A x|_2 <= rtol |b|_2``, the residual recomputed from ``x`` by one more matrix
  pass (not the recurrence's).  ``rtol=None`` is the project's bar for the dtype: ``1e-5`` for f32, ``1e-10`` for
  f64.  :class:`MathError` when ``maxiter`` iterations do not get there or the recurrence breaks down (a vanishing ``rho`` or
  ``omega``, a NaN) — a matrix with no useful diagonal (a permutation, say) can, where a QR would not;
* ``CSC.solve`` solves ``A x = b`` as its docstring promises; the reference's code path (``:2698-2734``) hands over the
  transposed arrays;
* results are bit-identical from call to call (no float atomics, fixed-order sums), and ``solve`` is differentiable in ``data``
  and ``b`` (``_autograd.Solve``).

A matrix without a nonzero off-diagonal entry is solved directly, ``x = b / D`` with one rounding, in zero iterations; ``x0``
is not used there."""
from typing import Optional

import numpy as np
import torch

from . import _array as A
from ._error import MathError
from ._lib import call, fn
from ._op import OpKernel

__all__ = ['csr_solve', 'csr_solve_p', 'csr_solve_p_call', 'container_solve', 'dense_solve', 'solve_arrays', 'default_rtol',
           'CHUNK', 'MAX_RESTARTS']

#: iterations enqueued between two reads of the device state
CHUNK = 8
#: restarts from the true residual when the recurrence's residual reported convergence and the true one missed ``rtol``
MAX_RESTARTS = 3

_RTOL = {torch.float32: 1e-5, torch.float64: 1e-10}
#: ``SolveState`` of csrc/be_solve.hip
_STATE = np.dtype([('rho', '<f8'), ('rho_old', '<f8'), ('alpha', '<f8'), ('omega', '<f8'), ('rr', '<f8'), ('status', '<i4'),
                   ('iters', '<i4'), ('first', '<i4'), ('offdiag', '<i4'), ('n_rr', '<i4'), ('half', '<i4'), ('pad', '<i4', (2,))])
_RUNNING, _CONVERGED, _BREAKDOWN = 0, 1, 2
_B_MESSAGE = "The number of rows in the matrix must match the size of the right-hand side vector b."


def default_rtol(dtype) -> float:
    return _RTOL[dtype]


def _arr(x):
    return x if isinstance(x, torch.Tensor) else np.asarray(x)


def _torch_dtype(x):
    return x.dtype if isinstance(x, torch.Tensor) else torch.from_numpy(np.empty(0, dtype=x.dtype)).dtype


def check_operands(data_dtype, shape, b) -> None:
    """The refusals that need no device.  ``b`` is 1-D of length ``shape[0]`` (the reference's assertion), the matrix square,
    ``data`` f32 or f64."""
    if len(shape) != 2 or int(shape[0]) != int(shape[1]):
        raise ValueError(f"solve needs a square matrix, got shape {tuple(shape)}.")
    if data_dtype not in _RTOL:
        raise ValueError(f"solve takes float32 or float64 data, got {data_dtype}.")
    if b.ndim == 2:
        raise NotImplementedError("solve takes one right-hand side: b must be 1-D (the reference states no batching).")
    assert b.ndim == 1 and int(shape[0]) == int(b.shape[0]), _B_MESSAGE


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    return t if t.data_ptr() % 16 == 0 else t.clone()


def solve_arrays(w: torch.Tensor, idx: torch.Tensor, ptr_: torch.Tensor, b: torch.Tensor, n: int, *, rtol: float, maxiter: int,
                 x0: Optional[torch.Tensor] = None):
    """The driver on device tensors: ``w [nse]`` f32 / f64, ``idx`` int32, ``ptr_`` int32 / int64, ``b [n]`` in ``w``'s dtype.
    Returns ``(x, info)``; never raises for non-convergence (``info['converged']``).  The host reads the 72-byte state back once
    for ``|b|``, once per chunk of :data:`CHUNK` iterations and once per true residual."""
    dev = A.device()
    w, idx, b = _aligned16(w.contiguous()), _aligned16(idx.contiguous()), b.contiguous()
    nnz, code, is64 = int(idx.numel()), A.wcode(w), int(ptr_.dtype == torch.int64)
    ws = A.workspace(fn('be_solve_workspace_bytes')(n, code))
    wsp, wsn, st = A.ptr(ws), ws.numel(), A.stream_ptr()
    mat = (A.ptr(w), code, A.ptr(idx), A.ptr(ptr_), is64, n, nnz)

    def state():
        return ws[:_STATE.itemsize].cpu().numpy().view(_STATE)[0]

    def residual(x):
        call('be_solve_residual', *mat, A.ptr(b), A.ptr(x), wsp, wsn, st)
        return state()

    info = {'iterations': 0, 'residual': 0.0, 'restarts': 0, 'converged': True}
    call('be_solve_setup', *mat, wsp, wsn, st)
    s = residual(None)
    bb = float(s['rr'])
    if bb == 0.0:                                        # b == 0: the norm was the only pass
        return torch.zeros(n, dtype=w.dtype, device=dev), info
    thr2 = float(rtol) * float(rtol) * bb
    if not np.isfinite(bb):
        info.update(converged=False, residual=float('nan'))
        return torch.zeros(n, dtype=w.dtype, device=dev), info
    restarts = 0
    if not int(s['offdiag']):                            # a diagonal matrix: one division per element
        x = torch.empty(n, dtype=w.dtype, device=dev)
        call('be_solve_diagonal', code, n, A.ptr(b), A.ptr(x), wsp, wsn, st)
        s = residual(x)
        ok = float(s['rr']) <= thr2
    else:
        if x0 is None:
            x = torch.zeros(n, dtype=w.dtype, device=dev)
        else:
            x = A.to_device(x0.detach() if isinstance(x0, torch.Tensor) else x0, dtype=w.dtype).clone()
            s = residual(x)
        while True:
            done = int(s['iters'])
            if done >= maxiter:
                s = residual(x)
                ok = float(s['rr']) <= thr2
                break
            call('be_solve_iterate', *mat, A.ptr(x), min(CHUNK, maxiter - done), thr2, wsp, wsn, st)
            s = state()
            status = int(s['status'])
            if status == _RUNNING:
                continue
            s = residual(x)                              # the TRUE residual; it also re-arms the recurrence from r, rh = r
            ok = float(s['rr']) <= thr2
            if ok or status == _BREAKDOWN or restarts == MAX_RESTARTS:
                break
            restarts += 1
    rr = float(s['rr'])
    info.update(iterations=int(s['iters']), residual=float(np.sqrt(rr / bb)) if np.isfinite(rr) else float('nan'),
                restarts=restarts, converged=bool(ok))
    return x, info


def _raise_unless_converged(info, rtol: float, who: str) -> None:
    if not info['converged']:
        raise MathError(f"{who}: BiCGSTAB did not reach |b - A x| <= {rtol:g} |b|: relative residual {info['residual']:.3e} after "
                        f"{info['iterations']} iterations and {info['restarts']} restarts (not converged, or the recurrence "
                        "broke down). The method is iterative with a Jacobi preconditioner: it needs a useful diagonal.")


# ------------------------------------------------------------------------------------------------ the primitive
def _csr_solve_hip(data, indices, indptr, b, *, shape, rtol, maxiter, x0=None):
    """``(x, info)`` on device tensors; a shared weight is expanded."""
    w = data.detach().reshape(-1)
    nse = int(indices.numel())
    if w.numel() == 1 and nse != 1:
        w = w.expand(nse).contiguous()
    return solve_arrays(w, indices, indptr, b.detach(), int(shape[0]), rtol=rtol, maxiter=maxiter, x0=x0)


csr_solve_p = OpKernel('csr_solve')
csr_solve_p.def_kernel('hip', 'gpu', _csr_solve_hip, asdefault=True)
csr_solve_p.def_tags('csr', 'float', 'solve')


def csr_solve_p_call(data, indices, indptr, b, *, shape, rtol=None, maxiter=1000, x0=None, backend=None):
    """Validate, then dispatch.  Returns the 1-list ``[(x, info)]``."""
    assert indptr.ndim == 1, "Indptr must be 1D."
    assert indices.ndim == 1, "Indices must be 1D."
    check_operands(_torch_dtype(data), shape, b)
    if int(maxiter) < 1:
        raise ValueError(f"maxiter must be at least 1, got {maxiter}.")
    if x0 is not None and tuple(x0.shape) != tuple(b.shape):
        raise ValueError(f"x0 must have b's shape {tuple(b.shape)}, got {tuple(x0.shape)}.")
    rtol = default_rtol(_torch_dtype(data)) if rtol is None else float(rtol)
    if not rtol > 0.0:
        raise ValueError(f"rtol must be positive, got {rtol}.")
    return [csr_solve_p(data, indices, indptr, b, shape=shape, rtol=rtol, maxiter=int(maxiter), x0=x0, backend=backend)]


csr_solve_p.def_call(csr_solve_p_call)


def _solve_recorded(w, idx, ptr_, b, n: int, *, rtol, maxiter, x0, return_info: bool, who: str, backend=None):
    """The solve on device arrays, recorded for ``torch.autograd`` when ``w`` or ``b`` requires grad."""
    from . import _autograd as _ag
    rtol = default_rtol(w.dtype) if rtol is None else float(rtol)

    def run():
        return csr_solve_p_call(w, idx, ptr_, b, shape=(n, n), rtol=rtol, maxiter=maxiter, x0=x0, backend=backend)[0]

    if _ag.needed(w, b):
        x, info = _ag.solve(run, w, b, idx, ptr_, n, rtol=rtol, maxiter=maxiter, who=who)
    else:
        x, info = run()
    if return_info:
        return x, info
    _raise_unless_converged(info, rtol, who)
    return x


def _rhs(b, dtype):
    """``b`` on the device in the matrix dtype; a tensor keeps its autograd history."""
    if isinstance(b, torch.Tensor):
        return b.to(device=A.device(), dtype=dtype).contiguous()
    return A.to_device(b, dtype=dtype)


def csr_solve(data, indices, indptr, b, tol=1e-6, reorder=1, *, shape=None, rtol=None, maxiter=1000, x0=None,
              return_info=False, backend=None):
    """Solve ``A x = b`` for the CSR matrix ``(data, indices, indptr)`` (reference ``csr_solve``, ``brainevent/_csr/spsolve.py``).

    The method here is ITERATIVE (Jacobi-preconditioned BiCGSTAB, see the module docstring): ``tol`` and ``reorder`` are accepted
    and unused.  ``shape`` defaults to the square shape ``indptr`` implies.  ``b`` is 1-D of length ``shape[0]`` and is converted
    to ``data``'s dtype (f32 / f64), which the result has; a shared weight (``data`` of size 1) is expanded; ``indptr`` int32 or
    int64; entries of a row in any order, duplicates add.  On return ``|b - A x|_2 <= rtol |b|_2`` (``rtol=None``: ``1e-5`` for
    f32, ``1e-10`` for f64), else :class:`MathError` with the residual reached and the iteration count.  ``x0`` is a warm start
    (not differentiated; unused for a matrix without off-diagonal entries, which is solved by one division).  ``return_info=True`` returns ``(x, {'iterations', 'residual', 'restarts', 'converged'})`` and raises
    nothing for non-convergence.  numpy in gives numpy out."""
    del tol, reorder
    data_a, indices_a, indptr_a, b_a = _arr(data), _arr(indices), _arr(indptr), _arr(b)
    assert indptr_a.ndim == 1, "Indptr must be 1D."
    n = int(indptr_a.shape[0]) - 1
    shape = (n, n) if shape is None else tuple(int(s) for s in shape)
    check_operands(_torch_dtype(data_a), shape, b_a)
    assert shape[0] == n, "indptr must have shape[0] + 1 entries."
    as_np = A.wants_numpy(data, indices, indptr, b)
    from ._misc import _as_indptr, _as_int32_indices, _check_compressed_structure
    idx = _as_int32_indices(A.to_device(indices_a), n, 'csr_solve')
    ptr_ = A.to_device(indptr_a)
    if ptr_.dtype not in (torch.int32, torch.int64):
        ptr_ = _as_indptr(ptr_, idx.shape[0], 'auto', 'csr_solve')
    _check_compressed_structure(idx, ptr_, shape, format='csr', check_values=True)
    w = data_a if isinstance(data_a, torch.Tensor) and data_a.device == A.device() else A.to_device(data_a)
    if w.ndim == 0:
        w = w.reshape(1)
    out = _solve_recorded(w, idx, ptr_, _rhs(b_a, w.dtype), n, rtol=rtol, maxiter=maxiter, x0=None if x0 is None else _arr(x0),
                          return_info=return_info, who='csr_solve', backend=backend)
    if return_info:
        return A.to_result(out[0], as_np), out[1]
    return A.to_result(out, as_np)


# ------------------------------------------------------------------------------------------------ containers
def container_solve(M, b, *, rtol=None, maxiter=1000, x0=None, return_info=False):
    """``M.solve(b)`` of CSR / CSC.  CSC goes through ``M.tocsr()`` (device conversion): the data gather of the conversion is a
    torch index, so gradients reach ``M.data`` in its own order."""
    b_a = _arr(b)
    check_operands(M.data.dtype, M.shape, b_a)
    who = f'{type(M).__name__}.solve'
    R = M.tocsr()
    as_np = M._numpy_result and A.wants_numpy(b)
    out = _solve_recorded(R.data, R.indices, R.indptr, _rhs(b_a, R.data.dtype), int(M.shape[0]), rtol=rtol, maxiter=maxiter,
                          x0=None if x0 is None else _arr(x0), return_info=return_info, who=who, backend=M.backend)
    if return_info:
        return A.to_result(out[0], as_np), out[1]
    return A.to_result(out, as_np)


def dense_solve(M, b, return_info=False):
    """``Dense.solve``: ``torch.linalg.solve`` with the reference's two assertions (``_dense/main.py:408-424``).  The info dict
    of ``return_info=True`` carries the measured relative residual of the direct solve."""
    b_a = _arr(b)
    assert M.shape[0] == M.shape[1], "Dense.solve requires a square matrix."
    assert M.shape[0] == b_a.shape[0], "The number of rows in the matrix must match the size of the right-hand side b."
    rhs = _rhs(b_a, M.data.dtype)
    x = torch.linalg.solve(M.data, rhs)
    out = A.to_result(x, M._numpy_result and A.wants_numpy(b))
    if not return_info:
        return out
    with torch.no_grad():
        bn = float(torch.linalg.vector_norm(rhs))
        res = float(torch.linalg.vector_norm(rhs - M.data @ x)) / bn if bn > 0.0 else 0.0
    return out, {'iterations': 0, 'residual': res, 'restarts': 0, 'converged': bool(np.isfinite(res))}
