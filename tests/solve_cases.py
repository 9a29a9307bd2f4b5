"""Test matrices, bounds and a CPU reference recurrence for ``solve`` — shared by tests/test_solve_cpu.py (which holds the
generator to its own claim) and tests/test_solve_gpu.py.  numpy only: nothing here needs a device.

The generator's claim: ``A`` is dominant by row AND by column with a factor two,

    sum_{j != i} |a_ij| <= 1/2 |a_ii|     and     sum_{i != j} |a_ij| <= 1/2 |a_jj|,

with diagonals of mixed sign.  Then (Varah 1975) ``|A^-1|_inf <= 1 / min_i(|a_ii| - sum_{j != i} |a_ij|)``, and the same for
``A.T`` with the column sums — which is what turns a residual into an error bound, for the forward solve and for the backward
solve of the gradients.  The dominance is checked on the values AS STORED (after the cast to f32), in f64.

The two bounds of the GPU tests, derived and not tuned (``eps`` the machine epsilon of the dtype, ``len`` the longest row):

    residual:  |b - A x|_2   <= rtol |b|_2 + gamma | |A| |x| |_2,        gamma = (len + 2) eps
    error:     |x - x*|_inf  <= (the same right-hand side) / min_i(|a_ii| - sum_{j != i} |a_ij|)

The first term is the solver's contract on the residual IT computes; the second is the rounding of that residual pass: a row of
``len`` products summed in any order and one subtraction is off by at most ``(len + 1) u (|A| |x|)_i + u |b_i|``, ``u = eps / 2``,
so ``gamma`` leaves a factor two.  The error bound is Varah's bound applied to ``|r|_inf <= |r|_2``."""
import numpy as np

__all__ = ['Case', 'dominant_case', 'block_case', 'dense_of', 'row_gap', 'col_gap', 'residual_bound', 'check_solution',
           'bicgstab_reference']


class Case:
    """CSR arrays (``data`` in the case's dtype, ``indices`` int32, ``indptr``), ``b`` in the dtype, ``n`` and — for the sizes
    that allow it — the dense f64 matrix ``A``."""

    def __init__(self, data, indices, indptr, b, n, name=''):
        self.data, self.indices, self.indptr, self.b, self.n, self.name = data, indices, indptr, b, int(n), name
        self._dense = None

    @property
    def dtype(self):
        return self.data.dtype

    @property
    def longest_row(self) -> int:
        return int(np.diff(self.indptr).max()) if self.n else 0

    @property
    def rows(self):
        return np.repeat(np.arange(self.n), np.diff(self.indptr))

    @property
    def A(self):
        if self._dense is None:
            self._dense = dense_of(self)
        return self._dense

    def matvec(self, x, absolute=False):
        """``A x`` (or ``|A| |x|``) in f64 from the stored entries: duplicates add."""
        w = self.data.astype(np.float64)
        x = np.asarray(x, dtype=np.float64)
        if absolute:
            w, x = np.abs(w), np.abs(x)
        return np.bincount(self.rows, weights=w * x[self.indices], minlength=self.n)

    def with_dtype(self, dtype):
        return Case(self.data.astype(dtype), self.indices, self.indptr, self.b.astype(dtype), self.n, self.name)


def dense_of(case) -> np.ndarray:
    out = np.zeros((case.n, case.n), dtype=np.float64)
    np.add.at(out, (case.rows, case.indices), case.data.astype(np.float64))
    return out


def _off_sums(case):
    """Per row and per column: the absolute sum of the stored entries off the diagonal, and the diagonal (duplicates added)."""
    w = case.data.astype(np.float64)
    r, c = case.rows, case.indices
    off = r != c
    rows = np.bincount(r[off], weights=np.abs(w[off]), minlength=case.n)
    cols = np.bincount(c[off], weights=np.abs(w[off]), minlength=case.n)
    diag = np.bincount(r[~off], weights=w[~off], minlength=case.n)
    return rows, cols, diag


def row_gap(case) -> float:
    rows, _, diag = _off_sums(case)
    return float(np.min(np.abs(diag) - rows))


def col_gap(case) -> float:
    _, cols, diag = _off_sums(case)
    return float(np.min(np.abs(diag) - cols))


def _finish(n, rows, cols, vals, rng, dtype, shuffle, indptr_dtype, name):
    """Add the dominant diagonal to the off-diagonal triplets, order the entries and build the case."""
    vals = vals.astype(dtype).astype(np.float64)                         # the sums below see the values as stored
    rs = np.bincount(rows, weights=np.abs(vals), minlength=n)
    cs = np.bincount(cols, weights=np.abs(vals), minlength=n)
    mag = 2.0 * np.maximum(rs, cs) * (1.0 + 0.01 + 0.5 * rng.random(n)) + 0.5
    diag = mag * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if n > 1:
        diag[0], diag[1] = abs(diag[0]), -abs(diag[1])                   # mixed signs whatever the draw
    r = np.concatenate([rows, np.arange(n)])
    c = np.concatenate([cols, np.arange(n)])
    v = np.concatenate([vals, diag])
    key = rng.random(r.size) if shuffle else c.astype(np.float64)
    order = np.lexsort((key, r))
    r, c, v = r[order], c[order], v[order]
    indptr = np.zeros(n + 1, dtype=indptr_dtype)
    np.cumsum(np.bincount(r, minlength=n), out=indptr[1:])
    b = (rng.standard_normal(n) + 0.25).astype(dtype)
    return Case(v.astype(dtype), c.astype(np.int32), indptr, b, n, name)


def dominant_case(n, counts, seed=0, dtype=np.float32, *, shuffle=False, dup_offdiag=False, dup_diag=False,
                  indptr_dtype=np.int32, name=''):
    """``n x n``, row ``i`` with ``counts[i]`` (a number: every row) off-diagonal entries at distinct random columns, values in
    ``[-1, -0.1] u [0.1, 1]``.  ``shuffle``: entries of a row in random order.  ``dup_offdiag``: every off-diagonal entry stored
    as two halves.  ``dup_diag``: every diagonal stored as two parts."""
    rng = np.random.default_rng(seed)
    counts = np.minimum(np.broadcast_to(np.asarray(counts, dtype=np.int64), (n,)), n - 1)
    rows = np.repeat(np.arange(n), counts)
    cols = np.empty(rows.size, dtype=np.int64)
    at = 0
    for i in range(n):
        k = int(counts[i])
        if k:
            pick = rng.choice(n - 1, size=k, replace=False)
            cols[at:at + k] = pick + (pick >= i)
            at += k
    vals = rng.uniform(0.1, 1.0, rows.size) * np.where(rng.random(rows.size) < 0.5, -1.0, 1.0)
    case = _finish(n, rows, cols, vals, rng, dtype, shuffle, indptr_dtype, name)
    if dup_offdiag or dup_diag:
        r, c = case.rows, case.indices.astype(np.int64)
        on = r == c
        split = (on & dup_diag) | (~on & dup_offdiag)
        w = case.data.astype(np.float64)
        first = np.where(split, (w * 0.375).astype(dtype).astype(np.float64), w)
        second = (w - first)[split]
        r2, c2, v2 = np.concatenate([r, r[split]]), np.concatenate([c, c[split]]), np.concatenate([first, second])
        order = np.lexsort((rng.random(r2.size) if shuffle else c2.astype(np.float64), r2))
        indptr = np.zeros(n + 1, dtype=indptr_dtype)
        np.cumsum(np.bincount(r2, minlength=n), out=indptr[1:])
        case = Case(v2[order].astype(dtype), c2[order].astype(np.int32), indptr, case.b, n, name)
    return case


def block_case(n, block, seed=0, dtype=np.float32, name=''):
    """Block diagonal with dense ``block x block`` blocks (the last one smaller), dominant as above: sizes whose dense matrix
    cannot be formed keep an exact reference, the batched ``numpy.linalg.solve`` of the blocks (:func:`block_solve`)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    base = (i // block) * block
    size = np.minimum(block, n - base)
    rows = np.repeat(i, size - 1)
    first = np.repeat(np.cumsum(size - 1) - (size - 1), size - 1)
    k = np.arange(rows.size) - first                                      # 0 .. size - 2 within the row
    local = rows - np.repeat(base, size - 1)
    cols = np.repeat(base, size - 1) + k + (k >= local)
    vals = rng.uniform(0.1, 1.0, rows.size) * np.where(rng.random(rows.size) < 0.5, -1.0, 1.0)
    return _finish(n, rows, cols, vals, rng, dtype, False, np.int32, name)


def block_solve(case, block, rhs=None) -> np.ndarray:
    """``numpy.linalg.solve`` in f64 on the densified blocks of a :func:`block_case`."""
    n = case.n
    full = (n // block) * block
    rhs = case.b.astype(np.float64) if rhs is None else np.asarray(rhs, dtype=np.float64)
    r, c, w = case.rows, case.indices.astype(np.int64), case.data.astype(np.float64)
    x = np.empty(n, dtype=np.float64)
    if full:
        m = r < full
        blocks = np.zeros((full // block, block, block), dtype=np.float64)
        np.add.at(blocks, (r[m] // block, r[m] % block, c[m] % block), w[m])
        x[:full] = np.linalg.solve(blocks, rhs[:full].reshape(-1, block, 1)).reshape(-1)
    if full < n:
        m = r >= full
        tail = np.zeros((n - full, n - full), dtype=np.float64)
        np.add.at(tail, (r[m] - full, c[m] - full), w[m])
        x[full:] = np.linalg.solve(tail, rhs[full:])
    return x


def residual_bound(case, x, rtol, rhs=None) -> float:
    """``rtol |b|_2 + gamma | |A| |x| |_2`` in f64, ``gamma = (longest row + 2) eps`` (module docstring)."""
    rhs = case.b if rhs is None else rhs
    gamma = (case.longest_row + 2) * float(np.finfo(case.dtype).eps)
    return float(rtol * np.linalg.norm(np.asarray(rhs, dtype=np.float64)) + gamma * np.linalg.norm(case.matvec(x, absolute=True)))


def check_solution(case, x, x_star, rtol, gap=None, rhs=None):
    """The two bounds for a result ``x`` of ``A x = rhs``: returns ``(residual, residual bound, error, error bound)`` and
    asserts both.  ``gap``: ``min_i(|a_ii| - sum_{j != i} |a_ij|)`` (default: the case's own)."""
    rhs = case.b if rhs is None else rhs
    x = np.asarray(x, dtype=np.float64)
    bound = residual_bound(case, x, rtol, rhs)
    res = float(np.linalg.norm(np.asarray(rhs, dtype=np.float64) - case.matvec(x)))
    gap = row_gap(case) if gap is None else gap
    err = float(np.max(np.abs(x - x_star))) if case.n else 0.0
    figures = (res, bound, err, bound / gap)
    print(f'{case.name or "case"} n={case.n} {np.dtype(case.dtype).name}: residual {res:.3e} <= {bound:.3e}, error {err:.3e} <= '
          f'{bound / gap:.3e}')
    assert np.all(np.isfinite(x)), figures
    assert res <= bound, figures
    assert err <= bound / gap, figures
    return figures


def bicgstab_reference(A, b, rtol, maxiter=1000, max_restarts=3):
    """The recurrence of csrc/be_solve.hip in f64 on a dense ``A``: right-preconditioned BiCGSTAB, ``D_ii = a_ii`` (1 where it
    is zero), the half-step exit, the breakdown rules and the restart from the true residual.  Returns ``(x, info)`` with the
    keys of ``solve(..., return_info=True)``."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    d = np.diag(A).copy()
    d[d == 0.0] = 1.0
    dinv = 1.0 / d
    bb = float(b @ b)
    x = np.zeros(n)
    info = {'iterations': 0, 'residual': 0.0, 'restarts': 0, 'converged': True}
    if bb == 0.0:
        return x, info
    thr2 = rtol * rtol * bb
    its = restarts = 0
    ok = False
    with np.errstate(all='ignore'):
        while True:
            r = b - A @ x
            rh = r.copy()
            first, status = True, 0
            rho_old = alpha = omega = 1.0
            p = v = np.zeros(n)
            while status == 0 and its < maxiter:
                rho, rr = float(rh @ r), float(r @ r)
                if rr <= thr2:
                    status = 1
                    break
                beta = 0.0 if first else (rho / rho_old) * (alpha / omega)
                if rho == 0.0 or not np.isfinite(rho) or not np.isfinite(beta):
                    status = 2
                    break
                p = r.copy() if first else r + beta * (p - omega * v)
                y = p * dinv
                v = A @ y
                rv = float(rh @ v)
                alpha = rho / rv if rv != 0.0 else np.inf
                if rv == 0.0 or not np.isfinite(rv) or alpha == 0.0 or not np.isfinite(alpha):
                    status = 2
                    break
                s = r - alpha * v
                if float(s @ s) <= thr2:
                    x = x + alpha * y
                    its += 1
                    status = 1
                    break
                z = s * dinv
                t = A @ z
                tt = float(t @ t)
                omega = float(t @ s) / tt if tt != 0.0 else np.inf
                if tt == 0.0 or not np.isfinite(tt) or omega == 0.0 or not np.isfinite(omega):
                    status = 2
                    break
                x = x + alpha * y + omega * z
                r = s - omega * t
                rho_old, first = rho, False
                its += 1
            true = b - A @ x
            rr = float(true @ true)
            ok = rr <= thr2
            if ok or status != 1 or restarts == max_restarts:
                break
            restarts += 1
    info.update(iterations=its, residual=float(np.sqrt(rr / bb)) if np.isfinite(rr) else float('nan'), restarts=restarts,
                converged=bool(ok))
    return x, info
