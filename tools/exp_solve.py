"""Timings of ``CSR.solve`` (csrc/be_solve.hip) against the same recurrence composed from what the library had
before it.

Two f32 systems of ``--n`` unknowns (default 1M): a random matrix with ``--conn`` (default 8) off-diagonal entries per row,
dominant by row and by column with a factor two, and the tridiagonal passive cable of examples/cable_implicit.py
(``I - dt L``, ``--alpha`` = dt g / (c dx^2), default 2).  Per system, medians of ``--reps`` repetitions timed with HIP
events, the two contenders taking turns inside one loop:

* ``fused``: ``M.solve(b, return_info=True)`` to the default ``rtol`` — whole-solve time, iterations, time per iteration (the
  whole solve over its iterations, and ``*_steady``: 128 against 64 iterations at a tolerance nobody reaches, which cancels
  the setup and the residual passes; ``null`` where the recurrence broke down on exact zeros before 128 iterations);
* ``composition``: the same right-preconditioned BiCGSTAB with ``be.csrmv`` for the two products, ``torch`` for the vector
  updates and ``torch.dot`` for the sums, reading its convergence test back every ``_solve.CHUNK`` iterations as the fused
  driver does.  It can therefore stop only at a multiple of the chunk and runs more iterations than the fused solve, which
  stops inside a chunk: that is this composition's choice, not a cost of its building blocks, so compare the two by the
  time per iteration (``*_steady``), not by the whole-solve times.

Also recorded: the per-iteration HBM floor — two matrix streams of ``nnz * 8`` B plus the vector traffic of the five kernels
(27 words per unknown: k_solve_p 6, each matrix pass 3 + the row pointer, k_solve_s 5, k_solve_x 8) — as a time at the
``out.copy_()`` bandwidth measured in the same run, and as a fraction of the fused time per iteration.  Prints one JSON line
and, with ``--out``, writes it.

    python tools/exp_solve.py [--n 1000000] [--conn 8] [--reps 5] [--out profiles/solve_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd import _solve  # noqa: E402
from exp_float_autograd import timed_alternating  # noqa: E402


def random_dominant(n, conn, dev, gen):
    """CSR arrays of a matrix with ``conn`` random off-diagonal entries per row and a diagonal of mixed sign twice as large as
    the larger of its row's and its column's absolute off-diagonal sum."""
    rows = torch.arange(n, device=dev).repeat_interleave(conn)
    cols = (rows + 1 + torch.randint(0, n - 1, (n * conn,), device=dev, generator=gen)) % n          # never the diagonal
    vals = (torch.rand(n * conn, device=dev, generator=gen) * 0.9 + 0.1) * (torch.randint(0, 2, (n * conn,), device=dev,
                                                                                          generator=gen) * 2 - 1)
    rs = torch.zeros(n, device=dev).index_add_(0, rows, vals.abs())
    cs = torch.zeros(n, device=dev).index_add_(0, cols, vals.abs())
    diag = (2.02 * torch.maximum(rs, cs) + 0.5) * (torch.randint(0, 2, (n,), device=dev, generator=gen) * 2 - 1)
    idx = torch.cat([torch.arange(n, device=dev).reshape(n, 1), cols.reshape(n, conn)], dim=1)
    w = torch.cat([diag.reshape(n, 1), vals.reshape(n, conn)], dim=1)
    order = torch.argsort(idx, dim=1)
    indptr = torch.arange(n + 1, device=dev, dtype=torch.int32) * (conn + 1)
    return (torch.gather(w, 1, order).reshape(-1).float().contiguous(), torch.gather(idx, 1, order).reshape(-1).to(torch.int32),
            indptr)


def cable(n, alpha, dev):
    """``I - dt L`` of a passive cable with sealed ends as ``diag_add`` builds it (examples/cable_implicit.py)."""
    i = torch.arange(n, device=dev)
    rows = torch.cat([i[1:], i[:-1]])
    cols = torch.cat([i[:-1], i[1:]])
    order = torch.argsort(rows * n + cols)
    counts = torch.bincount(rows, minlength=n)
    indptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    indptr[1:] = torch.cumsum(counts, 0)
    off = be.CSR((torch.full((2 * n - 2,), -alpha, device=dev), cols[order].to(torch.int32), indptr), shape=(n, n))
    M = off.diag_add(1.0 + alpha * counts.float())
    return M.data, M.indices, M.indptr


def composed_solve(w, idx, ptr, b, dinv, rtol, maxiter, chunk):
    """The recurrence of csrc/be_solve.hip on the parent's building blocks; returns ``(x, iterations, converged)``."""
    n = b.numel()
    kw = dict(shape=(n, n), transpose=False)
    x = torch.zeros_like(b)
    r = b.clone()
    rh = r.clone()
    thr2 = rtol * rtol * torch.dot(b, b)
    rho_old = alpha = omega = torch.ones((), device=b.device)
    p = v = torch.zeros_like(b)
    rho = torch.dot(rh, r)
    its = 0
    while its < maxiter:
        for _ in range(min(chunk, maxiter - its)):
            beta = (rho / rho_old) * (alpha / omega) if its else torch.zeros((), device=b.device)
            p = r + beta * (p - omega * v)
            y = p * dinv
            v = be.csrmv(w, idx, ptr, y, **kw)
            alpha = rho / torch.dot(rh, v)
            s = r - alpha * v
            z = s * dinv
            t = be.csrmv(w, idx, ptr, z, **kw)
            omega = torch.dot(t, s) / torch.dot(t, t)
            x = x + alpha * y + omega * z
            r = s - omega * t
            rho_old, rho = rho, torch.dot(rh, r)
            its += 1
        if bool(torch.dot(r, r) <= thr2):
            return x, its, True
    return x, its, False


def copy_bandwidth(dev, reps):
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev).zero_()
    out = torch.empty_like(src)
    ms, = timed_alternating([lambda: out.copy_(src)], reps)
    return 2 * src.numel() / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--conn', type=int, default=8)
    ap.add_argument('--alpha', type=float, default=2.0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    n = args.n
    rtol = _solve.default_rtol(torch.float32)
    bw = copy_bandwidth(dev, args.reps)
    line = {'device': torch.cuda.get_device_name(0), 'n': n, 'dtype': 'f32', 'rtol': rtol, 'reps': args.reps, 'chunk': _solve.CHUNK,
            'copy_GBps': round(bw / 1e9, 1), 'cases': []}
    for name, (w, idx, ptr) in (('random', random_dominant(n, args.conn, dev, gen)), ('cable', cable(n, args.alpha, dev))):
        M = be.CSR((w, idx, ptr), shape=(n, n))
        b = torch.randn(n, device=dev, generator=gen)
        rows = torch.arange(n, device=dev).repeat_interleave((ptr[1:] - ptr[:-1]).long())
        d = torch.zeros(n, device=dev).index_add_(0, rows, torch.where(rows == idx, w, torch.zeros_like(w)))
        dinv = 1.0 / d
        x, info = M.solve(b, return_info=True)
        xc, its_c, ok_c = composed_solve(w, idx, ptr, b, dinv, rtol, 1000, _solve.CHUNK)
        res = lambda v: float(torch.linalg.vector_norm(b - be.csrmv(w, idx, ptr, v, shape=(n, n))) / torch.linalg.vector_norm(b))
        fused_ms, comp_ms = timed_alternating([lambda: M.solve(b, return_info=True),
                                               lambda: composed_solve(w, idx, ptr, b, dinv, rtol, 1000, _solve.CHUNK)], args.reps)
        nnz = int(idx.numel())
        floor_bytes = 2 * nnz * 8 + 27 * n * 4
        floor_us = floor_bytes / bw * 1e6
        # the time of an iteration alone: 128 against 64 iterations at a tolerance nobody reaches (setup, |b| and the true
        # residual cancel; the chunk read-backs stay in).  The iteration counts are recorded: a breakdown would end a run early.
        tiny = 1e-30
        long_runs = [lambda k=k: M.solve(b, rtol=tiny, maxiter=k, return_info=True) for k in (64, 128)]
        long_runs += [lambda k=k: composed_solve(w, idx, ptr, b, dinv, 0.0, k, _solve.CHUNK) for k in (64, 128)]
        f64, f128, c64, c128 = timed_alternating(long_runs, args.reps)
        steady_its = [M.solve(b, rtol=tiny, maxiter=k, return_info=True)[1]['iterations'] for k in (64, 128)]
        steady = steady_its == [64, 128]          # (a system solved to the last bit breaks down on exact zeros before that)
        per_it = (f128 - f64) * 1e3 / 64 if steady else fused_ms * 1e3 / max(info['iterations'], 1)
        line['cases'].append({
            'steady_iterations': steady_its, 'fused_us_per_iteration_steady': round(per_it, 2) if steady else None,
            'composition_us_per_iteration_steady': round((c128 - c64) * 1e3 / 64, 2),
            'matrix': name, 'nnz': nnz, 'fused_ms': fused_ms, 'fused_iterations': info['iterations'], 'fused_restarts': info['restarts'],
            'fused_converged': info['converged'], 'fused_residual': res(x), 'fused_us_per_iteration': round(fused_ms * 1e3 / max(info['iterations'], 1), 2),
            'composition_ms': comp_ms, 'composition_iterations': its_c, 'composition_converged': ok_c, 'composition_residual': res(xc),
            'composition_us_per_iteration': round(comp_ms * 1e3 / max(its_c, 1), 2),
            'hbm_floor_bytes_per_iteration': floor_bytes, 'hbm_floor_us_at_copy_bandwidth': round(floor_us, 2),
            'floor_fraction_of_fused_iteration': round(floor_us / per_it, 3)})
        del M, x, xc
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
