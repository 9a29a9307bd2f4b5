"""A passive cable of N compartments stepped by implicit Euler: ``(I - dt L) v' = v + dt * i_inj``.

``L`` is the cable operator with sealed ends — axial coupling ``g (v[i-1] - 2 v[i] + v[i+1])`` and a leak ``-g_leak v[i]`` — stored
as a CSR matrix of its off-diagonal entries alone; the step matrix is built from it with ``(-dt * L_off).diag_add(...)`` and
advanced with ``solve`` (Jacobi-preconditioned BiCGSTAB on the device, ``brainevent_amd._solve``), warm-started from the previous
voltage.  Current is injected into the first compartment.  Prints the largest deviation from the dense solution
(``torch.linalg.solve`` on the same matrix) over the run.

    python examples/cable_implicit.py [--n 200] [--steps 50] [--dt 0.1] [--dtype f64]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


def step_matrix(n, dt, g, g_leak, dtype, dev):
    i = torch.arange(n, device=dev)
    rows, cols = torch.cat([i[1:], i[:-1]]), torch.cat([i[:-1], i[1:]])             # (i, i - 1) and (i, i + 1)
    order = torch.argsort(rows * n + cols)
    neighbours = torch.bincount(rows, minlength=n)
    indptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    indptr[1:] = torch.cumsum(neighbours, 0)
    l_off = be.CSR((torch.full((2 * n - 2,), g, dtype=dtype, device=dev), cols[order].to(torch.int32), indptr), shape=(n, n))
    return (l_off * (-dt)).diag_add(1.0 + dt * (g * neighbours.to(dtype) + g_leak))   # I - dt L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=200)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--dt', type=float, default=0.1)
    ap.add_argument('--g', type=float, default=20.0, help='axial conductance / (capacitance dx^2)')
    ap.add_argument('--g-leak', type=float, default=0.1)
    ap.add_argument('--dtype', choices=('f32', 'f64'), default='f64')
    args = ap.parse_args()
    dev = torch.device('cuda')
    dtype = torch.float32 if args.dtype == 'f32' else torch.float64
    A = step_matrix(args.n, args.dt, args.g, args.g_leak, dtype, dev)
    dense = torch.as_tensor(A.todense(), device=dev)
    inj = torch.zeros(args.n, dtype=dtype, device=dev)
    inj[0] = 1.0
    v = torch.zeros(args.n, dtype=dtype, device=dev)
    v_dense = v.clone()
    worst = iterations = 0
    for _ in range(args.steps):
        v, info = A.solve(v + args.dt * inj, x0=v, return_info=True)
        v_dense = torch.linalg.solve(dense, v_dense + args.dt * inj)
        worst = max(worst, float((v - v_dense).abs().max()))
        iterations += info['iterations']
    print(f"{args.n} compartments, {args.steps} implicit steps of dt={args.dt} ({args.dtype}): v[0]={float(v[0]):.6f}, "
          f"{iterations / args.steps:.1f} BiCGSTAB iterations per step, max |v - v_dense| = {worst:.3e}")


if __name__ == '__main__':
    main()
