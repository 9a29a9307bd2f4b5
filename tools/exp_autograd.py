"""Forward and backward timings of the differentiable event products (DESIGN.md section "Gradients").

CSR ``s @ A`` and ``A @ s`` with ``--n`` x ``--n`` neurons and ``--conn`` synapses per row (default 1M x 1M, 1000 per row:
1e9 synapses), ``--rate`` firing, batch ``B`` in {1, 32}, f32 weights that require grad; and ``Dense`` 8192^2 with B = 32.
Backward = ``torch.autograd.grad`` of the output against the weights (weight gradient only: int32 spikes do not require
grad).  Prints one JSON line per case with the median of ``--reps`` timed repetitions (HIP events) and the write floor of the
weight gradient (``nse * 4`` bytes at 6.2 TB/s).

    python tools/exp_autograd.py [--n 1000000] [--conn 1000] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402

HBM_BPS = 6.2e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--conn', type=int, default=1000)
    ap.add_argument('--rate', type=float, default=0.01)
    ap.add_argument('--dense', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n, c = args.n, args.conn
    nse = n * c
    indptr = torch.arange(n + 1, dtype=torch.int64 if nse >= 2 ** 31 else torch.int32, device=dev) * c
    indices = torch.randint(0, n, (nse,), dtype=torch.int32, device=dev, generator=g)
    w = torch.rand(nse, device=dev, generator=g).requires_grad_()
    floor_ms = nse * 4 / HBM_BPS * 1e3
    for transpose in (True, False):
        for B in (1, 32):
            s = torch.rand((n,) if B == 1 else (n, B), device=dev, generator=g) < args.rate
            f = be.binary_csrmv if B == 1 else be.binary_csrmm

            def fwd():
                return f(w, indices, indptr, s, shape=(n, n), transpose=transpose)
            y = fwd()
            gy = torch.randn(y.shape, device=dev, generator=g)
            with torch.no_grad():
                t_fwd = timed(fwd, args.reps)
            t_fwd_grad = timed(fwd, args.reps)
            t_bwd = timed(lambda: torch.autograd.grad(y, w, gy, retain_graph=True), args.reps)
            print(json.dumps({'case': f"csr {'s@A' if transpose else 'A@s'} B={B}", 'nse': nse, 'rate': args.rate,
                              'fwd_ms': round(t_fwd, 3), 'fwd_with_grad_ms': round(t_fwd_grad, 3), 'bwd_ms': round(t_bwd, 3),
                              'write_floor_ms': round(floor_ms, 3)}), flush=True)
            del y, gy, s
    del w, indices, indptr
    torch.cuda.empty_cache()
    R = args.dense
    W = torch.randn((R, R), device=dev, generator=g).requires_grad_()
    for transpose in (True, False):
        s = torch.rand((R, 32), device=dev, generator=g) < args.rate

        def fwd():
            return be.binary_densemm(W, s, transpose=transpose)
        y = fwd()
        gy = torch.randn(y.shape, device=dev, generator=g)
        with torch.no_grad():
            t_fwd = timed(fwd, args.reps)
        t_bwd = timed(lambda: torch.autograd.grad(y, W, gy, retain_graph=True), args.reps)
        print(json.dumps({'case': f"dense {'s@W' if transpose else 'W@s'} {R}^2 B=32", 'fwd_ms': round(t_fwd, 3),
                          'bwd_ms': round(t_bwd, 3), 'write_floor_ms': round(R * R * 4 / HBM_BPS * 1e3, 3)}), flush=True)


if __name__ == '__main__':
    main()
