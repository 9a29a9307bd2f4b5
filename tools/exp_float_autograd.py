"""Timings of the sampled dense-dense product and of the backward pass of the float-operand products.

CSR with ``--n`` x ``--n`` neurons and ``--conn`` synapses per row (default 1M x 1M, 1000 per row: 1e9 synapses), f32,
``nb`` in {1, 32}.  Per ``nb``:

* ``be_sddmm_rows`` over all entries (through ``_sddmm.sddmm_rows``), alternating in the same loop with ``out.zero_()`` of
  ``[nse]`` — the write floor of a per-entry result;
* ``be_sddmm_rows`` over the first ``--chunk`` entries (COO row source), alternating with the torch expression
  ``(P[row_ids] * Q[col_ids]).sum(1)`` over the same entries — a chunk, because the expression materialises two
  ``[entries, nb]`` arrays (256 GB at 1e9 entries and nb = 32);
* the full backward pass (weights and operand) of ``csr @ X`` and ``X @ csr`` (``csrmv`` / ``csrmm``, both ``transpose``).

Every figure is the median of ``--reps`` repetitions timed with HIP events.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_float_autograd.py [--n 1000000] [--conn 1000] [--reps 5] [--out profiles/float_autograd_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd import _sddmm as S  # noqa: E402


def timed_alternating(fns, reps):
    """Median ms of each function, the functions taking turns inside one loop."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [round(sorted(t)[len(t) // 2], 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--conn', type=int, default=1000)
    ap.add_argument('--chunk', type=int, default=1 << 24)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n, c = args.n, args.conn
    nse = n * c
    chunk = min(args.chunk, nse)
    indptr = torch.arange(n + 1, dtype=torch.int64 if nse >= 2 ** 31 else torch.int32, device=dev) * c
    indices = torch.randint(0, n, (nse,), dtype=torch.int32, device=dev, generator=g)
    w = torch.rand(nse, device=dev, generator=g).requires_grad_()
    row_ids = (torch.arange(chunk, dtype=torch.int64, device=dev) // c).to(torch.int32)
    col_ids = indices[:chunk].contiguous()
    out = torch.empty(nse, device=dev)
    line = {'device': torch.cuda.get_device_name(0), 'n': n, 'conn': c, 'nse': nse, 'dtype': 'f32', 'chunk_entries': chunk,
            'reps': args.reps, 'cases': []}
    for nb in (1, 32):
        P = torch.rand((n, nb), device=dev, generator=g)
        Q = torch.rand((n, nb), device=dev, generator=g)
        case = {'nb': nb}
        case['sddmm_ms'], case['zero_floor_ms'] = timed_alternating(
            [lambda: S.sddmm_rows(indices, indptr, -1, None, n, n, P, Q), lambda: out.zero_()], args.reps)
        rl, cl = row_ids.long(), col_ids.long()
        case['sddmm_chunk_ms'], case['torch_expr_chunk_ms'] = timed_alternating(
            [lambda: S.sddmm_rows(col_ids, None, -1, row_ids, n, n, P, Q), lambda: (P[rl] * Q[cl]).sum(1)], args.reps)
        del rl, cl
        for transpose in (False, True):
            X = torch.rand((n,) if nb == 1 else (n, nb), device=dev, generator=g).requires_grad_()
            f = be.csrmv if nb == 1 else be.csrmm
            y = f(w, indices, indptr, X, shape=(n, n), transpose=transpose)
            gy = torch.randn(y.shape, device=dev, generator=g)
            key = 'X@csr' if transpose else 'csr@X'
            case[f'{key}_bwd_ms'], = timed_alternating([lambda: torch.autograd.grad(y, (w, X), gy, retain_graph=True)], args.reps)
            case[f'{key}_bwd_weights_only_ms'], = timed_alternating([lambda: torch.autograd.grad(y, w, gy, retain_graph=True)],
                                                                    args.reps)
            del y, gy, X
        line['cases'].append(case)
        del P, Q
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
