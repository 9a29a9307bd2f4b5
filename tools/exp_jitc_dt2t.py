"""Cost of the JIT-connectivity per-synapse product (``JITCNormalR(corder=True).dt2t`` / ``.dt2t_transposed``, the fused route:
count walk, scan, one sorted fill that writes the products) on the MI355X against what a user had before it and against a
plain copy; prints one JSON line (and writes it to ``--out``).

Workload: 1M x 1M at prob 2e-3 (2e9 entries, f32 — the size of the stored-matrix line, ``tools/exp_dt2t.py``), both ``y`` sides.
Every candidate is timed call by call between two device events after a warm-up call; reported: the median over ``--calls``
calls, the minimum and the maximum.
  fused_cached_{row,col}     (a) ``M.dt2t(y, out=out)`` / ``M.dt2t_transposed`` with the row offsets cached on the object
  fused_counting_{row,col}   (b) the same with the cache dropped before every call: count walk + scan + fill
  stored_{row,col}           (c) what the parent commit offers: ``M.materialize('mv')`` (entries of a row in unspecified order),
                             a device sort of ``row * n + column``, the weights moved along, then ``be.csrmv_dt2t``
  copy                       ``out.copy_(x)`` on ``nnz`` f32: 8 bytes per entry and nothing else — the write-bound floor
(c) uses nothing this change adds: ``--only-stored`` runs it alone (the script as it runs at the parent commit).  Before
timing, (a) and (c) are compared bit for bit at full size.  ``decision``: the fused route stays the default of its orientation
only if (a) and (b) are each no slower than (c).

    python tools/exp_jitc_dt2t.py [--n 1000000] [--prob 2e-3] [--calls 20] [--only-stored] [--out profiles/jitc_dt2t_line.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


def timed(fn, calls):
    fn()                                    # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3), 'calls': calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--prob', type=float, default=2e-3)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--only-stored', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda')
    n = a.n
    M = be.JITCNormalR((torch.tensor(0.2), torch.tensor(1.3), a.prob, a.seed), shape=(n, n), corder=True)
    y = (torch.randint(0, 2, (n,), device=dev) * 2 - 1).float() * 0.75
    nnz = int(M.owner_counts('mv').to(torch.int64).sum().item())
    assert nnz < 2**31, "the stored baseline sorts its entries in one device sort"
    out = torch.empty(nnz, device=dev)
    res = {'tool': 'exp_jitc_dt2t', 'matrix': 'JITCNormalR(corder=True)', 'shape': [n, n], 'prob': a.prob, 'nnz': nnz, 'dtype': 'f32'}

    def put(name, value):                   # (kept on disk as it grows: a run that is cut short leaves what it measured)
        res[name] = value
        print(f'{name}: {value}', file=sys.stderr, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps(res) + '\n')

    def stored(by_row, dst):
        S = M.materialize('mv')
        ptr = S.indptr.to(torch.int64)
        key = torch.repeat_interleave(torch.arange(n, device=dev), ptr[1:] - ptr[:-1]) * n + S.indices
        key, order = torch.sort(key)
        w = S.data[order]
        del order
        cols = (key % n).to(torch.int32)
        del key
        return be.csrmv_dt2t(y, w, cols, S.indptr, shape=(n, n), transpose=not by_row, out=dst)

    fused = not a.only_stored and hasattr(M, 'dt2t') and type(M).dt2t is not be.DataRepresentation.dt2t
    if fused:
        same = {}
        ref = torch.empty(nnz, device=dev)
        for by_row in (True, False):
            (M.dt2t if by_row else M.dt2t_transposed)(y, out=out)
            try:
                stored(by_row, ref)
                same['row' if by_row else 'col'] = bool(torch.equal(out, ref))
            except RuntimeError as e:           # (a device sort of this size may not fit)
                same['row' if by_row else 'col'] = f'stored baseline failed: {str(e)[:200]}'
        del ref
        torch.cuda.empty_cache()
        put('fused_equals_stored_bitwise', same)
        key = [k for k in M.buffers if str(k).startswith('materialized_')]

        def counting(f):
            for k in key:
                M.buffers.pop(k, None)
            f(y, out=out)
        put('fused_cached_row', timed(lambda: M.dt2t(y, out=out), a.calls))
        put('fused_cached_col', timed(lambda: M.dt2t_transposed(y, out=out), a.calls))
        put('fused_counting_row', timed(lambda: counting(M.dt2t), a.calls))
        put('fused_counting_col', timed(lambda: counting(M.dt2t_transposed), a.calls))
    x = torch.rand(nnz, device=dev)
    put('copy', timed(lambda: out.copy_(x), a.calls))
    del x
    torch.cuda.empty_cache()
    try:
        put('stored_row', timed(lambda: stored(True, out), a.calls))
        put('stored_col', timed(lambda: stored(False, out), a.calls))
    except RuntimeError as e:
        put('stored_error', str(e)[:300])
    if fused and 'stored_row' in res:
        ok = all(res[f'fused_{k}_{s}']['median_ms'] <= res[f'stored_{s}']['median_ms'] for k in ('cached', 'counting') for s in ('row', 'col'))
        put('decision', 'fused stays the default' if ok else 'fused is slower than the stored route: route to the composed path')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
