"""Cost of reading rows out of a stored matrix (``csr[rows]``, ``be_slice.hip``) on the MI355X against the write floor of a
dense result and against the torch route a user had before it; prints one JSON line (and writes it to ``--out``).

Workload: the headline structure, 1M x 1M at 2000 entries per row (2e9 entries, f32 per-entry weights), built on the device as
``bench.py`` builds it; ``--select`` random rows (default 16 and 1024) are read.

Candidates per selection, alternated in one process, every timing a window of at least ``--min-seconds`` of back-to-back calls
between two device events, ``--repeats`` windows each; reported as the median ms per call and the spread (max - min):
  lib          ``csr[rows]``: the selector's bounds check (two scalars read back from the device), allocation of the result,
               ``be_slice_rows``
  lib_op       ``be.csr_slice_rows(...)`` on the same arrays: no bounds check, no read-back
  zero         ``out.zero_()`` on a tensor of the result's shape: the write floor of any dense result
  torch        ``torch.zeros(n_sel, n_cols).index_put_((k_of_entry, cols), vals, accumulate=True)`` with the gathers of the
               selected rows' entries included (the row starts come from ``indptr``; rows have one length here, so the entry
               list is an ``arange`` broadcast — a ragged matrix would need a ``repeat_interleave`` on top)
  lib_bwd      ``torch.autograd.grad`` of ``csr[rows]`` with respect to ``data`` for a given output gradient (``be_slice_rows_grad``:
               a fill of the 2e9-entry gradient and the selected rows' sums)
  torch_bwd    the same through torch's autograd of the ``index_put_`` route (a dense 2e9-entry gradient as well)
Before timing, the library's rows are compared with the torch route's at full size: equal bits where a row has no duplicate
column; rows with duplicates may differ in the last bit (torch's ``index_put_`` adds with float atomics in no fixed order), so
the check there is a tolerance of one f32 ulp of the sum of magnitudes, and it is reported, not asserted on bits.

    python tools/exp_slice_rows.py [--rows 1000000] [--conn 2000] [--select 16 1024] [--min-seconds 0.3] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--conn', type=int, default=2000)
    ap.add_argument('--select', type=int, nargs='+', default=[16, 1024])
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda')
    gen = torch.Generator(device=dev).manual_seed(0)
    n, conn = a.rows, a.conn
    nnz = n * conn
    assert nnz < 2**31, "this script keeps indptr int32, as the headline matrix has it"
    indptr = torch.arange(n + 1, dtype=torch.int32, device=dev) * conn
    indices = torch.randint(0, n, (nnz,), dtype=torch.int32, device=dev, generator=gen)
    w = (torch.rand(nnz, device=dev, generator=gen) + 0.5).requires_grad_()
    csr = be.CSR((w, indices, indptr), shape=(n, n), check_structure=False)
    w_plain = w.detach()
    lane = torch.arange(conn, device=dev)

    def torch_route(rows):
        entries = (indptr[rows].long()[:, None] + lane[None, :]).reshape(-1)
        k_of_entry = torch.repeat_interleave(torch.arange(rows.numel(), device=dev), conn)
        return torch.zeros(rows.numel(), n, device=dev).index_put_((k_of_entry, indices[entries].long()), w[entries], accumulate=True)

    res = {'tool': 'exp_slice_rows', 'shape': [n, n], 'nnz': nnz, 'dtype': 'f32', 'min_seconds': a.min_seconds, 'repeats': a.repeats,
           'tile_cols': int(be._lib.fn('be_slice_rows_tile_cols')(0)), 'selections': {}}
    for n_sel in a.select:
        rows = torch.randint(0, n, (n_sel,), device=dev, generator=gen)
        with torch.no_grad():
            mine, theirs = csr[rows], torch_route(rows)
        diff = (mine - theirs).abs()
        same = {'equal_elements': int((mine == theirs).sum()), 'elements': mine.numel(), 'max_abs_diff': float(diff.max()),
                'within_one_ulp_of_magnitudes': bool((diff <= 2.0 ** -23 * theirs.abs().clamp_min(1.0)).all())}
        assert same['within_one_ulp_of_magnitudes'], same
        out = torch.empty(n_sel, n, device=dev)
        g = torch.rand(n_sel, n, device=dev, generator=gen)
        del mine, theirs, diff
        lib_out, torch_out = csr[rows], torch_route(rows)          # (the graphs the two backward candidates replay)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run
        cands = {
            'lib': no_grad(lambda: csr[rows]),
            'lib_op': lambda: be.csr_slice_rows(w_plain, indices, indptr, rows, shape=(n, n)),
            'zero': lambda: out.zero_(),
            'torch': no_grad(lambda: torch_route(rows)),
            'lib_bwd': lambda: torch.autograd.grad(lib_out, w, g, retain_graph=True),
            'torch_bwd': lambda: torch.autograd.grad(torch_out, w, g, retain_graph=True),
        }
        calls = {}
        for name, fn in cands.items():          # warm-up, and the calls that fill a window
            fn()
            torch.cuda.synchronize()
            one = window_ms(fn, 3)
            calls[name] = max(3, int(a.min_seconds * 1e3 / one) + 1)
        runs = {name: [] for name in cands}
        for _ in range(a.repeats):
            for name, fn in cands.items():
                runs[name].append(window_ms(fn, calls[name]))
        med = {k: statistics.median(v) for k, v in runs.items()}
        res['selections'][str(n_sel)] = {
            'against_torch_route': same, 'calls_per_window': calls,
            'median_ms': {k: round(v, 4) for k, v in med.items()},
            'spread_ms': {k: round(max(v) - min(v), 4) for k, v in runs.items()},
            'result_GB': round(n_sel * n * 4 / 1e9, 3),
            'lib_over_zero': round(med['lib'] / med['zero'], 3), 'lib_over_torch': round(med['lib'] / med['torch'], 3),
            'lib_op_over_zero': round(med['lib_op'] / med['zero'], 3), 'lib_op_over_torch': round(med['lib_op'] / med['torch'], 3),
            'lib_bwd_over_torch_bwd': round(med['lib_bwd'] / med['torch_bwd'], 3),
        }
        del out, g, lib_out, torch_out, cands
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
