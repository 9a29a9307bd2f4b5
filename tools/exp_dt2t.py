"""Cost of the per-synapse products (``csrmv_dt2t`` / ``fcnmv_dt2t``) on the MI355X against what a user had before them and
against a plain copy; prints one JSON line (and writes it to ``--out``).

Workload: the plasticity measurement's matrix, 1M x 1M at 2000 entries per row (2e9 entries, f32), as CSR and as
fixed-number connectivity, plus a skewed CSR of the same entry count (one row holds half of the entries, the rest are
spread evenly) — the by-row kernel finds rows per tile of entries, so its time must not depend on that.

Candidates, alternated in one process, every timing a window of at least ``--min-seconds`` of back-to-back calls between two
device events, ``--repeats`` windows each; reported as the median ms per call and the spread (max - min) of the windows:
  lib_row / lib_col            ``be.csrmv_dt2t`` out of place (``out=`` a second array), by row / by column
  lib_row_inplace / lib_col_inplace                  the same with ``out=w``
  lib_row_skewed               by row on the skewed matrix
  fcn_row / fcn_col            ``be.fcnmv_dt2t``, the same entries as rows of 2000
  torch_row_i64 / torch_row_i32   ``torch.mul(w, y[row_ids], out=out)`` with ``row_ids`` precomputed (8 / 4 more bytes per entry)
  torch_col                    ``torch.mul(w, y[indices.long()], out=out)``
  copy                         ``out.copy_(w)``: the same 8 bytes per entry and nothing else — the ceiling
``y`` holds +-1 so that the in-place candidates can run any number of times.  Before timing, the library's results are
compared with torch's, bit for bit, at full size.  ``accept`` holds the three acceptance checks of the measurement: each
library timing against its torch baseline, the skewed matrix against the uniform one, both within the measured spread, and
the ratio of each library timing to the copy.

    python tools/exp_dt2t.py [--rows 1000000] [--conn 2000] [--min-seconds 0.5] [--repeats 5] [--out FILE]
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
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(0)
    n, conn = a.rows, a.conn
    nnz = n * conn
    assert nnz < 2**31, "this script keeps every indptr int32 so that the candidates compare like with like"
    indptr = torch.arange(n + 1, dtype=torch.int32, device=dev) * conn
    indices = torch.randint(0, n, (nnz,), dtype=torch.int32, device=dev, generator=g)
    w = torch.rand(nnz, device=dev, generator=g) + 0.5
    y = (torch.randint(0, 2, (n,), device=dev, generator=g) * 2 - 1).float()
    out = torch.empty_like(w)
    # the skewed twin: row n/2 holds half of the entries, the others share the rest evenly
    lens = torch.full((n,), (nnz // 2) // (n - 1), dtype=torch.int64, device=dev)
    lens[: (nnz // 2) % (n - 1)] += 1
    lens[n // 2] = 0
    lens[n // 2] = nnz - int(lens.sum())
    skew_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=skew_ptr[1:])
    assert int(skew_ptr[-1]) == nnz
    skew_ptr = skew_ptr.to(torch.int32)
    row_i32 = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), conn)
    row_i64 = row_i32.long()
    shape = (n, n)

    # the same numbers first (bit for bit, at the size that is timed)
    same = {}
    be.csrmv_dt2t(y, w, indices, indptr, shape=shape, out=out)
    same['row'] = bool(torch.equal(out, w * y[row_i64]))
    be.csrmv_dt2t(y, w, indices, indptr, shape=shape, transpose=True, out=out)
    same['col'] = bool(torch.equal(out, w * y[indices.long()]))
    be.fcnmv_dt2t(w.view(n, conn), indices.view(n, conn), y, shape=shape, transpose=False, out=out.view(n, conn))
    same['fcn_row'] = bool(torch.equal(out, w * y[row_i64]))
    be.csrmv_dt2t(y, w, indices, skew_ptr, shape=shape, out=out)
    skew_rows = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    same['row_skewed'] = bool(torch.equal(out, w * y[skew_rows]))
    del skew_rows
    torch.cuda.empty_cache()
    assert all(same.values()), same

    w2, i2, o2 = w.view(n, conn), indices.view(n, conn), out.view(n, conn)
    cands = {
        'lib_row': lambda: be.csrmv_dt2t(y, w, indices, indptr, shape=shape, out=out),
        'lib_col': lambda: be.csrmv_dt2t(y, w, indices, indptr, shape=shape, transpose=True, out=out),
        'lib_row_inplace': lambda: be.csrmv_dt2t(y, w, indices, indptr, shape=shape, out=w),
        'lib_col_inplace': lambda: be.csrmv_dt2t(y, w, indices, indptr, shape=shape, transpose=True, out=w),
        'lib_row_skewed': lambda: be.csrmv_dt2t(y, w, indices, skew_ptr, shape=shape, out=out),
        'fcn_row': lambda: be.fcnmv_dt2t(w2, i2, y, shape=shape, transpose=False, out=o2),
        'fcn_col': lambda: be.fcnmv_dt2t(w2, i2, y, shape=shape, transpose=True, out=o2),
        'torch_row_i64': lambda: torch.mul(w, y[row_i64], out=out),
        'torch_row_i32': lambda: torch.mul(w, y[row_i32], out=out),
        'torch_col': lambda: torch.mul(w, y[indices.long()], out=out),
        'copy': lambda: out.copy_(w),
    }
    try:                                    # (indexing by an int32 tensor: not in every torch)
        cands['torch_row_i32']()
        base_row = 'torch_row_i32'
    except (IndexError, RuntimeError, TypeError):
        del cands['torch_row_i32']
        base_row = 'torch_row_i64'
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
    spread = {k: max(v) - min(v) for k, v in runs.items()}

    def not_slower(x, base):
        return med[x] <= med[base] + max(spread[x], spread[base])

    accept = {
        'lib_row_vs_' + base_row: not_slower('lib_row', base_row),
        'lib_row_inplace_vs_' + base_row: not_slower('lib_row_inplace', base_row),
        'lib_col_vs_torch_col': not_slower('lib_col', 'torch_col'),
        'lib_col_inplace_vs_torch_col': not_slower('lib_col_inplace', 'torch_col'),
        'skewed_within_spread_of_uniform': abs(med['lib_row_skewed'] - med['lib_row']) <= max(spread['lib_row_skewed'], spread['lib_row']),
    }
    res = {
        'tool': 'exp_dt2t', 'shape': [n, n], 'nnz': nnz, 'dtype': 'f32', 'min_seconds': a.min_seconds, 'repeats': a.repeats,
        'same_bits_as_torch': same, 'calls_per_window': calls,
        'median_ms': {k: round(v, 4) for k, v in med.items()},
        'spread_ms': {k: round(v, 4) for k, v in spread.items()},
        'TBps_at_8B_per_entry': {k: round(nnz * 8 / (v * 1e-3) / 1e12, 3) for k, v in med.items()},
        'ratio_to_copy': {k: round(med['copy'] / v, 3) for k, v in med.items() if k != 'copy'},
        'accept': accept,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
