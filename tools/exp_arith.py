"""Cost of container arithmetic on the MI355X: ``csr * D`` (``be_entries_dense_op``) and ``csr.diag_add(d)`` (``be_diag_scan``
/ ``be_diag_move`` / ``be_diag_fill``) against what a user had before them and against a plain copy; prints one JSON line (and
writes it to ``--out``).

Workloads (f32):
  ``csr * D``          65 536 x 65 536 with 2000 entries per row (1.3e8 entries; ``D`` is 17 GB)
    sample_mul         ``(csr * D).data``
    torch_mul          the torch route ``w * D[row_ids, idx]`` (``row_ids`` and ``idx``: int64 ``[nse]``, built once, outside the timing)
    torch_row_ids      the build of ``row_ids`` alone (``repeat_interleave`` over the row lengths)
    copy               ``out.copy_(w)``: 8 bytes per entry and nothing else — the stream floor
  ``csr.diag_add(d)``  1M x 1M with 2000 entries per row (2e9 entries), the diagonal missing in about every row
    diag_first         the first call on a structure: scan, per-row plan, one host read-back, move + fill with the structure
    diag_later         a later call on the cached plan: move + fill of the values
    diag_scan          the scan kernel alone
    diag_copy          ``out.copy_(w)`` at that size
Every candidate is timed call by call between two device events after a warm-up call, the candidates of one workload taking
turns inside one loop; reported: the median over ``--calls`` calls, the minimum and the maximum.  Before timing, ``sample_mul``
is compared with ``torch_mul`` bit for bit at full size.

    python tools/exp_arith.py [--n 65536] [--diag-n 1000000] [--per-row 2000] [--calls 20] [--out profiles/arith_line.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd import _array as A  # noqa: E402
from brainevent_amd import _diag  # noqa: E402
from brainevent_amd._lib import call  # noqa: E402


def timed_in_turns(fns, calls):
    """``{name: fn}`` -> ``{name: stats}``; one warm-up call each, then ``calls`` rounds in which every candidate runs once."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(calls):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
                   'calls': calls} for name, v in ms.items()}


def fixed_rows(n, per_row, dev, seed):
    """CSR arrays of ``n`` rows with ``per_row`` random columns each (unsorted), int32 / int64 by the entry count."""
    g = torch.Generator(device=dev).manual_seed(seed)
    nse = n * per_row
    indices = torch.randint(0, n, (nse,), device=dev, generator=g, dtype=torch.int32)
    indptr = torch.arange(n + 1, device=dev, dtype=torch.int64) * per_row
    if nse <= 2**31 - 1 - n:
        indptr = indptr.to(torch.int32)
    return indices, indptr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--diag-n', type=int, default=1_000_000)
    ap.add_argument('--per-row', type=int, default=2000)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda')
    res = {'tool': 'exp_arith', 'dtype': 'f32', 'per_row': a.per_row}

    def put(name, value):                   # (kept on disk as it grows: a run that is cut short leaves what it measured)
        res[name] = value
        print(f'{name}: {value}', file=sys.stderr, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps(res) + '\n')

    # ---- csr * D
    n, k = a.n, a.per_row
    indices, indptr = fixed_rows(n, k, dev, 1)
    nse = n * k
    w = torch.rand(nse, device=dev) + 0.5
    D = torch.rand((n, n), device=dev) + 0.5
    M = be.CSR((w, indices, indptr), shape=(n, n), check_structure=False)
    put('mul_shape', [n, n])
    put('mul_nse', nse)

    def row_ids_of():
        ptr = indptr.to(torch.int64)
        return torch.repeat_interleave(torch.arange(n, device=dev), ptr[1:] - ptr[:-1])

    row_ids = row_ids_of()
    idx64 = indices.long()
    put('sample_equals_torch_bitwise', bool(torch.equal((M * D).data, w * D[row_ids, idx64])))
    out = torch.empty(nse, device=dev)
    keep = {}
    stats = timed_in_turns({
        'sample_mul': lambda: keep.__setitem__('r', (M * D).data),
        'torch_mul': lambda: keep.__setitem__('r', w * D[row_ids, idx64]),
        'torch_row_ids': lambda: keep.__setitem__('r', row_ids_of()),
        'copy': lambda: out.copy_(w),
    }, a.calls)
    for name, v in stats.items():
        put(name, v)
    del M, D, w, indices, indptr, row_ids, idx64, out, keep
    torch.cuda.empty_cache()

    # ---- csr.diag_add(d)
    n = a.diag_n
    indices, indptr = fixed_rows(n, k, dev, 2)
    nse = n * k
    w = torch.rand(nse, device=dev)
    d = torch.rand(n, device=dev)
    M = be.CSR((w, indices, indptr), shape=(n, n), check_structure=False)
    put('diag_shape', [n, n])
    put('diag_nse', nse)
    out = torch.empty(nse, device=dev)
    found = torch.empty((n, 2), dtype=torch.int64, device=dev)

    def first():
        M.buffers.pop('diag_positions', None)
        return M.diag_add(d)

    def scan():
        call('be_diag_scan', A.ptr(indices), A.ptr(indptr), int(indptr.dtype == torch.int64), n, n, nse, A.ptr(found),
             A.stream_ptr())

    R = first()
    put('diag_new_nse', int(R.nse))
    del R
    found[:, 0] = -1
    found[:, 1] = _diag._I64_MAX
    stats = timed_in_turns({'diag_first': first, 'diag_later': lambda: M.diag_add(d), 'diag_scan': scan,
                            'diag_copy': lambda: out.copy_(w)}, a.calls)
    for name, v in stats.items():
        put(name, v)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
