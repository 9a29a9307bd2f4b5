"""The gather direction ``W @ events`` with FP8 against f32 weights (csrc/be_csr_f8_gather.hip, the q8 plan over the mirror;
DESIGN.md §2.28).

A ``--n`` x ``--n`` matrix (default 1M x 1M) with ``--row`` entries per row (default 1000) at uniform random columns, weights N(0, 1),
``--rate`` (default 1 %) of the inputs firing.  Four sides on the same structure:
    (a) f32 ``csr @ spk`` through its mirror (the planned scatter over the active columns),
    (b) ``spk @ W8.T`` through the q8 mirror (``Float8CSR.build_mirror``),
    (c) the f32 streaming gather (``be_binary_csrmm_nt``: 8 bytes per entry),
    (d) the FP8 streaming gather (``be_binary_csrmm_nt_f8``: 5 bytes per entry),
the e4m3 codes quantised from the same weights by ``CSR.quantize_fp8``'s formula (``--fmt e5m2`` for the other format).  One loop
of ``--reps`` turns, the order of the sides shuffled inside every turn; HIP-event medians with quartiles.  Recorded with them: the
bytes and the build time (host clock around a synchronised build) of each mirror, and the matrix bytes per second of the two
streaming sides.

Correctness comes first: (b) and (d) must EQUAL each other bit for bit, and both must agree with (a) — and (c) — within the format's
quantisation bound summed over each row's active entries (e4m3: 2^-4 |w| where |w| >= 2^-6 scale, else 2^-10 scale; e5m2: 2^-3 |w|
where |w| >= 2^-14 scale, else 2^-17 scale) plus the f32 side's own 1e-5 of the row's sum of |w|.  A side counts as measured only if
its check holds.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_csr_f8_gather.py [--n 1000000] [--row 1000] [--rate 0.01] [--reps 21] [--out profiles/csr_f8_gather_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd import _array as A, _csr as C, _csr_f8 as F, _dense_f8 as F8  # noqa: E402
from exp_csr_f8 import BOUND, timed_shuffled, timed_build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--row', type=int, default=1000)
    ap.add_argument('--rate', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--fmt', default='e4m3', choices=('e4m3', 'e5m2'))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error('--reps must be at least 9')
    dev = torch.device('cuda')
    n, row, fmt = args.n, args.row, args.fmt
    nnz = n * row
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    idx = torch.empty(nnz, dtype=torch.int32, device=dev)
    w = torch.empty(nnz, dtype=torch.float32, device=dev)
    slab = 1 << 27
    for e0 in range(0, nnz, slab):
        e1 = min(nnz, e0 + slab)
        idx[e0:e1] = torch.randint(0, n, (e1 - e0,), device=dev, generator=g, dtype=torch.int32)
        w[e0:e1] = torch.randn(e1 - e0, device=dev, generator=g)
    ptr = torch.arange(0, nnz + 1, row, dtype=torch.int64 if nnz >= 2 ** 31 else torch.int32, device=dev)
    spikes = (torch.rand(n, device=dev, generator=g) < args.rate)
    sp_bm = spikes.to(torch.uint8).reshape(1, -1)
    ev = be.BinaryArray(spikes)
    amax = float(w.abs().max())
    scale = float(torch.tensor(amax, dtype=torch.float32) / torch.tensor(F8.FMT_MAX[fmt], dtype=torch.float32))
    codes = torch.empty(nnz, dtype=torch.uint8, device=dev)
    for e0 in range(0, nnz, slab):
        e1 = min(nnz, e0 + slab)
        codes[e0:e1] = (w[e0:e1] / torch.tensor(scale, dtype=torch.float32, device=dev)).clamp(
            -F8.FMT_MAX[fmt], F8.FMT_MAX[fmt]).to(F8._DTYPE_OF_FMT[fmt]).view(torch.uint8)
    code = F8._CODE_OF_FMT[fmt]

    res = {'what': 'W @ events: (a) f32 through its mirror, (b) FP8 through the q8 mirror, (c) the f32 streaming gather, (d) the FP8 '
                   'streaming gather; same structure, order shuffled inside every turn',
           'device': torch.cuda.get_device_name(0), 'n': n, 'row': row, 'nnz': nnz, 'rate': args.rate, 'reps': args.reps, 'fmt': fmt,
           'scale': scale, 'active_inputs': int(spikes.sum())}

    csr = C.CSR._from_parts(w, idx, ptr, shape=(n, n))
    mr, t_a = timed_build(csr.build_mirror)
    W8 = be.Float8CSR((codes.view(F8._DTYPE_OF_FMT[fmt]), idx, ptr), shape=(n, n), scale=scale)
    _, t_b = timed_build(W8.build_mirror)
    W8T = W8.T
    sides = {'a_f32_mirror': {'mirror_bytes': mr.nbytes(), 'build_s': t_a, 'planned': isinstance(mr.plan, C.ScatterPlan),
                              'raw_arrays_kept': not mr.released},
             'b_f8_mirror': {'mirror_bytes': W8._mirror.nbytes(), 'build_s': t_b, 'planned': W8._mirror.plan is not None},
             'c_f32_stream': {'matrix_bytes': nnz * 8}, 'd_f8_stream': {'matrix_bytes': nnz * 5}}
    outs = {}
    out_d = torch.empty((1, n), dtype=torch.float32, device=dev)

    def side_a():
        outs['a_f32_mirror'] = csr @ ev

    def side_b():
        outs['b_f8_mirror'] = ev @ W8T

    def side_c():
        outs['c_f32_stream'] = C.rows_step(w, idx, ptr, -1, sp_bm, A.BE_SPIKE_BOOL, m=n, k=n, transpose=False)[0]

    def side_d():
        F.f8_gather(codes, code, scale, idx, ptr, sp_bm, A.BE_SPIKE_BOOL, out_d, n, n)
        outs['d_f8_stream'] = out_d[0]

    names = ['a_f32_mirror', 'b_f8_mirror', 'c_f32_stream', 'd_f8_stream']
    fns = [side_a, side_b, side_c, side_d]

    # ---- correctness before any time is reported
    for f in fns:
        f()
    torch.cuda.synchronize()
    equal = torch.equal(outs['b_f8_mirror'].view(torch.int32), outs['d_f8_stream'].view(torch.int32))
    rel, min_normal, sub = BOUND[fmt]
    abs_row = torch.zeros(n, dtype=torch.float64, device=dev)
    bound = torch.zeros(n, dtype=torch.float64, device=dev)
    ref = torch.zeros(n, dtype=torch.float64, device=dev)
    rows_per = max(1, slab // row)
    for r0 in range(0, n, rows_per):
        r1 = min(n, r0 + rows_per)
        wa = w[r0 * row:r1 * row].double() * spikes[idx[r0 * row:r1 * row].long()].double()
        aw = wa.abs()
        per = torch.where(aw >= min_normal * scale, rel * aw, torch.where(aw > 0, torch.full_like(aw, sub * scale), torch.zeros_like(aw)))
        abs_row[r0:r1] = aw.view(r1 - r0, row).sum(1)
        bound[r0:r1] = per.view(r1 - r0, row).sum(1)
        ref[r0:r1] = wa.view(r1 - r0, row).sum(1)
        del wa, aw, per
    for nm in ('a_f32_mirror', 'c_f32_stream'):
        err = (outs[nm].double() - ref).abs()
        sides[nm]['max_err_over_1e-5_rowscale'] = round(float((err / (1e-5 * abs_row).clamp_min(1e-30)).max()), 4)
        sides[nm]['measured'] = bool((err <= 1e-5 * abs_row + 1e-30).all())
    full = bound + 1e-5 * abs_row + 1e-30
    for nm in ('b_f8_mirror', 'd_f8_stream'):
        within = {}
        for other in ('a_f32_mirror', 'c_f32_stream'):
            diff = (outs[nm].double() - outs[other].double()).abs()
            within[other] = bool((diff <= full).all())
            sides[nm][f'max_diff_over_bound_vs_{other[0]}'] = round(float((diff / full).max()), 4)
        sides[nm].update(equals_the_other_f8_route=bool(equal), within_quantisation_bound_of_f32=all(within.values()),
                         measured=bool(equal and all(within.values())))
    del abs_row, bound, ref, full

    # ---- the four sides, shuffled inside every turn
    t = timed_shuffled(fns, args.reps)
    for nm, tt in zip(names, t):
        sides[nm]['ms'] = tt
        if 'matrix_bytes' in sides[nm]:
            sides[nm]['matrix_GBps'] = round(sides[nm]['matrix_bytes'] / (tt['median'] * 1e-3) / 1e9, 1)
    res.update(sides)
    ms = {nm: sides[nm]['ms']['median'] for nm in names}
    res['b_over_a_time'] = round(ms['b_f8_mirror'] / ms['a_f32_mirror'], 4)
    res['d_over_c_time'] = round(ms['d_f8_stream'] / ms['c_f32_stream'], 4)
    res['b_over_a_mirror_bytes'] = round(sides['b_f8_mirror']['mirror_bytes'] / max(1, sides['a_f32_mirror']['mirror_bytes']), 4)
    res['all_measured'] = bool(all(sides[nm]['measured'] for nm in names))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0 if res['all_measured'] else 1


if __name__ == '__main__':
    sys.exit(main())
