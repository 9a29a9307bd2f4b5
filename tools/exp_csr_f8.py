"""FP8 against f32 weights on the planned CSR scatter ``events @ W`` (csrc/be_csr_plan.hip: the d8 and the q8 layout).

A ``--n`` x ``--n`` matrix (default 1M x 1M) with ``--row`` entries per row (default 1000) at uniform random columns, weights N(0, 1),
``--rate`` (default 1 %) of the rows firing.  Three sides on the same structure and the same slice geometry:
    (a) the f32 weights on their d8 plan (5 bytes per synapse),   (b) e4m3 and (c) e5m2 codes on the q8 plan (2 bytes per synapse),
the codes quantised from the same weights by ``CSR.quantize_fp8``'s formula.  One loop of ``--reps`` turns; the order of the three is
shuffled inside every turn; HIP-event medians with quartiles.  Recorded with them: the bytes of each plan, the build time of each plan
(host clock around a synchronised build), the block bytes a step reads (active rows' share of the blob), that figure over the median,
and the device's read-only streaming rate measured in the same run (``be_diag_stream_read``).

Correctness comes first: (b) and (c) must EQUAL their direct routes (``be_binary_csrmm_t_f8``) bit for bit, and (a) must agree with
(b) / (c) within the formats' quantisation bound summed over each column's active entries (e4m3: 2^-4 |w| where |w| >= 2^-6 scale, else
2^-10 scale; e5m2: 2^-3 |w| where |w| >= 2^-14 scale, else 2^-17 scale) plus the f32 route's own 1e-5 of the column's sum of |w|.  A
side counts as measured only if its check holds.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_csr_f8.py [--n 1000000] [--row 1000] [--rate 0.01] [--reps 21] [--out profiles/csr_f8_line.json]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd import _array as A, _csr as C, _csr_f8 as F, _dense_f8 as F8, _lib  # noqa: E402

BOUND = {'e4m3': (2.0 ** -4, 2.0 ** -6, 2.0 ** -10), 'e5m2': (2.0 ** -3, 2.0 ** -14, 2.0 ** -17)}


def quartiles(t):
    t = sorted(t)
    return {'median': round(t[len(t) // 2], 4), 'q1': round(t[len(t) // 4], 4), 'q3': round(t[(3 * len(t)) // 4], 4)}


def timed_shuffled(fns, reps, seed=0):
    """ms of each function over ``reps`` turns; every turn runs all of them once, in an order shuffled per turn."""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    rnd = random.Random(seed)
    ts = [[] for _ in fns]
    for _ in range(reps):
        order = list(range(len(fns)))
        rnd.shuffle(order)
        for i in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fns[i]()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [quartiles(t) for t in ts]


def read_ceiling_gbps(dev):
    buf = torch.zeros(1 << 29, dtype=torch.int32, device=dev)          # 2 GiB
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    ms = ctypes.c_float(0)
    torch.cuda.synchronize()
    _lib.call('be_diag_stream_read', A.ptr(buf), buf.numel() * 4, 5, A.ptr(sink), ctypes.byref(ms), A.stream_ptr())
    return round(buf.numel() * 4 / (ms.value * 1e-3) / 1e9, 1) if ms.value > 0 else None


def timed_build(build):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = build()
    torch.cuda.synchronize()
    return plan, round(time.perf_counter() - t0, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--row', type=int, default=1000)
    ap.add_argument('--rate', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error('--reps must be at least 9')
    dev = torch.device('cuda')
    n, row = args.n, args.row
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
    spikes = (torch.rand(n, device=dev, generator=g) < args.rate).to(torch.uint8)
    active = torch.nonzero(spikes).reshape(-1)
    n_active = int(active.numel())
    amax = float(w.abs().max())

    shift, width = F.Q8Plan.geometry(n, n, nnz)
    res = {'what': 'events @ W on the planned scatter: f32 weights on the d8 plan, e4m3 / e5m2 codes on the q8 plan; same structure and '
                   'slice geometry, order shuffled inside every turn',
           'device': torch.cuda.get_device_name(0), 'n': n, 'row': row, 'nnz': nnz, 'rate': args.rate, 'reps': args.reps,
           'active_rows': n_active, 'slice_shift': shift, 'slice_width': width, 'read_ceiling_GBps': read_ceiling_gbps(dev)}

    d8, t_d8 = timed_build(lambda: C.ScatterPlan.build(w, idx, ptr, shape=(n, n), slice_shift=shift, slice_width=width, layout='d8',
                                                       keep_order=False))
    sides = {'f32_d8': {'plan_bytes': d8.nbytes(), 'build_s': t_d8, 'bytes_per_synapse': round(d8.blob.numel() / nnz, 3),
                        'block_hint': d8.block_hint, 'parts': d8.default_parts(), 'n_slices': d8.n_slices}}
    sp_bm = spikes.reshape(1, -1)
    outs = {'f32_d8': torch.empty((1, n), dtype=torch.float32, device=dev)}
    fns = [lambda: C._plan_call(d8, w, sp_bm, A.BE_SPIKE_BOOL, outs['f32_d8'])]
    names = ['f32_d8']
    codes, scales, plans = {}, {}, {}
    for fmt in ('e4m3', 'e5m2'):
        scale = float(torch.tensor(amax, dtype=torch.float32) / torch.tensor(F8.FMT_MAX[fmt], dtype=torch.float32))
        c = torch.empty(nnz, dtype=torch.uint8, device=dev)
        for e0 in range(0, nnz, slab):
            e1 = min(nnz, e0 + slab)
            c[e0:e1] = (w[e0:e1] / torch.tensor(scale, dtype=torch.float32, device=dev)).clamp(
                -F8.FMT_MAX[fmt], F8.FMT_MAX[fmt]).to(F8._DTYPE_OF_FMT[fmt]).view(torch.uint8)
        codes[fmt], scales[fmt] = c, scale
        plans[fmt], t_q8 = timed_build(lambda: F.Q8Plan.build(c, idx, ptr, shape=(n, n), slice_shift=shift, slice_width=width))
        p = plans[fmt]
        sides[fmt] = {'plan_bytes': p.nbytes(), 'build_s': t_q8, 'bytes_per_synapse': round(p.blob.numel() / nnz, 3), 'scale': scale,
                      'block_hint': p.block_hint, 'parts': p.default_parts(), 'n_slices': p.n_slices}
        outs[fmt] = torch.empty((1, n), dtype=torch.float32, device=dev)
        fns.append(lambda fmt=fmt: plans[fmt].step(F8._CODE_OF_FMT[fmt], scales[fmt], sp_bm, A.BE_SPIKE_BOOL, outs[fmt]))
        names.append(fmt)

    # ---- correctness before any time is reported
    for f in fns:
        f()
    torch.cuda.synchronize()
    cols = idx.view(n, row)[active].reshape(-1).long()
    wa = w.view(n, row)[active].reshape(-1).double()
    abs_col = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, cols, wa.abs())
    ref = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, cols, wa)
    a_err = (outs['f32_d8'][0].double() - ref).abs()
    sides['f32_d8']['max_err_over_1e-5_colscale'] = round(float((a_err / (1e-5 * abs_col).clamp_min(1e-30)).max()), 4)
    sides['f32_d8']['measured'] = bool((a_err <= 1e-5 * abs_col + 1e-30).all())
    for fmt in ('e4m3', 'e5m2'):
        direct = torch.empty((1, n), dtype=torch.float32, device=dev)
        F.f8_direct(codes[fmt], F8._CODE_OF_FMT[fmt], scales[fmt], idx, ptr, sp_bm, A.BE_SPIKE_BOOL, direct, n, n)
        equal = torch.equal(direct.view(torch.int32), outs[fmt].view(torch.int32))
        rel, min_normal, sub = BOUND[fmt]
        s = scales[fmt]
        per = torch.where(wa.abs() >= min_normal * s, rel * wa.abs(), torch.full_like(wa, sub * s))
        bound = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, cols, per) + 1e-5 * abs_col + 1e-30
        diff = (outs[fmt][0].double() - outs['f32_d8'][0].double()).abs()
        within = bool((diff <= bound).all())
        sides[fmt].update(equals_direct_route=bool(equal), within_quantisation_bound_of_f32=within,
                          max_diff_over_bound=round(float((diff / bound).max()), 4), measured=bool(equal and within))
        del direct, per, bound, diff
    del cols, wa, abs_col, ref, a_err

    # ---- the three sides, shuffled inside every turn
    t = timed_shuffled(fns, args.reps)
    for nm, tt in zip(names, t):
        blob = (d8 if nm == 'f32_d8' else plans[nm]).blob.numel()
        step_bytes = blob * n_active / n
        gbps = step_bytes / (tt['median'] * 1e-3) / 1e9
        sides[nm].update(ms=tt, block_bytes_per_step=int(step_bytes), block_GBps=round(gbps, 1),
                         frac_of_read_ceiling=round(gbps / res['read_ceiling_GBps'], 4) if res['read_ceiling_GBps'] else None)
    res.update(sides)
    for fmt in ('e4m3', 'e5m2'):
        res[f'{fmt}_over_f32_time'] = round(sides[fmt]['ms']['median'] / sides['f32_d8']['ms']['median'], 4)
        res[f'{fmt}_over_f32_plan_bytes'] = round(sides[fmt]['plan_bytes'] / sides['f32_d8']['plan_bytes'], 4)
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
