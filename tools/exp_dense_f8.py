"""FP8 against f16 weights on the event-driven dense product, at the C5 shape (csrc/be_dense_f8.hip).

``S[--nb, --n]`` (default 32 x 65536) at ``--rate`` (default 1 %) firing per row, ``W[--n, --n]`` drawn from +-{1 ... 8} (exact in
f16, e4m3 and e5m2), the same values in the three matrices.  ``S @ W`` with f16 (the unchanged kernel of be_dense.hip: the
yardstick), e4m3 and e5m2 weights take turns inside one loop on the same spikes; HIP-event medians and quartiles of ``--reps``
turns.  The same for the 1-D product (batch row 0).  Recorded with them: the union rows the batch touches, the weight bytes a
product has to read (union rows x n x bytes per weight), that figure over the median time, and its fraction of the device's
read-only streaming rate measured in the same run (``be_diag_stream_read``).  Because every weight and every sum is a small
integer, the two FP8 outputs (f32) must be EQUAL, and equal to the f16 product's once rounded to f16; a shape counts as measured
only if they are.  Prints one JSON line and, with
``--out``, writes it.

    python tools/exp_dense_f8.py [--n 65536] [--nb 32] [--rate 0.01] [--reps 11] [--out profiles/dense_f8_line.json]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd import _array as A, _lib  # noqa: E402


def timed_turns(fns, reps):
    """``{median, q1, q3}`` in ms of each function: ``reps`` turns, every function once per turn between two HIP events."""
    for _ in range(3):
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
    out = []
    for t in ts:
        t = sorted(t)
        out.append({'median': round(t[len(t) // 2], 4), 'q1': round(t[len(t) // 4], 4), 'q3': round(t[(3 * len(t)) // 4], 4)})
    return out


def read_ceiling_gbps(dev):
    buf = torch.zeros(1 << 29, dtype=torch.int32, device=dev)          # 2 GiB
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    ms = ctypes.c_float(0)
    torch.cuda.synchronize()
    _lib.call('be_diag_stream_read', A.ptr(buf), buf.numel() * 4, 5, A.ptr(sink), ctypes.byref(ms), A.stream_ptr())
    return round(buf.numel() * 4 / (ms.value * 1e-3) / 1e9, 1) if ms.value > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--nb', type=int, default=32)
    ap.add_argument('--rate', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error('--reps must be at least 9')
    dev = torch.device('cuda')
    n, nb = args.n, args.nb
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    # the same +-{1 ... 8} in the three formats: 16-entry tables made by torch's CPU casts, indexed on the device slab by slab
    vals = torch.tensor([v for v in range(-8, 9) if v != 0], dtype=torch.float32)
    lut = {'f16': vals.to(torch.float16).to(dev), 'e4m3': vals.to(torch.float8_e4m3fn).view(torch.uint8).to(dev),
           'e5m2': vals.to(torch.float8_e5m2).view(torch.uint8).to(dev)}
    W = {'f16': torch.empty((n, n), dtype=torch.float16, device=dev), 'e4m3': torch.empty((n, n), dtype=torch.uint8, device=dev),
         'e5m2': torch.empty((n, n), dtype=torch.uint8, device=dev)}
    slab = max(1, (1 << 28) // max(n, 1))
    for r0 in range(0, n, slab):
        idx = torch.randint(0, 16, (min(slab, n - r0), n), device=dev, generator=g)
        for name in W:
            W[name][r0:r0 + idx.shape[0]] = lut[name][idx]
        del idx
    W['e4m3'], W['e5m2'] = W['e4m3'].view(torch.float8_e4m3fn), W['e5m2'].view(torch.float8_e5m2)
    S = torch.rand((nb, n), device=dev, generator=g) < args.rate
    union = int(S.any(dim=0).sum())
    active0 = int(S[0].sum())
    assert 8 * int(S.sum(dim=1).max()) < 2 ** 24                      # every sum is an exact integer in f16's f32 accumulator too
    ev, ev0 = be.BinaryArray(S), be.BinaryArray(S[0].contiguous())
    names = ['f16', 'e4m3', 'e5m2']
    ceiling = read_ceiling_gbps(dev)

    res = {'what': 'S @ W with f16 (be_dense.hip, unchanged), e4m3 and e5m2 weights (be_dense_f8.hip), alternating in one loop',
           'device': torch.cuda.get_device_name(0), 'n': n, 'nb': nb, 'rate': args.rate, 'reps': args.reps,
           'read_ceiling_GBps': ceiling, 'union_rows': union, 'active_rows_1d': active0}
    for tag, e, rows in (('batched', ev, union), ('vector_1d', ev0, active0)):
        outs = {}

        def make(name):
            def f():
                outs[name] = e @ W[name]
            return f
        t = timed_turns([make(nm) for nm in names], args.reps)
        torch.cuda.synchronize()
        # the f32 sums are exact integers; the f16 product rounds the same sums to f16 on output
        equal = torch.equal(outs['e4m3'], outs['e5m2']) and all(
            outs[nm].dtype == torch.float32 and torch.equal(outs['f16'], outs[nm].to(torch.float16)) for nm in ('e4m3', 'e5m2'))
        block = {'measured': bool(equal), 'outputs_equal_f16': bool(equal)}
        for nm, tt in zip(names, t):
            wbytes = rows * n * (2 if nm == 'f16' else 1)
            gbps = wbytes / (tt['median'] * 1e-3) / 1e9
            block[nm] = {'ms': tt, 'weight_bytes': wbytes, 'weight_GBps': round(gbps, 1),
                         'frac_of_read_ceiling': round(gbps / ceiling, 4) if ceiling else None}
        for nm in ('e4m3', 'e5m2'):
            block[f'f16_over_{nm}'] = round(block['f16']['ms']['median'] / block[nm]['ms']['median'], 3)
        res[tag] = block
    res['all_measured'] = bool(res['batched']['measured'] and res['vector_1d']['measured'])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0 if res['all_measured'] else 1


if __name__ == '__main__':
    sys.exit(main())
