"""Timings of the batched delayed product — ``SpikeRing(n, depth, batch=B)``, ``ring.push(S); ring @ D`` (csrc/be_delay.hip,
DESIGN.md §2.17) — against what a user could do without it.

§2.15's point: one f32 matrix of ``--n`` x ``--n`` (default 1M) with ``--conn`` (default 1000) entries per row, ``--depth``
(default 16) with delays uniform in ``[0, depth)``, ``--rate`` (default 1 %) firing per sample, ``D.prepare()``.  For every ``B`` of
``--batches`` (default 1, 8, 32), HIP-event medians and quartiles of ``--reps`` repetitions, the variants taking turns inside
one loop and all of them fed the same spikes in a turn:

* ``batched``: ``ring.push(S); ring @ D`` on a batched ring — one push, one unroll, one scatter over the stacked matrix;
* ``loop``: ``B`` one-sample rings, ``ring_b.push(S[b]); ring_b @ D`` in a loop — what the parent commit offers: ``B`` pushes,
  ``B`` compactions, ``B`` scatters;
* ``by_delay``: ``ring.push(S)`` and ``sum_d ring.events(d) @ W_d`` on a batched ring, over ``depth`` prepared sub-matrices (views
  of the stacked arrays);
* ``unroll`` and ``push``: ``ring.stacked_bits(ages=depth, row_mask=D.row_mask)`` and ``ring.push(S)`` alone (the push on a ring of
  its own), for their share of the batched step.

Because every variant saw the same spikes, the outputs of the last timed turn are comparable: ``batched`` against ``loop`` row by
row (and against ``by_delay``).  A ``B`` counts as measured only when ``batched`` and ``loop`` agree there: the largest difference
is at most ``--rtol`` (default 1e-5: f32 sums in another order) of the largest output.  Also recorded: the route the router
picked for ``D.stacked`` and its workspace size at each ``B``.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_delay_batch.py [--n 1000000] [--conn 1000] [--depth 16] [--rate 0.01] [--batches 1,8,32] [--reps 9]
                                    [--out profiles/delay_batch_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from exp_delay import route_of  # noqa: E402


def timed_turns(fns, reps, before_turn):
    """``{median, q1, q3}`` in ms of each function: ``reps`` turns, in each of which ``before_turn()`` runs untimed and then every
    function once, between two HIP events of its own."""
    before_turn()
    for f in fns:                          # warm-up: every shape the timed window uses
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        before_turn()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--conn', type=int, default=1000)
    ap.add_argument('--depth', type=int, default=16)
    ap.add_argument('--rate', type=float, default=0.01)
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--rtol', type=float, default=1e-5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error('--reps must be at least 7')
    dev = torch.device('cuda')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n, conn, depth = args.n, args.conn, args.depth
    nnz = n * conn
    ptr = torch.arange(n + 1, dtype=torch.int64 if nnz > 2**31 - 1 else torch.int32, device=dev) * conn
    idx = torch.randint(0, n, (nnz,), dtype=torch.int32, device=dev, generator=g)
    w = torch.rand(nnz, dtype=torch.float32, device=dev, generator=g)
    delays = torch.randint(0, depth, (nnz,), dtype=torch.int32, device=dev, generator=g)
    D = be.CSR((w, idx, ptr), shape=(n, n), check_structure=False).with_delays(delays, depth).prepare()
    del delays, w, idx
    st = D.stacked
    print(f'split and prepared: {st.shape[0]} stacked rows', file=sys.stderr, flush=True)
    subs = []
    for d in range(depth):                      # W_d: rows [d * n, (d + 1) * n) of the stacked matrix, as views
        p = st.indptr[d * n:(d + 1) * n + 1]
        lo, hi = int(p[0]), int(p[-1])
        subs.append(be.CSR((st.data[lo:hi], st.indices[lo:hi], p - lo), shape=(n, n), check_structure=False).prepare())
    print(f'built: stacked route {route_of(st)[0]}', file=sys.stderr, flush=True)

    per_batch = []
    for B in (int(b) for b in args.batches.split(',')):
        spikes = [torch.rand((B, n), device=dev, generator=g) < args.rate for _ in range(8)]
        ring, ring_c, ring_p = (be.SpikeRing(n, depth, batch=B) for _ in range(3))
        singles = [be.SpikeRing(n, depth) for _ in range(B)]
        for t in range(depth):                  # the same full history everywhere
            S = spikes[t % len(spikes)]
            ring.push(S)
            ring_c.push(S)
            for b, r in enumerate(singles):
                r.push(S[b])
        cur, last = {'S': None, 'turn': 0}, {}

        def before_turn():
            cur['turn'] += 1
            cur['S'] = spikes[cur['turn'] % len(spikes)]

        def batched():
            ring.push(cur['S'])
            last['batched'] = ring @ D

        def loop():
            S = cur['S']
            outs = []
            for b, r in enumerate(singles):
                r.push(S[b])
                outs.append(r @ D)
            last['loop'] = outs

        def by_delay():
            ring_c.push(cur['S'])
            acc = ring_c.events(0) @ subs[0]
            for d in range(1, depth):
                acc = acc + (ring_c.events(d) @ subs[d])
            last['by_delay'] = acc

        def unroll():
            ring.stacked_bits(ages=depth, row_mask=D.row_mask)

        def push():
            ring_p.push(cur['S'])

        ms = timed_turns([batched, loop, by_delay, unroll, push], args.reps, before_turn)
        torch.cuda.synchronize()
        a, c = last['batched'], last['by_delay']
        l = torch.stack(last['loop'])
        scale = float(a.abs().max())
        diff_loop, diff_by_delay = float((a - l).abs().max()), float((a - c).abs().max())
        agree = bool(scale > 0 and diff_loop <= args.rtol * scale)
        route, ws_bytes = route_of(st)
        rec = {'B': B, 'measured': agree, 'route_stacked': route, 'workspace_stacked_bytes': ws_bytes,
               'batched_ms': ms[0], 'loop_ms': ms[1], 'by_delay_ms': ms[2], 'unroll_ms': ms[3], 'push_ms': ms[4],
               'loop_over_batched': round(ms[1]['median'] / ms[0]['median'], 3),
               'by_delay_over_batched': round(ms[2]['median'] / ms[0]['median'], 3),
               'batched_ms_per_sample': round(ms[0]['median'] / B, 4),
               'unroll_share_of_batched': round(ms[3]['median'] / ms[0]['median'], 4),
               'max_abs_diff_batched_vs_loop': diff_loop, 'bit_equal_batched_vs_loop': bool(torch.equal(a, l)),
               'max_abs_diff_batched_vs_by_delay': diff_by_delay, 'max_abs_output': scale}
        print(json.dumps(rec), file=sys.stderr, flush=True)
        per_batch.append(rec)
        del ring, ring_c, ring_p, singles, spikes, last, a, c, l
        torch.cuda.empty_cache()

    line = {'what': 'batched ring @ DelayedCSR vs B one-sample rings in a loop and vs depth sub-matrices',
            'device': torch.cuda.get_device_name(0), 'n': n, 'conn': conn, 'depth': depth, 'rate': args.rate, 'reps': args.reps,
            'dtype': 'f32', 'rtol': args.rtol, 'routes_sub_matrices': sorted({route_of(s)[0] for s in subs}),
            'all_measured': all(r['measured'] for r in per_batch), 'batches': per_batch}
    print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
