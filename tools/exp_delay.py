"""Timings of the delayed product ``ring @ DelayedCSR`` (csrc/be_delay.hip) against the undelayed product and
against what the library offered before it.

One f32 matrix of ``--n`` x ``--n`` (default 1M) with ``--conn`` (default 1000) entries per row, ``--rate`` (default 1 %) firing,
``--depth`` (default 16) with delays uniform in ``[0, depth)``.  Medians of ``--reps`` repetitions timed with HIP events, the
variants taking turns inside one loop:

* ``undelayed``: the prepared ``BinaryArray(spk) @ csr`` — the floor: the same number of synaptic events, no delays;
* ``delayed``: ``ring.push(spk)`` + ``ring @ D`` with ``D.prepare()``;
* ``sixteen``: what a user could do before: ``depth`` prepared sub-matrices ``CSR(W_d)`` (views of the stacked arrays, so no
  extra copy of the matrix) and ``ring.push(spk)`` + ``sum_d ring.events(d) @ W_d``;
* ``compaction``: ``ring.ids(ages=depth, row_mask=D.row_mask)`` alone (the counter fill and the compaction kernel), for its
  share of the delayed step.

Also recorded: the route the router picked for ``D.stacked`` and for the undelayed matrix with their workspace sizes, the route
of the sub-matrices, and the largest difference between ``delayed`` and ``sixteen`` on one ring state.  Prints one JSON line and,
with ``--out``, writes it.

    python tools/exp_delay.py [--n 1000000] [--conn 1000] [--depth 16] [--rate 0.01] [--reps 7] [--out profiles/delay_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
import brainevent_amd._csr as C  # noqa: E402
from exp_float_autograd import timed_alternating  # noqa: E402


def route_of(M):
    """``(name, bytes)`` of the scatter workspace a prepared container holds."""
    ws = M.buffers.get('scatter_plan')
    if isinstance(ws, C.ScatterPlan):
        return 'plan', int(ws.nbytes())
    if isinstance(ws, C.BinnedScatter):
        return 'binned', int(ws.ws.numel() * ws.ws.element_size())
    return 'direct', 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--conn', type=int, default=1000)
    ap.add_argument('--depth', type=int, default=16)
    ap.add_argument('--rate', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n, conn, depth = args.n, args.conn, args.depth
    nnz = n * conn
    ptr = torch.arange(n + 1, dtype=torch.int64 if nnz > 2**31 - 1 else torch.int32, device=dev) * conn
    idx = torch.randint(0, n, (nnz,), dtype=torch.int32, device=dev, generator=g)
    w = torch.rand(nnz, dtype=torch.float32, device=dev, generator=g)
    delays = torch.randint(0, depth, (nnz,), dtype=torch.int32, device=dev, generator=g)
    csr = be.CSR((w, idx, ptr), shape=(n, n), check_structure=False).prepare()
    D = csr.with_delays(delays, depth).prepare()
    del delays
    st = D.stacked
    subs = []
    for d in range(depth):                      # W_d: rows [d * n, (d + 1) * n) of the stacked matrix, as views
        p = st.indptr[d * n:(d + 1) * n + 1]
        lo, hi = int(p[0]), int(p[-1])
        subs.append(be.CSR((st.data[lo:hi], st.indices[lo:hi], p - lo), shape=(n, n), check_structure=False).prepare())
    spikes = [torch.rand(n, device=dev, generator=g) < args.rate for _ in range(8)]
    ring = be.SpikeRing(n, depth)
    for t in range(depth):
        ring.push(spikes[t % len(spikes)])
    turn = [0]

    def next_spikes():
        turn[0] += 1
        return spikes[turn[0] % len(spikes)]

    def sixteen_no_push():
        acc = ring.events(0) @ subs[0]
        for d in range(1, depth):
            acc = acc + (ring.events(d) @ subs[d])
        return acc

    def undelayed():
        return be.BinaryArray(next_spikes()) @ csr

    def delayed():
        ring.push(next_spikes())
        return ring @ D

    def sixteen():
        ring.push(next_spikes())
        return sixteen_no_push()

    def compaction():
        return ring.ids(ages=depth, row_mask=D.row_mask)

    # one ring state, both formulations
    a, b = ring @ D, sixteen_no_push()
    diff = float((a - b).abs().max())
    scale = float(a.abs().max())
    events = int(sum(int((ring.events(d).value & (st.indptr[d * n + 1:(d + 1) * n + 1] > st.indptr[d * n:(d + 1) * n])).sum())
                     for d in range(depth)))
    ms = timed_alternating([undelayed, delayed, sixteen, compaction], args.reps)
    r_und, r_st = route_of(csr), route_of(st)
    line = {
        'what': 'ring @ DelayedCSR vs the undelayed product and vs depth sub-matrices', 'device': torch.cuda.get_device_name(0),
        'n': n, 'conn': conn, 'depth': depth, 'rate': args.rate, 'reps': args.reps, 'dtype': 'f32',
        'undelayed_ms': ms[0], 'delayed_ms': ms[1], 'sixteen_ms': ms[2], 'compaction_ms': ms[3],
        'delayed_over_undelayed': round(ms[1] / ms[0], 3), 'sixteen_over_delayed': round(ms[2] / ms[1], 3),
        'compaction_share_of_delayed': round(ms[3] / ms[1], 4),
        'route_undelayed': r_und[0], 'workspace_undelayed_bytes': r_und[1],
        'route_stacked': r_st[0], 'workspace_stacked_bytes': r_st[1],
        'workspace_stacked_over_undelayed': round(r_st[1] / r_und[1], 3) if r_und[1] else None,
        'routes_sub_matrices': sorted({route_of(s)[0] for s in subs}),
        'workspace_sub_matrices_bytes': int(sum(route_of(s)[1] for s in subs)),
        'active_stacked_rows_of_the_checked_state': events,
        'max_abs_diff_delayed_vs_sixteen': diff, 'max_abs_output': scale,
    }
    print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
