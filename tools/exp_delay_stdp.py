"""Timings of the plasticity updates of delayed synapses (``DelayedCSR.update_on_pre`` / ``update_on_post``)
against the undelayed updates of the same matrix, at §2.15's point.

One f32 matrix of ``--n`` x ``--n`` (default 1M) with ``--conn`` (default 1000) entries per row, delays uniform in ``[0, depth)``
(``--depth``, default 16), ``--rate`` (default 1 %) firing on both sides, both matrices armed with ``prepare(plastic=(0, 1))`` and
every update ``inplace=True`` (certified).  HIP-event times over ``--reps`` (default 21) repetitions, the variants taking turns
inside one loop; each is reported as its median with the quartiles of its own repeats beside it (``*_q``), which is the spread
the comparison between two variants has to exceed:

* ``on_pre``: ``D.update_on_pre(ring, post_trace)`` (ring compaction + the row-driven kernel + the workspace upkeep);
* ``on_post_ring``: ``D.update_on_post(hist, post_spike)`` — the aged kernel reads the ``ValueRing`` in place;
* ``on_post_by_age``: ``D.update_on_post(hist.by_age()[:depth], post_spike)`` — the rotation copy of the history, then the
  existing permuted kernel;
* ``undelayed_on_pre`` / ``undelayed_on_post``: the same matrix without delays, ``csr.update_on_pre`` / ``update_on_post``;
* ``step`` / ``step_graph``: the whole learning step (``ring.push``, ``hist.push``, ``ring @ D``, both updates), eager and as a
  replayed ``capture_step`` graph.

Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_delay_stdp.py [--n 1000000] [--conn 1000] [--depth 16] [--rate 0.01] [--reps 21] [--out profiles/delay_stdp_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from exp_delay import route_of  # noqa: E402


def say(msg):
    print(f'[exp_delay_stdp] {msg}', file=sys.stderr, flush=True)


def timed_alternating_quartiles(fns, reps):
    """``(median, [q1, q3])`` ms of each function, the functions taking turns inside one loop."""
    for f in fns:
        f()
        torch.cuda.synchronize()
        say(f'{f.__name__ if hasattr(f, "__name__") else "graph"} ran once')
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
        out.append((round(t[len(t) // 2], 3), [round(t[len(t) // 4], 3), round(t[(3 * len(t)) // 4], 3)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--conn', type=int, default=1000)
    ap.add_argument('--depth', type=int, default=16)
    ap.add_argument('--rate', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error('--reps must be at least 20')
    dev = torch.device('cuda')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n, conn, depth = args.n, args.conn, args.depth
    nnz = n * conn
    ptr = torch.arange(n + 1, dtype=torch.int64 if nnz > 2**31 - 1 else torch.int32, device=dev) * conn
    idx = torch.randint(0, n, (nnz,), dtype=torch.int32, device=dev, generator=g)
    w = torch.rand(nnz, dtype=torch.float32, device=dev, generator=g) * 0.5 + 0.25
    delays = torch.randint(0, depth, (nnz,), dtype=torch.int32, device=dev, generator=g)
    csr = be.CSR((w, idx, ptr), shape=(n, n), check_structure=False)
    say('arrays drawn; splitting by delay and arming')
    D = csr.with_delays(delays, depth).prepare(plastic=(0.0, 1.0))
    del delays
    csr.prepare(plastic=(0.0, 1.0))
    say('both matrices armed')
    spikes = [torch.rand(n, device=dev, generator=g) < args.rate for _ in range(8)]
    traces = [(torch.rand(n, device=dev, generator=g) - 0.5) * 1e-3 for _ in range(8)]
    ring, hist = be.SpikeRing(n, depth), be.ValueRing(n, depth)
    for t in range(depth):
        ring.push(spikes[t % 8])
        hist.push(traces[t % 8])
    turn = [0]

    def nxt(pool):
        turn[0] += 1
        return pool[turn[0] % 8]

    def on_pre():
        D.update_on_pre(ring, nxt(traces), 0.0, 1.0, inplace=True)

    def on_post_ring():
        D.update_on_post(hist, nxt(spikes), 0.0, 1.0, inplace=True)

    def on_post_by_age():
        D.update_on_post(hist.by_age()[:depth], nxt(spikes), 0.0, 1.0, inplace=True)

    def undelayed_on_pre():
        csr.update_on_pre(nxt(spikes), nxt(traces), 0.0, 1.0, inplace=True)

    def undelayed_on_post():
        csr.update_on_post(nxt(traces), nxt(spikes), 0.0, 1.0, inplace=True)

    s_buf, x_buf, t_buf, k_buf = spikes[0].clone(), traces[0].clone(), traces[1].clone(), spikes[1].clone()
    out = torch.zeros(n, device=dev)

    def step():
        ring.push(s_buf)
        hist.push(x_buf)
        out.copy_(ring @ D)
        D.update_on_pre(ring, t_buf, 0.0, 1.0, inplace=True)
        D.update_on_post(hist, k_buf, 0.0, 1.0, inplace=True)

    step_graph = be.capture_step(step)
    say('step captured; timing')
    names = ['on_pre', 'on_post_ring', 'on_post_by_age', 'undelayed_on_pre', 'undelayed_on_post', 'step', 'step_graph']
    res = timed_alternating_quartiles([on_pre, on_post_ring, on_post_by_age, undelayed_on_pre, undelayed_on_post, step, step_graph],
                                      args.reps)
    assert D.plastic_state is not None and csr.plastic_state is not None
    line = {'what': 'STDP updates of delayed synapses vs the undelayed updates', 'device': torch.cuda.get_device_name(0), 'n': n,
            'conn': conn, 'depth': depth, 'rate': args.rate, 'reps': args.reps, 'dtype': 'f32'}
    for name, (med, q) in zip(names, res):
        line[name + '_ms'], line[name + '_q'] = med, q
    ms = {name: med for name, (med, _) in zip(names, res)}
    line.update({
        'ring_over_by_age': round(ms['on_post_ring'] / ms['on_post_by_age'], 3),
        'on_pre_over_undelayed': round(ms['on_pre'] / ms['undelayed_on_pre'], 3),
        'on_post_ring_over_undelayed': round(ms['on_post_ring'] / ms['undelayed_on_post'], 3),
        'route_stacked': D.plastic_state['route'], 'route_undelayed': csr.plastic_state['route'],
        'workspace_stacked_bytes': route_of(D.stacked)[1], 'workspace_undelayed_bytes': route_of(csr)[1],
    })
    print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
