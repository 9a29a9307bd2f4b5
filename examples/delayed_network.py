"""A current-based LIF network whose synapses have conduction delays: the CUBA benchmark network (Vogels & Abbott 2005, the
parameters of examples/cuba_2005.py) with one delay per synapse, uniform in ``[1, depth)`` steps, run eagerly and as a captured
HIP graph (``capture_step``), with the spike counts compared.

    python examples/delayed_network.py                          # 4000 neurons, 80 synapses each, delays up to 1.5 ms
    python examples/delayed_network.py --n 1000000 --conn 1000 --steps 50

Each step: ``ring.push(spikes)`` stores the spikes of the last update in the population's ``SpikeRing``; ``ring @ D_exc`` and
``ring @ D_inh`` deliver every synapse's spike of ``delay`` steps ago — one ordinary scatter each, over the matrix split by delay
(``DelayedCSR``); ``lif_cuba_step`` advances the neurons in place.  The ring's head lives on the device, so the
replayed graph walks through the ring as the eager loop does.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


def projection(n, rows_lo, rows_hi, conn, weight, depth, seed, dev):
    """``n x n`` with ``conn`` random targets for the neurons ``[rows_lo, rows_hi)`` (the other rows are empty), one shared
    weight, and a delay in ``[1, depth)`` per synapse."""
    g = torch.Generator(device=dev).manual_seed(seed)
    lens = torch.zeros(n, dtype=torch.int64, device=dev)
    lens[rows_lo:rows_hi] = conn
    nnz = (rows_hi - rows_lo) * conn
    ptr = torch.zeros(n + 1, dtype=torch.int64 if nnz > 2**31 - 1 else torch.int32, device=dev)
    ptr[1:] = torch.cumsum(lens, 0)
    idx = torch.randint(0, n, (nnz,), dtype=torch.int32, device=dev, generator=g)
    delays = torch.randint(1, depth, (nnz,), dtype=torch.int32, device=dev, generator=g)
    csr = be.CSR((torch.tensor([weight], dtype=torch.float32, device=dev), idx, ptr), shape=(n, n), check_structure=False)
    return csr.with_delays(delays, depth).prepare()


def run(args, d_exc, d_inh, graph: bool):
    dev = torch.device('cuda')
    n = args.n
    g = torch.Generator(device=dev).manual_seed(7)
    v0 = torch.rand(n, device=dev, generator=g) * 10.0 - 60.0
    v = v0.clone()
    g_exc, g_inh, refr = (torch.zeros(n, device=dev) for _ in range(3))
    in_exc, in_inh, count = (torch.zeros(n, device=dev) for _ in range(3))
    spikes = torch.zeros(n, dtype=torch.bool, device=dev)
    ring = be.SpikeRing(n, args.depth)

    def step():
        ring.push(spikes)
        in_exc.copy_(ring @ d_exc)
        in_inh.copy_(ring @ d_inh)
        be.lif_cuba_step(v, g_exc, g_inh, refr, in_exc, in_inh, spikes, count, dt=args.dt)

    if graph:
        step_g = be.capture_step(step)                 # warm-up runs advance the state: restore it
        for t in (g_exc, g_inh, refr, count):
            t.zero_()
        v.copy_(v0)
        spikes.zero_()
        ring.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step_g() if graph else step()
    torch.cuda.synchronize()
    return count, (time.perf_counter() - t0) / args.steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--n', type=int, default=4000)
    ap.add_argument('--conn', type=int, default=80, help='synapses per neuron')
    ap.add_argument('--depth', type=int, default=16, help='delays are uniform in [1, depth) steps')
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--dt', type=float, default=0.1)
    args = ap.parse_args()
    if not 2 <= args.depth <= 256:
        ap.error('--depth must lie in [2, 256]')
    dev = torch.device('cuda')
    n_exc = args.n * 4 // 5
    d_exc = projection(args.n, 0, n_exc, args.conn, 1.62, args.depth, 1, dev)
    d_inh = projection(args.n, n_exc, args.n, args.conn, -9.0, args.depth, 2, dev)
    print(f"{args.n} LIF neurons, {d_exc.nse + d_inh.nse} synapses with delays of 1..{args.depth - 1} steps of {args.dt} ms, "
          f"{args.steps} steps")
    eager, ms_e = run(args, d_exc, d_inh, graph=False)
    graphed, ms_g = run(args, d_exc, d_inh, graph=True)
    rate = float(eager.sum()) / args.n / (args.steps * args.dt * 1e-3)
    same = torch.equal(eager, graphed)
    print(f"  eager : {rate:.1f} Hz mean rate, {ms_e * 1e3:.3f} ms/step")
    print(f"  graph : {ms_g * 1e3:.3f} ms/step")
    print(f"  spike counts identical (eager vs replayed graph): {same}")
    if not same:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
