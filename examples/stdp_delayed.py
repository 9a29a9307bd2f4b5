"""A current-based LIF network whose delayed excitatory synapses learn: the network of examples/delayed_network.py (CUBA, Vogels &
Abbott 2005, one conduction delay per synapse) with pair-based STDP on the excitatory projection, run eagerly and as a captured
HIP graph (``capture_step``), with the final weights and spike counts compared bit for bit.

    python examples/stdp_delayed.py                          # 4000 neurons, 80 synapses each, delays up to 1.5 ms
    python examples/stdp_delayed.py --n 1000000 --conn 1000 --steps 50

The delays are axonal, so a synapse sees its pre neuron's spike — and its pre neuron's trace — ``delay`` steps late.  Each step:

  ``ring.push(spikes)``, ``hist.push(a_plus * trace)``   the spikes and the (scaled) trace of the last update enter the histories
  ``ring @ D_exc``, ``ring @ D_inh``                      every synapse delivers its spike of ``delay`` steps ago
  ``D_exc.update_on_pre(ring, -a_minus * trace)``         LTD at a spike's ARRIVAL: the post neuron's trace as it is now
  ``D_exc.update_on_post(hist, spikes)``                  LTP at a POST spike: the pre trace each synapse saw arrive (``hist`` by age)

both in place under ``prepare(plastic=(0, w_max))``, which keeps the scatter workspace of ``D_exc`` current from launch to launch
(DESIGN.md 2.6, 2.16).  The traces are plain torch.  The heads of both histories live on the device, so the replayed graph walks
through them as the eager loop does.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402

WARMUP = 3          # eager steps before the capture; they are steps of the simulation like any other


def projection(n, rows_lo, rows_hi, conn, weight, depth, seed, dev, plastic_max=None):
    """``n x n`` with ``conn`` random targets for the neurons ``[rows_lo, rows_hi)`` (the other rows are empty) and a delay in
    ``[1, depth)`` per synapse; one shared weight, or (``plastic_max``) one weight per synapse, armed for learning in
    ``[0, plastic_max]``."""
    g = torch.Generator(device=dev).manual_seed(seed)
    lens = torch.zeros(n, dtype=torch.int64, device=dev)
    lens[rows_lo:rows_hi] = conn
    nnz = (rows_hi - rows_lo) * conn
    ptr = torch.zeros(n + 1, dtype=torch.int64 if nnz > 2**31 - 1 else torch.int32, device=dev)
    ptr[1:] = torch.cumsum(lens, 0)
    idx = torch.randint(0, n, (nnz,), dtype=torch.int32, device=dev, generator=g)
    delays = torch.randint(1, depth, (nnz,), dtype=torch.int32, device=dev, generator=g)
    w = torch.full((1 if plastic_max is None else nnz,), weight, dtype=torch.float32, device=dev)
    d = be.CSR((w, idx, ptr), shape=(n, n), check_structure=False).with_delays(delays, depth)
    return d.prepare() if plastic_max is None else d.prepare(plastic=(0.0, plastic_max))


def run(args, graph: bool):
    dev = torch.device('cuda')
    n, n_exc = args.n, args.n * 4 // 5
    d_exc = projection(n, 0, n_exc, args.conn, args.w_exc, args.depth, 1, dev, plastic_max=args.w_max)
    d_inh = projection(n, n_exc, n, args.conn, -9.0, args.depth, 2, dev)
    g = torch.Generator(device=dev).manual_seed(7)
    v = torch.rand(n, device=dev, generator=g) * 10.0 - 60.0
    g_exc, g_inh, refr = (torch.zeros(n, device=dev) for _ in range(3))
    in_exc, in_inh, count, trace = (torch.zeros(n, device=dev) for _ in range(4))
    spikes = torch.zeros(n, dtype=torch.bool, device=dev)
    ring, hist = be.SpikeRing(n, args.depth), be.ValueRing(n, args.depth)
    decay = math.exp(-args.dt / args.tau)

    def step():
        trace.mul_(decay).add_(spikes.float())
        ring.push(spikes)
        hist.push(trace * args.a_plus)
        in_exc.copy_(ring @ d_exc)
        in_inh.copy_(ring @ d_inh)
        d_exc.update_on_pre(ring, trace * -args.a_minus, 0.0, args.w_max, inplace=True)
        d_exc.update_on_post(hist, spikes, 0.0, args.w_max, inplace=True)
        be.lif_cuba_step(v, g_exc, g_inh, refr, in_exc, in_inh, spikes, count, dt=args.dt)

    if graph:
        step_g = be.capture_step(step, warmup=WARMUP)         # WARMUP eager steps, then the capture (which runs nothing)
    else:
        for _ in range(WARMUP):
            step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps - WARMUP):
        step_g() if graph else step()
    torch.cuda.synchronize()
    assert d_exc.plastic_state is not None
    return d_exc.data, count, (time.perf_counter() - t0) / (args.steps - WARMUP)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--n', type=int, default=4000)
    ap.add_argument('--conn', type=int, default=80, help='synapses per neuron')
    ap.add_argument('--depth', type=int, default=16, help='delays are uniform in [1, depth) steps')
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--dt', type=float, default=0.1)
    ap.add_argument('--tau', type=float, default=20.0, help='time constant of the spike traces (ms)')
    ap.add_argument('--w-exc', dest='w_exc', type=float, default=1.62, help='initial excitatory weight')
    ap.add_argument('--w-max', dest='w_max', type=float, default=3.24)
    ap.add_argument('--a-plus', dest='a_plus', type=float, default=0.01)
    ap.add_argument('--a-minus', dest='a_minus', type=float, default=0.0105)
    args = ap.parse_args()
    if not 2 <= args.depth <= 256:
        ap.error('--depth must lie in [2, 256]')
    if args.steps <= WARMUP:
        ap.error(f'--steps must exceed the {WARMUP} warm-up steps')
    print(f"{args.n} LIF neurons, {args.n * args.conn} synapses with delays of 1..{args.depth - 1} steps of {args.dt} ms, "
          f"STDP on the excitatory ones, {args.steps} steps")
    w_e, c_e, ms_e = run(args, graph=False)
    w_g, c_g, ms_g = run(args, graph=True)
    rate = float(c_e.sum()) / args.n / (args.steps * args.dt * 1e-3)
    same = torch.equal(w_e, w_g) and torch.equal(c_e, c_g)
    print(f"  eager : {rate:.1f} Hz mean rate, excitatory weights {args.w_exc:.3f} -> mean {float(w_e.double().mean()):.4f} in "
          f"[{float(w_e.min()):.3f}, {float(w_e.max()):.3f}], {ms_e * 1e3:.3f} ms/step")
    print(f"  graph : {ms_g * 1e3:.3f} ms/step")
    print(f"  final weights and spike counts (eager vs replayed graph): {'identical' if same else 'DIFFERENT'}")
    if not same:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
