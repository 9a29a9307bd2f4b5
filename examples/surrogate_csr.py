"""Surrogate-gradient training through the event-driven products.

A small recurrent spiking network: leaky integrate-and-fire neurons driven by a fixed input current and a sparse recurrent
projection (a ``CSR`` container whose weights are a ``torch.nn.Parameter``), read out through a ``Dense`` projection.  The
spike function is a Heaviside step in the forward pass and a fast-sigmoid derivative in the backward pass (the surrogate);
``BinaryArray(spikes) @ csr`` and ``BinaryArray(spikes) @ dense`` are differentiated by ``brainevent_amd``: straight-through
for the spikes, per-synapse for the weights.  The task is synthetic and generated here: each of two input patterns must drive
its own readout unit.  Trained with ``torch.optim.SGD``; the loss falls.

    python examples/surrogate_csr.py [--steps 60] [--fused [--learn-beta | --synaptic [--adapt] [--learn-neuron] [--fused-recurrent [--rec-delays DEPTH]]]]

``--fused`` replaces the hand-written neuron (about six elementwise launches forwards and twice that backwards per time step) by
``be.lif_step`` (one launch each way; the same leak, threshold, hard reset to 0 and fast-sigmoid surrogate, the reset's gradient
kept), trains the hand-written network from the same start next to it and prints the end points of both loss curves.
``--learn-beta`` (with ``--fused``) makes the leak a per-neuron ``torch.nn.Parameter`` that starts at 0.9 and is trained with the
weights: ``be.lif_step`` reads it on the device and hands back its gradient, summed over the batch.
``--synaptic`` (with ``--fused``) puts a synaptic current in front of the membrane: ``be.synaptic_lif_step`` in the recurrent loop,
its state the tuple ``(c, v)``, and the readout becomes a feed-forward layer of non-spiking leaky integrators — all ``T`` readout
currents through one ``be.synaptic_lif_sequence`` with ``v_th=inf``, the mean membrane as the logits.  ``--adapt`` (with
``--synaptic``) adds the adaptive threshold (``adapt=(rho, kappa)``, state ``(c, v, a)``).  ``--fused-recurrent`` (with ``--synaptic``)
runs the whole recurrent layer — all ``T`` steps, the recurrent product included — as ONE ``be.recurrent_lif_sequence`` call and
the readout product once over all ``T * batch`` spike rows.  ``--learn-neuron`` (with ``--synaptic``) makes ``syn_decay``, ``beta``,
``v_th`` and, with ``--adapt``, ``rho`` and ``kappa`` per-neuron ``torch.nn.Parameter``s that start at the constants and are trained with
the weights: ``be.parametric_synaptic_lif_step`` reads them on the device and hands back their gradients — or, together with
``--fused-recurrent``, ``be.parametric_recurrent_lif_sequence`` does, still as one launch each way.  ``--rec-delays DEPTH`` (with
``--fused-recurrent``, without ``--learn-neuron``) gives every recurrent synapse a conduction delay drawn uniformly from ``[0, DEPTH)``
steps: ``rec.with_delays(delays, DEPTH)`` goes into the same ``be.recurrent_lif_sequence`` call, and the trained leaf is the
``DelayedCSR``'s ``stacked.data``.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


class SpikeFn(torch.autograd.Function):
    """Heaviside forward, fast-sigmoid surrogate backward: d(spike)/dV = 1 / (1 + 10 |V - 1|)^2."""

    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return (v > 1.0).to(v.dtype)

    @staticmethod
    def backward(ctx, g):
        v, = ctx.saved_tensors
        return g / (1.0 + 10.0 * (v - 1.0).abs()) ** 2


def train(args, fused=False, learn_beta=False, synaptic=False, adapt=False, fused_recurrent=False, learn_neuron=False,
          rec_delays=0):
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    torch.manual_seed(0)

    n, n_conn, n_out, batch = args.n, 50, 2, 32
    # sparse recurrent projection, CSR rows = presynaptic neurons
    indptr = torch.arange(n + 1, dtype=torch.int32, device=dev) * n_conn
    indices = torch.tensor(rng.integers(0, n, n * n_conn).astype(np.int32), device=dev)
    w_rec = torch.nn.Parameter(torch.tensor(rng.normal(0.0, 0.05, n * n_conn), dtype=torch.float32, device=dev))
    rec = be.CSR((w_rec, indices, indptr), shape=(n, n))
    if rec_delays:                                                      # a delay per synapse: the stacked weights are the leaf
        delays = torch.tensor(rng.integers(0, rec_delays, n * n_conn).astype(np.int32), device=dev)
        rec = be.CSR((w_rec.detach(), indices, indptr), shape=(n, n)).with_delays(delays, rec_delays)
        w_rec = rec.stacked.data.requires_grad_()
    w_out = torch.nn.Parameter(torch.tensor(rng.normal(0.0, 0.05, (n, n_out)), dtype=torch.float32, device=dev))
    readout = be.Dense(w_out)
    # two input patterns: each drives a different random half of the neurons
    patterns = torch.tensor(rng.random((2, n)) < 0.5, dtype=torch.float32, device=dev) * 0.35
    # the leak: one constant, or (--learn-beta) one learnable value per neuron, read by the kernel from device memory
    beta = torch.nn.Parameter(torch.full((n,), 0.9, device=dev)) if learn_beta else 0.9
    syn_decay = 0.8
    # --learn-neuron: the synaptic neuron's constants as per-neuron Parameters (the readout layer keeps the numbers)
    start = dict(syn_decay=syn_decay, beta=0.9, v_th=1.0, **(dict(rho=0.95, kappa=0.3) if adapt else {}))
    neuron = {k: torch.nn.Parameter(torch.full((n,), c, device=dev)) for k, c in start.items()} if learn_neuron else {}
    limits = dict(syn_decay=(0.0, 1.0), beta=(0.0, 1.0), v_th=(0.1, 10.0), rho=(0.0, 1.0), kappa=(0.0, 10.0))
    opt = torch.optim.SGD([w_rec, w_out] + ([beta] if learn_beta else []) + list(neuron.values()), lr=0.05)

    def trial(labels):
        drive = patterns[labels]                                        # [batch, n]
        v = torch.zeros(batch, n, device=dev)
        s = torch.zeros(batch, n, device=dev)
        acc = torch.zeros(batch, n_out, device=dev)
        if fused_recurrent:                                             # the recurrent layer as one launch each way
            x = ((1.0 - syn_decay) * drive).expand(args.T, batch, n)
            if learn_neuron:                                            # the same call with the neuron's Parameters
                q = neuron
                s_all, _ = be.parametric_recurrent_lif_sequence(x, rec, syn_decay=q['syn_decay'], beta=q['beta'], v_th=q['v_th'],
                                                                adapt=(q['rho'], q['kappa']) if adapt else None)
            else:
                s_all, _ = be.recurrent_lif_sequence(x, rec, syn_decay=syn_decay, beta=0.9, v_th=1.0,
                                                     adapt=(0.95, 0.3) if adapt else None)
            out = (be.BinaryArray(s_all.reshape(args.T * batch, n)) @ readout).reshape(args.T, batch, n_out)
            _, v_seq, _ = be.synaptic_lif_sequence(out, syn_decay=syn_decay, beta=0.9, v_th=float('inf'), return_v=True)
            return v_seq.mean(0) * (1.0 - syn_decay) * (1.0 - 0.9)
        if synaptic:                                                    # current, membrane (and spike trace): one launch per step
            state = tuple(torch.zeros(batch, n, device=dev) for _ in range(3 if adapt else 2))
            out = []
            for _ in range(args.T):                                     # the drive scaled so that the filtered current settles at it
                if learn_neuron:
                    q = neuron
                    s, state = be.parametric_synaptic_lif_step(state, (1.0 - syn_decay) * drive + be.BinaryArray(s) @ rec,
                                                               syn_decay=q['syn_decay'], beta=q['beta'], v_th=q['v_th'],
                                                               adapt=(q['rho'], q['kappa']) if adapt else None)
                    out.append(be.BinaryArray(s) @ readout)
                    continue
                s, state = be.synaptic_lif_step(state, (1.0 - syn_decay) * drive + be.BinaryArray(s) @ rec, syn_decay=syn_decay,
                                                beta=0.9, v_th=1.0, adapt=(0.95, 0.3) if adapt else None)
                out.append(be.BinaryArray(s) @ readout)
            # the readout layer is feed-forward: its whole input sequence in one launch, leaky integrators that never spike
            _, v_seq, _ = be.synaptic_lif_sequence(torch.stack(out), syn_decay=syn_decay, beta=0.9, v_th=float('inf'), return_v=True)
            return v_seq.mean(0) * (1.0 - syn_decay) * (1.0 - 0.9)
        for _ in range(args.T):
            if fused:                                                   # the same step as one launch: v is the membrane after the reset
                s, v = be.lif_step(v, drive + be.BinaryArray(s) @ rec, beta=beta, v_th=1.0, v_reset=0.0, alpha=10.0)
            else:
                v = 0.9 * v * (1.0 - s) + drive + be.BinaryArray(s) @ rec   # reset, leak, input, recurrent events
                s = SpikeFn.apply(v)
            acc = acc + be.BinaryArray(s) @ readout
        return acc / args.T

    t0 = time.perf_counter()
    losses = []
    for step in range(args.steps):
        labels = torch.tensor(rng.integers(0, 2, batch), device=dev)
        logits = trial(labels)
        loss = torch.nn.functional.cross_entropy(logits * 4.0, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if learn_beta:
            beta.data.clamp_(0.0, 1.0)
        for k, t in neuron.items():
            t.data.clamp_(*limits[k])
        losses.append(loss.item())
        if step % 10 == 0 or step == args.steps - 1:
            print(f"step {step:3d}  loss {losses[-1]:.4f}")
    head, tail = np.mean(losses[:5]), np.mean(losses[-5:])
    print(f"loss {head:.4f} -> {tail:.4f} in {time.perf_counter() - t0:.1f} s ({'falling' if tail < head else 'NOT falling'})")
    if learn_beta:
        b = beta.detach()
        print(f"beta: started at 0.9 everywhere, now {b.min().item():.4f} .. {b.max().item():.4f} (mean {b.mean().item():.4f})")
    for k, t in neuron.items():
        t = t.detach()
        print(f"{k}: started at {start[k]} everywhere, now {t.min().item():.4f} .. {t.max().item():.4f} (mean {t.mean().item():.4f})")
    return head, tail


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--n', type=int, default=2000, help='recurrent neurons')
    ap.add_argument('--T', type=int, default=25, help='time steps per trial')
    ap.add_argument('--fused', action='store_true', help='the neuron as one launch (be.lif_step) instead of elementwise torch ops')
    ap.add_argument('--learn-beta', action='store_true', help='with --fused: the leak as a learnable per-neuron Parameter')
    ap.add_argument('--synaptic', action='store_true',
                    help='with --fused: a synaptic current in front of the membrane (be.synaptic_lif_step) and a leaky-integrator readout')
    ap.add_argument('--adapt', action='store_true', help='with --synaptic: an adaptive threshold (adapt=(rho, kappa))')
    ap.add_argument('--fused-recurrent', action='store_true',
                    help='with --synaptic: the whole recurrent layer as one launch (be.recurrent_lif_sequence)')
    ap.add_argument('--rec-delays', type=int, default=0, metavar='DEPTH',
                    help='with --fused-recurrent: a conduction delay per recurrent synapse, uniform in [0, DEPTH) steps '
                         '(be.recurrent_lif_sequence on rec.with_delays(delays, DEPTH))')
    ap.add_argument('--learn-neuron', action='store_true',
                    help='with --synaptic: syn_decay, beta, v_th (and rho, kappa) as learnable per-neuron Parameters '
                         '(be.parametric_synaptic_lif_step; with --fused-recurrent be.parametric_recurrent_lif_sequence)')
    args = ap.parse_args()
    if args.learn_neuron and not args.synaptic:
        ap.error('--learn-neuron needs --fused --synaptic')
    if args.fused_recurrent and not args.synaptic:
        ap.error('--fused-recurrent needs --fused --synaptic (it is the synaptic neuron with the recurrence inside)')
    if args.rec_delays and (not args.fused_recurrent or args.learn_neuron):
        ap.error('--rec-delays needs --fused-recurrent and no --learn-neuron (learnable neuron parameters with delays are not built)')
    if not 0 <= args.rec_delays <= 256:
        ap.error('--rec-delays takes a depth of 1 .. 256 (0: no delays)')
    if args.learn_beta and not args.fused:
        ap.error('--learn-beta needs --fused (the hand-written neuron keeps its constant leak)')
    if args.synaptic and not args.fused:
        ap.error('--synaptic needs --fused (the hand-written neuron has no synaptic current)')
    if args.adapt and not args.synaptic:
        ap.error('--adapt needs --synaptic')
    if args.synaptic and args.learn_beta:
        ap.error('--learn-beta is for be.lif_step: the synaptic neuron has --learn-neuron')
    if not args.fused:
        train(args)
        return 0
    if args.synaptic:
        print('fused neuron (' + ('be.parametric_recurrent_lif_sequence, learnable per-neuron parameters'
                                  if args.fused_recurrent and args.learn_neuron else
                                  f'be.recurrent_lif_sequence, synaptic delays below {args.rec_delays} steps' if args.rec_delays else
                                  'be.recurrent_lif_sequence' if args.fused_recurrent else
                                  'be.parametric_synaptic_lif_step, learnable per-neuron parameters' if args.learn_neuron else
                                  'be.synaptic_lif_step') +
              (', adaptive threshold' if args.adapt else '') + '; be.synaptic_lif_sequence readout):')
    else:
        print('fused neuron (be.lif_step' + (', learnable per-neuron beta):' if args.learn_beta else '):'))
    fused = train(args, fused=True, learn_beta=args.learn_beta, synaptic=args.synaptic, adapt=args.adapt,
                  fused_recurrent=args.fused_recurrent, learn_neuron=args.learn_neuron, rec_delays=args.rec_delays)
    print('hand-written neuron (torch elementwise ops), same start:')
    plain = train(args)
    print(f"end points: fused {fused[0]:.4f} -> {fused[1]:.4f}, hand-written {plain[0]:.4f} -> {plain[1]:.4f}")
    return 0 if fused[1] < fused[0] else 1


if __name__ == '__main__':
    sys.exit(main())
