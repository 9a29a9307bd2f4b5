"""Surrogate-gradient training through the event-driven products.

A small recurrent spiking network: leaky integrate-and-fire neurons driven by a fixed input current and a sparse recurrent
projection (a ``CSR`` container whose weights are a ``torch.nn.Parameter``), read out through a ``Dense`` projection.  The
spike function is a Heaviside step in the forward pass and a fast-sigmoid derivative in the backward pass (the surrogate);
``BinaryArray(spikes) @ csr`` and ``BinaryArray(spikes) @ dense`` are differentiated by ``brainevent_amd``: straight-through
for the spikes, per-synapse for the weights.  The task is synthetic and generated here: each of two input patterns must drive
its own readout unit.  Trained with ``torch.optim.SGD``; the loss falls.

    python examples/surrogate_csr.py [--steps 60] [--fused [--learn-beta]]

``--fused`` replaces the hand-written neuron (about six elementwise launches forwards and twice that backwards per time step) by
``be.lif_step`` (one launch each way; the same leak, threshold, hard reset to 0 and fast-sigmoid surrogate, the reset's gradient
kept), trains the hand-written network from the same start next to it and prints the end points of both loss curves.
``--learn-beta`` (with ``--fused``) makes the leak a per-neuron ``torch.nn.Parameter`` that starts at 0.9 and is trained with the
weights: ``be.lif_step`` reads it on the device and hands back its gradient, summed over the batch.
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


def train(args, fused=False, learn_beta=False):
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    torch.manual_seed(0)

    n, n_conn, n_out, batch = args.n, 50, 2, 32
    # sparse recurrent projection, CSR rows = presynaptic neurons
    indptr = torch.arange(n + 1, dtype=torch.int32, device=dev) * n_conn
    indices = torch.tensor(rng.integers(0, n, n * n_conn).astype(np.int32), device=dev)
    w_rec = torch.nn.Parameter(torch.tensor(rng.normal(0.0, 0.05, n * n_conn), dtype=torch.float32, device=dev))
    rec = be.CSR((w_rec, indices, indptr), shape=(n, n))
    w_out = torch.nn.Parameter(torch.tensor(rng.normal(0.0, 0.05, (n, n_out)), dtype=torch.float32, device=dev))
    readout = be.Dense(w_out)
    # two input patterns: each drives a different random half of the neurons
    patterns = torch.tensor(rng.random((2, n)) < 0.5, dtype=torch.float32, device=dev) * 0.35
    # the leak: one constant, or (--learn-beta) one learnable value per neuron, read by the kernel from device memory
    beta = torch.nn.Parameter(torch.full((n,), 0.9, device=dev)) if learn_beta else 0.9
    opt = torch.optim.SGD([w_rec, w_out] + ([beta] if learn_beta else []), lr=0.05)

    def trial(labels):
        drive = patterns[labels]                                        # [batch, n]
        v = torch.zeros(batch, n, device=dev)
        s = torch.zeros(batch, n, device=dev)
        acc = torch.zeros(batch, n_out, device=dev)
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
        losses.append(loss.item())
        if step % 10 == 0 or step == args.steps - 1:
            print(f"step {step:3d}  loss {losses[-1]:.4f}")
    head, tail = np.mean(losses[:5]), np.mean(losses[-5:])
    print(f"loss {head:.4f} -> {tail:.4f} in {time.perf_counter() - t0:.1f} s ({'falling' if tail < head else 'NOT falling'})")
    if learn_beta:
        b = beta.detach()
        print(f"beta: started at 0.9 everywhere, now {b.min().item():.4f} .. {b.max().item():.4f} (mean {b.mean().item():.4f})")
    return head, tail


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--n', type=int, default=2000, help='recurrent neurons')
    ap.add_argument('--T', type=int, default=25, help='time steps per trial')
    ap.add_argument('--fused', action='store_true', help='the neuron as one launch (be.lif_step) instead of elementwise torch ops')
    ap.add_argument('--learn-beta', action='store_true', help='with --fused: the leak as a learnable per-neuron Parameter')
    args = ap.parse_args()
    if args.learn_beta and not args.fused:
        ap.error('--learn-beta needs --fused (the hand-written neuron keeps its constant leak)')
    if not args.fused:
        train(args)
        return 0
    print('fused neuron (be.lif_step' + (', learnable per-neuron beta):' if args.learn_beta else '):'))
    fused = train(args, fused=True, learn_beta=args.learn_beta)
    print('hand-written neuron (torch elementwise ops), same start:')
    plain = train(args)
    print(f"end points: fused {fused[0]:.4f} -> {fused[1]:.4f}, hand-written {plain[0]:.4f} -> {plain[1]:.4f}")
    return 0 if fused[1] < fused[0] else 1


if __name__ == '__main__':
    sys.exit(main())
