"""What the synaptic current and the adaptive threshold cost in the fused differentiable neuron (csrc/be_neuron_sg.hip,
DESIGN.md §2.21), next to the one-state neuron of §2.19 and to the only other route to them.

One training step = forward + ``torch.autograd.grad`` over ``--T`` 25 steps, hard reset to 0, fast sigmoid.  For each shape
(default ``[32, 2000]`` and ``[32, 65536]``) four sides take turns inside one loop on the same inputs:

  ``lif``         ``be.lif_sequence`` (§2.19's kernels, untouched), the floor: gradients of x, v0;
  ``synaptic``    ``be.synaptic_lif_sequence`` without adaptation: gradients of x, c0, v0;
  ``adaptive``    ``be.synaptic_lif_sequence`` with ``adapt=(rho, kappa)``: gradients of x, c0, v0, a0;
  ``torch_loop``  the same adaptive neuron composed from torch elementwise ops — what a user has without the kernels.

HIP-event medians and quartiles of ``--reps`` turns, the order shuffled (seeded) for every turn (DESIGN.md §2.20 records why).  A
shape counts as measured only if ``adaptive`` and ``torch_loop`` agree: spikes equal, every gradient within 1e-5 of the
yardstick's scale, as tools/exp_lif_sg.py asks.  Recorded with the times: the [T, N] floats a training step moves — 6 for ``lif``
and ``synaptic`` (x, s, h written and h, g_s read, g_x written), 8 for ``adaptive`` (th written and read on top) — and the TB/s
they come to.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_lif_syn_sg.py [--T 25] [--reps 21] [--out profiles/lif_syn_sg_line.json]
"""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402

SYN_DECAY, BETA, V_TH, RHO, KAPPA, ALPHA = 0.8, 0.9, 1.0, 0.95, 0.3, 10.0


def timed_turns(fns, reps):
    """``{median, q1, q3}`` in ms of each function: ``reps`` turns, every function once per turn between two HIP events, in an order
    shuffled anew (seeded) for every turn, so that every side follows every other side about equally often."""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    order, shuffle = list(range(len(fns))), random.Random(0).shuffle
    for _ in range(reps):
        shuffle(order)
        for i in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fns[i]()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    out = []
    for t in ts:
        t = sorted(t)
        out.append({'median': round(t[len(t) // 2], 4), 'q1': round(t[len(t) // 4], 4), 'q3': round(t[(3 * len(t)) // 4], 4)})
    return out


class SpikeFn(torch.autograd.Function):
    """Heaviside of ``h - th`` forwards, the fast sigmoid's derivative backwards — to the membrane and, negated, to the threshold."""

    @staticmethod
    def forward(ctx, h, th):
        ctx.save_for_backward(h, th)
        return (h >= th).to(h.dtype)

    @staticmethod
    def backward(ctx, g):
        h, th = ctx.saved_tensors
        gs = g / (1.0 + ALPHA * (h - th).abs()) ** 2
        return gs, -gs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=25)
    ap.add_argument('--shapes', default='32x2000,32x65536')
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error('--reps must be at least 9')
    dev = torch.device('cuda')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    T = args.T
    kw = dict(v_th=V_TH, v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=ALPHA)
    names = ['lif', 'synaptic', 'adaptive', 'torch_loop']
    floats_per_slot_step = {'lif': 6, 'synaptic': 6, 'adaptive': 8}
    res = {'what': 'forward + backward of T LIF steps: be.lif_sequence, be.synaptic_lif_sequence without and with the adaptive '
                   'threshold, and the torch elementwise composition of the adaptive neuron; alternating in one loop, the order '
                   'shuffled for every turn',
           'device': torch.cuda.get_device_name(0), 'T': T, 'reps': args.reps, 'shapes': {}}
    for shape in (tuple(int(d) for d in s.split('x')) for s in args.shapes.split(',')):
        randn = lambda *lead: torch.randn(tuple(lead) + shape, device=dev, generator=g)
        x = (randn(T) * 0.25 + 0.12).requires_grad_()
        c0 = (randn() * 0.3 + 0.2).requires_grad_()
        v0 = (randn() * 0.5 + 0.3).requires_grad_()
        a0 = (randn() * 0.5 + 0.5).abs().requires_grad_()
        g_s, g_c, g_v, g_a = randn(T), randn(), randn(), randn()
        outs = {}

        def lif():
            s_all, v_last = be.lif_sequence(x, v0, beta=BETA, **kw)
            outs['lif'] = (s_all,) + torch.autograd.grad([s_all, v_last], [x, v0], [g_s, g_v])

        def synaptic():
            s_all, (c, v) = be.synaptic_lif_sequence(x, (c0, v0), syn_decay=SYN_DECAY, beta=BETA, **kw)
            outs['synaptic'] = (s_all,) + torch.autograd.grad([s_all, c, v], [x, c0, v0], [g_s, g_c, g_v])

        def adaptive():
            s_all, (c, v, a) = be.synaptic_lif_sequence(x, (c0, v0, a0), syn_decay=SYN_DECAY, beta=BETA, adapt=(RHO, KAPPA), **kw)
            outs['adaptive'] = (s_all,) + torch.autograd.grad([s_all, c, v, a], [x, c0, v0, a0], [g_s, g_c, g_v, g_a])

        def torch_loop():
            c, v, a, ss = c0, v0, a0, []
            for t in range(T):
                c = SYN_DECAY * c + x[t]
                h = BETA * v + c
                s = SpikeFn.apply(h, V_TH + KAPPA * a)
                v = h * (1.0 - s)
                a = RHO * a + s
                ss.append(s)
            s_all = torch.stack(ss)
            outs['torch_loop'] = (s_all,) + torch.autograd.grad([s_all, c, v, a], [x, c0, v0, a0], [g_s, g_c, g_v, g_a])

        times = timed_turns([lif, synaptic, adaptive, torch_loop], args.reps)
        torch.cuda.synchronize()
        outs = {nm: tuple(t.detach() for t in ts) for nm, ts in outs.items()}
        ref, got = outs['torch_loop'], outs['adaptive']
        scale = [float(t.abs().max()) for t in ref]
        worst = [float((a - b).abs().max()) / max(sc, 1.0) for a, b, sc in zip(got[1:], ref[1:], scale[1:])]
        spikes_equal = bool(torch.equal(got[0], ref[0]))
        agree = spikes_equal and all(w <= 1e-5 for w in worst)
        slots = 1
        for d in shape:
            slots *= d
        block = {'measured': bool(agree), 'spikes_equal': spikes_equal,
                 'spike_rate': {nm: round(float(outs[nm][0].mean()), 4) for nm in names},
                 'worst_gradient_difference_over_scale': {k: float(f'{w:.3g}') for k, w in zip(('x', 'c0', 'v0', 'a0'), worst)}}
        med = {}
        for nm, tt in zip(names, times):
            block[nm] = {'ms': tt}
            med[nm] = tt['median']
            if nm in floats_per_slot_step:
                nbytes = floats_per_slot_step[nm] * T * slots * 4
                block[nm]['sequence_bytes_per_training_step'] = nbytes
                block[nm]['tb_per_s'] = round(nbytes / (tt['median'] * 1e-3) / 1e12, 3)
        block['synaptic_over_lif'] = round(med['synaptic'] / med['lif'], 3)
        block['adaptive_over_lif'] = round(med['adaptive'] / med['lif'], 3)
        block['bytes_ratio'] = {'synaptic_over_lif': 1.0, 'adaptive_over_lif': round(8 / 6, 4)}
        block['torch_loop_over_adaptive'] = round(med['torch_loop'] / med['adaptive'], 2)
        res['shapes']['x'.join(str(d) for d in shape)] = block
        del x, c0, v0, a0, g_s, g_c, g_v, g_a, outs
    res['all_measured'] = all(b['measured'] for b in res['shapes'].values())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0 if res['all_measured'] else 1


if __name__ == '__main__':
    sys.exit(main())
