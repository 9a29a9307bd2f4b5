"""The price of learnable, per-neuron ``beta`` / ``v_th`` in the fused differentiable neuron (csrc/be_neuron_sg.hip,
DESIGN.md §2.20), and what the only other route to them costs.

One training step = forward + ``torch.autograd.grad`` over ``--T`` 25 steps, hard reset to 0, fast sigmoid.  For each shape
(default ``[32, 2000]`` and ``[32, 65536]``) four sides take turns inside one loop on the same inputs:

  ``float``       ``be.lif_sequence`` with ``beta`` / ``v_th`` as Python floats (§2.19's kernels, untouched): gradients of x, v0;
  ``per_neuron``  ``be.lif_sequence`` with ``beta [n]`` and ``v_th [n]`` learnable: gradients of x, v0, beta, v_th (forward, backward
                  with the two per-slot accumulators, two reduces over the batch rows);
  ``shared``      the same with ``beta [1]`` and ``v_th [1]`` learnable (the reduces are the two-stage tree over all slots);
  ``torch_loop``  the torch elementwise composition with the same learnable per-neuron parameters — what a user has without the
                  kernels.

HIP-event medians and quartiles of ``--reps`` turns, the order shuffled (seeded) for every turn.  A shape counts as measured only if ``per_neuron`` and ``torch_loop`` agree:
spikes equal, every gradient within 1e-5 of the yardstick's scale, as tools/exp_lif_sg.py asks.  Recorded with the times: the
bytes of a training step of the sequence and what the parameters add to them (their two ``[n]`` reads each way and the two ``[N]``
per-slot arrays written and read back).  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_lif_sg_param.py [--T 25] [--reps 21] [--out profiles/lif_sg_param_line.json]
"""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


def timed_turns(fns, reps):
    """``{median, q1, q3}`` in ms of each function: ``reps`` turns, every function once per turn between two HIP events, in an order
    shuffled anew (seeded) for every turn.  The side that runs right after the long torch loop pays for it — with a fixed order,
    and with one that only rotates (the predecessor stays the same), that side's median was 15–20 % higher and its quartiles three
    times as wide — so every side has to follow every other side about equally often."""
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
    """Heaviside of ``v - th`` forwards, the fast sigmoid's derivative backwards — to the membrane and, negated, to the threshold."""

    @staticmethod
    def forward(ctx, v, th):
        ctx.save_for_backward(v, th)
        return (v >= th).to(v.dtype)

    @staticmethod
    def backward(ctx, g):
        v, th = ctx.saved_tensors
        gs = g / (1.0 + 10.0 * (v - th).abs()) ** 2
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
    kw = dict(v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=10.0)
    names = ['float', 'per_neuron', 'shared', 'torch_loop']
    res = {'what': 'forward + backward of T LIF steps: be.lif_sequence with float beta / v_th, with learnable per-neuron ones, with '
                   'learnable shared ones, and the torch elementwise composition with the per-neuron ones; alternating in one loop, the '
                   'order shuffled for every turn',
           'device': torch.cuda.get_device_name(0), 'T': T, 'reps': args.reps, 'shapes': {}}
    for shape in (tuple(int(d) for d in s.split('x')) for s in args.shapes.split(',')):
        n = shape[-1]
        x = (torch.randn((T,) + shape, device=dev, generator=g) * 0.6 + 0.45).requires_grad_()
        v0 = (torch.randn(shape, device=dev, generator=g) * 0.5 + 0.3).requires_grad_()
        g_s = torch.randn((T,) + shape, device=dev, generator=g)
        g_v = torch.randn(shape, device=dev, generator=g)
        beta = (0.8 + 0.15 * torch.rand(n, device=dev, generator=g)).requires_grad_()
        v_th = (0.9 + 0.2 * torch.rand(n, device=dev, generator=g)).requires_grad_()
        beta1, v_th1 = torch.full((1,), 0.9, device=dev, requires_grad=True), torch.full((1,), 1.0, device=dev, requires_grad=True)
        outs = {}

        def float_seq():
            s_all, v_last = be.lif_sequence(x, v0, beta=0.9, v_th=1.0, **kw)
            outs['float'] = (s_all,) + torch.autograd.grad([s_all, v_last], [x, v0], [g_s, g_v])

        def per_neuron():
            s_all, v_last = be.lif_sequence(x, v0, beta=beta, v_th=v_th, **kw)
            outs['per_neuron'] = (s_all,) + torch.autograd.grad([s_all, v_last], [x, v0, beta, v_th], [g_s, g_v])

        def shared():
            s_all, v_last = be.lif_sequence(x, v0, beta=beta1, v_th=v_th1, **kw)
            outs['shared'] = (s_all,) + torch.autograd.grad([s_all, v_last], [x, v0, beta1, v_th1], [g_s, g_v])

        def torch_loop():
            v, s, ss = v0, torch.zeros_like(v0), []
            for t in range(T):
                v = beta * v * (1.0 - s) + x[t]
                s = SpikeFn.apply(v, v_th.expand_as(v))
                ss.append(s)
            s_all, v_last = torch.stack(ss), v * (1.0 - s)
            outs['torch_loop'] = (s_all,) + torch.autograd.grad([s_all, v_last], [x, v0, beta, v_th], [g_s, g_v])

        times = timed_turns([float_seq, per_neuron, shared, torch_loop], args.reps)
        torch.cuda.synchronize()
        outs = {nm: tuple(t.detach() for t in ts) for nm, ts in outs.items()}
        ref, got = outs['torch_loop'], outs['per_neuron']
        scale = [float(t.abs().max()) for t in ref]
        worst = [float((a - b).abs().max()) / max(sc, 1.0) for a, b, sc in zip(got[1:], ref[1:], scale[1:])]
        agree = torch.equal(got[0], ref[0]) and all(w <= 1e-5 for w in worst)
        slots = 1
        for d in shape:
            slots *= d
        step_bytes = (6 * T * slots + 4 * slots) * 4
        extra_bytes = (4 * n + 5 * slots) * 4      # beta, v_th read each way; v0 read backwards; two [N] slot arrays written and read
        block = {'measured': bool(agree), 'spike_rate': round(float(ref[0].mean()), 4),
                 'worst_gradient_difference_over_scale': {k: float(f'{w:.3g}') for k, w in zip(('x', 'v0', 'beta', 'v_th'), worst)},
                 'sequence_bytes_per_training_step': step_bytes, 'parameter_bytes_on_top': extra_bytes}
        for nm, tt in zip(names, times):
            block[nm] = {'ms': tt}
        med = {nm: tt['median'] for nm, tt in zip(names, times)}
        block['per_neuron_over_float'] = round(med['per_neuron'] / med['float'], 3)
        block['shared_over_float'] = round(med['shared'] / med['float'], 3)
        block['torch_loop_over_per_neuron'] = round(med['torch_loop'] / med['per_neuron'], 2)
        block['bytes_ratio'] = round((step_bytes + extra_bytes) / step_bytes, 4)
        res['shapes']['x'.join(str(d) for d in shape)] = block
        del x, v0, g_s, g_v, outs
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
