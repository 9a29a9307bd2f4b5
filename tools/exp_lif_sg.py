"""One training step (forward + backward) of the fused differentiable neuron against the same dynamics composed from torch
elementwise ops (csrc/be_neuron_sg.hip).

For each shape (default ``[32, 2000]`` and ``[32, 65536]``, ``--T`` 25 steps) three ways of running ``T`` steps of
``h = 0.9 v + x[t]; s = h >= 1; v = 0 where s else h`` and then ``torch.autograd.grad`` of ``(s, v_last)`` against ``(x, v0)``:

  ``torch_loop``   the hand-written neuron of ``examples/surrogate_csr.py`` (its ``SpikeFn``: Heaviside forwards, fast sigmoid
                   backwards; about six elementwise launches a step forwards, twice that backwards) — the yardstick;
  ``fused_loop``   ``be.lif_step`` inside the same recurrent loop (one launch a step each way);
  ``fused_seq``    ``be.lif_sequence`` (one launch each way for all ``T`` steps).

The three take turns inside one loop on the same inputs; HIP-event medians and quartiles of ``--reps`` turns.  A shape counts as
measured only if the three agree: spikes equal, gradients within 1e-5 of the yardstick's scale (the yardstick's own rounding:
torch's ``/`` and ``**``).  Recorded with the times: the bytes a training step of the sequence has to move (forwards x in, s and h
out; backwards h and g_s in, g_x out; the ``[N]`` vectors) and that figure over the median time.  Prints one JSON line and, with
``--out``, writes it.

    python tools/exp_lif_sg.py [--T 25] [--reps 21] [--out profiles/lif_sg_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


class SpikeFn(torch.autograd.Function):
    """The spike function of examples/surrogate_csr.py (with ``>=`` for its ``>``: a membrane exactly on the threshold, which some
    of the 5e7 values here are, then counts the same on both sides; the launches and their cost are the same)."""

    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return (v >= 1.0).to(v.dtype)

    @staticmethod
    def backward(ctx, g):
        v, = ctx.saved_tensors
        return g / (1.0 + 10.0 * (v - 1.0).abs()) ** 2


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
    kw = dict(beta=0.9, v_th=1.0, v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=10.0)
    res = {'what': 'forward + backward of T LIF steps: torch elementwise composition (yardstick), be.lif_step in the same loop, '
                   'be.lif_sequence; alternating in one loop', 'device': torch.cuda.get_device_name(0), 'T': T, 'reps': args.reps,
           'shapes': {}}
    for shape in (tuple(int(d) for d in s.split('x')) for s in args.shapes.split(',')):
        x = (torch.randn((T,) + shape, device=dev, generator=g) * 0.6 + 0.45).requires_grad_()
        v0 = (torch.randn(shape, device=dev, generator=g) * 0.5 + 0.3).requires_grad_()
        g_s = torch.randn((T,) + shape, device=dev, generator=g)
        g_v = torch.randn(shape, device=dev, generator=g)
        outs = {}

        def torch_loop():
            v, s, ss = v0, torch.zeros_like(v0), []
            for t in range(T):
                v = 0.9 * v * (1.0 - s) + x[t]
                s = SpikeFn.apply(v)
                ss.append(s)
            s_all, v_last = torch.stack(ss), v * (1.0 - s)
            outs['torch_loop'] = (s_all,) + torch.autograd.grad([s_all, v_last], [x, v0], [g_s, g_v])

        def fused_loop():
            v, ss = v0, []
            for t in range(T):
                s, v = be.lif_step(v, x[t], **kw)
                ss.append(s)
            s_all = torch.stack(ss)
            outs['fused_loop'] = (s_all,) + torch.autograd.grad([s_all, v], [x, v0], [g_s, g_v])

        def fused_seq():
            s_all, v_last = be.lif_sequence(x, v0, **kw)
            outs['fused_seq'] = (s_all,) + torch.autograd.grad([s_all, v_last], [x, v0], [g_s, g_v])

        names = ['torch_loop', 'fused_loop', 'fused_seq']
        times = timed_turns([torch_loop, fused_loop, fused_seq], args.reps)
        torch.cuda.synchronize()
        outs = {nm: tuple(t.detach() for t in ts) for nm, ts in outs.items()}
        ref = outs['torch_loop']
        scale = [float(t.abs().max()) for t in ref]
        agree = all(torch.equal(outs[nm][0], ref[0]) and
                    all(float((a - b).abs().max()) <= 1e-5 * max(sc, 1.0) for a, b, sc in zip(outs[nm][1:], ref[1:], scale[1:]))
                    for nm in names[1:])
        exact = all(torch.equal(a, b) for a, b in zip(outs['fused_loop'], outs['fused_seq']))
        n = 1
        for d in shape:
            n *= d
        step_bytes = (6 * T * n + 4 * n) * 4
        block = {'measured': bool(agree), 'fused_loop_equals_fused_seq_bitwise': bool(exact), 'spike_rate': round(float(ref[0].mean()), 4),
                 'sequence_bytes_per_training_step': step_bytes}
        for nm, tt in zip(names, times):
            block[nm] = {'ms': tt}
        block['fused_seq']['GBps'] = round(step_bytes / (times[2]['median'] * 1e-3) / 1e9, 1)
        for nm in names[1:]:
            block[f'torch_loop_over_{nm}'] = round(times[0]['median'] / block[nm]['ms']['median'], 2)
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
