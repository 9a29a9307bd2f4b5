"""What FP8 weights buy the fused recurrent layer with a dense recurrence (csrc/be_neuron_sg_rec_dense_f8.hip) next
to the bf16 layer (csrc/be_neuron_sg_rec_dense_half.hip, §2.30) and to the per-step loop.

``--T`` 25 steps of ``--batch`` 32 samples, the adaptive neuron, hard reset to 0, fast sigmoid, ``W [N, N]`` drawn from
N(0, ``--w-scale`` / sqrt(N)) — tools/exp_lif_rec_dense_sg.py's distribution and inputs — quantised once by ``quantize_fp8(W, fmt)``.
For each ``N`` (default 256, 1024 and 4096) and each format three sides take turns inside one loop on the same inputs:

  ``f8``      ``be.recurrent_lif_sequence(x, W8)``: this layer, no exponent;
  ``bf16``    the same call on ``be.Dense(W8.todense().bfloat16())`` with ``scale_exp`` given (the fastest dense path before FP8);
  ``loop``    ``synaptic_lif_step(state, x[t] + BinaryArray(s) @ W8)`` for every step (the spikes enter the product detached: the
              ``events @ W8`` products refuse an operand that requires grad, so the loop's gradient lacks the recurrent path).

Two timings per side: the forward pass alone (no autograd), and forward + ``torch.autograd.grad`` in ``x``.  The layer's spikes
equal the loop's wherever the loop's f32 sums are exact; with these weights they need not be (one flipped spike changes every later
step), so the script asserts the first step equal and reports the share of equal spikes.  HIP-event medians and quartiles of
``--reps`` turns, the order shuffled (seeded) for every turn.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_lif_rec_dense_f8_sg.py [--T 25] [--batch 32] [--sizes 256,1024,4096] [--reps 21] [--out profiles/lif_rec_dense_f8_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd._csr import fixed_point_exponent  # noqa: E402
from exp_lif_syn_sg import timed_turns  # noqa: E402

SYN_DECAY, BETA, V_TH, RHO, KAPPA, ALPHA = 0.8, 0.9, 1.0, 0.95, 0.3, 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=25)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--sizes', default='256,1024,4096')
    ap.add_argument('--formats', default='e4m3,e5m2')
    ap.add_argument('--w-scale', type=float, default=0.5)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error('--reps must be at least 9')
    dev = torch.device('cuda')
    T, B = args.T, args.batch
    kw = dict(syn_decay=SYN_DECAY, beta=BETA, v_th=V_TH, v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=ALPHA,
              adapt=(RHO, KAPPA))
    names = ('f8', 'bf16', 'loop')
    res = {'what': 'T steps of a recurrent adaptive LIF layer with a dense [N, N] recurrence: be.recurrent_lif_sequence on a Float8Dense '
                   '(f8), on be.Dense(W8.todense().bfloat16()) with scale_exp given (bf16), and the per-step loop BinaryArray(s) @ W8 + '
                   'synaptic_lif_step (loop); forward alone, and forward + gradient of x; alternating in one loop, the order shuffled '
                   'for every turn',
           'device': torch.cuda.get_device_name(0), 'T': T, 'batch': B, 'w_scale': args.w_scale, 'reps': args.reps, 'sizes': {}}
    for n in (int(s) for s in args.sizes.split(',')):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        w0 = torch.randn((n, n), device=dev, generator=g) * (args.w_scale / n ** 0.5)
        x = (torch.randn((T, B, n), device=dev, generator=g) * 0.25 + 0.12).requires_grad_()
        g_s = torch.randn((T, B, n), device=dev, generator=g)
        cols = torch.arange(n, dtype=torch.int32, device=dev).repeat(n)
        res['sizes'][str(n)] = {}
        for fmt in args.formats.split(','):
            w8 = be.quantize_fp8(w0, fmt)
            wb = be.Dense(w8.todense().bfloat16())
            e = fixed_point_exponent(wb.data.float().reshape(-1), cols, n)
            outs = {}

            def fused(name, rec, grad, **extra):
                def run():
                    with torch.set_grad_enabled(grad):
                        s_all, _ = be.recurrent_lif_sequence(x if grad else x.detach(), rec, **extra, **kw)
                        outs[name] = (s_all,) + (torch.autograd.grad([s_all], [x], [g_s]) if grad else ())
                return run

            def loop(grad):
                def run():
                    with torch.set_grad_enabled(grad):
                        xs = x if grad else x.detach()
                        state = tuple(torch.zeros((B, n), device=dev) for _ in range(3))
                        s, spikes = None, []
                        for t in range(T):
                            xin = xs[t] if s is None else xs[t] + be.BinaryArray(s.detach()) @ w8
                            s, state = be.synaptic_lif_step(state, xin, **kw)
                            spikes.append(s)
                        s_all = torch.stack(spikes)
                        outs['loop'] = (s_all,) + (torch.autograd.grad([s_all], [x], [g_s]) if grad else ())
                return run

            block = {'scale': w8.scale, 'bf16_scale_exp': int(e)}
            for what, grad in (('forward_ms', False), ('forward_grad_x_ms', True)):
                times = timed_turns([fused('f8', w8, grad), fused('bf16', wb, grad, scale_exp=e), loop(grad)], args.reps)
                torch.cuda.synchronize()
                for nm, tt in zip(names, times):
                    block.setdefault(nm, {})[what] = tt
            for nm in names:
                block[nm]['spike_rate'] = round(float(outs[nm][0].mean()), 4)
            same = float((outs['f8'][0] == outs['loop'][0]).float().mean())
            assert torch.equal(outs['f8'][0][0], outs['loop'][0][0]), f'N = {n}, {fmt}: the first step differs from the loop\'s'
            block['spikes_equal_to_the_loop'] = round(same, 6)
            for nm in names[1:]:
                block[f'{nm}_over_f8'] = {what: round(block[nm][what]['median'] / block['f8'][what]['median'], 2)
                                          for what in ('forward_ms', 'forward_grad_x_ms')}
            res['sizes'][str(n)][fmt] = block
            outs.clear()
            del w8, wb
        del x, g_s, cols, w0
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
