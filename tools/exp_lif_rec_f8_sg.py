"""What FP8 weights buy the fused recurrent layer with a SPARSE recurrence (csrc/be_neuron_sg_rec_f8.hip) next to the
f32 layer (csrc/be_neuron_sg_rec.hip, §2.22) on the dequantised matrix.

``--T`` 25 steps of ``--batch`` 32 samples, the adaptive neuron, hard reset to 0, fast sigmoid; a CSR ``[N, N]`` with ``--row`` entries
in every row at random columns, weights N(0, ``--w-scale`` / sqrt(row)), quantised once by ``CSR.quantize_fp8(fmt)``.  For each ``N``
and format two sides take turns inside one loop on the same inputs:

  ``f8``     ``be.recurrent_lif_sequence(x, W8)``: this layer, no exponent;
  ``f32``    the same call on ``W8.tocsr()`` with ``scale_exp`` computed once beforehand (no host synchronisation in the timed call).

Two timings per side: the forward pass alone (no autograd), and forward + ``torch.autograd.grad`` in ``x``.  The two sides compute
the same sums only up to the f32 side's fixed-point rounding, so spikes may differ; the script reports the share of equal spikes.
HIP-event medians and quartiles of ``--reps`` turns, the order shuffled (seeded) for every turn.  Prints one JSON line and, with
``--out``, writes it.

    python tools/exp_lif_rec_f8_sg.py [--T 25] [--batch 32] [--sizes 1024,4096,8192] [--row 64] [--reps 21] [--out profiles/lif_rec_f8_line.json]
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
    ap.add_argument('--sizes', default='1024,4096,8192')
    ap.add_argument('--row', type=int, default=64)
    ap.add_argument('--formats', default='e4m3,e5m2')
    ap.add_argument('--w-scale', type=float, default=0.5)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error('--reps must be at least 9')
    dev = torch.device('cuda')
    T, B, row = args.T, args.batch, args.row
    kw = dict(syn_decay=SYN_DECAY, beta=BETA, v_th=V_TH, v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=ALPHA,
              adapt=(RHO, KAPPA))
    names = ('f8', 'f32')
    res = {'what': 'T steps of a recurrent adaptive LIF layer with a CSR [N, N] recurrence of `row` entries per row: '
                   'be.recurrent_lif_sequence on a Float8CSR (f8) and on W8.tocsr() with scale_exp given (f32); forward alone, and '
                   'forward + gradient of x; alternating in one loop, the order shuffled for every turn',
           'device': torch.cuda.get_device_name(0), 'T': T, 'batch': B, 'row': row, 'w_scale': args.w_scale, 'reps': args.reps,
           'sizes': {}}
    for n in (int(s) for s in args.sizes.split(',')):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        w0 = torch.randn(n * row, device=dev, generator=g) * (args.w_scale / row ** 0.5)
        indices = torch.randint(0, n, (n * row,), device=dev, generator=g, dtype=torch.int32)
        indptr = torch.arange(n + 1, device=dev, dtype=torch.int32) * row
        x = (torch.randn((T, B, n), device=dev, generator=g) * 0.25 + 0.12).requires_grad_()
        g_s = torch.randn((T, B, n), device=dev, generator=g)
        res['sizes'][str(n)] = {}
        for fmt in args.formats.split(','):
            w8 = be.CSR((w0, indices, indptr), shape=(n, n)).quantize_fp8(fmt)
            w32 = w8.tocsr()
            e = fixed_point_exponent(w32.data, w32.indices, n)
            outs = {}

            def fused(name, rec, grad, **extra):
                def run():
                    with torch.set_grad_enabled(grad):
                        s_all, _ = be.recurrent_lif_sequence(x if grad else x.detach(), rec, **extra, **kw)
                        outs[name] = (s_all,) + (torch.autograd.grad([s_all], [x], [g_s]) if grad else ())
                return run

            block = {'scale': w8.scale, 'f32_scale_exp': int(e)}
            for what, grad in (('forward_ms', False), ('forward_grad_x_ms', True)):
                times = timed_turns([fused('f8', w8, grad), fused('f32', w32, grad, scale_exp=e)], args.reps)
                torch.cuda.synchronize()
                for nm, tt in zip(names, times):
                    block.setdefault(nm, {})[what] = tt
            for nm in names:
                block[nm]['spike_rate'] = round(float(outs[nm][0].mean()), 4)
            assert torch.equal(outs['f8'][0][0], outs['f32'][0][0]), f'N = {n}, {fmt}: the first step differs (no recurrent input yet)'
            block['spikes_equal'] = round(float((outs['f8'][0] == outs['f32'][0]).float().mean()), 6)
            block['f32_over_f8'] = {what: round(block['f32'][what]['median'] / block['f8'][what]['median'], 2)
                                    for what in ('forward_ms', 'forward_grad_x_ms')}
            res['sizes'][str(n)][fmt] = block
            outs.clear()
            del w8, w32
        del x, g_s, w0, indices, indptr
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
