"""What two-byte weights buy the fused recurrent layer with a dense recurrence (csrc/be_neuron_sg_rec_dense_half.hip, DESIGN.md
§2.30) next to the f32 layer (csrc/be_neuron_sg_rec_dense.hip, §2.29).

One training step = forward + ``torch.autograd.grad`` in ``x`` and the weights over ``--T`` 25 steps of ``--batch`` 32 samples, the
adaptive neuron, hard reset to 0, fast sigmoid, ``W [N, N]`` drawn from N(0, ``--w-scale`` / sqrt(N)) — tools/exp_lif_rec_dense_sg.py's
distribution and inputs.  For each ``N`` (default 256, 1024 and 4096) three sides take turns inside one loop on the same inputs,
``scale_exp`` given:

  ``f32``     ``be.recurrent_lif_sequence(x, be.Dense(W))``;
  ``f16``     the same call on ``be.Dense(W.half())``;
  ``bf16``    the same call on ``be.Dense(W.bfloat16())``.

Each side has the weights its dtype can hold, so the spikes of the three differ (their rates are printed); before any time is
printed the script asserts that each half side's spikes equal the f32 layer's on its up-converted matrix and that its gradients agree
with that call's within 1e-4 of the gradient's scale (``x``; two summation orders) and one rounding of the dtype (the weights).  A
second loop times the forward launch and the backward launch of each side alone (``_forward`` / ``_backward`` on the Dense adapter: no
weight gradient, no autograd).  HIP-event medians and quartiles of ``--reps`` turns, the order shuffled (seeded) for every turn.
Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_lif_rec_dense_half.py [--T 25] [--batch 32] [--sizes 256,1024,4096] [--reps 21] [--out profiles/lif_rec_dense_half_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd import _neuron_rec_sg as R  # noqa: E402
from brainevent_amd._csr import fixed_point_exponent  # noqa: E402
from brainevent_amd._neuron_syn_sg import _Params  # noqa: E402
from exp_lif_syn_sg import timed_turns  # noqa: E402

SYN_DECAY, BETA, V_TH, RHO, KAPPA, ALPHA = 0.8, 0.9, 1.0, 0.95, 0.3, 10.0
SIDES = {'f32': (torch.float32, 0.0), 'f16': (torch.float16, 2.0 ** -11), 'bf16': (torch.bfloat16, 2.0 ** -8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=25)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--sizes', default='256,1024,4096')
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
    p = _Params('exp', SYN_DECAY, BETA, V_TH, 0.0, 'hard', 'fast_sigmoid', ALPHA, False, (RHO, KAPPA))
    names = list(SIDES)
    res = {'what': 'forward + backward (gradients of x and the weights) of T steps of a recurrent adaptive LIF layer with a dense '
                   '[N, N] recurrence, be.recurrent_lif_sequence on be.Dense(W) with W in f32, f16 and bf16; alternating in one loop, '
                   'the order shuffled for every turn; then the forward and the backward launch of each side alone',
           'device': torch.cuda.get_device_name(0), 'T': T, 'batch': B, 'w_scale': args.w_scale, 'reps': args.reps, 'sizes': {}}
    for n in (int(s) for s in args.sizes.split(',')):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        w0 = torch.randn((n, n), device=dev, generator=g) * (args.w_scale / n ** 0.5)
        w0 = torch.round(w0 * 4096.0) / 4096.0
        ws = {nm: w0.to(dt).requires_grad_() for nm, (dt, _) in SIDES.items()}
        x = (torch.randn((T, B, n), device=dev, generator=g) * 0.25 + 0.12).requires_grad_()
        g_s = torch.randn((T, B, n), device=dev, generator=g)
        cols = torch.arange(n, dtype=torch.int32, device=dev).repeat(n)
        e = fixed_point_exponent(w0.reshape(-1), cols, n) - 1          # (one bit of room: a side's rounded weights may sum higher)
        del cols
        outs = {}

        def step(name, w):
            rec = be.Dense(w)

            def run():
                s_all, _ = be.recurrent_lif_sequence(x, rec, scale_exp=e, **kw)
                outs[name] = (s_all,) + torch.autograd.grad([s_all], [x, w], [g_s])
            return run

        times = timed_turns([step(nm, ws[nm]) for nm in names], args.reps)
        torch.cuda.synchronize()
        block = {'scale_exp': int(e)}
        for nm, tt in zip(names, times):
            block[nm] = {'ms': tt, 'spike_rate': round(float(outs[nm][0].mean()), 4)}
        for nm in names[1:]:                                           # a half side against the f32 layer on its up-converted matrix
            up = ws[nm].detach().float().requires_grad_()
            s_all, _ = be.recurrent_lif_sequence(x, be.Dense(up), scale_exp=e, **kw)
            g_x, g_w = torch.autograd.grad([s_all], [x, up], [g_s])
            assert torch.equal(s_all, outs[nm][0]), f'N = {n}: {nm} spikes differ from the f32 layer on the up-converted matrix'
            d_x = float((g_x - outs[nm][1]).abs().max()) / max(float(g_x.abs().max()), 1.0)
            d_w = float((g_w - outs[nm][2].float()).abs().max()) / max(float(g_w.abs().max()), 1.0)
            assert d_x <= 1e-4 and d_w <= 1e-4 + SIDES[nm][1], f'N = {n}: {nm} gradients differ by {d_x}, {d_w} of their scale'
            block[nm]['worst_gradient_difference_over_scale'] = {'x': float(f'{d_x:.3g}'), 'w': float(f'{d_w:.3g}')}
            del up, s_all, g_x, g_w
        outs.clear()

        # the two launches alone
        xd, saved = x.detach(), {}
        recs = {nm: R._recurrence('exp', be.Dense(ws[nm].detach()), n) for nm in names}

        def forward(nm):
            def run():
                saved[nm] = R._forward(xd, recs[nm], None, None, None, None, T, B, n, p, e, False, True)[2:4]
            return run

        def backward(nm):
            def run():
                h, th = saved[nm]
                R._backward(h, th, recs[nm], g_s, None, [None] * 3, T, B, n, p, [False] * 4)
            return run

        for nm in names:
            forward(nm)()
        launches = timed_turns([forward(nm) for nm in names] + [backward(nm) for nm in names], args.reps)
        for k, nm in enumerate(names):
            block[nm]['forward_ms'], block[nm]['backward_ms'] = launches[k], launches[len(names) + k]
        for nm in names[1:]:
            block[f'f32_over_{nm}'] = {what: round(block['f32'][what]['median'] / block[nm][what]['median'], 2)
                                       for what in ('ms', 'forward_ms', 'backward_ms')}
        res['sizes'][str(n)] = block
        del x, xd, ws, recs, saved, g_s
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
