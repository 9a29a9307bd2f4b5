"""What the fused recurrent layer costs with a DENSE recurrence (csrc/be_neuron_sg_rec_dense.hip) next to the two
other routes to the same function.

One training step = forward + ``torch.autograd.grad`` in ``x`` and the weights over ``--T`` 25 steps of ``--batch`` 32 samples, the
adaptive neuron, hard reset to 0, fast sigmoid, ``W [N, N]`` drawn from N(0, ``--w-scale`` / sqrt(N)) and rounded to multiples of
2**-12 (every sum of a column's entries is then exact in f32 in any order, so the three sides have to produce THE SAME spikes).  For
each ``N`` (default 256 and 1024) three sides take turns inside one loop on the same inputs, ``scale_exp`` given:

  ``dense``          ``be.recurrent_lif_sequence(x, be.Dense(W))``;
  ``stored_csr``     the same call on the ``be.CSR`` that stores all ``N * N`` entries of ``W``;
  ``step_loop``      per step one ``BinaryArray(s) @ be.Dense(W)`` and one ``be.synaptic_lif_step``.

HIP-event medians and quartiles of ``--reps`` turns, the order shuffled (seeded) for every turn.  Before any time is printed the
script asserts that the three sides' spikes are equal and that the gradients of ``dense`` and ``stored_csr`` — the same products,
summed in f32 in two different orders — agree within 1e-4 of the gradient's scale (tools/exp_lif_rec_sg.py's criterion).  Prints one
JSON line and, with ``--out``, writes it.

    python tools/exp_lif_rec_dense_sg.py [--T 25] [--batch 32] [--sizes 256,1024] [--reps 21] [--out profiles/lif_rec_dense_sg_line.json]
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
    ap.add_argument('--sizes', default='256,1024')
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
    names = ['dense', 'stored_csr', 'step_loop']
    res = {'what': 'forward + backward (gradients of x and the weights) of T steps of a recurrent adaptive LIF layer with a dense '
                   '[N, N] recurrence: be.recurrent_lif_sequence on be.Dense(W), on the CSR storing all N * N entries of W, and the '
                   'per-step loop of BinaryArray(s) @ Dense + be.synaptic_lif_step; alternating in one loop, the order shuffled for '
                   'every turn',
           'device': torch.cuda.get_device_name(0), 'T': T, 'batch': B, 'w_scale': args.w_scale, 'reps': args.reps, 'sizes': {}}
    for n in (int(s) for s in args.sizes.split(',')):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        w0 = torch.randn((n, n), device=dev, generator=g) * (args.w_scale / n ** 0.5)
        w0 = torch.round(w0 * 4096.0) / 4096.0
        w_d, w_c, w_l = (w0.clone().requires_grad_() for _ in range(3))
        cols = torch.arange(n, dtype=torch.int32, device=dev).repeat(n)
        indptr = torch.arange(n + 1, dtype=torch.int32, device=dev) * n
        dense, loop_dense = be.Dense(w_d), be.Dense(w_l)
        csr = be.CSR((w_c.reshape(-1), cols, indptr), shape=(n, n))
        x = (torch.randn((T, B, n), device=dev, generator=g) * 0.25 + 0.12).requires_grad_()
        g_s = torch.randn((T, B, n), device=dev, generator=g)
        e = fixed_point_exponent(w0.reshape(-1), cols, n)
        outs = {}

        def fused(name, rec, w):
            def run():
                s_all, _ = be.recurrent_lif_sequence(x, rec, scale_exp=e, **kw)
                outs[name] = (s_all,) + torch.autograd.grad([s_all], [x, w], [g_s])
            return run

        def step_loop():
            state = tuple(torch.zeros(B, n, device=dev) for _ in range(3))
            s, ss = torch.zeros(B, n, device=dev), []
            for t in range(T):
                s, state = be.synaptic_lif_step(state, x[t] + be.BinaryArray(s) @ loop_dense, **kw)
                ss.append(s)
            s_all = torch.stack(ss)
            outs['step_loop'] = (s_all,) + torch.autograd.grad([s_all], [x, w_l], [g_s])

        times = timed_turns([fused('dense', dense, w_d), fused('stored_csr', csr, w_c), step_loop], args.reps)
        torch.cuda.synchronize()
        outs = {nm: tuple(t.detach().reshape(-1) for t in ts) for nm, ts in outs.items()}
        assert torch.equal(outs['dense'][0], outs['stored_csr'][0]), f'N = {n}: dense and stored_csr spikes differ'
        assert torch.equal(outs['dense'][0], outs['step_loop'][0]), f'N = {n}: dense and step_loop spikes differ'
        scale = [max(float(t.abs().max()), 1.0) for t in outs['stored_csr'][1:]]
        worst = [float((a - b).abs().max()) / sc for a, b, sc in zip(outs['dense'][1:], outs['stored_csr'][1:], scale)]
        assert all(d <= 1e-4 for d in worst), f'N = {n}: dense and stored_csr gradients differ by {worst} of their scale'
        block = {'scale_exp': int(e), 'spike_rate': round(float(outs['dense'][0].mean()), 4),
                 'worst_gradient_difference_over_scale': {k: float(f'{d:.3g}') for k, d in zip(('x', 'w'), worst)}}
        for nm, tt in zip(names, times):
            block[nm] = {'ms': tt}
        block['stored_csr_over_dense'] = round(block['stored_csr']['ms']['median'] / block['dense']['ms']['median'], 2)
        block['step_loop_over_dense'] = round(block['step_loop']['ms']['median'] / block['dense']['ms']['median'], 2)
        res['sizes'][str(n)] = block
        del x, w_d, w_c, w_l, dense, csr, loop_dense, g_s, outs
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
