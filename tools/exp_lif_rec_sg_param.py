"""What per-neuron, learnable parameters cost inside the fused recurrent spiking layer (csrc/be_neuron_sg_rec.hip),
next to the layer with Python numbers and next to the only other route to a recurrent layer with learnable neurons: the per-step
loop.

One training step = forward + ``torch.autograd.grad`` over ``--T`` 25 steps of ``--batch`` 32 samples, the adaptive neuron, hard
reset to 0, fast sigmoid, a CSR recurrence with ``--conn`` 50 entries per row and N(0, 0.05) weights, ``scale_exp`` given.  For each
``N`` (default 2000 and 8192) five sides take turns inside one loop on the same inputs; every tensor holds the numbers of side (a):

  ``numbers``        (a) ``be.recurrent_lif_sequence`` with five numbers; gradients of ``x`` and ``rec.data``;
  ``tensors``        (b) ``be.parametric_recurrent_lif_sequence`` with five ``[N]`` tensors, none requiring grad; the same gradients;
  ``learn_n``        (c) all five ``[N]`` and learnable: the gradients of ``x``, ``rec.data`` and the five;
  ``learn_1``        (d) all five one-element and learnable;
  ``step_loop``      (e) per step one ``BinaryArray(s) @ rec`` and one ``be.parametric_synaptic_lif_step`` with the tensors of (c) —
                     what a user had.

HIP-event medians and quartiles of ``--reps`` turns, the order shuffled (seeded) for every turn (DESIGN.md §2.20 records why).
Checked and recorded before anything is reported: (b) equals (a) bit for bit; (c) and (e) agree — spikes equal on at least 99.9 %
of the [T, B, N] slots (the loop's recurrent sums are f32 atomics in an order of their own) and, where the spikes are all equal,
every gradient within 1e-4 of its scale (the parameters' sums differ in order).  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_lif_rec_sg_param.py [--T 25] [--batch 32] [--sizes 2000,8192] [--reps 21] [--out profiles/lif_rec_sg_param_line.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd._csr import fixed_point_exponent  # noqa: E402
from exp_lif_syn_sg import timed_turns  # noqa: E402

SYN_DECAY, BETA, V_TH, RHO, KAPPA, ALPHA = 0.8, 0.9, 1.0, 0.95, 0.3, 10.0
NAMES = ('syn_decay', 'beta', 'v_th', 'rho', 'kappa')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=25)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--conn', type=int, default=50)
    ap.add_argument('--sizes', default='2000,8192')
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error('--reps must be at least 9')
    dev = torch.device('cuda')
    T, B = args.T, args.batch
    values = (SYN_DECAY, BETA, V_TH, RHO, KAPPA)
    fixed = dict(v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=ALPHA)
    kw = lambda q: dict(fixed, syn_decay=q[0], beta=q[1], v_th=q[2], adapt=(q[3], q[4]))
    sides = ['numbers', 'tensors', 'learn_n', 'learn_1', 'step_loop']
    res = {'what': 'forward + backward of T steps of a recurrent adaptive LIF layer, scale_exp given: be.recurrent_lif_sequence with '
                   'numbers; be.parametric_recurrent_lif_sequence with five [N] tensors (no grad), five learnable [N], five learnable '
                   'one-element tensors; and the per-step loop of BinaryArray(s) @ rec + be.parametric_synaptic_lif_step with the '
                   'learnable [N] tensors; alternating in one loop, the order shuffled for every turn',
           'device': torch.cuda.get_device_name(0), 'T': T, 'batch': B, 'entries_per_row': args.conn, 'reps': args.reps, 'sizes': {}}
    for n in (int(s) for s in args.sizes.split(',')):
        rng = np.random.default_rng(0)
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        indptr = torch.arange(n + 1, dtype=torch.int32, device=dev) * args.conn
        indices = torch.tensor(rng.integers(0, n, n * args.conn).astype(np.int32), device=dev)
        w = torch.tensor(rng.normal(0.0, 0.05, n * args.conn), dtype=torch.float32, device=dev).requires_grad_()
        rec = be.CSR((w, indices, indptr), shape=(n, n))
        x = (torch.randn((T, B, n), device=dev, generator=g) * 0.25 + 0.12).requires_grad_()
        g_s = torch.randn((T, B, n), device=dev, generator=g)
        e = fixed_point_exponent(w.detach(), indices, n)
        q_plain = [torch.full((n,), v, device=dev) for v in values]
        q_n = [torch.full((n,), v, device=dev).requires_grad_() for v in values]
        q_1 = [torch.full((1,), v, device=dev).requires_grad_() for v in values]
        outs = {}

        def numbers():
            s_all, _ = be.recurrent_lif_sequence(x, rec, scale_exp=e, **kw(values))
            outs['numbers'] = (s_all,) + torch.autograd.grad([s_all], [x, w], [g_s])

        def tensors():
            s_all, _ = be.parametric_recurrent_lif_sequence(x, rec, scale_exp=e, **kw(q_plain))
            outs['tensors'] = (s_all,) + torch.autograd.grad([s_all], [x, w], [g_s])

        def learn_n():
            s_all, _ = be.parametric_recurrent_lif_sequence(x, rec, scale_exp=e, **kw(q_n))
            outs['learn_n'] = (s_all,) + torch.autograd.grad([s_all], [x, w] + q_n, [g_s])

        def learn_1():
            s_all, _ = be.parametric_recurrent_lif_sequence(x, rec, scale_exp=e, **kw(q_1))
            outs['learn_1'] = (s_all,) + torch.autograd.grad([s_all], [x, w] + q_1, [g_s])

        def step_loop():
            state = tuple(torch.zeros(B, n, device=dev) for _ in range(3))
            s, ss = torch.zeros(B, n, device=dev), []
            for t in range(T):
                s, state = be.parametric_synaptic_lif_step(state, x[t] + be.BinaryArray(s) @ rec, **kw(q_n))
                ss.append(s)
            s_all = torch.stack(ss)
            outs['step_loop'] = (s_all,) + torch.autograd.grad([s_all], [x, w] + q_n, [g_s])

        times = timed_turns([numbers, tensors, learn_n, learn_1, step_loop], args.reps)
        torch.cuda.synchronize()
        outs = {nm: tuple(t.detach() for t in ts) for nm, ts in outs.items()}
        ref, got = outs['step_loop'], outs['learn_n']
        same = float((got[0] == ref[0]).float().mean())
        spikes_equal = bool(torch.equal(got[0], ref[0]))
        scale = [float(t.abs().max()) for t in ref]
        worst = [float((a - b).abs().max()) / max(sc, 1.0) for a, b, sc in zip(got[1:], ref[1:], scale[1:])]
        agree = same >= 0.999 and (not spikes_equal or all(d <= 1e-4 for d in worst))
        tensors_equal_numbers = bool(all(torch.equal(a, b) for a, b in zip(outs['numbers'], outs['tensors'])))
        # the one-element gradients are the sums of the per-neuron ones, in another order
        sums = [float((a.sum() - b.sum()).abs()) / max(float(b.abs().sum()), 1.0) for a, b in zip(outs['learn_n'][3:], outs['learn_1'][3:])]
        block = {'measured': bool(agree and tensors_equal_numbers), 'tensors_equal_numbers': tensors_equal_numbers,
                 'spikes_equal': spikes_equal, 'spike_slots_equal': round(same, 6), 'scale_exp': int(e),
                 'spike_rate': round(float(outs['learn_n'][0].mean()), 4),
                 'worst_gradient_difference_over_scale': {k: float(f'{d:.3g}') for k, d in zip(('x', 'w') + NAMES, worst)},
                 'one_element_sum_difference_over_terms': {k: float(f'{d:.3g}') for k, d in zip(NAMES, sums)}}
        med = {}
        for nm, tt in zip(sides, times):
            block[nm] = {'ms': tt}
            med[nm] = tt['median']
        block['tensors_over_numbers'] = round(med['tensors'] / med['numbers'], 3)
        block['learn_n_over_tensors'] = round(med['learn_n'] / med['tensors'], 3)
        block['learn_1_over_learn_n'] = round(med['learn_1'] / med['learn_n'], 3)
        block['step_loop_over_learn_n'] = round(med['step_loop'] / med['learn_n'], 2)
        res['sizes'][str(n)] = block
        del x, w, rec, g_s, outs, q_plain, q_n, q_1
    res['all_measured'] = all(b['measured'] for b in res['sizes'].values())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0 if res['all_measured'] else 1


if __name__ == '__main__':
    sys.exit(main())
