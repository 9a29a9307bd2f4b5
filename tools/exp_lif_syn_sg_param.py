"""The price of learnable, per-neuron ``syn_decay`` / ``beta`` / ``v_th`` / ``rho`` / ``kappa`` in the fused adaptive neuron
(csrc/be_neuron_sg.hip), what the only other route to them costs, and which access width the all-learnable
training step should take.

One training step = forward + ``torch.autograd.grad`` over ``--T`` 25 steps of the ADAPTIVE neuron, hard reset to 0, fast sigmoid.
For each shape (default ``[32, 2000]`` and ``[32, 65536]``) the sides take turns inside one loop on the same inputs:

  ``float``         (a) ``be.synaptic_lif_sequence`` with five Python floats (§2.21's kernels, untouched): gradients of x and the state;
  ``per_neuron``    (b) ``be.parametric_synaptic_lif_sequence`` with all five ``[n]`` and learnable: forward (h, a_save, c_save kept),
                    backward with five per-slot accumulators, five reduces over the batch rows;
  ``shared``        (c) the same with all five ``[1]`` and learnable (the reduces are the two-stage tree over all slots);
  ``torch_loop``    (d) the torch elementwise composition with the same learnable per-neuron tensors — what a user has without the
                    kernels;
  ``beta_vth``      (e) (b) with only ``beta`` and ``v_th`` learnable, the other three ``[n]`` but fixed: no c_save, two reduces;
  ``per_neuron_4b`` (b) with ``kappa``'s base 4 bytes past a 16-byte boundary, which sends both launches to the 4-byte kernels —
                    the other side of the width decision (the 16-byte adaptive backward kernel holds ~207 VGPRs: 2 waves per SIMD).

HIP-event medians and quartiles of ``--reps`` turns, the order shuffled (seeded) for every turn.  A shape counts as measured only
if (b) and (d) agree: spikes equal, the gradients of x and the state within 1e-5 of the yardstick's scale (as tools/exp_lif_syn_sg.py
asks), and the parameter gradients within 1e-4 of theirs — each is a sum of ``T * batch`` f32 terms that torch adds in another order,
``T * batch * 2**-24`` ~ 5e-5 of the sum of their absolute values for 25 x 32.  (b) and ``per_neuron_4b`` must agree bit for bit.
Recorded with the times: the f32 values a training step moves per slot and step — (a) and (e) 8 (x, s, h, a_save / th_save written or
read forwards, h, a_save, g_s read and g_x written backwards), (b) 10 (c_save written and read back) — and the ``[N]``-sized vectors
on top.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_lif_syn_sg_param.py [--T 25] [--reps 21] [--out profiles/lif_syn_sg_param_line.json]
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
PARAMS = ('syn_decay', 'beta', 'v_th', 'rho', 'kappa')


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
    kw = dict(v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=ALPHA)
    names = ['float', 'per_neuron', 'shared', 'torch_loop', 'beta_vth', 'per_neuron_4b']
    res = {'what': 'forward + backward of T adaptive LIF steps: be.synaptic_lif_sequence with five floats, '
                   'be.parametric_synaptic_lif_sequence with all five learnable per neuron, shared, only beta / v_th learnable, and '
                   'all five per neuron through the 4-byte kernels; the torch elementwise composition with the per-neuron tensors; '
                   'alternating in one loop, the order shuffled for every turn',
           'device': torch.cuda.get_device_name(0), 'T': T, 'reps': args.reps, 'shapes': {}}
    for shape in (tuple(int(d) for d in s.split('x')) for s in args.shapes.split(',')):
        n = shape[-1]
        randn = lambda *lead: torch.randn(tuple(lead) + shape, device=dev, generator=g)
        spread = lambda mid, width, k=n: mid + width * (torch.rand(k, device=dev, generator=g) - 0.5)
        x = (randn(T) * 0.25 + 0.12).requires_grad_()
        c0 = (randn() * 0.3 + 0.2).requires_grad_()
        v0 = (randn() * 0.5 + 0.3).requires_grad_()
        a0 = (randn() * 0.5 + 0.5).abs().requires_grad_()
        g_s, g_c, g_v, g_a = randn(T), randn(), randn(), randn()
        per = [spread(SYN_DECAY, 0.1), spread(BETA, 0.1), spread(V_TH, 0.2), spread(RHO, 0.06), spread(KAPPA, 0.2)]
        leaves = [t.clone().requires_grad_() for t in per]
        fixed3 = [per[0], leaves[1], leaves[2], per[3], per[4]]
        one = [torch.full((1,), c, device=dev, requires_grad=True) for c in (SYN_DECAY, BETA, V_TH, RHO, KAPPA)]
        k_store = torch.zeros(n + 1, device=dev)
        k_store[1:].copy_(per[4])
        kappa_off = k_store[1:].detach().requires_grad_()      # a leaf of its own on the offset storage: no extra autograd node
        assert kappa_off.data_ptr() % 16 == 4 and kappa_off.is_leaf
        outs = {}

        def fused(q, wrt):
            s_all, (c, v, a) = be.parametric_synaptic_lif_sequence(x, (c0, v0, a0), syn_decay=q[0], beta=q[1], v_th=q[2],
                                                                   adapt=(q[3], q[4]), **kw)
            return (s_all,) + torch.autograd.grad([s_all, c, v, a], [x, c0, v0, a0] + wrt, [g_s, g_c, g_v, g_a])

        def float_seq():
            s_all, (c, v, a) = be.synaptic_lif_sequence(x, (c0, v0, a0), syn_decay=SYN_DECAY, beta=BETA, v_th=V_TH, adapt=(RHO, KAPPA), **kw)
            outs['float'] = (s_all,) + torch.autograd.grad([s_all, c, v, a], [x, c0, v0, a0], [g_s, g_c, g_v, g_a])

        def per_neuron():
            outs['per_neuron'] = fused(leaves, leaves)

        def shared():
            outs['shared'] = fused(one, one)

        def beta_vth():
            outs['beta_vth'] = fused(fixed3, [leaves[1], leaves[2]])

        def per_neuron_4b():
            outs['per_neuron_4b'] = fused(leaves[:4] + [kappa_off], leaves[:4] + [kappa_off])

        def torch_loop():
            sd, beta, v_th, rho, kappa = leaves
            c, v, a, ss = c0, v0, a0, []
            for t in range(T):
                c = sd * c + x[t]
                h = beta * v + c
                s = SpikeFn.apply(h, v_th + kappa * a)
                v = h * (1.0 - s)
                a = rho * a + s
                ss.append(s)
            s_all = torch.stack(ss)
            outs['torch_loop'] = (s_all,) + torch.autograd.grad([s_all, c, v, a], [x, c0, v0, a0] + leaves, [g_s, g_c, g_v, g_a])

        times = timed_turns([float_seq, per_neuron, shared, torch_loop, beta_vth, per_neuron_4b], args.reps)
        torch.cuda.synchronize()
        outs = {nm: tuple(t.detach() for t in ts) for nm, ts in outs.items()}
        ref, got, narrow = outs['torch_loop'], outs['per_neuron'], outs['per_neuron_4b']
        scale = [float(t.abs().max()) for t in ref]
        worst = [float((a - b).abs().max()) / max(sc, 1.0) for a, b, sc in zip(got[1:], ref[1:], scale[1:])]
        spikes_equal = bool(torch.equal(got[0], ref[0]))
        widths_equal = all(torch.equal(a, b) for a, b in zip(got, narrow))
        agree = spikes_equal and widths_equal and all(w <= 1e-5 for w in worst[:4]) and all(w <= 1e-4 for w in worst[4:])
        slots = 1
        for d in shape:
            slots *= d
        block = {'measured': bool(agree), 'spikes_equal': spikes_equal, 'both_widths_bit_equal': bool(widths_equal),
                 'spike_rate': round(float(ref[0].mean()), 4),
                 'worst_gradient_difference_over_scale': {k: float(f'{w:.3g}') for k, w in zip(('x', 'c0', 'v0', 'a0') + PARAMS, worst)}}
        floats = {'float': 8 * T * slots + 8 * slots, 'beta_vth': 8 * T * slots + (8 + 1 + 4) * slots + 10 * n,
                  'per_neuron': 10 * T * slots + (8 + 2 + 10) * slots + 10 * n, 'per_neuron_4b': 10 * T * slots + (8 + 2 + 10) * slots + 10 * n,
                  'shared': 10 * T * slots + (8 + 2 + 10) * slots}
        med = {}
        for nm, tt in zip(names, times):
            block[nm] = {'ms': tt}
            med[nm] = tt['median']
            if nm in floats:
                block[nm]['bytes_per_training_step'] = floats[nm] * 4
                block[nm]['tb_per_s'] = round(floats[nm] * 4 / (tt['median'] * 1e-3) / 1e12, 3)
        for nm in ('per_neuron', 'shared', 'beta_vth', 'per_neuron_4b'):
            block[f'{nm}_over_float'] = round(med[nm] / med['float'], 3)
            block[f'{nm}_bytes_over_float'] = round(floats[nm] / floats['float'], 4)
        block['per_neuron_16b_over_4b'] = round(med['per_neuron'] / med['per_neuron_4b'], 3)
        block['torch_loop_over_per_neuron'] = round(med['torch_loop'] / med['per_neuron'], 2)
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
