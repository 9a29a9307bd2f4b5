"""What synaptic delays cost inside the fused recurrent spiking layer (csrc/be_neuron_sg_rec_delay.hip), next to
the layer without delays and to the only route to delays there was before.

One training step = forward + ``torch.autograd.grad`` in ``x`` and the weights over ``--T`` 25 steps of ``--batch`` 32 samples, the
adaptive neuron, hard reset to 0, fast sigmoid, a CSR recurrence with ``--conn`` 50 entries per row, N(0, 0.05) weights and delays
drawn uniformly from ``[0, --depth 16)``.  For each ``N`` (default 2000 and 8192) three sides take turns inside one loop on the same
inputs:

  ``delayed``        ``be.recurrent_lif_sequence(x, csr.with_delays(delays, depth), scale_exp=e)``: the new call;
  ``undelayed``      ``be.recurrent_lif_sequence(x, csr, scale_exp=e)`` on the same matrix without its delays — another network, the
                     same amount of synapses: the floor;
  ``step_loop``      per step ``depth`` products ``BinaryArray(s[t-1-d]) @ W_d`` (the rows of delay ``d`` as a CSR of their own) and
                     one ``be.synaptic_lif_step`` — what was possible before.

HIP-event medians and quartiles of ``--reps`` turns, the order shuffled (seeded) for every turn (DESIGN.md §2.20 records why).  A
size counts as measured only if ``delayed`` and ``step_loop`` agree: spikes equal on at least 99.9 % of the [T, B, N] slots (the
loop's recurrent sums are f32 in an order of their own, so a membrane on the threshold may fall either way) and, where the spikes
are all equal, every gradient within 1e-4 of the yardstick's scale.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_lif_rec_delay_sg.py [--T 25] [--batch 32] [--depth 16] [--sizes 2000,8192] [--reps 21]
                                         [--out profiles/lif_rec_delay_sg_line.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=25)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--conn', type=int, default=50)
    ap.add_argument('--depth', type=int, default=16)
    ap.add_argument('--sizes', default='2000,8192')
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error('--reps must be at least 9')
    dev = torch.device('cuda')
    T, B, depth = args.T, args.batch, args.depth
    kw = dict(syn_decay=SYN_DECAY, beta=BETA, v_th=V_TH, v_reset=0.0, reset='hard', surrogate='fast_sigmoid', alpha=ALPHA,
              adapt=(RHO, KAPPA))
    names = ['delayed', 'undelayed', 'step_loop']
    res = {'what': 'forward + backward (gradients of x and the weights) of T steps of a recurrent adaptive LIF layer with uniform '
                   'synaptic delays in [0, depth): be.recurrent_lif_sequence on a DelayedCSR, the same call on the matrix without '
                   'delays (another network: the floor), and the per-step loop of depth products BinaryArray(s[t-1-d]) @ W_d + '
                   'be.synaptic_lif_step; alternating in one loop, the order shuffled for every turn',
           'device': torch.cuda.get_device_name(0), 'T': T, 'batch': B, 'entries_per_row': args.conn, 'depth': depth,
           'reps': args.reps, 'sizes': {}}
    for n in (int(s) for s in args.sizes.split(',')):
        rng = np.random.default_rng(0)
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        indptr = torch.arange(n + 1, dtype=torch.int32, device=dev) * args.conn
        indices = torch.tensor(rng.integers(0, n, n * args.conn).astype(np.int32), device=dev)
        w0 = torch.tensor(rng.normal(0.0, 0.05, n * args.conn), dtype=torch.float32, device=dev)
        delays = torch.tensor(rng.integers(0, depth, n * args.conn).astype(np.int32), device=dev)
        w = w0.clone().requires_grad_()
        rec = be.CSR((w, indices, indptr), shape=(n, n))
        drec = be.CSR((w0, indices, indptr), shape=(n, n)).with_delays(delays, depth)
        ws = drec.stacked.data.requires_grad_()
        st = drec.stacked
        # the rows of every delay as a CSR of their own, over slices of the one stacked weight array (the loop's leaf too)
        ptr = st.indptr.cpu().numpy().astype(np.int64)
        parts = []
        for d in range(depth):
            lo, hi = int(ptr[d * n]), int(ptr[(d + 1) * n])
            parts.append((lo, hi, st.indices[lo:hi].contiguous(), (st.indptr[d * n:(d + 1) * n + 1] - lo).contiguous()))
        x = (torch.randn((T, B, n), device=dev, generator=g) * 0.25 + 0.12).requires_grad_()
        g_s = torch.randn((T, B, n), device=dev, generator=g)
        e = fixed_point_exponent(ws.detach(), st.indices, n)
        outs = {}

        def delayed():
            s_all, _ = be.recurrent_lif_sequence(x, drec, scale_exp=e, **kw)
            outs['delayed'] = (s_all,) + torch.autograd.grad([s_all], [x, ws], [g_s])

        def undelayed():
            s_all, _ = be.recurrent_lif_sequence(x, rec, scale_exp=e, **kw)
            outs['undelayed'] = (s_all,) + torch.autograd.grad([s_all], [x, w], [g_s])

        def step_loop():
            state = tuple(torch.zeros(B, n, device=dev) for _ in range(3))
            mats = [be.CSR((ws[lo:hi], idx, p), shape=(n, n), check_structure=False) for lo, hi, idx, p in parts]   # (no host read)
            ss = []
            for t in range(T):
                xin = x[t]
                for d in range(min(depth, t)):
                    xin = xin + be.BinaryArray(ss[t - 1 - d]) @ mats[d]
                s, state = be.synaptic_lif_step(state, xin, **kw)
                ss.append(s)
            s_all = torch.stack(ss)
            outs['step_loop'] = (s_all,) + torch.autograd.grad([s_all], [x, ws], [g_s])

        times = timed_turns([delayed, undelayed, step_loop], args.reps)
        torch.cuda.synchronize()
        outs = {nm: tuple(t.detach() for t in ts) for nm, ts in outs.items()}
        ref, got = outs['step_loop'], outs['delayed']
        same = float((got[0] == ref[0]).float().mean())
        spikes_equal = bool(torch.equal(got[0], ref[0]))
        scale = [float(t.abs().max()) for t in ref]
        worst = [float((a - b).abs().max()) / max(sc, 1.0) for a, b, sc in zip(got[1:], ref[1:], scale[1:])]
        agree = same >= 0.999 and (not spikes_equal or all(d <= 1e-4 for d in worst))
        lens = (st.indptr[1:] - st.indptr[:-1]).float()
        block = {'measured': bool(agree), 'spikes_equal': spikes_equal, 'spike_slots_equal': round(same, 6), 'scale_exp': int(e),
                 'spike_rate': {nm: round(float(outs[nm][0].mean()), 4) for nm in names},
                 'stacked_rows_not_empty': round(float((lens > 0).float().mean()), 4),
                 'entries_per_stacked_row_not_empty': round(float(lens.sum() / (lens > 0).sum()), 3),
                 'worst_gradient_difference_over_scale': {k: float(f'{d:.3g}') for k, d in zip(('x', 'w'), worst)}}
        med = {}
        for nm, tt in zip(names, times):
            block[nm] = {'ms': tt}
            med[nm] = tt['median']
        block['step_loop_over_delayed'] = round(med['step_loop'] / med['delayed'], 2)
        block['delayed_over_undelayed'] = round(med['delayed'] / med['undelayed'], 2)
        res['sizes'][str(n)] = block
        del x, w, ws, rec, drec, g_s, outs
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
