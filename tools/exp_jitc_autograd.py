"""Timings of the fused parameter-gradient walk of the JIT-connectivity products and of their backward pass.

``JITCNormalR`` with ``--n`` x ``--n`` neurons at ``--prob`` (default 1M x 1M at 2e-3: 2e9 drawn edges), f32, ``nb`` in {1, 32},
both ``corder``.  Per case:

* ``be_jit_param_grad`` (through ``jit_param_sums``: one walk, both sums), alternating in the same loop with the reference's rule
  built from what the library had before it: two float-twin products with the parameters ``(1, 0)`` and ``(0, 1)`` and one
  ``torch.sum(r * g)`` each;
* the full backward pass (both parameters and the operand) of ``M @ x`` and ``x @ M``;
* at ``nb = 1``: the parameter gradients of ``BinaryArray(s) @ M`` at ``--fire`` (default 1 %) in the scatter orientation,
  fused against the same composition on the 0/1 activity.

Operands are drawn from [0.5, 1.5): one scale, so the float-operand scatter twin takes its fixed-point route.  Every figure is
the median of ``--reps`` repetitions timed with HIP events.  Prints one JSON line and, with ``--out``, writes it.

    python tools/exp_jitc_autograd.py [--n 1000000] [--prob 2e-3] [--reps 5] [--out profiles/jitc_autograd_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402
from brainevent_amd import _jitc as J  # noqa: E402
from exp_float_autograd import timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--prob', type=float, default=2e-3)
    ap.add_argument('--fire', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n, seed = args.n, args.seed
    clen = J._initialize_conn_length(args.prob)
    one, zero = torch.tensor(1.0), torch.tensor(0.0)

    def draw(*shape):
        return torch.rand(shape, device=dev, generator=g) + 0.5

    def composition(x, gy, corder):
        """The reference's rule: the product with the parameters replaced, then a dot product — once per parameter."""
        call = J.jitnmv_p_call if x.ndim == 1 else J.jitnmm_p_call
        kw = dict(shape=(n, n), transpose=False, corder=corder)
        s0 = torch.sum(call(one, zero, clen, x, seed, **kw)[0] * gy)
        s1 = torch.sum(call(zero, one, clen, x, seed, **kw)[0] * gy)
        return s0, s1

    line = {'device': torch.cuda.get_device_name(0), 'n': n, 'prob': args.prob, 'dtype': 'f32', 'reps': args.reps, 'cases': []}
    for nb in (1, 32):
        for corder in (True, False):
            case = {'nb': nb, 'corder': corder}
            x, gy = draw(n, nb), draw(n, nb)
            xv, gv = (x[:, 0].contiguous(), gy[:, 0].contiguous()) if nb == 1 else (x, gy)
            P, Q = (gy, x) if corder else (x, gy)
            stride = 32 if nb == 1 else 4
            case['fused_ms'], case['composition_ms'] = timed_alternating(
                [lambda: J.jit_param_sums('n', P, Q, clen=clen, seed=seed, shape1=n, stride=stride),
                 lambda: composition(xv, gv, corder)], args.reps)
            fused = J.jit_param_sums('n', P, Q, clen=clen, seed=seed, shape1=n, stride=stride).tolist()
            comp = [float(s) for s in composition(xv, gv, corder)]
            case['fused_sums'], case['composition_sums'] = fused, comp
            loc, scale = torch.tensor(0.1, device=dev, requires_grad=True), torch.tensor(0.5, device=dev, requires_grad=True)
            M = be.JITCNormalR((loc, scale, args.prob, seed), shape=(n, n), corder=corder)
            for left in (False, True):
                xo = (draw(n) if nb == 1 else (draw(nb, n) if left else draw(n, nb))).requires_grad_()
                y = (xo @ M) if left else (M @ xo)
                go = draw(*y.shape)
                key = 'x@M' if left else 'M@x'
                case[f'{key}_bwd_ms'], = timed_alternating(
                    [lambda: torch.autograd.grad(y, (loc, scale, xo), go, retain_graph=True)], args.reps)
                case[f'{key}_bwd_params_only_ms'], = timed_alternating(
                    [lambda: torch.autograd.grad(y, (loc, scale), go, retain_graph=True)], args.reps)
                del y, go, xo
            if nb == 1 and corder:          # events @ M runs the scatter kernel for corder=True (the generator rows are the inputs)
                s = torch.rand(n, device=dev, generator=g) < args.fire
                act = s.to(torch.float32)
                y = be.BinaryArray(s) @ M
                go = draw(n)
                case['events@M_fire'] = args.fire
                ekw = dict(shape=(n, n), transpose=True, corder=False)
                case['events@M_bwd_params_ms'], case['events@M_composition_ms'] = timed_alternating(
                    [lambda: torch.autograd.grad(y, (loc, scale), go, retain_graph=True),
                     lambda: (torch.sum(J.jitnmv_p_call(one, zero, clen, act, seed, **ekw)[0] * go),
                              torch.sum(J.jitnmv_p_call(zero, one, clen, act, seed, **ekw)[0] * go))], args.reps)
                del y, go, s, act
            line['cases'].append(case)
            del x, gy, P, Q, M
            torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
