"""Pair-based STDP on a CSR matrix: the loop of the reference's plasticity tutorial
(docs/tutorials/data-structures/05_synaptic_plasticity.ipynb, section 3: 100 x 50 CSR, p = 0.1, 500 steps, random pre / post
spikes at 5 %, traces decaying with tau = 20 ms, A+ = A- = 0.005, weights clipped to [0, 1]), run eagerly and as a captured
HIP graph (``capture_step``), with the final weights compared bit for bit.

    python examples/stdp_csr.py                       # the tutorial's size
    python examples/stdp_csr.py --n 1000000 --conn 10000 --steps 20 --rate 0.01
                                                      # a large run (1e10 synapses): in-place, certified updates

Each step: traces decay and add this step's spikes, ``update_on_pre`` (LTP: + A+ * post_trace) and ``update_on_post``
(LTD: - A- * pre_trace), both ``inplace=True`` — after the first step the container holds a clip certificate and the kernels
clip the touched synapses only.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


def build(n_pre, n_post, conn, p, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    if conn is None:                                   # Bernoulli(p) connectivity, the tutorial's matrix
        rng = np.random.default_rng(seed)
        mask = rng.random((n_pre, n_post)) < p
        w = rng.uniform(0.0, 1.0, (n_pre, n_post)).astype(np.float32) * mask
        return be.CSR.fromdense(torch.tensor(w, device=dev))
    nnz = n_pre * conn                                 # fixed fan-out rows (large run)
    ptr = torch.arange(n_pre + 1, dtype=torch.int64 if nnz > 2**31 - 1 else torch.int32, device=dev) * conn
    idx = torch.randint(0, n_post, (nnz,), dtype=torch.int32, device=dev, generator=g)
    w = torch.rand(nnz, dtype=torch.float32, device=dev, generator=g)
    return be.CSR((w, idx, ptr), shape=(n_pre, n_post), check_structure=False)


def run(args, graph: bool):
    dev = torch.device('cuda')
    csr = build(args.n_pre, args.n_post, args.conn, args.p, 0, dev)
    g = torch.Generator(device=dev).manual_seed(100)
    pre_all = torch.rand((args.steps, args.n_pre), device=dev, generator=g) < args.rate
    post_all = torch.rand((args.steps, args.n_post), device=dev, generator=g) < args.rate
    decay = float(np.exp(-args.dt / args.tau))
    pre_spk = torch.zeros(args.n_pre, dtype=torch.bool, device=dev)
    post_spk = torch.zeros(args.n_post, dtype=torch.bool, device=dev)
    pre_tr = torch.zeros(args.n_pre, device=dev)
    post_tr = torch.zeros(args.n_post, device=dev)
    state = (csr.data.clone(), )

    def step():
        pre_tr.mul_(decay).add_(pre_spk.float())
        post_tr.mul_(decay).add_(post_spk.float())
        csr.update_on_pre(pre_spk, post_tr * args.a_plus, 0.0, 1.0, inplace=True)
        csr.update_on_post(pre_tr * -args.a_minus, post_spk, 0.0, 1.0, inplace=True)

    if graph:
        step_g = be.capture_step(step)                 # warm-up runs advance the state: restore it
        csr.data.copy_(state[0])
        pre_tr.zero_()
        post_tr.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        pre_spk.copy_(pre_all[t])
        post_spk.copy_(post_all[t])
        step_g() if graph else step()
    torch.cuda.synchronize()
    return csr, (time.perf_counter() - t0) / args.steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--n', type=int, default=None, help='n_pre = n_post (default: the tutorial\'s 100 x 50)')
    ap.add_argument('--conn', type=int, default=None, help='synapses per pre neuron (default: Bernoulli p)')
    ap.add_argument('--p', type=float, default=0.1)
    ap.add_argument('--steps', type=int, default=500)
    ap.add_argument('--rate', type=float, default=0.05)
    ap.add_argument('--dt', type=float, default=1.0)
    ap.add_argument('--tau', type=float, default=20.0)
    ap.add_argument('--a-plus', dest='a_plus', type=float, default=0.005)
    ap.add_argument('--a-minus', dest='a_minus', type=float, default=0.005)
    args = ap.parse_args()
    args.n_pre, args.n_post = (100, 50) if args.n is None else (args.n, args.n)
    w0 = build(args.n_pre, args.n_post, args.conn, args.p, 0, torch.device('cuda')).data
    print(f"STDP on a {args.n_pre} x {args.n_post} CSR, {int(w0.numel())} synapses, {args.steps} steps at {args.rate:.0%} firing")
    mean0 = float(w0.double().mean())
    del w0
    eager, ms_e = run(args, graph=False)
    w_eager = eager.data.clone()
    del eager
    graphed, ms_g = run(args, graph=True)
    same = torch.equal(w_eager, graphed.data)
    print(f"  eager : mean weight {mean0:.4f} -> {float(w_eager.double().mean()):.4f}, range "
          f"[{float(w_eager.min()):.3f}, {float(w_eager.max()):.3f}], {ms_e * 1e3:.3f} ms/step")
    print(f"  graph : mean weight {mean0:.4f} -> {float(graphed.data.double().mean()):.4f}, {ms_g * 1e3:.3f} ms/step")
    print(f"  final weights identical (eager vs replayed graph): {same}")
    if not same:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
