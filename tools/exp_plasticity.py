"""Cost of the spike-triggered plasticity updates on the MI355X; prints one JSON line.

Sizes (the C2 shape, 1M x 1M, at 2000 synapses per row = 2e9 entries: the structure, its permuted index and the plan of the
refresh measurement fit one card together; C2 itself holds 1e4 per row):
  * pre_ms / post_ms: ``update_on_pre`` (row-driven) / ``update_on_post`` (permuted) in place, 1 % of the rows firing,
    certified (touched entries clipped in registers) and uncertified (unclipped kernel + a clamp of the whole array);
  * refresh_ms: what the next ``spk @ csr`` pays after an in-place update to re-derive its scatter plan, with and without
    ``keep_order`` (the product after an update minus the same product on unchanged weights);
  * ref_point_ms: the reference's one published point (5000 x 5000, 10 % spikes, 2.30 ms on its GPU,
    ``_csr/plasticity_binary_on_pre.cu:37-38``), here at 10 % connectivity.
  * ``--plastic``: only the learning step ``update_on_pre`` + ``update_on_post`` + ``spk @ M`` (all in place, bounds (0, 1)):
    ``step_ms_refresh`` — the product re-derives the plan after the updates (``keep_order=True``) — and ``step_ms_plastic`` — the
    container armed with ``prepare(plastic=(0, 1))``, where the updates keep the plan current themselves —, the latter also
    replayed from one captured graph (``step_ms_plastic_graph``).  A build without plastic mode reports the first figure only.
Times are HIP-event means over ``--reps`` calls after a warm-up.  Under rocprofv3 use ``--reps 5``.

    python tools/exp_plasticity.py [--rows 1000000] [--conn 2000] [--reps 20] [--plastic]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brainevent_amd as be  # noqa: E402


def timed(fn, reps, before=None):
    """mean ms of fn() over reps calls (before(): untimed work ahead of each call)."""
    tot = 0.0
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        tot += a.elapsed_time(b)
    return tot / reps


def make(n, conn, dev, g):
    nnz = n * conn
    ptr = torch.arange(n + 1, dtype=torch.int64 if nnz > 2**31 - 1 else torch.int32, device=dev) * conn
    idx = torch.randint(0, n, (nnz,), dtype=torch.int32, device=dev, generator=g)
    w = torch.rand(nnz, device=dev, generator=g) * 0.5 + 0.25
    return be.CSR((w, idx, ptr), shape=(n, n), check_structure=False)


def step_legs(M, spk, tr, reps):
    """The learning step on the refresh path and in plastic mode (see the module docstring)."""
    x = be.BinaryArray(spk)
    res = {}

    def step():
        M.update_on_pre(spk, tr, 0.0, 1.0, inplace=True)
        M.update_on_post(tr, spk, 0.0, 1.0, inplace=True)
        return x @ M

    M.prepare(keep_order=True)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    res['step_ms_refresh'] = timed(step, reps)
    res['route'] = type(M.buffers.get('scatter_plan')).__name__
    try:
        M.prepare(plastic=(0.0, 1.0))
    except TypeError:                       # a build without plastic mode
        res['step_ms_plastic'] = None
        return res
    res['plastic_state'] = M.plastic_state
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    assert M.plastic_state is not None
    res['step_ms_plastic'] = timed(step, reps)
    res['pre_ms_plastic'] = timed(lambda: M.update_on_pre(spk, tr, 0.0, 1.0, inplace=True), reps)
    res['post_ms_plastic'] = timed(lambda: M.update_on_post(tr, spk, 0.0, 1.0, inplace=True), reps)
    res['product_ms_plastic'] = timed(lambda: x @ M, reps)
    graphed = be.capture_step(step)
    torch.cuda.synchronize()
    res['step_ms_plastic_graph'] = timed(graphed, reps)
    ws = M.buffers.get('scatter_plan')
    res['plan_bytes'] = ws.nbytes() if hasattr(ws, 'nbytes') else None
    assert M.plastic_state is not None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--conn', type=int, default=2000)
    ap.add_argument('--rate', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--plastic', action='store_true', help='measure the learning step only: refresh path vs plastic mode')
    a = ap.parse_args()
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(0)
    n = a.rows
    M = make(n, a.conn, dev, g)
    spk = torch.rand(n, device=dev, generator=g) < a.rate
    tr = (torch.rand(n, device=dev, generator=g) - 0.5) * 1e-3
    n_act = int(spk.sum())
    upd = n_act * a.conn
    out = {'tool': 'exp_plasticity', 'shape': [n, n], 'nnz': n * a.conn, 'active_rows': n_act, 'updated_synapses_pre': upd}
    if a.plastic:
        out.update(step_legs(M, spk, tr, a.reps))
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in out.items()}))
        return
    # warm-up: builds the plasticity index (once, structure only) and the clip certificate
    M.update_on_pre(spk, tr, 0.0, 1.0, inplace=True)
    M.update_on_post(tr, spk, 0.0, 1.0, inplace=True)
    torch.cuda.synchronize()
    out['pre_ms_certified'] = timed(lambda: M.update_on_pre(spk, tr, 0.0, 1.0, inplace=True), a.reps)
    out['post_ms_certified'] = timed(lambda: M.update_on_post(tr, spk, 0.0, 1.0, inplace=True), a.reps)
    out['pre_ms_unclipped'] = timed(lambda: M.update_on_pre(spk, tr, inplace=True), a.reps)
    out['post_ms_unclipped'] = timed(lambda: M.update_on_post(tr, spk, inplace=True), a.reps)
    void = lambda: M.buffers.pop('plasticity_clip', None)            # noqa: E731  (forces the whole-array clamp)
    out['pre_ms_uncertified'] = timed(lambda: M.update_on_pre(spk, tr, 0.0, 1.0, inplace=True), a.reps, before=void)
    out['post_ms_uncertified'] = timed(lambda: M.update_on_post(tr, spk, 0.0, 1.0, inplace=True), a.reps, before=void)
    out['pre_bytes_per_synapse'] = 12
    out['pre_TBps_at_12B'] = upd * 12 / (out['pre_ms_unclipped'] * 1e-3) / 1e12
    out['post_updates_per_s'] = int(spk.sum()) * a.conn / (out['post_ms_unclipped'] * 1e-3)   # (same expected count per column)
    # refresh of the scatter plan after an in-place update
    del M.buffers['plasticity_index']
    for keep in (False, True):
        M.buffers.pop('scatter_plan', None)
        M.prepare(keep_order=keep)
        x = be.BinaryArray(spk)
        for _ in range(3):
            x @ M
        torch.cuda.synchronize()
        steady = timed(lambda: x @ M, a.reps)
        after = timed(lambda: x @ M, a.reps, before=lambda: (M.update_on_pre(spk, tr, inplace=True), torch.cuda.synchronize()))
        route = type(M.buffers.get('scatter_plan')).__name__
        out[f'product_ms_steady_keep_order_{keep}'] = steady
        out[f'refresh_ms_keep_order_{keep}'] = after - steady
        out[f'route_keep_order_{keep}'] = route
    del M
    torch.cuda.empty_cache()
    # the reference's published point
    R = be.CSR.fromdense((torch.rand((5000, 5000), device=dev, generator=g) < 0.1).float()
                         * torch.rand((5000, 5000), device=dev, generator=g))
    s5 = torch.rand(5000, device=dev, generator=g) < 0.1
    t5 = torch.rand(5000, device=dev, generator=g)
    R.update_on_pre(s5, t5, inplace=True)
    out['ref_point_ms'] = timed(lambda: R.update_on_pre(s5, t5, inplace=True), a.reps)
    out['ref_point_reference_ms'] = 2.30
    print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == '__main__':
    main()
