"""The LIF neuron with ``beta`` / ``v_th`` read from device memory (csrc/be_neuron_sg.hip, brainevent_amd/_neuron_sg.py) on the
device.  The two passes are compared with the numpy restatement of tests/lif_sg_param_cases.py as EQUALITIES, bit for bit
(``same_bits``), the per-slot gradient partials included; the reduce is compared with ``math.fsum`` within

    |f64(out[p]) - E| <= 2**-24 |E| + R 2**-52 A + 2**-149

(the final rounding to f32, and twice the first-order error of an R-term f64 sum in any order).  Nothing here is compared with
torch's device kernels.  tests/test_lif_sg_param_cpu.py holds the restatement to CPU autograd and the sizes used here to the
kernels' source."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lif_sg_cases as C
import lif_sg_param_cases as PC
from lif_sg_cases import F, Params, same_bits

pytestmark = pytest.mark.gpu

INVALID = -1
NULLABLE = ('g_v0', 'g_beta_slot', 'g_vth_slot')
NULL_SETS = [frozenset(c) for k in range(4) for c in itertools.combinations(NULLABLE, k)]


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()          # (a copy: the shared inputs are read-only)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def misaligned(a):
    """The same values as a contiguous device tensor whose base is 4 bytes past a 16-byte boundary (a sliced view)."""
    if a is None:
        return None
    a = np.asarray(a)
    flat = torch.empty(a.size + 1, dtype=torch.float32, device='cuda')
    flat[1:].copy_(torch.tensor(a.reshape(-1)))
    view = flat[1:].view(a.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def case(T, N, seed):
    arrays = C.inputs(T, N, seed)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def params(Pb, Pt, seed):
    arrays = PC.param_inputs(Pb, Pt, seed)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def ptr(t):
    from brainevent_amd import _array as A
    return A.ptr(t)


def c_forward(x, v0, beta, v_th, p, T, N, want_v=True, want_h=True):
    """be_lif_sg_forward_params on device tensors: ``(status, s, v_seq, h, v_last)``; outputs are pre-filled with 7."""
    from brainevent_amd import _array as A, _lib
    s, v_seq, h = (torch.full((T, N), 7.0, device='cuda') for _ in range(3))
    v_last = torch.full((N,), 7.0, device='cuda')
    rc = _lib.fn('be_lif_sg_forward_params')(ptr(x), ptr(v0), ptr(beta), beta.numel(), ptr(v_th), v_th.numel(), ptr(s),
                                             ptr(v_seq if want_v else None), ptr(h if want_h else None), ptr(v_last), T, N,
                                             p.v_reset, C.RESETS.index(p.reset), A.stream_ptr())
    return rc, s, v_seq, h, v_last


def c_backward(h, v0, g_s, g_vseq, g_vlast, beta, v_th, p, T, N, null=frozenset(), wrap=None):
    """be_lif_sg_backward_params: ``(status, {name: tensor})``; the outputs named in ``null`` go in as NULL."""
    from brainevent_amd import _array as A, _lib
    make = (lambda shape: torch.full(shape, 7.0, device='cuda')) if wrap is None else (lambda shape: wrap(np.full(shape, 7.0, F)))
    out = {'g_x': make((T, N))}
    out.update({name: make((N,)) for name in NULLABLE if name not in null})
    rc = _lib.fn('be_lif_sg_backward_params')(ptr(h), ptr(v0), ptr(g_s), ptr(g_vseq), ptr(g_vlast), ptr(beta), beta.numel(), ptr(v_th),
                                              v_th.numel(), ptr(out['g_x']), ptr(out.get('g_v0')), ptr(out.get('g_beta_slot')),
                                              ptr(out.get('g_vth_slot')), T, N, p.v_reset, C.RESETS.index(p.reset),
                                              C.SURROGATES.index(p.surrogate), p.alpha, int(p.detach_reset), A.stream_ptr())
    return rc, out


def check_direct(T, N, Pb, Pt, p, which='all', nulls=(frozenset(),), wrap=dev, wrap_param=dev, use_v0=True, seed=0):
    """Both passes by direct C call at one size against the restatement; ``which``: the gradients that arrive; ``nulls``: the sets of
    outputs that go in as NULL, one backward call each."""
    x, v0, g_s, g_vseq, g_vlast = case(T, N, seed)
    beta, v_th = params(Pb, Pt, seed)
    if not use_v0:
        v0 = None
    use = C.GRAD_SETS[which]
    g_s, g_vseq, g_vlast = (g if u else None for g, u in zip((g_s, g_vseq, g_vlast), use))
    what = (T, N, Pb, Pt, p, which)
    fw_ref = PC.forward(x, v0, beta, v_th, p)
    bw_ref = dict(zip(('g_x',) + NULLABLE, PC.backward(fw_ref[2], v0, g_s, g_vseq, g_vlast, beta, v_th, p)))
    xd, v0d, bd, td = wrap(x), wrap(v0), wrap_param(beta), wrap_param(v_th)
    rc, *fw = c_forward(xd, v0d, bd, td, p, T, N)
    assert rc == 0, what
    for name, got, ref in zip(('s', 'v_seq', 'h_save', 'v_last'), fw, fw_ref):
        assert same_bits(host(got), ref), (name, what)
    gd = [wrap(g) for g in (g_s, g_vseq, g_vlast)]
    for null in nulls:
        rc, out = c_backward(fw[2], v0d, *gd, bd, td, p, T, N, null=null, wrap=None if wrap is dev else wrap)
        assert rc == 0 and set(out) == set(bw_ref) - null, what
        for name, got in out.items():
            assert same_bits(host(got), bw_ref[name]), (name, sorted(null), what)
    return fw_ref, bw_ref


def period_cases(N):
    """(beta's period, v_th's period): shared, one per slot, one per neuron under R = 2 and 3 rows, and two different ones."""
    out = {(1, 1), (N, N), (N, 1), (1, N)}
    for R in (2, 3):
        if N % R == 0 and N > R:
            out |= {(N // R, N // R), (N // R, 1)}
    if N % 6 == 0:
        out.add((N // 2, N // 3))
    return sorted(out)


# ======================================================================================================== sizes
@pytest.mark.parametrize('N', PC.N_SIZES + (84, 96))
def test_sizes_and_periods(N):
    """One slot, a wave less one, a wave, a wave and one; 84 and 96 for R = 2 and 3 with periods that are (28, 48, 32) and are not
    (42) a multiple of 4: the latter falls to the 4-byte kernel although N % 4 == 0.  One step, two, the ring's depth and its
    neighbours, and 25."""
    k = PC.CONSTS['kSgVec']
    assert N != 84 or {(42 % k == 0), (28 % k == 0)} == {False, True}
    for T in PC.T_SIZES:
        for (Pb, Pt), p in zip(period_cases(N), itertools.cycle((Params(), Params(reset='soft', surrogate='atan', v_reset=-0.25)))):
            fw_ref, bw_ref = check_direct(T, N, Pb, Pt, p, seed=T)
    assert N < 8 or (0 < fw_ref[0].mean() < 1 and all(np.abs(g).max() > 0 for g in bw_ref.values()))


@pytest.mark.parametrize('N', PC.N_PAST_ONE_PASS)
def test_past_one_pass_of_the_capped_grid(N):
    """A second trip of the grid-stride loop at T = 2: of the 4-byte kernel (one slot) and of the 16-byte kernel (one lane), with a
    per-neuron beta under three rows (both N are multiples of 3) and a shared v_th."""
    k = PC.CONSTS['kSgVec']
    assert N % 3 == 0 and (N % k == 0) == ((N // 3) % k == 0)
    check_direct(2, N, N // 3, 1, Params(surrogate='triangle', alpha=2.0), seed=3)


@pytest.mark.parametrize('N', (64, 96))
def test_bases_off_16_bytes(N):
    """A parameter base, and then every base, 4 bytes past a 16-byte boundary: only the alignment refuses the 16-byte kernel."""
    for T in (1, 6):
        for Pb, Pt in ((N, 1), (N // 2, N), (1, 1)):
            check_direct(T, N, Pb, Pt, Params(), wrap_param=misaligned)
            check_direct(T, N, Pb, Pt, Params(reset='soft', surrogate='triangle', alpha=2.0), wrap=misaligned, which='g_vseq',
                         nulls=(frozenset(), frozenset(NULLABLE)))


def test_one_element_tensor_equals_the_float_path():
    """A one-element tensor holding the f32 value of the float: every output of both passes equals the float entry points'."""
    from brainevent_amd import _array as A, _lib
    for N, mode in ((132, ('hard', 'fast_sigmoid', False)), (65, ('soft', 'atan', False)), (64, ('soft', 'triangle', True))):
        T = 6
        p = Params(beta=0.9, v_th=1.1, v_reset=-0.25, reset=mode[0], surrogate=mode[1], detach_reset=mode[2], alpha=2.0)
        x, v0, g_s, g_vseq, g_vlast = (dev(a) for a in case(T, N, 4))
        bd, td = dev(np.array([p.beta], F)), dev(np.array(p.v_th, F))
        rc, *new = c_forward(x, v0, bd, td, p, T, N)
        old = [torch.empty_like(t) for t in new]
        st = A.stream_ptr()
        assert rc == 0 and _lib.fn('be_lif_sg_forward')(ptr(x), ptr(v0), *(ptr(t) for t in old), T, N, p.beta, p.v_th, p.v_reset,
                                                        C.RESETS.index(p.reset), st) == 0
        assert all(same_bits(host(a), host(b)) for a, b in zip(new, old)) and 0 < float(old[0].mean()) < 1
        rc, out = c_backward(new[2], v0, g_s, g_vseq, g_vlast, bd, td, p, T, N)
        g_x, g_v0 = torch.empty_like(out['g_x']), torch.empty_like(out['g_v0'])
        assert rc == 0 and _lib.fn('be_lif_sg_backward')(ptr(old[2]), ptr(g_s), ptr(g_vseq), ptr(g_vlast), ptr(g_x), ptr(g_v0), T, N,
                                                         p.beta, p.v_th, p.v_reset, C.RESETS.index(p.reset),
                                                         C.SURROGATES.index(p.surrogate), p.alpha, int(p.detach_reset), st) == 0
        assert same_bits(host(out['g_x']), host(g_x)) and same_bits(host(out['g_v0']), host(g_v0))
        # ... and through the Python interface
        xt, vt = x.clone().requires_grad_(), v0.clone().requires_grad_()
        a = be_sequence(xt, vt, p, beta=p.beta, v_th=p.v_th)
        b = be_sequence(xt, vt, p, beta=bd, v_th=td)
        c = be_sequence(xt, vt, p, beta=p.beta, v_th=td)                    # one number, one tensor: the new path
        for other in (b, c):
            assert all(same_bits(host(i), host(j)) for i, j in zip(a, other))
            ga = torch.autograd.grad(a, [xt, vt], [g_s, g_vseq, g_vlast], retain_graph=True)
            gb = torch.autograd.grad(other, [xt, vt], [g_s, g_vseq, g_vlast])
            assert all(same_bits(host(i), host(j)) for i, j in zip(ga, gb))


def be_sequence(x, v0, p, beta, v_th, **kw):
    import brainevent_amd as be
    return be.lif_sequence(x, v0, beta=beta, v_th=v_th, v_reset=p.v_reset, reset=p.reset, surrogate=p.surrogate, alpha=p.alpha,
                           detach_reset=p.detach_reset, return_v=True, **kw)


# ======================================================================================================== modes
@pytest.mark.parametrize('reset,surrogate,detach', C.MODES)
def test_modes_gradient_sets_and_null_outputs(reset, surrogate, detach):
    """Every reset x surrogate x detach_reset, with g_s only, g_vlast only, g_vseq only and all three, with each subset of
    {g_v0, g_beta_slot, g_vth_slot} NULL: the outputs that are given do not change."""
    p = Params(reset=reset, surrogate=surrogate, detach_reset=detach, v_reset=-0.25, alpha=2.0 if surrogate == 'triangle' else 10.0)
    assert len(NULL_SETS) == 8
    for which in C.GRAD_SETS:
        for N, Pb, Pt in ((132, 44, 12), (65, 13, 5)):              # the 16-byte and the 4-byte kernel
            fw_ref, bw_ref = check_direct(5, N, Pb, Pt, p, which=which, nulls=NULL_SETS, seed=7)
            # (a detached hard reset without g_s has g_sp = 0: its v_th partials are all zero, rightly)
            assert 0 < fw_ref[0].mean() < 1 and np.count_nonzero(bw_ref['g_x']) > 0 and np.count_nonzero(bw_ref['g_beta_slot']) > 0
            assert np.count_nonzero(bw_ref['g_vth_slot']) > 0 or (reset == 'hard' and detach and which != 'g_s' and which != 'all')


def test_v0_null_is_zeros():
    for N, Pb, Pt in ((64, 32, 64), (65, 13, 1)):
        for p in (Params(), Params(reset='soft')):
            check_direct(5, N, Pb, Pt, p, use_v0=False)
            x, _, g_s, g_vseq, g_vlast = (dev(a) for a in case(5, N, 0))
            bd, td = (dev(a) for a in params(Pb, Pt, 0))
            zeros = torch.zeros(N, device='cuda')
            rc_a, *a = c_forward(x, None, bd, td, p, 5, N)
            rc_b, *b = c_forward(x, zeros, bd, td, p, 5, N)
            assert rc_a == rc_b == 0 and all(same_bits(host(i), host(j)) for i, j in zip(a, b))
            _, ga = c_backward(a[2], None, g_s, g_vseq, g_vlast, bd, td, p, 5, N)
            _, gb = c_backward(a[2], zeros, g_s, g_vseq, g_vlast, bd, td, p, 5, N)
            assert all(same_bits(host(ga[k]), host(gb[k])) for k in ga)


# ======================================================================================================== edge values
def test_threshold_met_exactly_per_neuron():
    """h == th_i spikes, one ulp under it does not, with thresholds that differ across neurons (and rows that share them)."""
    th = np.array([0.5, 1.0, 1.5, 2.0, 0.75, 1.25, 3.0, 0.125], F)
    x = np.stack([np.tile(th, 2), np.tile(np.nextafter(th, F(0)), 2)])          # [2, 16]; beta = 0: h = x
    for reset in C.RESETS:
        p = Params(reset=reset, v_reset=-2.0)
        for wrap in (dev, misaligned):
            rc, s, v_seq, h, v_last = c_forward(wrap(x), None, dev(np.zeros(1, F)), wrap(th), p, 2, 16)
            assert rc == 0 and host(s).tolist() == [[1.0] * 16, [0.0] * 16]
            assert host(v_seq)[0].tolist() == ([-2.0] * 16 if reset == 'hard' else [0.0] * 16) and same_bits(host(v_last), x[1])
        ref = PC.forward(x, None, np.zeros(1, F), th, p)
        assert same_bits(host(s), ref[0]) and same_bits(host(v_seq), ref[1])


@pytest.mark.parametrize('drive,rate', ((-1.0, 0.0), (3.0, 1.0)))
def test_no_spike_at_all_and_a_spike_at_every_step(drive, rate):
    T, N = 6, 68
    x = np.full((T, N), drive, F)
    v0, g_s, g_vseq, g_vlast = case(T, N, 0)[1:]
    beta, v_th = params(17, 4, 0)
    for reset, surrogate, detach in C.MODES:
        p = Params(reset=reset, surrogate=surrogate, detach_reset=detach)
        ref = PC.forward(x, v0, beta, v_th, p)
        assert ref[0][1:].mean() == rate
        rc, *fw = c_forward(dev(x), dev(v0), dev(beta), dev(v_th), p, T, N)
        assert rc == 0 and all(same_bits(host(a), b) for a, b in zip(fw, ref))
        rc, out = c_backward(fw[2], dev(v0), dev(g_s), dev(g_vseq), dev(g_vlast), dev(beta), dev(v_th), p, T, N)
        bw_ref = dict(zip(('g_x',) + NULLABLE, PC.backward(ref[2], v0, g_s, g_vseq, g_vlast, beta, v_th, p)))
        assert rc == 0 and all(same_bits(host(out[k]), bw_ref[k]) for k in bw_ref), p


def test_nan_poisons_only_its_slot():
    T, N = 5, 72
    x, v0, g_s, g_vseq, g_vlast = (a.copy() for a in case(T, N, 0))
    x[1, 3] = x[0, 70] = np.nan
    beta, v_th = params(24, 36, 0)
    for reset in C.RESETS:
        p = Params(reset=reset)
        ref = PC.forward(x, v0, beta, v_th, p)
        rc, *fw = c_forward(dev(x), dev(v0), dev(beta), dev(v_th), p, T, N)
        assert rc == 0 and all(same_bits(host(a), b) for a, b in zip(fw, ref))
        rc, out = c_backward(fw[2], dev(v0), dev(g_s), dev(g_vseq), dev(g_vlast), dev(beta), dev(v_th), p, T, N)
        bw_ref = dict(zip(('g_x',) + NULLABLE, PC.backward(ref[2], v0, g_s, g_vseq, g_vlast, beta, v_th, p)))
        assert rc == 0 and all(same_bits(host(out[k]), bw_ref[k]) for k in bw_ref)
        for name in ('g_beta_slot', 'g_vth_slot'):
            assert list(np.flatnonzero(np.isnan(host(out[name])))) == [3, 70], name


def test_no_step_and_no_slot():
    import brainevent_amd as be
    beta, v_th = torch.full((5,), 0.9, device='cuda', requires_grad=True), torch.ones((), device='cuda', requires_grad=True)
    v0 = torch.ones(2, 5, device='cuda', requires_grad=True)
    s, v_last = be.lif_sequence(torch.empty(0, 2, 5, device='cuda'), v0, beta=beta, v_th=v_th)       # T = 0: the state passes through
    assert s.shape == (0, 2, 5) and host(v_last).tolist() == [[1.0] * 5] * 2
    gv, gb, gt = torch.autograd.grad(v_last, [v0, beta, v_th], torch.full((2, 5), 3.0, device='cuda'))
    assert host(gv).tolist() == [[3.0] * 5] * 2 and host(gb).tolist() == [0.0] * 5 and gt.shape == () and float(gt) == 0.0
    x = torch.empty(3, 0, device='cuda', requires_grad=True)                                         # N = 0
    s, v_last = be.lif_sequence(x, beta=torch.empty(0, device='cuda'), v_th=v_th)
    assert s.shape == (3, 0) and v_last.shape == (0,)
    assert torch.autograd.grad(s, x, torch.empty(3, 0, device='cuda'))[0].shape == (3, 0)


# ======================================================================================================== the reduce
def c_reduce(slot, N, P, out=None, ws_bytes=None):
    from brainevent_amd import _array as A, _lib
    need = _lib.fn('be_lif_sg_reduce_slots_workspace_bytes')(N, P)
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device='cuda') if nbytes else None
    out = torch.full((P,), 7.0, device='cuda') if out is None else out
    return _lib.fn('be_lif_sg_reduce_slots')(ptr(slot), N, P, ptr(out), ptr(ws), nbytes, A.stream_ptr()), out, need


REDUCE_CASES = [(N, 1) for N in PC.REDUCE_N_SHARED] + [(R * P, P) for P in PC.REDUCE_PERIODS for R in PC.REDUCE_ROWS]


@pytest.mark.parametrize('N,P', REDUCE_CASES)
def test_reduce_within_the_f64_bound_and_deterministic(N, P):
    R = N // P
    slot = PC.cancelling(R, P, seed=N + P)
    sd = dev(slot)
    rc, out, need = c_reduce(sd, N, P)
    assert rc == 0 and need == (8 * min(-(-N // PC.CONSTS['kSgpRedTile']), PC.CONSTS['kSgpRedGridCap']) if P == 1 else 0)
    got = host(out)
    err = np.abs(got.astype(np.float64) - PC.reduce_exact(slot, P))
    print(f'N {N} P {P}: max error {err.max():.3e}, bound there {PC.reduce_bound(slot, P)[err.argmax()]:.3e}')
    assert PC.within_reduce_bound(got, slot, P)
    rc, again, _ = c_reduce(sd, N, P)
    assert rc == 0 and np.array_equal(host(again).view(np.uint32), got.view(np.uint32))           # two calls: identical bits
    if R >= 33:                                    # the bound tells an f64 accumulation from a plain f32 running sum
        running = np.cumsum(slot.reshape(R, P), axis=0, dtype=F)[-1]
        assert not PC.within_reduce_bound(running, slot, P)


# ======================================================================================================== Python
def grads_against_the_restatement(x_shape, beta_of, vth_of, p, seed, need=(True, True)):
    """lif_sequence on x [T, B, n] with parameters made by ``beta_of`` / ``vth_of`` from leaves: the values, g_x and g_v0 are the
    restatement's bit for bit, each parameter gradient is within the reduce's bound of the restatement's per-slot partials."""
    T, slots = x_shape[0], x_shape[1:]
    N = int(np.prod(slots))
    x, v0, g_s, g_vseq, g_vlast = case(T, N, seed)
    (lb, beta), (lt, v_th) = beta_of(), vth_of()
    xt, vt = dev(x.reshape(x_shape)).requires_grad_(), dev(v0.reshape(slots)).requires_grad_()
    outs = be_sequence(xt, vt, p, beta=beta, v_th=v_th)
    bn, tn = (host(t).reshape(-1) if isinstance(t, torch.Tensor) else np.array([t], F) for t in (beta, v_th))
    fw_ref = PC.forward(x, v0, bn, tn, p)
    rx, rv0, slot_b, slot_t = PC.backward(fw_ref[2], v0, g_s, g_vseq, g_vlast, bn, tn, p)
    for got, ref in zip(outs, (fw_ref[0], fw_ref[1], fw_ref[3])):
        assert same_bits(host(got).reshape(ref.shape), ref)
    leaves = [xt, vt] + [leaf for leaf, n in zip((lb, lt), need) if n]
    got = list(torch.autograd.grad(outs, leaves, [dev(g.reshape(o.shape)) for g, o in zip((g_s, g_vseq, g_vlast), outs)]))
    assert same_bits(host(got[0]).reshape(T, N), rx) and same_bits(host(got[1]).reshape(N), rv0)
    return got[2:], (slot_b, slot_t), (bn, tn)


def test_parameter_gradients_in_the_tensor_s_shape(monkeypatch):
    """A leaf, a non-leaf (sigmoid(w)), a 0-d tensor, a [1] tensor and a [n] tensor under x [T, B, n]; a [B, n] tensor is its own
    slots.  Only the parameter that requires grad gets a gradient (the other's slot pointer is NULL)."""
    T, B, n = 5, 3, 44
    p = Params(reset='soft', v_reset=-0.25)

    def leaf(a):
        t = dev(np.asarray(a, F)).requires_grad_()
        return t, t
    for beta_shape, vth_shape in (((n,), (n,)), ((), (1,)), ((1,), ()), ((B, n), (n,)), ((n,), (B, n))):
        b0, t0 = PC.param_inputs(int(np.prod(beta_shape)), int(np.prod(vth_shape)), 5)
        (gb, gt), (slot_b, slot_t), _ = grads_against_the_restatement((T, B, n), lambda: leaf(b0.reshape(beta_shape)),
                                                                     lambda: leaf(t0.reshape(vth_shape)), p, seed=6)
        assert gb.shape == beta_shape and gt.shape == vth_shape
        assert PC.within_reduce_bound(host(gb), slot_b, b0.size) and PC.within_reduce_bound(host(gt), slot_t, t0.size)
        assert np.count_nonzero(host(gb)) and np.count_nonzero(host(gt))

    # a non-leaf: beta = sigmoid(w); the gradient reaches w through torch's own sigmoid backward
    w0 = np.log(PC.param_inputs(n, 1, 8)[0] / (1 - PC.param_inputs(n, 1, 8)[0])).astype(F)

    def sigmoid_of_w():
        w = dev(w0).requires_grad_()
        beta = torch.sigmoid(w)
        return (beta, beta)
    (gb,), (slot_b, _), (bn, _) = grads_against_the_restatement((T, B, n), sigmoid_of_w, lambda: (None, 1.0), p, seed=9, need=(True, False))
    assert gb.shape == (n,) and PC.within_reduce_bound(host(gb), slot_b, n)
    w = dev(w0).requires_grad_()
    s, _, v_last = be_sequence(dev(case(T, B * n, 9)[0].reshape(T, B, n)), None, p, beta=torch.sigmoid(w), v_th=1.0)
    (s.sum() + v_last.sum()).backward()
    assert w.grad is not None and w.grad.shape == (n,) and torch.count_nonzero(w.grad).item() > 0

    # only the parameter that requires grad gets one, and the other's partials are not computed
    from brainevent_amd import _neuron_sg
    for need in ((True, False), (False, True)):
        beta, v_th = dev(PC.param_inputs(n, 1, 5)[0]), dev(np.array(1.0, F))
        beta.requires_grad_(need[0]), v_th.requires_grad_(need[1])
        calls = []
        real = _neuron_sg.call

        def spy(name, *a):
            calls.append((name, a))
            return real(name, *a)
        with monkeypatch.context() as m:
            m.setattr(_neuron_sg, 'call', spy)
            s, _, v_last = be_sequence(dev(case(T, B * n, 9)[0].reshape(T, B, n)), None, p, beta=beta, v_th=v_th)
            (s.sum() + v_last.sum()).backward()
        assert (beta.grad is not None, v_th.grad is not None) == need
        args = dict(calls)['be_lif_sg_backward_params']
        assert (args[11].value is not None, args[12].value is not None) == need and args[10].value is None


def test_non_contiguous_parameter_is_made_contiguous():
    """beta as a column of an [n, 2] leaf: the values are the column's, and the gradient comes back into the column."""
    T, B, n = 4, 2, 44
    p = Params()
    x, v0, g_s, g_vseq, g_vlast = case(T, B * n, 12)
    b0, t0 = PC.param_inputs(n, n, 12)
    wide = dev(np.stack([b0, np.zeros_like(b0)], axis=1)).requires_grad_()
    beta = wide[:, 0]
    assert not beta.is_contiguous()
    outs = be_sequence(dev(x.reshape(T, B, n)), dev(v0.reshape(B, n)), p, beta=beta, v_th=dev(t0))
    fw_ref = PC.forward(x, v0, b0, t0, p)
    for got, ref in zip(outs, (fw_ref[0], fw_ref[1], fw_ref[3])):
        assert same_bits(host(got).reshape(ref.shape), ref)
    g, = torch.autograd.grad(outs, [wide], [dev(a.reshape(o.shape)) for a, o in zip((g_s, g_vseq, g_vlast), outs)])
    slot_b = PC.backward(fw_ref[2], v0, g_s, g_vseq, g_vlast, b0, t0, p)[2]
    g = host(g)
    assert g.shape == (n, 2) and PC.within_reduce_bound(g[:, 0], slot_b, n) and np.count_nonzero(g[:, 0]) and not g[:, 1].any()


@pytest.mark.parametrize('reset,surrogate,detach', C.MODES[::3] + C.MODES[1::5])
def test_sequence_equals_steps(reset, surrogate, detach):
    """Outputs, g_x and g_v0 bit for bit; the parameter gradients within the any-order f32 bound of their T * R terms, since
    autograd adds the per-step gradients in another order than the kernel adds a slot's steps."""
    import brainevent_amd as be
    T, B, n = 6, 3, 44
    N = B * n
    p = Params(reset=reset, surrogate=surrogate, detach_reset=detach, alpha=2.0 if surrogate == 'triangle' else 10.0)
    kw = dict(v_reset=p.v_reset, reset=p.reset, surrogate=p.surrogate, alpha=p.alpha, detach_reset=p.detach_reset)
    x, v0, g_s, g_vseq, g_vlast = case(T, N, 11)
    b0, t0 = PC.param_inputs(n, 1, 11)
    gs = [dev(g_s.reshape(T, B, n)), dev(g_vseq.reshape(T, B, n)), dev(g_vlast.reshape(B, n))]
    la = [dev(x.reshape(T, B, n)).requires_grad_(), dev(v0.reshape(B, n)).requires_grad_(), dev(b0).requires_grad_(), dev(t0).requires_grad_()]
    outs_a = be.lif_sequence(la[0], la[1], beta=la[2], v_th=la[3], return_v=True, **kw)
    lb = [dev(x.reshape(T, B, n)).requires_grad_(), dev(v0.reshape(B, n)).requires_grad_(), dev(b0).requires_grad_(), dev(t0).requires_grad_()]
    v, ss, vs = lb[1], [], []
    for t in range(T):
        s, v = be.lif_step(v, lb[0][t], beta=lb[2], v_th=lb[3], **kw)
        ss.append(s)
        vs.append(v)
    outs_b = (torch.stack(ss), torch.stack(vs), v)
    assert all(same_bits(host(a), host(b)) for a, b in zip(outs_a, outs_b))
    ga, gb = torch.autograd.grad(outs_a, la, gs), torch.autograd.grad(outs_b, lb, gs)
    assert same_bits(host(ga[0]), host(gb[0])) and same_bits(host(ga[1]), host(gb[1])) and torch.count_nonzero(ga[0]).item() > 0
    fw = PC.forward(x, v0, b0, t0, p)
    info = PC.backward(fw[2], v0, g_s, g_vseq, g_vlast, b0, t0, p, with_bound=True)[4]
    for name, i, P in (('beta', 2, n), ('vth', 3, 1)):
        bound = PC.any_order_bound(info[f'{name}_terms'], P)
        diff = np.abs(host(ga[i]).astype(np.float64) - host(gb[i]))
        print(f'{name}: max difference {diff.max():.3e}, bound there {bound[diff.argmax()]:.3e}')
        assert (diff <= bound).all() and np.count_nonzero(host(ga[i])) > 0, name


# ======================================================================================================== integration
class HostLif(torch.autograd.Function):
    """lif_step with per-neuron beta / v_th, both passes and the reduction computed by the restatement on the host."""
    slots = []

    @staticmethod
    def forward(ctx, v, x, beta, v_th, p):
        ctx.set_materialize_grads(False)
        bn, tn = host(beta).reshape(-1), host(v_th).reshape(-1)
        v0 = host(v).reshape(-1)
        s, _, h, v_new = PC.forward(host(x).reshape(1, -1), v0, bn, tn, p)
        ctx.saved = (h, v0, bn, tn, p, x.shape, beta.shape, v_th.shape)
        return dev(s).reshape(x.shape), dev(v_new).reshape(x.shape)

    @staticmethod
    def backward(ctx, g_s, g_v):
        h, v0, bn, tn, p, shape, b_shape, t_shape = ctx.saved
        g_x, g_v0, slot_b, slot_t = PC.backward(h, v0, None if g_s is None else host(g_s).reshape(1, -1), None,
                                                None if g_v is None else host(g_v).reshape(-1), bn, tn, p)
        HostLif.slots.append((slot_b, slot_t))
        return (dev(g_v0).reshape(shape), dev(g_x).reshape(shape), dev(PC.reduce_ref(slot_b, bn.size)).reshape(b_shape),
                dev(PC.reduce_ref(slot_t, tn.size)).reshape(t_shape), None)


def test_recurrent_loop_through_a_csr_parameter():
    """BinaryArray(s) @ csr -> lif_step, three steps, a Parameter in the CSR and per-neuron beta / v_th Parameters, against the same
    loop with the neuron computed on the host.  s, v, w.grad, x.grad, v0.grad are equal (weights and sums are small dyadic numbers:
    the scatter's sums are exact in any order).  beta.grad / v_th.grad are the f32 sums, in autograd's one order, of three per-step
    gradients that each differ by at most twice the reduce's bound: within ``sum 2 bound_t + 2 T 2**-24 sum |E_t|``."""
    import brainevent_amd as be
    rng = np.random.default_rng(21)
    batch, n, n_conn, T = 4, 96, 12, 3
    indptr = torch.arange(n + 1, dtype=torch.int32, device='cuda') * n_conn
    indices = dev(rng.integers(0, n, n * n_conn).astype(np.int32))
    w0 = (rng.integers(-8, 9, n * n_conn) / 32.0).astype(F)
    x0 = (rng.integers(0, 64, (T, batch, n)) / 32.0).astype(F)
    v00 = (rng.integers(-16, 32, (batch, n)) / 32.0).astype(F)
    b0, t0 = (rng.integers(2, 8, n) / 8.0).astype(F), (rng.integers(6, 11, n) / 8.0).astype(F)
    g_s, g_v = (rng.integers(-8, 9, (batch, n)) / 8.0).astype(F), (rng.integers(-8, 9, (batch, n)) / 8.0).astype(F)
    p = Params()
    kw = dict(v_reset=p.v_reset, reset=p.reset, surrogate=p.surrogate, alpha=p.alpha, detach_reset=p.detach_reset)

    def loop(neuron):
        w, beta, v_th = (torch.nn.Parameter(dev(a)) for a in (w0, b0, t0))
        csr = be.CSR((w, indices, indptr), shape=(n, n))
        x, v0 = dev(x0).requires_grad_(), dev(v00).requires_grad_()
        v, s, rate = v0, torch.zeros(batch, n, device='cuda'), []
        for t in range(T):
            s, v = neuron(v, x[t] + be.BinaryArray(s) @ csr, beta, v_th)
            rate.append(float(s.detach().mean()))
        ((s * dev(g_s)).sum() + (v * dev(g_v)).sum()).backward()
        return rate, [host(t) for t in (s, v, w.grad, x.grad, v0.grad)], [host(beta.grad), host(v_th.grad)]

    rate_a, a, pa = loop(lambda v, i, beta, v_th: be.lif_step(v, i, beta=beta, v_th=v_th, **kw))
    HostLif.slots = []
    rate_b, b, pb = loop(lambda v, i, beta, v_th: HostLif.apply(v, i, beta, v_th, p))
    assert all(0.05 < r < 0.95 for r in rate_a) and rate_a == rate_b
    for name, i, j in zip(('s', 'v', 'w.grad', 'x.grad', 'v0.grad'), a, b):
        assert same_bits(i, j) and np.count_nonzero(i) > 0, name
    assert len(HostLif.slots) == T
    for k, name in enumerate(('beta.grad', 'v_th.grad')):
        bound = sum(2 * PC.reduce_bound(sl[k], n) for sl in HostLif.slots)
        bound = bound + 2 * T * 2.0 ** -24 * sum(np.abs(PC.reduce_exact(sl[k], n)) for sl in HostLif.slots)
        diff = np.abs(pa[k].astype(np.float64) - pb[k])
        assert pa[k].shape == (n,) and (diff <= bound).all() and np.count_nonzero(pa[k]) > 0, name


def test_no_grad_keeps_nothing(monkeypatch):
    import brainevent_amd as be
    from brainevent_amd import _neuron_sg
    h_ptrs = []
    real = _neuron_sg.call

    def spy(name, *args):
        if name == 'be_lif_sg_forward_params':
            h_ptrs.append(args[8].value)
        return real(name, *args)
    monkeypatch.setattr(_neuron_sg, 'call', spy)
    x, v0, *_ = case(4, 132, 0)
    b0, t0 = params(44, 1, 0)
    xt, vt = dev(x.reshape(4, 3, 44)), dev(v0.reshape(3, 44))
    beta, v_th = dev(b0).requires_grad_(), dev(t0).requires_grad_()
    want = be.lif_sequence(xt, vt, beta=beta, v_th=v_th, return_v=True)            # only the parameters require grad
    assert h_ptrs[-1] is not None and all(o.grad_fn is not None for o in want)
    with torch.no_grad():
        got = be.lif_sequence(xt, vt, beta=beta, v_th=v_th, return_v=True)
        got1 = be.lif_step(vt, xt[0], beta=beta, v_th=v_th)
    plain = be.lif_sequence(xt, vt, beta=beta.detach(), v_th=v_th.detach(), return_v=True)      # nothing requires grad
    assert h_ptrs[-3:] == [None, None, None]
    for outs in (got, plain):
        assert all(o.grad_fn is None and not o.requires_grad for o in outs)
        assert all(same_bits(host(a), host(b)) for a, b in zip(outs, want))
    assert same_bits(host(got1[0]), host(want[0][0])) and got1[1].grad_fn is None


# ======================================================================================================== graph capture
def test_capture_forward_and_backward_follows_an_in_place_update():
    """A captured forward + backward step, replayed with new inputs and then after ``beta.data.mul_(0.5)``: the replay follows the
    new value, so nothing went through the host when the graph was recorded."""
    import brainevent_amd as be
    T, B, n = 3, 2, 100
    N = B * n
    p = Params(reset='soft', surrogate='atan')
    kw = dict(v_reset=p.v_reset, reset=p.reset, surrogate=p.surrogate, alpha=p.alpha, detach_reset=p.detach_reset)
    x_in, v_in = torch.zeros(T, B, n, device='cuda'), torch.zeros(B, n, device='cuda')
    g_in = [torch.zeros(T, B, n, device='cuda'), torch.zeros(T, B, n, device='cuda'), torch.zeros(B, n, device='cuda')]
    b0, t0 = params(n, 1, 2)
    beta, v_th = torch.nn.Parameter(dev(b0)), torch.nn.Parameter(dev(t0).reshape(()))

    def step():
        x, v0 = x_in.detach().requires_grad_(), v_in.detach().requires_grad_()
        s, v = be.lif_step(v0, x[0], beta=beta, v_th=v_th, **kw)
        outs = be.lif_sequence(x, v, beta=beta, v_th=v_th, return_v=True, **kw)
        return (s,) + tuple(outs) + tuple(torch.autograd.grad(outs, [x, v0, beta, v_th], g_in))

    def load(seed):
        for t, a in zip([x_in, v_in] + g_in, case(T, N, seed)):
            t.copy_(dev(a).reshape(t.shape))

    load(1)
    graphed = be.capture_step(step)
    replays = []
    for seed, scale in ((2, None), (3, None), (3, 0.5)):
        load(seed)
        if scale is not None:
            beta.data.mul_(scale)
        got = [t.detach().clone() for t in graphed()]
        want = step()
        assert all(same_bits(host(a), host(b)) for a, b in zip(got, want))
        assert 0 < float(got[1].mean()) < 1 and all(torch.count_nonzero(g).item() > 0 for g in got[-4:])
        replays.append(got)
    assert not same_bits(host(replays[1][2]), host(replays[2][2]))                 # the membranes moved with beta
    # ... and the last eager result is the restatement's at the halved beta
    x, v0, g_s, g_vseq, g_vlast = case(T, N, 3)
    bn = (b0 * F(0.5)).astype(F)
    assert same_bits(host(beta), bn)
    v1 = PC.forward(x[:1], v0, bn, t0, p)[3]
    fw = PC.forward(x, v1, bn, t0, p)
    assert same_bits(host(want[1]).reshape(T, N), fw[0]) and same_bits(host(want[2]).reshape(T, N), fw[1])


# ======================================================================================================== C error codes
def test_c_error_codes_then_a_clean_call():
    from brainevent_amd import _array as A, _lib
    fwd, bwd, red = (_lib.fn(f'be_lif_sg_{n}') for n in ('forward_params', 'backward_params', 'reduce_slots'))
    T, N, Pb, Pt = 3, 64, 32, 16
    x, v0, g_s, g_vseq, g_vlast = (dev(a) for a in case(T, N, 0))
    beta, v_th = (dev(a) for a in params(Pb, Pt, 0))
    s, v_seq, h, g_x = (torch.full((T, N), 7.0, device='cuda') for _ in range(4))
    v_last, g_v0, slot_b, slot_t = (torch.full((N,), 7.0, device='cuda') for _ in range(4))
    out, ws = torch.full((Pb,), 7.0, device='cuda'), torch.zeros(64, dtype=torch.float64, device='cuda')
    null, st = ptr(None), A.stream_ptr()

    def forward(x=ptr(x), beta=ptr(beta), Pb=Pb, v_th=ptr(v_th), Pt=Pt, s=ptr(s), v_last=ptr(v_last), T=T, N=N, mode=0):
        return fwd(x, ptr(v0), beta, Pb, v_th, Pt, s, ptr(v_seq), ptr(h), v_last, T, N, 0.0, mode, st)

    def backward(h=ptr(h), beta=ptr(beta), Pb=Pb, v_th=ptr(v_th), Pt=Pt, g_x=ptr(g_x), T=T, N=N, mode=0, sur=0, alpha=10.0):
        return bwd(h, ptr(v0), ptr(g_s), ptr(g_vseq), ptr(g_vlast), beta, Pb, v_th, Pt, g_x, ptr(g_v0), ptr(slot_b), ptr(slot_t), T, N,
                   0.0, mode, sur, alpha, 0, st)

    def reduce(slot=ptr(slot_b), N=N, P=Pb, out=ptr(out), ws=ptr(ws), nbytes=64 * 8):
        return red(slot, N, P, out, ws, nbytes, st)

    periods = (dict(Pb=0), dict(Pt=0), dict(Pb=-1), dict(Pb=3), dict(Pt=48), dict(Pb=128))
    for bad in periods + (dict(x=null), dict(beta=null), dict(v_th=null), dict(s=null), dict(v_last=null), dict(T=-1), dict(N=-1),
                          dict(mode=2)):
        assert forward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_sg_forward_params: ')
    for bad in periods + (dict(h=null), dict(beta=null), dict(v_th=null), dict(g_x=null), dict(T=-1), dict(N=-1), dict(mode=2),
                          dict(sur=3), dict(alpha=0.0), dict(alpha=float('nan'))):
        assert backward(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_sg_backward_params: ')
    need1 = _lib.fn('be_lif_sg_reduce_slots_workspace_bytes')(N, 1)
    assert need1 == 8 and _lib.fn('be_lif_sg_reduce_slots_workspace_bytes')(N, Pb) == 0
    for bad in (dict(P=0), dict(P=-1), dict(P=3), dict(P=128), dict(N=-1), dict(slot=null), dict(out=null),
                dict(P=1, nbytes=need1 - 1), dict(P=1, ws=null)):
        assert reduce(**bad) == INVALID, bad
        assert _lib.last_error().startswith('be_lif_sg_reduce_slots: ')
    # a zero period is refused before anything divides by it, also where there is nothing to do
    assert forward(T=0, Pb=0) == INVALID and backward(N=0, Pt=0) == INVALID
    # nothing to do: BE_OK and nothing written, whatever the pointers
    assert forward(T=0) == 0 and forward(N=0) == 0 and forward(T=0, x=null, beta=null, s=null, v_last=null) == 0
    assert backward(T=0) == 0 and backward(N=0) == 0 and backward(N=0, h=null, g_x=null) == 0 and reduce(N=0, slot=null, out=null) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (s, v_seq, h, g_x, v_last, g_v0, slot_b, slot_t, out))
    # a clean call after the refused ones
    p = Params()
    bn, tn = params(Pb, Pt, 0)
    fw_ref = PC.forward(host(x), host(v0), bn, tn, p)
    assert forward() == 0 and all(same_bits(host(a), b) for a, b in zip((s, v_seq, h, v_last), fw_ref))
    bw_ref = PC.backward(fw_ref[2], host(v0), host(g_s), host(g_vseq), host(g_vlast), bn, tn, p)
    assert backward() == 0 and all(same_bits(host(a), b) for a, b in zip((g_x, g_v0, slot_b, slot_t), bw_ref))
    assert reduce(ws=null, nbytes=0) == 0 and PC.within_reduce_bound(host(out), bw_ref[2], Pb)
    assert reduce(P=1) == 0 and PC.within_reduce_bound(host(out)[:1], bw_ref[2], 1)


# ======================================================================================================== Python refusals
def test_python_refusals(monkeypatch):
    import brainevent_amd as be
    from brainevent_amd import _neuron_sg

    def no_call(*a, **k):
        raise AssertionError('a refusal reached the device call')
    monkeypatch.setattr(_neuron_sg, 'call', no_call)
    v, x, seq = torch.zeros(3, 4, device='cuda'), torch.zeros(3, 4, device='cuda'), torch.zeros(5, 3, 4, device='cuda')
    for name in ('beta', 'v_th'):
        def both(value, error, match):
            with pytest.raises(error, match=match):
                be.lif_step(v, x, **{'beta': 0.9, name: value})
            with pytest.raises(error, match=match):
                be.lif_sequence(seq, v, **{'beta': 0.9, name: value})
        for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
            both(torch.ones(4, dtype=dtype, device='cuda'), TypeError, 'must be float32')
        both(torch.ones(4), ValueError, 'must be a device tensor')
        both(torch.ones(()), ValueError, 'must be a device tensor')
        for shape in ((3,), (5,), (4, 3), (1, 4), (1, 1), (5, 3, 4), (3, 4, 1)):
            both(torch.ones(shape, device='cuda'), ValueError, 'shape of the last dimensions')
