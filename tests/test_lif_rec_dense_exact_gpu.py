"""csrc/be_neuron_sg_rec_dense.hip on the device, exactly and in every kernel instance: the C entry points on
crafted spike masks, sizes and addresses, against tests/lif_rec_dense_cases.py.  Every forward comparison is an equality of bits
with ``forward_dense`` (``lif_rec_sg_cases.forward`` on the stored matrix, summed from the rows of ``W``); ``g_s0`` is an equality
of bits with ``row_product``, the statement of ``dense_rows``' order of additions; aligned against unaligned ``W`` and a sample in
a batch against the sample alone are equalities of bits.  The one tolerance is the propagated bound of
``lif_rec_sg_cases.backward``, for the backward outputs behind the in-loop product.  Every output buffer starts full of SENTINEL with
a padded tail that must keep it.  The sizes come from the tables of tests/lif_rec_dense_cases.py, which
tests/test_lif_rec_dense_thresholds_cpu.py ties to the source."""
import functools

import numpy as np
import pytest
import torch

import lif_rec_dense_cases as D
import lif_rec_sg_cases as C
from lif_rec_sg_cases import F, Params, same_bits
from test_lif_rec_dense_gpu import BWD, FWD, RESET, SENTINEL, SURROGATE, out
from test_lif_rec_sg_gpu import dev, host, within

pytestmark = pytest.mark.gpu

#: the crafted masks are forced through x = +-FORCE: with these decays a neuron's current and membrane never outweigh one input
FORCE = F(100.0)
CRAFT = dict(syn_decay=0.25, beta=0.25)


@functools.lru_cache(maxsize=4)
def dense_w(N, seed=0):
    """Dense N(0, 0.05) weights and the exponent of their stored matrix; read-only."""
    W = np.random.default_rng(seed).standard_normal((N, N), dtype=F) * F(0.05)
    W.setflags(write=False)
    return W, D.exponent(W)


@functools.lru_cache(maxsize=None)
def case(T, B, N, seed=0):
    x, s0, state, grads = C.inputs(T, B, N, seed)
    for a in (x, s0) + state + grads:
        a.setflags(write=False)
    return x, s0, state, grads


def forced(mask):
    """The step input that makes exactly ``mask`` spike."""
    return np.where(mask, FORCE, -FORCE).astype(F)


def on_device(W, offset=0):
    """``W`` on the device, ``offset`` elements past a 16-byte boundary inside a larger buffer."""
    N = W.shape[0]
    buf = torch.zeros(N * N + 8, dtype=torch.float32, device='cuda')
    w = buf[offset:offset + N * N].view(N, N)
    w.copy_(dev(W))
    assert w.data_ptr() % 16 == 4 * offset and w.is_contiguous()
    return w


def scalars(p):
    return p.syn_decay, p.beta, p.v_th, p.v_reset, p.rho, p.kappa


def forward(w, x, s0, state, p, e):
    """``be_lif_rec_dense_sg_forward`` into SENTINEL-filled buffers: name -> ``(view, whole)``."""
    from brainevent_amd import _array as A, _lib
    T, B, N = x.shape
    ins = [dev(x), w, dev(s0)] + [dev(a) for a in state]
    outs = dict(zip(FWD, [out(T, B, N) for _ in range(4)] + [out(B, N) for _ in range(3)]))
    rc = _lib.fn('be_lif_rec_dense_sg_forward')(*[A.ptr(t) for t in ins], *[A.ptr(outs[n][0]) for n in FWD], T, B, N, *scalars(p),
                                                RESET[p.reset], int(p.adaptive), e, A.stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return outs


def backward(w, h_save, th_save, grads, p):
    """``be_lif_rec_dense_sg_backward`` on host arrays of what a forward call saved: name -> ``(view, whole)``."""
    from brainevent_amd import _array as A, _lib
    T, B, N = h_save.shape
    ins = [dev(h_save), dev(th_save), w] + [dev(g) for g in grads]
    outs = dict(zip(BWD, [out(T, B, N)] + [out(B, N) for _ in range(4)]))
    rc = _lib.fn('be_lif_rec_dense_sg_backward')(*[A.ptr(t) for t in ins], *[A.ptr(outs[n][0]) for n in BWD], T, B, N, *scalars(p),
                                                 RESET[p.reset], SURROGATE[p.surrogate], p.alpha, int(p.adaptive),
                                                 int(p.detach_reset), A.stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return outs


def tails_kept(outs, ref, what):
    """An output the mode does not write is all SENTINEL, and so is every tail."""
    for name, (view, whole) in outs.items():
        kept = whole if getattr(ref, name) is None else whole[view.numel():]
        assert bool((kept == SENTINEL).all()), (name, what)


def equal_bits(outs, ref, what):
    tails_kept(outs, ref, what)
    for name, (view, _) in outs.items():
        want = getattr(ref, name)
        if want is not None:
            got = host(view)
            assert same_bits(got, want), (name, what, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())


def same_outputs(a, b, what):
    assert all(same_bits(host(a[n][1]), host(b[n][1])) for n in a), what


def one_sample(arrays, b):
    return tuple(None if a is None else np.ascontiguousarray(a[..., b:b + 1, :]) for a in arrays)


# ================================================================================================================ forward
@pytest.mark.parametrize('N', [n for sizes in D.COUNT_N.values() for n in sizes])
def test_active_row_counts(be, N):
    """One sample per (count, placement): the mask of step 0 is ``s0``, the mask of step 1 is forced through ``x[0]``."""
    combos = [(A, how) for A in D.active_counts(N) for how in D.PLACEMENTS]
    masks = np.stack([D.place(N, A, how) for A, how in combos])
    T, B = 2, len(combos)
    W, e = dense_w(N)
    _, _, state, _ = case(T, B, N)
    x = np.stack([forced(masks), case(T, B, N)[0][1]])
    p = Params(adaptive=N % 3 == 0, reset='soft' if N % 2 else 'hard', **CRAFT)
    ref = D.forward_dense(x, W, masks.astype(F), *state, p, e)
    assert np.array_equal(ref.s_out[0] != 0, masks)
    for t in range(T):
        assert [bool(np.count_nonzero(ref.r[t, b])) for b in range(B)] == [bool(masks[b].any()) for b in range(B)]
    equal_bits(forward(on_device(W), x, masks.astype(F), state, p, e), ref, (N, combos))


@pytest.mark.parametrize('N', D.SEQUENCE_N)
def test_consecutive_masks(be, N):
    """``M0``, a disjoint ``M1``, ``M2`` inside ``M1``, then no spike: the double buffer and the cleared partial sums."""
    T, B = 4, 2
    rng = np.random.default_rng(N)
    order = np.stack([rng.permutation(N) for _ in range(B)])
    third = N // 3
    m0, m1, m2 = (np.zeros((B, N), bool) for _ in range(3))
    for b in range(B):
        m0[b, order[b, :third]] = True
        m1[b, order[b, third:2 * third]] = True
        m2[b, order[b, third:third + third // 2]] = True
    m0[0, 0], m1[0, 0], m2[0, 0], m1[0, N - 1], m2[0, N - 1] = True, False, False, True, True
    m0[0, N - 1] = False
    assert not (m0 & m1).any() and not (m2 & ~m1).any() and (m1 & ~m2).any()
    W, e = dense_w(N)
    _, _, state, _ = case(T, B, N, 1)
    x = np.stack([forced(m1), forced(m2), forced(np.zeros((B, N), bool)), case(T, B, N, 1)[0][3]])
    p = Params(adaptive=True, **CRAFT)
    ref = D.forward_dense(x, W, m0.astype(F), *state, p, e)
    assert np.array_equal(ref.s_out[0] != 0, m1) and np.array_equal(ref.s_out[1] != 0, m2) and not ref.s_out[2].any()
    assert all(np.count_nonzero(ref.r[t, b]) > N // 2 for t in range(3) for b in range(B)) and not ref.r[3].any()
    assert not same_bits(ref.r[1], ref.r[2]) and not same_bits(ref.r[0], ref.r[1])
    equal_bits(forward(on_device(W), x, m0.astype(F), state, p, e), ref, N)


@pytest.mark.parametrize('N', D.CHUNK_N)
def test_per_thread_chunks(be, N):
    """About 13 active rows in the first, a middle and the last mask word, row ``N - 1`` among them; dense random ``W``."""
    T, B = 2, 2
    W, e = dense_w(N)
    m0, m1 = (np.stack([D.spread_rows(N, seed + b) for b in range(B)]) for seed in (0, 10))
    _, _, state, _ = case(T, B, N, 2)
    x = np.stack([forced(m1), case(T, B, N, 2)[0][1]])
    p = Params(adaptive=N % 2 == 1, **CRAFT)
    ref = D.forward_dense(x, W, m0.astype(F), *state, p, e)
    assert np.array_equal(ref.s_out[0] != 0, m1) and m0[:, N - 1].all() and m1[:, N - 1].all()
    assert all(np.count_nonzero(ref.r[t, b]) > N // 2 for t in range(T) for b in range(B)) and 0 < ref.s_out[1].mean() < 1
    equal_bits(forward(on_device(W), x, m0.astype(F), state, p, e), ref, N)


@pytest.mark.parametrize('e,log2', D.EXPONENT_EDGES)
def test_exponent_edges(be, e, log2):
    """The two valid edges of the exponent.  No input and no start state: ``h_save[0]`` is the recurrent input itself."""
    T, B, N = 3, 2, D.EDGE_N
    W = D.edge_weights(e, log2)
    x, s0 = np.zeros((T, B, N), F), case(T, B, N, 3)[1]
    for p in (Params(v_th=0.0), Params(v_th=0.0, adaptive=True, reset='soft')):
        ref = D.forward_dense(x, W, s0, None, None, None, p, e)
        assert same_bits(ref.h_save[0], ref.r[0]) and np.isfinite(ref.h_save).all()
        assert (np.abs(ref.r[0]) >= np.finfo(F).tiny).all() and 0 < ref.s_out[0].mean() < 1 and np.count_nonzero(ref.r[1]) > N // 2
        equal_bits(forward(on_device(W), x, s0, (None, None, None), p, e), ref, (e, p))


@pytest.mark.parametrize('N', (64, 260))
def test_w_one_element_off_a_16_byte_boundary_forward(be, N):
    T, B = 3, 2
    W, e = dense_w(N)
    x, s0, state, _ = case(T, B, N, 4)
    p = Params(adaptive=True)
    ref = D.forward_dense(x, W, s0, *state, p, e)
    assert 0 < ref.s_out[:-1].mean() < 1 and np.count_nonzero(ref.r) > 0
    aligned, off = forward(on_device(W), x, s0, state, p, e), forward(on_device(W, 1), x, s0, state, p, e)
    equal_bits(aligned, ref, N)
    same_outputs(aligned, off, N)


@pytest.mark.parametrize('N', D.INDEPENDENCE_N)
def test_forward_samples_are_independent(be, N):
    """Nine different samples in one call: each has the bits of that sample alone."""
    T, B = 3, 9
    W, e = dense_w(N)
    x, s0, state, _ = case(T, B, N, 5)
    p = Params(adaptive=True)
    ref = D.forward_dense(x, W, s0, *state, p, e)
    assert all(0 < ref.s_out[:-1, b].mean() < 1 and np.count_nonzero(ref.r[:, b]) > 0 for b in range(B))
    assert len({ref.s_out[:, b].tobytes() for b in range(B)}) == B
    w = on_device(W)
    whole = forward(w, x, s0, state, p, e)
    equal_bits(whole, ref, N)
    for b in range(B):
        (xb, s0b), stateb = one_sample((x, s0), b), one_sample(state, b)
        alone = forward(w, xb, s0b, stateb, p, e)
        tails_kept(alone, ref, (N, b))
        assert all(same_bits(host(alone[n][0]), host(whole[n][0][..., b:b + 1, :])) for n in FWD), (N, b)


# ================================================================================================================ backward
def saved(T, B, N, p, seed):
    """What a forward call saves, from the restatement: ``(W, h_save, th_save, grads)``."""
    W, e = dense_w(N)
    x, s0, state, grads = case(T, B, N, seed)
    ref = D.forward_dense(x, W, s0, *state, p, e)
    return W, ref.h_save, ref.th_save, grads


def g_s0_is_the_row_product(W, outs, what):
    g_x0 = host(outs['g_x'][0])[0]
    assert np.isfinite(g_x0).all() and all(np.count_nonzero(g) > g.size // 2 for g in g_x0), what
    got, want = host(outs['g_s0'][0]), D.row_products(W, g_x0)
    assert same_bits(got, want), (what, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())


@pytest.mark.parametrize('N', [n for sizes in D.GS0_N.values() for n in sizes])
def test_g_s0_bits(be, N):
    """``g_s0`` is ``row_product`` of the device's own ``g_x[0]``, bit for bit (``T = 1``: only the final product runs); with
    ``T = 3`` the other outputs, behind the in-loop product, stay within the restatement's propagated bound."""
    B = 2 if N <= 1032 else 1
    for T, p in ((1, Params(adaptive=True)), (3, Params(reset='soft', surrogate='atan', v_reset=-0.25))):
        W, h, th, grads = saved(T, B, N, p, 6)
        outs = backward(on_device(W), h, th, grads, p)
        r, b = C.backward(h, th, D.stored(W), *grads[:4], grads[4] if p.adaptive else None, p, with_bound=True)
        tails_kept(outs, r, (N, T))
        for name in BWD:
            if getattr(r, name) is not None:
                within(outs[name][0], getattr(r, name), getattr(b, name), (name, N, T))
        g_s0_is_the_row_product(W, outs, (N, T))


def test_g_s0_bits_at_the_limit(be):
    """``N = 8192``, one step, a dense random ``W``: every lane of every row takes 32 trips."""
    T, B, N = 1, 1, D.GS0_LIMIT
    W, _ = dense_w(N)
    x, _, state, grads = case(T, B, N, 7)
    p = Params(adaptive=True)
    ref = C.forward(x, C.empty_matrix(N), None, *state, p, 0)          # (one step without s0: W is not read)
    outs = backward(on_device(W), ref.h_save, ref.th_save, grads, p)
    r, b = C.backward(ref.h_save, ref.th_save, C.empty_matrix(N), *grads, p, with_bound=True)   # (T = 1: only g_s0 reads W)
    tails_kept(outs, r, N)
    for name in BWD[:4]:
        within(outs[name][0], getattr(r, name), getattr(b, name), (name, N))
    g_s0_is_the_row_product(W, outs, N)


@pytest.mark.parametrize('N', D.FALLBACK_N)
def test_fallback_path(be, N):
    """``N % 4 == 0`` and ``W`` one element off a 16-byte boundary: the 4-byte loads give the bits of the 16-byte ones."""
    T, B = 3, 2
    p = Params(adaptive=True)
    W, h, th, grads = saved(T, B, N, p, 8)
    assert D.vec(N, 0) and not D.vec(N, 4)
    aligned, off = backward(on_device(W), h, th, grads, p), backward(on_device(W, 1), h, th, grads, p)
    same_outputs(aligned, off, N)
    g_s0_is_the_row_product(W, off, N)


@pytest.mark.parametrize('N', D.INDEPENDENCE_N)
def test_backward_samples_are_independent(be, N):
    T, B = 3, 9
    p = Params(adaptive=True)
    W, h, th, grads = saved(T, B, N, p, 9)
    w = on_device(W)
    whole = backward(w, h, th, grads, p)
    g_s0_is_the_row_product(W, whole, N)
    assert len({host(whole['g_x'][0])[:, b].tobytes() for b in range(B)}) == B
    for b in range(B):
        alone = backward(w, *one_sample((h, th), b), one_sample(grads, b), p)
        assert all(bool((alone[n][1][alone[n][0].numel():] == SENTINEL).all()) for n in BWD), (N, b)
        assert all(same_bits(host(alone[n][0]), host(whole[n][0][..., b:b + 1, :])) for n in BWD), (N, b)


# ================================================================================================================ from Python
def test_python_dense_at_an_element_offset(be):
    """``be.Dense`` over a contiguous view one element into a buffer keeps that offset down to the kernels."""
    T, B, N = 4, 3, 260
    W, e = dense_w(N)
    x, s0, state, grads = case(T, B, N, 11)
    p = Params(adaptive=True)
    results = []
    for offset in (0, 1):
        w = on_device(W, offset).requires_grad_()
        assert w.data_ptr() % 16 == 4 * offset
        leaves = [dev(a).requires_grad_() for a in (x,) + state + (s0,)]
        s, v_seq, last = be.recurrent_lif_sequence(leaves[0], be.Dense(w), tuple(leaves[1:4]), leaves[4], return_v=True, scale_exp=e,
                                                   **p.kwargs())
        got = torch.autograd.grad((s, v_seq) + tuple(last), leaves + [w], [dev(g) for g in grads])
        results.append([host(t) for t in (s, v_seq) + tuple(last) + tuple(got)])
    ref = D.forward_dense(x, W, s0, *state, p, e)
    assert same_bits(results[0][0], ref.s_out) and same_bits(results[0][1], ref.v_seq) and 0 < ref.s_out[:-1].mean() < 1
    assert len(results[0]) == 5 + 6 and all(np.count_nonzero(a) > 0 for a in results[0])
    assert all(same_bits(a, b) for a, b in zip(*results))
