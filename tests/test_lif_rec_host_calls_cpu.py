"""The host path of the fused recurrent layer (brainevent_amd/_neuron_rec_sg.py), spied on without a device: which entry point every
recurrence family reaches, forwards and backwards, and with which arguments — each pointer named as the input tensor it is, NULL, or
a tensor the layer allocated ('fresh'), every scalar as it is — and what the autograd node keeps.  The technique is
test_lif_rec_sg_cpu.py::test_the_call's: ``FakeDevice`` tensors, containers made with ``object.__new__``, ``_neuron_rec_sg.call`` and
``A.stream_ptr`` replaced.  Only the public functions are called, and the expected transcripts are written from the argument order
of include/brainevent_amd.h (the counts are held to the ctypes table), not from the module: the file does not change when the host
path is restated.

Families: CSR; CSR with a tensor parameter; DelayedCSR at depth 3 with ``s0`` ``[B, N]``, ``[2, B, N]`` and None; Dense f32, f16 and
bf16; Float8Dense e4m3 and e5m2 — each crossed with adaptive or not, ``return_v`` or not, a state (and ``s0``) given or None, and
``T = 0`` versus ``T = 5`` at ``B = 3, N = 4``; ``N = 0`` once per family.  The weights and parameters are grad-free (their gradient
functions need a device); ``x``, and ``v0`` / ``s0`` where given, require grad."""
import ctypes
import itertools

import pytest
import torch

from test_lif_rec_delay_cpu import fake_delayed
from test_lif_rec_sg_cpu import fake_csr
from test_lif_syn_sg_cpu import FakeDevice

fake = FakeDevice.wrap
B, N, DEPTH, EXP, SCALE = 3, 4, 3, -3, 0.5
KW = dict(syn_decay=0.5, beta=0.25, v_th=2.0, v_reset=-0.5, reset='soft', surrogate='atan', alpha=4.0, detach_reset=True)
RHO, KAPPA = 0.75, 0.125
SOFT, ATAN, F16, BF16, E4M3, E5M2 = 1, 1, 2, 3, 0, 1       # BE_LIF_RESET_SOFT, BE_LIF_SG_ATAN, BE_F16, BE_BF16, BE_F8_E4M3, BE_F8_E5M2


def csr(be, n):
    rec = fake_csr(be, n, nse=None if n else 0)
    return rec, dict(w=rec.data, indices=rec.indices, indptr=rec.indptr)


def delayed(be, n):
    rec = fake_delayed(be, n, DEPTH, nse=None if n else 0)
    st = rec.stacked
    return rec, dict(w=st.data, indices=st.indices, indptr=st.indptr, row_mask=rec.row_mask)


def dense(dtype):
    def make(be, n):
        rec = object.__new__(be.Dense)
        rec.data, rec.shape = torch.zeros(n, n, dtype=dtype), (n, n)
        return rec, dict(w=rec.data)
    return make


def float8(fmt):
    def make(be, n):
        rec = object.__new__(be.Float8Dense)
        rec._dev, rec.fmt, rec.scale, rec.shape = torch.zeros(n, n, dtype=torch.uint8), fmt, SCALE, (n, n)
        return rec, dict(codes=rec._dev)
    return make


# family: the container, the two entry points and their argument counts, the arguments that stand for the matrix (with an empty
# matrix: 'fresh' where one unused element is handed over), whether the calls take an exponent, the past steps s0 holds (delays
# only: 'step' is s0 [B, N]), and the tensors the node keeps
FAMILIES = {
    'csr': (csr, 'be_lif_rec_sg_forward', 28, 'be_lif_rec_sg_backward', 30, ('w', 'indices', 'indptr'),
            ('fresh', 'fresh', 'indptr'), True, None, 5),
    'csr_param': (csr, 'be_lif_rec_sg_forward_params', 34, 'be_lif_rec_sg_backward_params', 43, ('w', 'indices', 'indptr'),
                  None, True, None, 13),
    'delay_step': (delayed, 'be_lif_rec_delay_sg_forward', 31, 'be_lif_rec_delay_sg_backward', 33,
                   ('w', 'indices', 'indptr', 'row_mask', DEPTH), ('fresh', 'fresh', 'indptr', 'NULL', DEPTH), True, 'step', 5),
    'delay_hist': (delayed, 'be_lif_rec_delay_sg_forward', 31, 'be_lif_rec_delay_sg_backward', 33,
                   ('w', 'indices', 'indptr', 'row_mask', DEPTH), ('fresh', 'fresh', 'indptr', 'NULL', DEPTH), True, 2, 5),
    'delay_none': (delayed, 'be_lif_rec_delay_sg_forward', 31, 'be_lif_rec_delay_sg_backward', 33,
                   ('w', 'indices', 'indptr', 'row_mask', DEPTH), ('fresh', 'fresh', 'indptr', 'NULL', DEPTH), True, 0, 5),
    'dense_f32': (dense(torch.float32), 'be_lif_rec_dense_sg_forward', 26, 'be_lif_rec_dense_sg_backward', 28, ('w',),
                  ('fresh',), True, None, 5),
    'dense_f16': (dense(torch.float16), 'be_lif_rec_dense_half_sg_forward', 27, 'be_lif_rec_dense_half_sg_backward', 29, ('w', F16),
                  ('fresh', F16), True, None, 5),
    'dense_bf16': (dense(torch.bfloat16), 'be_lif_rec_dense_half_sg_forward', 27, 'be_lif_rec_dense_half_sg_backward', 29, ('w', BF16),
                   ('fresh', BF16), True, None, 5),
    'f8_e4m3': (float8('e4m3'), 'be_lif_rec_dense_f8_sg_forward', 27, 'be_lif_rec_dense_f8_sg_backward', 30, ('codes', E4M3, SCALE),
                ('fresh', E4M3, SCALE), False, None, 2),
    'f8_e5m2': (float8('e5m2'), 'be_lif_rec_dense_f8_sg_forward', 27, 'be_lif_rec_dense_f8_sg_backward', 30, ('codes', E5M2, SCALE),
                ('fresh', E5M2, SCALE), False, None, 2),
}
FLAGS = list(itertools.product((False, True), repeat=3))    # adaptive, return_v, state (and s0) given


class Case:
    """One call's inputs.  ``grad``: x, and v0 / s0 where given, require grad."""

    def __init__(self, be, family, T, n, adaptive, return_v, given, grad):
        make, self.fwd, self.n_fwd, self.bwd, self.n_bwd, full, empty, self.exp, ages, self.kept = FAMILIES[family]
        self.family, self.T, self.n, self.adaptive, self.return_v, self.given, self.grad = family, T, n, adaptive, return_v, given, grad
        self.matrix = full if n else empty
        self.rec, arrays = make(be, n)
        self.leaf = arrays.get('w')
        leaf = lambda *shape: fake(torch.rand(shape)).requires_grad_(grad)
        self.x = leaf(T, B, n)
        self.c0, self.a0 = fake(torch.rand(B, n)), fake(torch.rand(B, n))
        self.v0 = leaf(B, n)
        self.state = None if not given else (self.c0, self.v0, self.a0) if adaptive else (self.c0, self.v0)
        self.ages = (1 if ages == 'step' else ages) if ages is not None else None
        if ages is None:
            self.s0 = leaf(B, n) if given else None
        else:
            self.s0 = leaf(B, n) if ages == 'step' else leaf(ages, B, n) if ages else None
        tensors = dict(arrays, x=self.x, s0=self.s0)
        if given:
            tensors.update(c0=self.c0, v0=self.v0, a0=self.a0)
        self.known = {t.data_ptr(): name for name, t in tensors.items() if t is not None and t.numel()}
        self.kw = dict(KW, return_v=return_v, scale_exp=EXP if self.exp else None)
        if adaptive:
            self.kw['adapt'] = (RHO, KAPPA)
        self.run = be.recurrent_lif_sequence
        if family == 'csr_param':               # beta per neuron, read on the device: the parametric entry points
            self.beta = fake(torch.full((n,), 0.25))
            self.known[self.beta.data_ptr()] = 'beta'
            self.kw['beta'] = self.beta
            self.run = be.parametric_recurrent_lif_sequence

    def __call__(self):
        outs = self.run(self.x, self.rec, self.state, self.s0, **self.kw)
        return outs[0], (outs[1] if self.return_v else None), outs[-1]

    def named(self, args):
        return [(self.known.get(a.value, 'fresh') if a.value else 'NULL') if isinstance(a, ctypes.c_void_p) else a for a in args]

    # ---------------------------------------------------------------------------- the transcripts, from the header's argument order
    def s0_part(self, t):
        return [t] if self.ages is None else [t, self.ages]

    def forward_args(self):
        on, rho, kappa = int(self.adaptive), (RHO if self.adaptive else 0.0), (KAPPA if self.adaptive else 0.0)
        state = ['c0', 'v0', 'a0' if self.adaptive else 'NULL'] if self.given else ['NULL'] * 3
        s0 = self.s0_part('NULL' if self.s0 is None else 's0')
        opt = lambda yes: 'fresh' if yes else 'NULL'
        last = ['fresh', 'fresh', opt(self.adaptive)]
        if self.family == 'csr_param':          # five (pointer, period) pairs; c_save only for syn_decay's gradient; a_save for th
            pairs = ['fresh', 1, 'beta', self.n, 'fresh', 1] + (['fresh', 1] * 2 if self.adaptive else ['NULL', 1] * 2)
            return (['x', *self.matrix, *s0, *state, *pairs, 'fresh', opt(self.return_v), opt(self.grad), 'NULL',
                     opt(self.grad and self.adaptive), *last, self.T, B, self.n, -0.5, SOFT, on, EXP, None])
        return (['x', *self.matrix, *s0, *state, 'fresh', opt(self.return_v), opt(self.grad), opt(self.grad and self.adaptive), *last,
                 self.T, B, self.n, 0.5, 0.25, 2.0, -0.5, rho, kappa, SOFT, on] + ([EXP] if self.exp else []) + [None])

    def backward_args(self):
        """The gradients of ``s`` and the last state arrive, ``v_seq``'s does not; wanted: x's, and v0's / s0's where given."""
        on, rho, kappa = int(self.adaptive), (RHO if self.adaptive else 0.0), (KAPPA if self.adaptive else 0.0)
        opt = lambda yes: 'fresh' if yes else 'NULL'
        g_in = ['fresh', 'NULL', 'fresh', 'fresh', opt(self.adaptive)]
        g_out = ['fresh', 'NULL', opt(self.given), 'NULL'] + self.s0_part(opt(self.s0 is not None))
        if self.family == 'csr_param':
            pairs = ['fresh', 1, 'beta', self.n, 'fresh', 1] + (['fresh', 1] * 2 if self.adaptive else ['NULL', 1] * 2)
            return (['h', 'NULL', 'th' if self.adaptive else 'NULL', 'NULL', 'NULL', *self.matrix, *g_in, *pairs,
                     *g_out, *['NULL'] * 5, self.T, B, self.n, -0.5, SOFT, ATAN, 4.0, on, 1, None])
        return (['h', 'th' if self.adaptive else 'NULL', *self.matrix, *g_in, *g_out, self.T, B, self.n, 0.5, 0.25, 2.0, -0.5, rho, kappa,
                 SOFT, ATAN, 4.0, on, 1, None])

    def saved_positions(self):
        """Where the forward call's arguments hold what the backward call names 'h' and 'th' (``a_save`` in th's place)."""
        h = 1 + len(self.matrix) + len(self.s0_part(0)) + 3 + (10 if self.family == 'csr_param' else 0) + 2
        return h, h + (2 if self.family == 'csr_param' else 1)


@pytest.fixture
def spied(monkeypatch):
    from brainevent_amd import _neuron_rec_sg
    calls = []
    monkeypatch.setattr(_neuron_rec_sg, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(_neuron_rec_sg.A, 'stream_ptr', lambda: None)
    return calls


def node_of(t):
    """The layer's autograd node behind an output (the public function reshapes it)."""
    fn = t.grad_fn
    while not hasattr(fn, 'saved_tensors'):
        fn = fn.next_functions[0][0]
    return fn


def check_forward(case, calls):
    """The forward transcript of a case that has just run; with no step nothing is called and the state passes through."""
    if case.T == 0 or (case.family == 'csr_param' and case.n == 0):
        assert calls == []
        return
    (name, args), = calls
    assert name == case.fwd and len(args) == case.n_fwd
    if case.n:
        assert case.named(args) == case.forward_args(), (case.family, case.named(args), case.forward_args())
    else:                                       # no neuron: every tensor of the call is empty; the matrix still has an address
        k = len(case.matrix)
        assert case.named(args[1:1 + k]) == list(case.matrix) and list(args[-len(case.forward_args()[-12:]):]) == case.forward_args()[-12:]


def test_the_counts_are_the_tables(be):
    from brainevent_amd import _abi
    for make, fwd, n_fwd, bwd, n_bwd, *_ in FAMILIES.values():
        assert (len(_abi.PROTOTYPES[fwd][1]), len(_abi.PROTOTYPES[bwd][1])) == (n_fwd, n_bwd), (fwd, bwd)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_forward_without_grad(be, spied, family):
    for T, (adaptive, return_v, given) in itertools.product((0, 5), FLAGS):
        del spied[:]
        case = Case(be, family, T, N, adaptive, return_v, given, grad=False)
        s, v_seq, last = case()
        check_forward(case, spied)
        assert s.shape == (T, B, N) and (v_seq is None) == (not return_v) and len(last) == 2 + adaptive and s.grad_fn is None
        if T == 0:
            for out, start in zip(last, (case.c0, case.v0, case.a0)):
                assert torch.equal(out, start if given else torch.zeros(B, N))


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_forward_and_backward(be, spied, family):
    for T, (adaptive, return_v, given) in itertools.product((0, 5), FLAGS):
        del spied[:]
        case = Case(be, family, T, N, adaptive, return_v, given, grad=True)
        s, v_seq, last = case()
        check_forward(case, spied)
        kept = node_of(s).saved_tensors
        assert len(kept) == case.kept
        if case.kept > 2:                       # h, th (a_save), s, the weights, s0
            assert kept[0] is not None and (kept[1] is None) == (not adaptive) and kept[2].data_ptr() == s.data_ptr()
            assert kept[3].data_ptr() == case.leaf.data_ptr() and (kept[4] is None) == (case.s0 is None)
        if spied:
            ih, ith = case.saved_positions()
            case.known.update({spied[0][1][k].value: name for k, name in ((ih, 'h'), (ith, 'th')) if spied[0][1][k].value})
        del spied[:]
        (s.sum() + sum(t.sum() for t in last)).backward()
        if T == 0:
            assert spied == []
        else:
            (name, args), = spied
            assert name == case.bwd and len(args) == case.n_bwd
            assert case.named(args) == case.backward_args(), (family, case.named(args), case.backward_args())
        assert case.x.grad.shape == (T, B, N) and (case.v0.grad is not None) == given
        assert case.s0 is None or case.s0.grad.shape == case.s0.shape
        if T == 0:                              # no step: the state's gradient passes through, s0's is zero
            assert (not given or torch.equal(case.v0.grad, torch.ones(B, N)))
            assert case.s0 is None or not case.s0.grad.any()


class Dropped(torch.autograd.Function):
    """Hands no gradient back: the node before it runs with every gradient None."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_no_gradient_arrives(be, spied, family):
    for adaptive, return_v, given in FLAGS:
        case = Case(be, family, 5, N, adaptive, return_v, given, grad=True)
        s, v_seq, last = case()
        del spied[:]
        Dropped.apply(s).sum().backward()
        assert spied == [] and case.x.grad is None and case.v0.grad is None


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_no_neuron(be, spied, family):
    """``N = 0``: the call is made (the parametric one is not), and an empty matrix hands over one unused element, not NULL."""
    case = Case(be, family, 5, 0, True, False, False, grad=False)
    s, _, last = case()
    check_forward(case, spied)
    assert s.shape == (5, B, 0) and len(last) == 3
    del spied[:]
    case = Case(be, family, 5, 0, True, False, False, grad=True)
    s, _, last = case()
    check_forward(case, spied)
    del spied[:]
    (s.sum() + sum(t.sum() for t in last)).backward()
    if family == 'csr_param':
        assert spied == []
    else:
        (name, args), = spied
        k = len(case.matrix)
        assert name == case.bwd and len(args) == case.n_bwd and case.named(args[2:2 + k]) == list(case.matrix)
        assert list(args[-15:]) == case.backward_args()[-15:]
