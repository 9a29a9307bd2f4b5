"""The constants and host formulas the dense-recurrence GPU cases are sized by (tests/lif_rec_dense_cases.py: CONSTS, groups,
lanes_shift, vec) are the ones in csrc/be_neuron_sg_rec_dense.hip, the restatement restates what it says it does, and the case tables
reach every class of the kernels.  No GPU needed: the source is read as text.  When this fails after a retune, move the table with
the source and re-size the GPU cases named in the message."""
import re
import time
from pathlib import Path

import numpy as np
import pytest

import lif_rec_dense_cases as D
import lif_rec_sg_cases as C
from lif_rec_dense_cases import CONSTS
from lif_rec_sg_cases import F, Params, same_bits

SOURCE = Path(__file__).resolve().parent.parent / 'brainevent_amd' / 'csrc' / 'be_neuron_sg_rec_dense.hip'
EXACT = 'tests/test_lif_rec_dense_exact_gpu.py'

# table key -> (regular expression with one group, matches expected, GPU cases sized by it)
PATTERNS = {
    'kDenThreads': (r'constexpr int kDenThreads = (\d+);', 1, 'every case: COUNT_N, CHUNK_N and GS0_N'),
    'kDenMaxN': (r'constexpr int kDenMaxN = (\d+);', 1, 'test_per_thread_chunks[8191], test_g_s0_bits_at_the_limit'),
    'kDenGroupN': (r'constexpr int kDenGroupN = (\d+);', 1, 'test_active_row_counts (COUNT_N)'),
    'kDenRowBatch': (r'constexpr int kDenRowBatch = (\d+);', 1, 'test_active_row_counts (active_counts: 6G - 1, 6G, 6G + 1, 12G + 1)'),
    'kDenRows': (r'constexpr int kDenRows = (\d+), kDenChunks = \d+;', 1, 'test_g_s0_bits (GS0_N)'),
    'kDenChunks': (r'constexpr int kDenRows = \d+, kDenChunks = (\d+);', 1, 'test_g_s0_bits, test_fallback_path (GS0_N, FALLBACK_N)'),
    'kDenEarly': (r'constexpr int kDenEarly = (\d+);', 1, 'test_per_thread_chunks (CHUNK_N)'),
    'kWave': (r'constexpr int kWave = (\d+);', 1, 'every case'),
    'kDenMinExp': (r'constexpr int kDenMinExp = (-?\d+), kDenMaxExp = -?\d+;', 1, 'test_exponent_edges'),
    'kDenMaxExp': (r'constexpr int kDenMinExp = -?\d+, kDenMaxExp = (-?\d+);', 1, 'test_exponent_edges'),
}
SOURCES = {'kWave': SOURCE.parent / 'be_common.h'}

# the formulas tests/lif_rec_dense_cases.py restates on the host, and the lines row_product / forward_dense restate
FORMULA_TEXT = [
    # groups(N): the P loop of k_lif_rec_dense_forward
    ('  int P = kDenThreads;\n  if (N <= kDenGroupN) {\n    P = kWave;\n    while (P < N) P <<= 1;\n  }\n'
     '  const uint32_t G = (uint32_t)(kDenThreads / P);', 1),
    ('constexpr int kDenPerThread = kDenMaxN / kDenThreads;', 1),
    ('if ((ord++ & (G - 1u)) != g) continue;', 1),
    ('if (q < n) wv[q] = (w + (size_t)row * (size_t)N)[(uint32_t)j];', 1),
    # lanes_shift(N): the lsh loop of k_lif_rec_dense_backward
    ('  int lsh = 0;\n  while ((1 << lsh) < kWave && (kDenChunks << lsh) < ((N + 3) >> 2)) ++lsh;', 1),
    # vec(N, address)
    ('const int vec = N % 4 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0;', 1),
    # row_product: the lanes' chunks, the order inside a chunk, the butterfly
    ('for (int ch = sub; ch < chunks; ch += kDenChunks * L) {', 1),
    ('const int cu = ch + u * L;', 1),
    ('    s = j < N ? s + t0 : s;\n          s = j + 1 < N ? s + t1 : s;\n          s = j + 2 < N ? s + t2 : s;\n'
     '          s = j + 3 < N ? s + t3 : s;', 1),
    ('for (int off = L >> 1; off > 0; off >>= 1) s = s + __shfl_xor(s, off);', 1),
    ('#pragma clang fp contract(off)', 3),
    # forward_dense: the sum is scaled back in f64 and rounded once
    ('const float r = (float)((double)(long long)R[k] * inv);', 1),
    ('for (int q = 0; q < kDenRowBatch; ++q) acc[k] += fixed_from_f32(wv[q], scale);', 1),
]


def test_every_table_entry_has_a_pattern():
    assert set(PATTERNS) == set(CONSTS)


@pytest.mark.parametrize('key', sorted(PATTERNS))
def test_constant_matches_the_source(key):
    pattern, matches, cases = PATTERNS[key]
    source = SOURCES.get(key, SOURCE)
    found = re.findall(pattern, source.read_text())
    assert len(found) == matches, f"{key}: {source.name} holds /{pattern}/ {len(found)} times, not {matches} — look at {cases} in {EXACT}"
    assert {int(v) for v in found} == {CONSTS[key]}, (f"{key}: {source.name} says {sorted(set(found))}, tests/lif_rec_dense_cases.py "
                                                      f"assumes {CONSTS[key]}: re-size {cases} in {EXACT}")


def test_formulas_are_the_ones_restated():
    text = SOURCE.read_text()
    for line, times in FORMULA_TEXT:
        assert text.count(line) == times, (f"be_neuron_sg_rec_dense.hip holds {line!r} {text.count(line)} times, not {times}: "
                                           f"tests/lif_rec_dense_cases.py restates it on the host — move both together")


def test_formulas_restated():
    assert [D.groups(N) for N in (1, 64, 65, 128, 129, 512, 513, 8192)] == \
        [(64, 16), (64, 16), (128, 8), (128, 8), (256, 4), (512, 2), (1024, 1), (1024, 1)]
    assert [D.lanes_shift(N) for N in (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 8192)] == \
        [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    assert D.vec(64, 4096) and not D.vec(64, 4100) and not D.vec(65, 4096) and not D.vec(66, 4104)
    assert D.thread_chunks(1024) == (1, False) and D.thread_chunks(1025) == (2, True) and D.thread_chunks(8192) == (8, False)


def test_the_tables_reach_every_class():
    D.check_tables()


def test_active_counts_and_placements():
    assert D.active_counts(40) == [0, 1, 15, 16, 17, 40] and D.active_counts(513) == [0, 1, 2, 5, 6, 7, 13, 513]
    assert D.active_counts(1100) == [0, 1, 2, 5, 6, 7, 13, 1100] and D.active_counts(300) == [0, 1, 2, 3, 11, 12, 13, 25, 300]
    for N in (n for sizes in D.COUNT_N.values() for n in sizes):
        for A in D.active_counts(N):
            low, high, edges = (D.place(N, A, how) for how in D.PLACEMENTS)
            assert low.sum() == high.sum() == A and (A == 0 or (low[0] and high[N - 1]))
            on = np.flatnonzero(edges)
            assert len(on) == min(A, 2 * (N // 64) + (N % 64 > 0)) and all(i % 64 in (0, 63) for i in on)
    assert D.place(1100, 7, 'edges')[[0, 63, 64, 127, 128, 191, 192]].all() and D.place(1100, 2, 'edges')[[1087, 1088]].all()
    for N in D.CHUNK_N:
        rows = D.spread_rows(N, 0)
        assert 10 <= rows.sum() <= 13 and rows[0] and rows[63] and rows[N - 1] and rows[64 * ((N - 1) // 64)]


@pytest.mark.parametrize('N', (1, 7, 65, 260))
def test_forward_dense_is_forward_on_the_stored_matrix(N):
    rng = np.random.default_rng(N)
    W = rng.normal(0.0, 0.05, (N, N)).astype(F)
    W[rng.random((N, N)) < 0.1] = 0
    m = D.stored(W)
    for k, (T, B) in enumerate(((3, 2), (1, 1), (4, 3))):
        x, s0, state, _ = C.inputs(T, B, N, k)
        p = Params(adaptive=k != 1, reset='soft' if k == 2 else 'hard')
        args = (s0 if k != 1 else None, state[0], state[1], state[2] if p.adaptive else None, p, C.exponent(m) - k)
        a, b = C.forward(x, m, *args), D.forward_dense(x, W, *args)
        assert D.exponent(W) == C.exponent(m)
        assert all(q is None and w is None or same_bits(q, w) for q, w in zip(a, b))
        assert k == 1 or N == 1 or (np.count_nonzero(a.r) > 0 and 0 < a.s_out.mean() < 1)    # (k = 1: one step, no s0)


def test_forward_dense_wraps_as_the_stored_matrix_does():
    """Two rows of 2**30 at exponent 32 sum to 2**63: the int64 wraps in both restatements, to the same bits."""
    W = np.full((2, 2), 2.0 ** 30, F)
    x = np.zeros((1, 1, 2), F)
    args = (np.ones((1, 2), F), None, None, None, Params(), 32)
    a, b = C.forward(x, D.stored(W), *args), D.forward_dense(x, W, *args)
    assert same_bits(a.r, b.r) and (a.r == F(-2.0 ** 31)).all()


@pytest.mark.parametrize('N', sorted({n for sizes in D.GS0_N.values() for n in sizes} | {2, 3, 4, 5, 12, 31, 511, 1029}))
def test_row_product_is_a_product(N):
    """Within ``N * 2**-24 * sum |W[i, j] G[j]|`` of the f64 product — and, where one lane adds everything, the plain ascending sum."""
    rng = np.random.default_rng(N)
    W, G = rng.normal(0.0, 0.05, (N, N)).astype(F), rng.normal(0.0, 1.0, N).astype(F)
    got = D.row_product(W, G, N)
    terms = W.astype(np.float64) * G.astype(np.float64)
    assert got.dtype == F and (np.abs(got - terms.sum(axis=1)) <= N * 2.0 ** -24 * np.abs(terms).sum(axis=1)).all()
    if D.lanes_shift(N) == 0:
        plain = np.zeros(N, F)
        for j in range(N):
            plain = plain + W[:, j] * G[j]
        assert same_bits(got, plain)


def test_row_product_order_by_hand():
    """N = 12 (three chunks, two lanes): lane 0 adds elements 0..3 then 8..11, lane 1 elements 4..7; then lane 0 + lane 1."""
    N = 12
    rng = np.random.default_rng(5)
    W, G = rng.normal(0.0, 1.0, (N, N)).astype(F), rng.normal(0.0, 1.0, N).astype(F)
    want = np.empty(N, F)
    for i in range(N):
        lane = [F(0), F(0)]
        for sub, js in ((0, (0, 1, 2, 3, 8, 9, 10, 11)), (1, (4, 5, 6, 7))):
            for j in js:
                lane[sub] = F(lane[sub] + F(W[i, j] * G[j]))
        want[i] = F(lane[0] + lane[1])
    assert same_bits(D.row_product(W, G, N), want)
    flipped = np.zeros(N, F)
    for j in range(N):
        flipped = flipped + W[:, j] * G[j]
    assert not same_bits(want, flipped), 'the order is visible at these values'


def test_row_product_at_the_limit_is_quick():
    N = CONSTS['kDenMaxN']
    rng = np.random.default_rng(0)
    W, G = rng.standard_normal((N, N), dtype=F), rng.standard_normal(N, dtype=F)
    start = time.perf_counter()
    got = D.row_product(W, G, N)
    took = time.perf_counter() - start
    rows = np.array([0, 1, N // 2, N - 1])
    terms = W[rows].astype(np.float64) * G.astype(np.float64)
    assert (np.abs(got[rows] - terms.sum(axis=1)) <= N * 2.0 ** -24 * np.abs(terms).sum(axis=1)).all()
    assert took < 1.0, took


@pytest.mark.parametrize('e,log2', D.EXPONENT_EDGES)
def test_exponent_edge_weights_are_within_fixed_from_f32(e, log2):
    """The weights of test_exponent_edges pass fixed_from_f32's own assertions at the edge, their sums stay far from 2**63, and the
    recurrent input they give is a normal f32."""
    W = D.edge_weights(e, log2)
    fixed = C.fixed_from_f32(W, e)
    assert np.abs(fixed.astype(np.float64)).sum(axis=0).max() < 2.0 ** 62
    r = D.recurrent_rows(W, np.ones(D.EDGE_N, bool), e)
    assert np.isfinite(r).all() and (np.abs(r) >= np.finfo(F).tiny).all()
    assert np.abs(np.log2(np.abs(r)).mean() - (log2 + 3)) < 2
