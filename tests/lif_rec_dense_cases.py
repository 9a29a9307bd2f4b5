"""Shared by tests/test_lif_rec_dense_thresholds_cpu.py and tests/test_lif_rec_dense_exact_gpu.py: the host restatement of
csrc/be_neuron_sg_rec_dense.hip and the case tables the GPU tests are sized by.  numpy only.

Forward: :func:`forward_dense` is ``lif_rec_sg_cases.forward`` with the recurrent input summed from the ROWS of ``W`` — the same
wrapping int64 sums of ``fixed_from_f32``, so the same bits as the restatement on the fully stored matrix, at O(active rows x N)
and without an ``N * N``-entry ``Matrix``.  Backward: :func:`row_product` is ``dense_rows``' own order of additions in f32 — the
statement of that order: ``g_s0`` is compared with it as an equality.

The constants (:data:`CONSTS`) and the three host formulas (:func:`groups`, :func:`lanes_shift`, :func:`vec`) are tied to the source
text by tests/test_lif_rec_dense_thresholds_cpu.py; :func:`check_tables` says which GPU cases to re-size when one of them moves."""
import numpy as np

import lif_rec_sg_cases as C
from lif_rec_sg_cases import F

#: the constants of csrc/be_neuron_sg_rec_dense.hip the GPU sizes are derived from
CONSTS = {'kDenThreads': 1024, 'kDenMaxN': 8192, 'kDenGroupN': 512, 'kDenRowBatch': 6, 'kDenRows': 4, 'kDenChunks': 2,
          'kDenEarly': 2, 'kWave': 64, 'kDenMinExp': -90, 'kDenMaxExp': 150}
K = CONSTS


# ------------------------------------------------------------------------------------------------ the host formulas
def groups(N):
    """``(P, G)`` of k_lif_rec_dense_forward: ``P`` columns per row group, ``G`` row groups."""
    P = K['kDenThreads']
    if N <= K['kDenGroupN']:
        P = K['kWave']
        while P < N:
            P <<= 1
    return P, K['kDenThreads'] // P


def lanes_shift(N):
    """``lsh`` of k_lif_rec_dense_backward: ``1 << lsh`` lanes work on a row."""
    lsh = 0
    while (1 << lsh) < K['kWave'] and (K['kDenChunks'] << lsh) < ((N + 3) >> 2):
        lsh += 1
    return lsh


def vec(N, address):
    """Whether the row product loads 16 bytes at a time."""
    return N % 4 == 0 and address % 16 == 0


def thread_chunks(N):
    """``(count, partial)``: how many neurons a forward thread can own, and whether the last such chunk is not full."""
    return -(-N // K['kDenThreads']), N % K['kDenThreads'] != 0


# ------------------------------------------------------------------------------------------------ the forward pass
def recurrent_rows(W, active, e):
    """``r [N]`` of one sample from the active rows of ``W``: ``lif_rec_sg_cases.recurrent_input`` on the stored matrix."""
    R = C.fixed_from_f32(W[np.flatnonzero(active)], e).sum(axis=0, dtype=np.int64)                  # (wraps, as the device's does)
    return (R.astype(np.float64) * np.ldexp(1.0, -e)).astype(F)


def forward_dense(x, W, s0, c0, v0, a0, p, e):
    """``lif_rec_sg_cases.forward(x, stored(W), ...)`` without the stored matrix: -> ``lif_rec_sg_cases.Forward``."""
    assert W.dtype == F and W.shape == (x.shape[2],) * 2
    return C.forward_with(x, lambda active: recurrent_rows(W, active, e), s0, c0, v0, a0, p)


def exponent(W):
    """``lif_rec_sg_cases.exponent`` of the stored matrix, from the columns of ``W``."""
    bound = np.abs(W).sum(axis=0, dtype=np.float64).max() * 1.001 if W.size else 0.0
    eb = int(np.frexp(bound)[1]) if bound > 0 else 0
    return int(np.clip(62 - eb, K['kDenMinExp'], K['kDenMaxExp']))


def stored(W):
    """The CSR that stores every entry of ``W``, as ``lif_rec_sg_cases`` takes it."""
    N = W.shape[0]
    return C.Matrix(W.reshape(-1), np.tile(np.arange(N, dtype=np.int32), N), (np.arange(N + 1) * N).astype(np.int32), N)


# ------------------------------------------------------------------------------------------------ the backward row product
def row_product(W, G, N):
    """``out[i] = sum_j W[i, j] * G[j]`` in ``dense_rows``' order, f32: lane ``sub`` of a row's ``L = 1 << lanes_shift(N)`` starts
    at 0 and adds the rounded products of the elements ``j < N`` of its 16-byte chunks ``sub, sub + L, ...`` in ascending ``j``; the
    ``L`` partial sums meet in the xor butterfly ``off = L / 2 .. 1``.  (The 4-byte path loads the same elements: one function.)"""
    assert W.dtype == F and G.dtype == F and W.shape == (N, N) and G.shape == (N,)
    L = 1 << lanes_shift(N)
    span = 4 * L                                                     # the elements one trip of a row's lanes covers
    s = np.zeros((N, L), F)
    for lo in range(0, N, span):
        prod = W[:, lo:lo + span] * G[lo:lo + span]                  # every product rounded on its own
        for k in range(4):                                           # element k of every lane's chunk, then the next
            term = prod[:, k::4]
            s[:, :term.shape[1]] = s[:, :term.shape[1]] + term
    lanes = np.arange(L)
    off = L >> 1
    while off:
        s = s + s[:, lanes ^ off]
        off >>= 1
    assert s.dtype == F
    return s[:, 0].copy()


def row_products(W, G):
    """:func:`row_product` for every sample of ``G [B, N]``."""
    return np.stack([row_product(W, g, W.shape[0]) for g in G])


# ------------------------------------------------------------------------------------------------ the case tables
#: forward, the crafted masks: per row-group count G one N with P > N and one with P == N (G = 1: past the groups, past a chunk)
COUNT_N = {16: (40, 64), 8: (100, 128), 4: (200, 256), 2: (300, 512), 1: (513, 1100)}
#: where the active rows sit: packed from row 0, packed up to row N - 1, on bits 0 and 63 of the mask words only
PLACEMENTS = ('low', 'high', 'edges')
#: consecutive masks (M0, a disjoint M1, M2 inside M1, none): a group count each way, one and three columns per thread
SEQUENCE_N = (100, 300, 513, 2049)
#: forward, the per-thread chunks: the last full one-wave word of chunk 1, the chunk's end, one neuron / one word into a late
#: (k >= kDenEarly) chunk, every count of chunks up to the limit with a partial last wave, word and chunk
CHUNK_N = (2047, 2048, 2049, 2112, 3500, 4100, 5121, 6208, 8191)
#: backward, g_s0 bit for bit: both ends of every lanes-per-row class
GS0_N = {0: (1, 8), 1: (9, 16), 2: (17, 32), 3: (33, 64), 4: (65, 128), 5: (129, 256), 6: (257, 260, 512, 513, 1032, 2052)}
GS0_LIMIT = 8192
#: backward, N % 4 == 0 with W one element off a 16-byte boundary: the 4-byte path for the second reason
FALLBACK_N = (64, 260, 1032)
#: the exponent's edges
EXPONENT_EDGES = ((-90, 118), (150, -100))                           # (e, log2 of the weights' scale)
EDGE_N = 65
INDEPENDENCE_N = (129, 1100)


def edge_weights(e, log2, seed=0):
    """N(0, 2**log2) weights for the exponent edge ``e`` (see EXPONENT_EDGES): their fixed-point values are around 2**(log2 + e)."""
    W = (np.random.default_rng(seed).normal(0.0, 1.0, (EDGE_N, EDGE_N)) * 2.0 ** log2).astype(F)
    W.setflags(write=False)
    return W


def active_counts(N):
    """The numbers of active rows run at ``N``: around one row per group, around a full batch per group and around two."""
    G, R = groups(N)[1], K['kDenRowBatch']
    return sorted({min(max(a, 0), N) for a in (0, 1, G - 1, G, G + 1, R * G - 1, R * G, R * G + 1, 2 * R * G + 1, N)})


def place(N, A, how):
    """At most ``A`` active rows of ``N`` as a bool mask (fewer only where 'edges' has no more bits)."""
    mask = np.zeros(N, bool)
    if how == 'low':
        mask[:A] = True
    elif how == 'high':
        mask[N - A:] = True
    else:
        bits = np.array([i for i in range(N) if i % 64 in (0, 63)])
        mask[bits[:A] if A % 2 else bits[len(bits) - min(A, len(bits)):]] = True      # from the first word, or up to the last
    return mask


def spread_rows(N, seed):
    """About 13 active rows: bits 0, 1 and 63 of the first word, five in a middle word, the last word's first bit and its last
    three rows (row ``N - 1`` among them), and one random row."""
    words, rng = -(-N // 64), np.random.default_rng(seed)
    mid = 64 * (words // 2)
    rows = [0, 1, 63, mid, mid + 1, mid + 31, mid + 62, mid + 63, 64 * (words - 1), N - 3, N - 2, N - 1, int(rng.integers(0, N))]
    mask = np.zeros(N, bool)
    mask[[r for r in rows if 0 <= r < N]] = True
    return mask


def check_tables():
    """Every class of the kernels is reached by a table above (a retune of a constant lands here: the message names the table)."""
    for G, sizes in COUNT_N.items():
        got = [groups(N) for N in sizes]
        assert all(g == G for _, g in got), f'COUNT_N[{G}] = {sizes} has row-group counts {[g for _, g in got]}: re-size ' \
                                            f'test_active_row_counts (tests/lif_rec_dense_cases.py, COUNT_N)'
        if G > 1:
            assert got[0][0] > sizes[0] and got[1][0] == sizes[1], f'COUNT_N[{G}] = {sizes} must hold one N below its P and one ' \
                                                                   f'equal to it, P = {[q for q, _ in got]}: re-size COUNT_N'
        else:
            assert sizes[0] == K['kDenGroupN'] + 1 and thread_chunks(sizes[1]) == (2, True), \
                f'COUNT_N[1] = {sizes}: the first N past the row groups and one past a column per thread — re-size COUNT_N'
    every = {groups(N)[1] for N in range(1, K['kDenMaxN'] + 1)}
    assert set(COUNT_N) == every, f'COUNT_N holds {sorted(COUNT_N)}, the kernel has the row-group counts {sorted(every)}: re-size ' \
                                  f'test_active_row_counts'
    for N in (n for sizes in COUNT_N.values() for n in sizes):
        counts, G, R = active_counts(N), groups(N)[1], K['kDenRowBatch']
        assert counts[0] == 0 and counts[-1] == N and (N <= R * G or {R * G, R * G + 1} <= set(counts)), (N, counts)
    forward_n = [n for sizes in COUNT_N.values() for n in sizes] + list(CHUNK_N)
    per_thread = K['kDenMaxN'] // K['kDenThreads']
    partial = {thread_chunks(N)[0] for N in forward_n if thread_chunks(N)[1]}
    assert partial == set(range(1, per_thread + 1)), f'chunks per thread with a partial last one: {sorted(partial)}, not 1 .. ' \
                                                     f'{per_thread}: re-size CHUNK_N (test_per_thread_chunks)'
    late = [N for N in CHUNK_N if thread_chunks(N)[0] > K['kDenEarly']]
    assert any(N % K['kWave'] for N in late) and any(N % 64 == 0 and N % K['kDenThreads'] for N in late) and \
        any(thread_chunks(N) == (K['kDenEarly'], False) for N in CHUNK_N) and max(CHUNK_N) == K['kDenMaxN'] - 1, \
        f'CHUNK_N = {CHUNK_N}: a partial wave and a partial chunk of whole words past chunk kDenEarly, the full early chunks, and ' \
        f'the odd N at the limit — re-size test_per_thread_chunks'
    assert all(thread_chunks(N)[0] in (1, K['kDenEarly'] + 1) for N in SEQUENCE_N[2:]) and \
        sorted(groups(N)[1] for N in SEQUENCE_N) == [1, 1, 2, 8], f'SEQUENCE_N = {SEQUENCE_N}: re-size test_consecutive_masks'
    top = K['kWave'].bit_length() - 1
    assert sorted(GS0_N) == list(range(top + 1)), f'GS0_N must hold every lsh 0 .. {top}: re-size test_g_s0_bits'
    for lsh, sizes in GS0_N.items():
        assert all(lanes_shift(N) == lsh for N in sizes), f'GS0_N[{lsh}] = {sizes} has lsh {[lanes_shift(N) for N in sizes]}: ' \
                                                          f're-size test_g_s0_bits (tests/lif_rec_dense_cases.py, GS0_N)'
        assert lsh == 0 or lanes_shift(sizes[0] - 1) == lsh - 1, f'GS0_N[{lsh}] must start at the first N of its class'
        assert lsh == top or lanes_shift(sizes[1] + 1) == lsh + 1, f'GS0_N[{lsh}] must hold the last N of its class'
    six = GS0_N[top]
    trip = 4 * K['kDenChunks'] * K['kWave']                            # the elements a row's lanes take in one trip
    assert any(N > trip and N % trip for N in six) and any(N > 2 * trip for N in six) and GS0_LIMIT == K['kDenMaxN'], \
        f'GS0_N[{top}] = {six}: a second lane trip with idle lanes and a third — re-size test_g_s0_bits'
    aligned = {vec(N, 0) for sizes in GS0_N.values() for N in sizes}
    assert aligned == {True, False} and all(vec(N, 0) and not vec(N, 4) for N in FALLBACK_N), \
        f'both row-product paths, and FALLBACK_N = {FALLBACK_N} on the 4-byte one by its address alone: re-size test_fallback_path'
    assert {lanes_shift(N) for N in FALLBACK_N} >= {3, top} and max(FALLBACK_N) > trip
    assert all(K['kDenMinExp'] == e or K['kDenMaxExp'] == e for e, _ in EXPONENT_EDGES) and len(EXPONENT_EDGES) == 2, \
        f'EXPONENT_EDGES = {EXPONENT_EDGES} must be the two valid edges: re-size test_exponent_edges'
