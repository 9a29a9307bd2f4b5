"""Shared by the FP8 dense tests: the CONSTS table of csrc/be_dense_f8.hip (tests/test_dense_f8_thresholds_cpu.py compares it with
the source), the dispatch restated on the host, the reference, and the shapes of the GPU cases with the bound each one crosses.

Reference: torch's CPU decode of the codes (`codes.float()`), multiplied as float64 with the 0/1 activity, rounded once to f32,
then multiplied by `np.float32(scale)` in f32.  The weights are drawn from +-{1 ... 8} (exact in e4m3 and in e5m2) and every
case asserts on the host that the sum of |w| over an output's active entries is below 2^24: every partial sum is then an exact
integer in any order, so the comparisons carry NO tolerance (the policy of tests/test_dense_kernels_at_scale_gpu.py)."""
import numpy as np
import torch

FORMATS = {'e4m3': torch.float8_e4m3fn, 'e5m2': torch.float8_e5m2}
NONFINITE_MASK = {'e4m3': 0x7f, 'e5m2': 0x7c}

CONSTS = {
    'k8Group': 4, 'k8MaxChunk': 32, 'k8Tile': 2048, 'k8Vec': 16,
    'masks.grid_cap': 2048, 'reduce.grid_cap': 2048, 'self_scan.max_tiles': 1024, 'scan.block': 1024,
    't.UNR': 4, 'nt.U': 2, 'nt.rows_per_block': 4, 'nt.grid_cap': 2048,
    'k8MfmaCols': 512, 'k8MfmaChunk': 64, 'mfma.D': 2, 'mfma.wg_target': 768, 'mfma.parts_clamp': 16, 't_mfma.min_nb': 8,
    'parts_for.target_one_group': 2048, 'parts_for.target': 1024, 'parts_for.cap_one_group': 32, 'parts_for.cap': 16,
}
K = CONSTS


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def route(shape, nb, transpose, aligned=True):
    """Which kernel f8_any picks for weights of `shape` (16-byte aligned base or not) and `nb` batch rows."""
    vec_ok = shape[1] % K['k8Vec'] == 0 and aligned
    if transpose:
        if vec_ok and nb >= K['t_mfma.min_nb']:
            return 't_mfma'
        return 't_vec16' if vec_ok else 't_vec1'
    return 'nt_vec16' if vec_ok else 'nt_vec1'


def groups_of(nb):
    return (min(nb, K['k8MaxChunk']) + K['k8Group'] - 1) // K['k8Group']


def parts_for(n, vec, n_groups):
    tasks = ((n + 64 * vec - 1) // (64 * vec)) * n_groups
    wgs = (tasks + 3) // 4
    one = n_groups == 1
    p = (K['parts_for.target_one_group'] if one else K['parts_for.target']) // max(wgs, 1)
    return max(1, min(p, K['parts_for.cap_one_group'] if one else K['parts_for.cap']))


def mfma_parts(n):
    tiles = (n + K['k8MfmaCols'] - 1) // K['k8MfmaCols']
    return max(1, min(K['mfma.wg_target'] // max(tiles, 1), K['mfma.parts_clamp']))


def mfma_geom(n, n_union):
    """(parts, K-steps in all, K-steps per part) of k8_densemm_mfma."""
    parts = mfma_parts(n)
    steps = (n_union + 15) // 16
    return parts, steps, (steps + parts - 1) // parts


def passes(nb):
    return (nb + K['k8MaxChunk'] - 1) // K['k8MaxChunk']


def n_tiles_of(k):
    return (k + K['k8Tile'] - 1) // K['k8Tile']


def list_launches(k, nb, transpose, aligned=True, n=16):
    """How f8_lists builds the lists of a pass: 'fused+self_scan' | 'fused+scan' | 'general' (masks, count, scan, write)."""
    r = route((k, n), nb, transpose, aligned)
    one_list = r == 't_mfma' or groups_of(nb) == 1
    if not one_list:
        return 'general'
    return 'fused+self_scan' if n_tiles_of(k) <= K['self_scan.max_tiles'] else 'fused+scan'


# ------------------------------------------------------------------------------------------------ operands and reference
def int_weights(seed, shape):
    """int8 from +-{1 ... 8}, no zeros."""
    v = np.random.default_rng([seed, 1]).integers(0, 16, shape, dtype=np.int8)
    return np.where(v < 8, v - 8, v - 7).astype(np.int8)


def codes_of(W8, fmt):
    """The FP8 tensor (CPU) of small-integer weights; the cast is exact (asserted)."""
    c = torch.from_numpy(W8.astype(np.float32)).to(FORMATS[fmt])
    assert np.array_equal(c.float().numpy(), W8.astype(np.float32)), 'the weights must be exact in the format'
    return c


def draw(seed, nb, k, firing, last=False):
    """[nb, k] bool, batch-major as the kernels take it.  `last`: entry k - 1 of batch row 0 set."""
    S = np.random.default_rng([seed, 2]).random((nb, k)) < firing
    if last and k:
        S[0, -1] = True
    return S


def float_values(S):
    """Float spikes from {0.7, 0, -1.0}: active when > 0, and only there."""
    off = np.random.default_rng(S.size + 1).random(S.shape) < 0.5
    return np.where(S, 0.7, np.where(off, 0.0, -1.0)).astype(np.float32)


def pack_rows(S):
    """[nb, k] bool (host) -> [nb, ceil(k / 32)] words on the device, bit i % 32 of word i // 32."""
    pad = (-S.shape[1]) % 32
    b = np.packbits(np.pad(S, ((0, 0), (0, pad))), axis=1, bitorder='little')
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int32)).cuda()


def decode64(codes):
    """torch's CPU decode of FP8 codes, as float64."""
    return codes.cpu().float().numpy().astype(np.float64)


def reference(codes, S, transpose, scale=1.0):
    """f32 [nb, out_len] as the issue states it; asserts the exactness condition."""
    W = decode64(codes)
    assert S.dtype == bool and S.shape[1] == (W.shape[0] if transpose else W.shape[1])
    A = S.astype(np.float64)
    absum = A @ (np.abs(W) if transpose else np.abs(W).T)
    assert np.array_equal(W, np.rint(W)) or np.array_equal(W * 2.0 ** 16, np.rint(W * 2.0 ** 16))
    assert absum.size == 0 or float(absum.max()) < 2 ** 24, 'every partial sum must be exact in f32'
    ref = (A @ (W if transpose else W.T)).astype(np.float32)
    return ref * np.float32(scale)


def operand(S, kind):
    """(device operand, spike dtype code).  kind: 'bool' | 'float' | 'bits'."""
    from brainevent_amd import _array as A
    if kind == 'bool':
        return torch.from_numpy(S).cuda(), A.BE_SPIKE_BOOL
    if kind == 'float':
        v = float_values(S)
        assert ((v > 0) == S).all() and (v < 0).any()
        return torch.from_numpy(v).cuda(), A.BE_SPIKE_FLOAT
    assert kind == 'bits'
    return pack_rows(S), A.BE_SPIKE_BITS


def misaligned(codes_dev):
    """A contiguous copy of a device FP8 matrix whose base is one byte off a 16-byte boundary."""
    n = codes_dev.numel()
    buf = torch.zeros(n + 32, dtype=torch.uint8, device=codes_dev.device)
    view = buf[1:1 + n].view(codes_dev.shape)
    view.copy_(codes_dev.view(torch.uint8))
    view = view.view(codes_dev.dtype)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


def run(codes_dev, S, kind, transpose, ref, tag, scale=1.0, expect=None):
    """One product through the package's host path (_dense_f8.dense_f8_batched -> be_binary_densemm_f8), compared exactly."""
    from brainevent_amd import _dense_f8 as F
    if expect is not None:
        got_route = route(tuple(codes_dev.shape), S.shape[0], transpose, codes_dev.data_ptr() % 16 == 0)
        assert got_route == expect, (tag, got_route, expect)
    op, sd = operand(S, kind)
    got = F.dense_f8_batched(codes_dev, scale, op, sd, transpose)
    tag = f'{tag} shape={tuple(codes_dev.shape)} nb={S.shape[0]} {codes_dev.dtype} {kind} transpose={transpose} scale={scale}'
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape, tag
    g = got.cpu().numpy()
    bad = np.flatnonzero(g.ravel() != ref.ravel())
    assert bad.size == 0, (f'{tag}: {bad.size} of {g.size} outputs differ, first at {np.unravel_index(bad[0], g.shape)}: '
                           f'{g.ravel()[bad[0]]!r} != {ref.ravel()[bad[0]]!r}')
    return got


def union(S, b0=0, nc=None):
    return int(S[b0:(None if nc is None else b0 + nc)].any(axis=0).sum())


def finite_codes(fmt):
    """uint8[256]: code c, the non-finite ones replaced by 0."""
    c = np.arange(256, dtype=np.uint8)
    m = NONFINITE_MASK[fmt]
    return np.where((c & m) == m, 0, c).astype(np.uint8)


def decode_table(fmt):
    """(codes uint8 [256, 32]: row c holds code c in every column (non-finite -> 0), decode float32 [256])."""
    c = finite_codes(fmt)
    table = np.repeat(c[:, None], 32, axis=1)
    dec = torch.from_numpy(c.copy()).view(FORMATS[fmt]).float().numpy()
    assert np.isfinite(dec).all()
    return table, dec


# ------------------------------------------------------------------------------------------------ the GPU cases' shapes
# (name, (k, n), nb, firing): S @ W8 on the MFMA route
MFMA_CASES = {
    # 16 parts, 79 steps per part: a second staged chunk of 15 steps (no multiple of the ring depth), the last part and the last
    # K step ragged; n = one tile + 16
    'two_chunks_16_parts': ((19_990, K['k8MfmaCols'] + 16), 9, 0.9),
    # 7 parts over 19 steps: 3 per part, the last part holds 1
    'seven_parts': ((300, 100 * K['k8MfmaCols']), 8, 0.5),
    # 1 part: 768 column tiles and a partly filled 769th
    'one_part': ((40, 768 * K['k8MfmaCols'] + 16), 8, 0.5),
    # 16 parts over 7 steps: parts 7 ... 15 have an empty K range
    'empty_ranges': ((100, K['k8MfmaCols'] + 16), 32, 0.3),
}


def cross_mfma():
    for name, ((k, n), nb, firing) in MFMA_CASES.items():
        assert route((k, n), nb, True) == 't_mfma' and n % K['k8Vec'] == 0, name
    (k, n), nb, firing = MFMA_CASES['two_chunks_16_parts']
    u = union(draw(11, nb, k, firing, last=True))
    parts, steps, per = mfma_geom(n, u)
    assert parts == 16 and per > K['k8MfmaChunk'] and (per - K['k8MfmaChunk']) % K['mfma.D'] != 0 and u % 16 != 0, (parts, steps, per, u)
    assert n == K['k8MfmaCols'] + 16
    (k, n), nb, firing = MFMA_CASES['seven_parts']
    parts, steps, per = mfma_geom(n, union(draw(12, nb, k, firing, last=True)))
    assert parts == 7 and 1 < per and (parts - 1) * per < steps < parts * per, (parts, steps, per)
    (k, n), nb, firing = MFMA_CASES['one_part']
    parts, steps, per = mfma_geom(n, union(draw(13, nb, k, firing, last=True)))
    assert parts == 1 and steps == per and n % K['k8MfmaCols'] == 16, (parts, steps, per)
    (k, n), nb, firing = MFMA_CASES['empty_ranges']
    parts, steps, per = mfma_geom(n, union(draw(14, nb, k, firing, last=True)))
    assert parts == 16 and per == 1 and steps < parts, (parts, steps, per)


MFMA_NBS = (8, 9, 32, 33, 65)

# S @ W8 on the vector route: (k, n), nb, firing, aligned, expected kernel, parts
T_VEC_CASES = {
    'more_rows_than_parts': ((500, 48), 1, 0.5, True, 't_vec16'),      # 32 parts, ~250 rows: the UNR loop and its tail
    'fewer_rows_than_parts': ((20, 48), 4, 0.5, True, 't_vec16'),      # 32 parts, ~19 rows
    'two_groups_two_strips': ((300, 1040), 7, 0.3, True, 't_vec16'),   # 16 parts, 2 groups, a second strip of 16 columns
    'odd_columns': ((300, 37), 4, 0.5, True, 't_vec1'),                # n % 16 != 0: the scalar-load variant
    'odd_columns_batched': ((70, 37), 33, 0.5, True, 't_vec1'),        # ... for a batch the MFMA route cannot take; two passes
    'misaligned': ((300, 48), 7, 0.5, False, 't_vec1'),                # a base pointer one byte off
}


def cross_t_vec():
    for name, ((k, n), nb, firing, aligned, expect) in T_VEC_CASES.items():
        assert route((k, n), nb, True, aligned) == expect, name
    (k, n), nb, firing, _, _ = T_VEC_CASES['more_rows_than_parts']
    S = draw(21, nb, k, firing, last=True)
    p = parts_for(n, 16, groups_of(nb))
    assert p == K['parts_for.cap_one_group'] and union(S) > K['t.UNR'] * p and union(S) % (K['t.UNR'] * p) != 0
    (k, n), nb, firing, _, _ = T_VEC_CASES['fewer_rows_than_parts']
    assert parts_for(n, 16, groups_of(nb)) == 32 and union(draw(22, nb, k, firing, last=True)) < 32
    (k, n), nb, firing, _, _ = T_VEC_CASES['two_groups_two_strips']
    assert groups_of(nb) == 2 and parts_for(n, 16, 2) == K['parts_for.cap'] and 64 * 16 < n < 2 * 64 * 16
    assert passes(T_VEC_CASES['odd_columns_batched'][1]) == 2


# W8 @ S.T: (m, k), nb, firing, aligned, expected kernel
NT_CASES = {
    'second_trip': ((K['nt.rows_per_block'] * K['nt.grid_cap'] + 3, 16), 8, 0.5, True, 'nt_vec16'),
    'unroll_and_tail': ((5, K['nt.U'] * 1024 + 1024 + 16), 33, 0.2, True, 'nt_vec16'),
    'odd_k': ((70, 40), 8, 0.5, True, 'nt_vec1'),
    'odd_k_long': ((9, 64 * K['nt.U'] + 64 + 7), 1, 0.5, True, 'nt_vec1'),
    'misaligned': ((70, 48), 33, 0.5, False, 'nt_vec1'),
    'k1': ((70, 1), 1, 1.0, True, 'nt_vec1'),
    'k15': ((70, 15), 8, 0.5, True, 'nt_vec1'),
    'k16': ((70, 16), 33, 0.5, True, 'nt_vec16'),
    'k17': ((70, 17), 8, 0.5, True, 'nt_vec1'),
}


def cross_nt():
    for name, ((m, k), nb, firing, aligned, expect) in NT_CASES.items():
        assert route((m, k), nb, False, aligned) == expect, name
    assert NT_CASES['second_trip'][0][0] > K['nt.rows_per_block'] * K['nt.grid_cap']
    k = NT_CASES['unroll_and_tail'][0][1]
    assert k % 16 == 0 and K['nt.U'] * 64 * 16 < k < 2 * K['nt.U'] * 64 * 16        # one unrolled round, then one tail piece
    k = NT_CASES['odd_k_long'][0][1]
    assert K['nt.U'] * 64 < k < 2 * K['nt.U'] * 64 and k % 16 != 0
    assert {c[1] for c in NT_CASES.values()} >= {1, 8, 33}


# spike kinds on every route; k % 32 != 0 throughout: (shape, nb, transpose, aligned, route)
KIND_CASES = [
    ((80, 272), 9, True, True, 't_mfma'),
    ((80, 48), 4, True, True, 't_vec16'),
    ((80, 37), 4, True, True, 't_vec1'),
    ((33, 48), 9, False, True, 'nt_vec16'),
    ((33, 41), 9, False, True, 'nt_vec1'),
]


def cross_kinds():
    for shape, nb, transpose, aligned, expect in KIND_CASES:
        assert route(shape, nb, transpose, aligned) == expect
        assert (shape[0] if transpose else shape[1]) % 32 != 0


# list building past the self-scan limit and past one trip of the scan: (k, n), nb, firing -> how the lists are built
SCAN_K = K['self_scan.max_tiles'] * K['k8Tile'] + 5
SCAN_CASES = {
    'one_group_scan': ((SCAN_K, 16), 1, 0.004, 'fused+scan', 't_vec16'),
    'two_groups_scan_second_trip': ((SCAN_K, 16), 5, 0.004, 'general', 't_vec16'),
    'union_scan': ((SCAN_K, 16), 8, 0.004, 'fused+scan', 't_mfma'),
    'union_at_the_limit': ((SCAN_K - 5, 16), 8, 0.004, 'fused+self_scan', 't_mfma'),
}


def cross_scan():
    for name, ((k, n), nb, firing, how, r) in SCAN_CASES.items():
        assert list_launches(k, nb, True, n=n) == how and route((k, n), nb, True) == r, name
    assert n_tiles_of(SCAN_K) == K['self_scan.max_tiles'] + 1 > K['scan.block'] and n_tiles_of(SCAN_K - 5) == K['self_scan.max_tiles']
    assert SCAN_K < 2 ** 28


def check_all_crossings():
    cross_scan()
    cross_mfma()
    cross_t_vec()
    cross_nt()
    cross_kinds()
