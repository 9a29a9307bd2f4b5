"""The gather kernels of csrc/be_csr.hip (CSR @ spikes: k_csrmv_nt_wave, k_csrmv_nt_vec, k_csrmm_nt_fused, k_csrmm_nt_fused_vec),
compared EXACTLY with the f64 oracle at the smallest shapes that reach each of their paths: every lanes-per-row tier with rows
around one pass, two passes and a second trip of the long-row walk, rows of one fixed length, the wave-per-row kernel around
its 256-entry head and 512-entry trips, the coarse bitmap, a wave's second batch of 64 rows, and the kernels fused over the
batch with a group holding two rows longer than two passes.

Weights are small multiples of 0.5 and the row sums stay below what the weight dtype holds exactly (checked here, on the CPU,
for every case): every partial sum is exact in any order of additions, so a dropped entry, an entry counted twice or a tail
entry past a row's end changes the result and `assert_array_equal` sees it — the tolerance tests cannot.  Equal values cannot
show a weight taken from a neighbouring position; one f32 test with random-mantissa weights does, at the project's tolerance."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-5
K = 2048
TORCH_DT = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
# multiples of 0.5 are all exact up to here: 2^(significand bits) halves; f16 / bf16 accumulate in f32 and round once, at the store
EXACT_MAX = {'f32': 2.0 ** 23, 'f64': 2.0 ** 52, 'f16': 2.0 ** 10, 'bf16': 2.0 ** 7}
W_UNITS = {'f32': 8, 'f64': 8, 'f16': 8, 'bf16': 2}            # weights 0.5 ... W_UNITS / 2
FIRE = {'f32': 0.25, 'f64': 0.25, 'f16': 0.25, 'bf16': 0.06}   # (bf16 holds sums up to 128 only)
HOMO_W = 0.5
# lanes per row -> (lowest, highest) average row length that selects them for rows with an indptr
TIERS = {2: (0, 8), 4: (9, 20), 8: (21, 45), 16: (46, 100), 32: (101, 200)}
WAVE_LENS = [255, 256, 257, 767, 768, 769, 1281]


def _with_total(rng, special, m, total):
    """m row lengths: `special` at random rows, the others random with everything summing to `total`."""
    rest = rng.multinomial(total - sum(special), np.full(m - len(special), 1.0 / (m - len(special))))
    lens = np.concatenate([np.asarray(special, np.int64), rest])
    rng.shuffle(lens)
    return lens


@functools.lru_cache(maxsize=None)
def tier_lens(lpr, m=200):
    """Ragged rows that select `lpr` lanes per row (two passes hold P = 8 lpr entries): the lengths around one pass, around two
    passes, one row that needs a second trip of the 512-entry walk, short rows for the rest."""
    P = 8 * lpr
    lo, hi = TIERS[lpr]
    special = [0, 1, 4 * lpr - 1, 4 * lpr, 4 * lpr + 1, P - 1, P, P + 1, P + 512 + 1]
    lens = _with_total(np.random.default_rng(lpr), special, m, (lo + hi + 1) // 2 * m + m // 2)
    assert lo <= int(lens.sum()) // m <= hi
    return lens


@functools.lru_cache(maxsize=None)
def wave_lens(m=70):
    rng = np.random.default_rng(70)
    lens = np.concatenate([WAVE_LENS, np.zeros(7, np.int64), rng.integers(200, 400, m - 14)])
    rng.shuffle(lens)
    assert int(lens.sum()) // m > 200
    return lens


def structure(lens, k, seed, last_columns=0):
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, k, int(ptr[-1])).astype(np.int32)
    if last_columns:                       # the tail of the bitmaps: the last columns, spread over the rows
        at = rng.choice(idx.size, min(idx.size, 4 * last_columns), replace=False)
        idx[at] = k - 1 - rng.integers(0, last_columns, at.size)
    return idx, ptr


def exact_weights(seed, n, dt, homo):
    if homo:
        return np.asarray([HOMO_W])
    return np.random.default_rng(seed + 1).integers(1, W_UNITS[dt] + 1, n) * 0.5


def spikes(seed, k, p, last_columns=0):
    v = np.random.default_rng(seed + 2).random(k) < p
    v[k - last_columns:] = True
    return v


def exact_ref(oracle, w, idx, ptr, v, shape, dt):
    """The f64 oracle's result, after checking that the kernel can reproduce it exactly in any order of additions: weights
    positive (every partial sum is below the row's sum), multiples of 0.5, the sums within the dtype's exact range."""
    ref = oracle.binary_csrmv(np.asarray(w, np.float64), idx, ptr, v, shape, False)
    assert np.all(np.asarray(w) > 0) and np.all(np.asarray(w) * 2 == np.round(np.asarray(w) * 2))
    assert ref.max() <= EXACT_MAX[dt]
    np.testing.assert_array_equal(torch.from_numpy(ref).to(TORCH_DT[dt]).double().numpy(), ref)
    return ref


def gpu_mv(be, w, idx, ptr, v, shape, dt):
    d = torch.device('cuda', 0)
    got = be.binary_csrmv(torch.from_numpy(np.asarray(w, np.float64)).to(TORCH_DT[dt]).to(d), torch.from_numpy(idx).to(d),
                          torch.from_numpy(ptr).to(d), torch.from_numpy(v).to(d), shape=shape, transpose=False)
    assert got.dtype == TORCH_DT[dt] and got.shape == (shape[0],)
    return got.double().cpu().numpy()


def check_mv(be, oracle, lens, k, dt, homo, seed, last_columns=0):
    idx, ptr = structure(lens, k, seed, last_columns)
    w = exact_weights(seed, idx.size, dt, homo)
    v = spikes(seed, k, FIRE[dt], last_columns)
    ref = exact_ref(oracle, w, idx, ptr, v, (len(lens), k), dt)
    np.testing.assert_array_equal(gpu_mv(be, w, idx, ptr, v, (len(lens), k), dt), ref)


# a: every lanes-per-row tier, ragged rows, m no multiple of 64;  g: every dtype on the 8-lane tier
@pytest.mark.parametrize('homo', [True, False])
@pytest.mark.parametrize('lpr,dt', [(2, 'f32'), (4, 'f32'), (8, 'f32'), (16, 'f32'), (32, 'f32'), (8, 'f64'), (8, 'f16'), (8, 'bf16')])
def test_lanes_per_row_tiers(be, oracle, lpr, dt, homo):
    check_mv(be, oracle, tier_lens(lpr), K, dt, homo, seed=lpr)


# c: the wave-per-row kernel around its 256-entry head and its 512-entry trips;  g: every dtype
@pytest.mark.parametrize('homo', [True, False])
@pytest.mark.parametrize('dt', ['f32', 'f64', 'f16', 'bf16'])
def test_wave_per_row(be, oracle, dt, homo):
    check_mv(be, oracle, wave_lens(), K, dt, homo, seed=300)


# b: rows of one known length (no indptr): exactly two passes of 8 / 16 lanes, where ragged rows would get 16 / 32
@pytest.mark.parametrize('homo', [True, False])
@pytest.mark.parametrize('n_conn', [64, 128])
def test_fixed_rows_of_exactly_two_passes(be, oracle, n_conn, homo):
    m, d = 130, torch.device('cuda', 0)
    idx, ptr = structure(np.full(m, n_conn), K, n_conn)
    w = exact_weights(n_conn, idx.size, 'f32', homo)
    v = spikes(n_conn, K, FIRE['f32'])
    ref = exact_ref(oracle, w, idx, ptr, v, (m, K), 'f32')
    wt = torch.from_numpy(w).float().to(d)
    conn = be.FixedNumPerPost((wt if homo else wt.view(m, n_conn), torch.from_numpy(idx).to(d).view(m, n_conn)), shape=(K, m))
    got = be.BinaryArray(torch.from_numpy(v).to(d)) @ conn
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    np.testing.assert_array_equal(got, ref)


# d: more columns than LDS holds bits for (a coarse bitmap in LDS, the exact one in memory), the bitmaps' last words in use
@pytest.mark.parametrize('homo', [True, False])
@pytest.mark.parametrize('rows', ['lpr2', 'lpr32', 'wave'])
def test_coarse_bitmap(be, oracle, rows, homo):
    lens = {'lpr2': lambda: tier_lens(2), 'lpr32': lambda: tier_lens(32), 'wave': wave_lens}[rows]()
    check_mv(be, oracle, lens, 1_300_000, 'f32', homo, seed=len(lens), last_columns=64)


# e: more rows than one sweep of the grid (256 workgroups x 16 waves x 64 rows with 8 spike columns): a wave's second batch
@pytest.mark.parametrize('homo', [True, False])
def test_second_batch_of_a_wave(be, oracle, homo):
    m, k, nb = 262_144 + 1024 + 37, 4096, 8
    lens = np.random.default_rng(5).integers(0, 5, m)
    idx, ptr = structure(lens, k, 5)
    w = exact_weights(5, idx.size, 'f32', homo)
    B = np.random.default_rng(6).random((k, nb)) < FIRE['f32']
    got = np.asarray(be.binary_csrmm(w.astype(np.float32), idx, ptr, B, shape=(m, k), transpose=False), np.float64)
    assert got.shape == (m, nb)
    for c in range(nb):
        np.testing.assert_array_equal(got[:, c], exact_ref(oracle, w, idx, ptr, B[:, c], (m, k), 'f32'), err_msg=f'column {c}')


# f: fused over the batch: a wave per row (lpr 0) and 8 / 16 / 32 lanes per row; rows 2, 3 and 70, 71 share a group at every
# lanes-per-row count and are longer than two passes, one of each pair by more than one 64-entry trip of its tail
@pytest.mark.parametrize('homo', [True, False])
@pytest.mark.parametrize('lpr,avg', [(8, 30), (16, 98), (32, 150), (0, 300)])
def test_fused_over_the_batch(be, oracle, lpr, avg, homo):
    m, rng = 300, np.random.default_rng(avg)
    if lpr:
        P = 8 * lpr
        lens = rng.multinomial(avg * m + m // 2 - 4 * P - 140, np.full(m - 4, 1.0 / (m - 4)))
        lens = np.insert(lens, [2, 2, 68, 68], [P + 64 + 1, P + 3, P + 1, P + 64 + 1])
        assert list(lens[[2, 3, 70, 71]]) == [P + 65, P + 3, P + 1, P + 65]
    else:
        lens = np.concatenate([WAVE_LENS, np.zeros(7, np.int64), rng.integers(200, 400, m - 14)])
        rng.shuffle(lens)
    assert int(lens.sum()) // m == avg or (lpr == 0 and int(lens.sum()) // m > 200)
    idx, ptr = structure(lens, K, avg)
    w = exact_weights(avg, idx.size, 'f32', homo)
    for nb in (8, 40):                    # 40: a second pass of 32 columns
        if (int(lens.sum()) // m) * nb < 768:
            continue                      # (below the fused route's work threshold: 8 lanes per row need more columns)
        B = np.random.default_rng(avg + nb).random((K, nb)) < 0.1
        got = np.asarray(be.binary_csrmm(w.astype(np.float32), idx, ptr, B, shape=(m, K), transpose=False), np.float64)
        assert got.shape == (m, nb)
        for c in range(nb):
            np.testing.assert_array_equal(got[:, c], exact_ref(oracle, w, idx, ptr, B[:, c], (m, K), 'f32'), err_msg=f'nb {nb} column {c}')


def test_random_mantissa_weights_come_from_their_own_positions(be, oracle):
    """Exactly representable weights cannot show a weight read from a neighbouring position when both hold the same value:
    f32 weights with random mantissas (neighbours differ), every tier and the wave kernel, at the project's tolerance."""
    for lens in [tier_lens(lpr) for lpr in TIERS] + [wave_lens()]:
        idx, ptr = structure(lens, K, 9)
        w = np.random.default_rng(10).uniform(0.1, 1.0, idx.size).astype(np.float32)
        assert np.all(w[1:] != w[:-1])
        v = spikes(9, K, 0.25)
        got = be.binary_csrmv(w, idx, ptr, v, shape=(len(lens), K), transpose=False)
        np.testing.assert_allclose(got, oracle.binary_csrmv(w.astype(np.float64), idx, ptr, v, (len(lens), K), False), rtol=RTOL, atol=ATOL)
